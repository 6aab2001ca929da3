"""Winograd convolutions in float64 (and emulated fp32) with the kernels' own transform matrices, their rigorous
componentwise error bounds, and a Python mirror of the host rules that pick a kernel path for a shape.

Transforms (Y = A^T [ (G g G^T) .* (B^T d B) ] A per tile, 1-D: y = A^T [ (G g) .* (B^T d) ]):
  F23  F(2x2,3x3), csrc/conv3x3.hip (conv3x3_pack_kernel, mfma_chunk's row w of B^T d, the epilogue's A^T . A)
  F43  F(4x4,3x3), csrc/conv3x3_f43.hip, interpolation points 0, +-1, +-2, inf (f43_pack_kernel, `operands`, epilogue)
  F25  1-D F(2,5), csrc/sepconv5_wino.hip, the same six points (sc5_wino_pack_kernel, the input / output transforms)
Every stage the kernels evaluate (row and column stage of B^T d B, of A^T M A, of G g G^T) is a sum of distinct
entries of one matrix row, so the product of the absolute stage matrices equals |B^T| |d| |B| etc.

Rigorous bound.  Run with |B^T|, |G|, |A^T|, |d| and |g| the same evaluator gives P = |A^T| [sum_k (|G||g_k||G^T|) .*
(|B^T||d_k||B|)] |A|, and a computed output satisfies |Y - Y64| <= c gamma_n P + tiny (module tests/fenced.py), where
n counts the roundings on the longest path through the kernel's order of operations:
  F23: weight transform 4 (two 3-term sums in fp32, the 0.5 is exact), input transform 2 (fma row stage, one add),
       K terms (one MFMA accumulation each), splits - 1 partial additions (KS = 2 in the workgroup, or K slices in the
       finish pass), output transform 4 (two 3-term sums), bias 1, mask slope 1, addend 1:   n = K + splits + 12
  F43: weight transform 1 (computed in double, rounded once), input transform 6 (row stage: one product and three
       fmas; column stage: two operations), K terms, 1 for the two channel groups of the workgroup, ksplit - 1
       partial additions, output transform 6 (3 + 3), bias, mask slope, addend 3:        n = K + ksplit + 16
  F25: weight transform 1, input transform 2, Cin terms, KS - 1 <= 3 group partials, output transform 3, accumulate
       into the output 1:                                                                 n = Cin + 10
  direct sepconv5 (implicit GEMM): 5 Cin products, the split2 partial addition 1, accumulate 1:   n = 5 Cin + 2
  The fused SepConvGRU epilogues of both sepconv5 kernels (tests/gru_epilogue.py) add to the convolution's n:
    mode 1 gates_fwd : + 1 (add_zr); z, r: the device sigmoid (c_sigmoid u |z|);  rh = r h: 1
    mode 2 update_fwd: + 1 (add_q);  q: the device tanhf (c_tanh u |q|);  hnew = (1 - z) h + z q: 4
    mode 3 gates_bwd : dzr[:, :C] = dz (1 - z) z: 3 (no convolution);  dzr[:, C:] = ((drh h)(1 - r)) r: 4;
                       dh = drh r + dh_in: 2 (1 without dh_in);  d_rest: the plain accumulate of n
    mode 4 update_bwd: + 1 (g = dh_acc + ddh);  dz = g q - g h: 3;  dqc = (g z)(1 - q q): 4;  dh = g (1 - z): 2;
                       d_rest: the plain accumulate of n
  each product and each addition of the expression counted once, which covers a contraction to fma either way.
c = 2 covers an MFMA that rounds each product and each addition separately; tiny = n 2^-126 covers flushed
subnormals.  Tests add 2 spare roundings to each count.  The activation is applied to the float64 pre-activation:
ReLU and LeakyReLU are 1-Lipschitz, so the bound of the pre-activation holds for the activated value as well; a mask
factor (1 or the slope) scales both the value and P.
"""
import math
import os

import torch

# --------------------------------------------------------------------------- transform matrices
F23_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
F23_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
F23_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]

F6_BT = [[4, 0, -5, 0, 1, 0],      # points 0, +-1, +-2, inf: shared by F(4x4,3x3) and F(2,5)
         [0, -4, -4, 1, 1, 0],
         [0, 4, -4, -1, 1, 0],
         [0, -2, -1, 2, 1, 0],
         [0, 2, -1, -2, 1, 0],
         [0, 4, 0, -5, 0, 1]]
F43_G = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
         [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
F43_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
F25_G = [[1 / 4, 0, 0, 0, 0], [-1 / 6, -1 / 6, -1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6, 1 / 6, -1 / 6],
         [1 / 24, 2 / 24, 4 / 24, 8 / 24, 16 / 24], [1 / 24, -2 / 24, 4 / 24, -8 / 24, 16 / 24], [0, 0, 0, 0, 1]]
F25_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1]]

ALGOS = {"f23": (F23_BT, F23_G, F23_AT), "f43": (F6_BT, F43_G, F43_AT), "f25": (F6_BT, F25_G, F25_AT)}


def _mats(algo, dtype, absval):
    bt, g, at = (torch.tensor(m, dtype=torch.float64) for m in ALGOS[algo])
    if absval:
        bt, g, at = bt.abs(), g.abs(), at.abs()
    return bt.to(dtype), g, at.to(dtype)


def _accumulate(V, U, eq, partials, dtype):
    """sum_k over the channel axis of V (dim 1) and U (dim 1): one einsum in float64, or -- emulated fp32 -- the kernel's
    order: each partial (a list of channels) summed term by term from zero, the partials added in index order."""
    if partials is None:
        return torch.einsum(eq, V, U)
    out = None
    for part in partials:
        acc = None
        for k in part:
            t = torch.einsum(eq, V[:, k:k + 1], U[:, k:k + 1])
            acc = t if acc is None else acc + t
        if acc is not None:
            out = acc if out is None else out + acc
    return out


def winograd_conv3x3(x, w, algo, absval=False, dtype=torch.float64, partials=None, weight_f64=None):
    """3x3 / pad 1 convolution of x [B][K][H][W] with w [N][K][3][3] through `algo` ("f23" | "f43"), ragged edges padded
    with zero tiles.  absval: the bound's P (|matrices|, |x|, |w|).  dtype float32 + partials: the fp32 emulation
    (partials: channel lists, see _accumulate); weight_f64: the weight transform in float64, rounded once (F43)."""
    BT, G, AT = _mats(algo, dtype, absval)
    m, a = AT.shape[0], BT.shape[0]
    B, K, H, W = x.shape
    th, tw = -(-H // m), -(-W // m)
    xp = torch.zeros(B, K, th * m + 2, tw * m + 2, dtype=dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x.abs() if absval else x
    d = xp.unfold(2, a, m).unfold(3, a, m)                            # [B, K, th, tw, a, a]
    V = BT @ d @ BT.T
    wd = w.abs() if absval else w
    if weight_f64 is None:
        weight_f64 = algo == "f43"
    if weight_f64:
        U = (G @ wd.double() @ G.T).to(dtype)
    else:
        U = G.to(dtype) @ wd.to(dtype) @ G.T.to(dtype)                # [N, K, a, a]
    M = _accumulate(V, U, "bkhwij,nkij->bnhwij", partials, dtype)
    Y = AT @ M @ AT.T                                                 # [B, N, th, tw, m, m]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, th * m, tw * m)[:, :, :H, :W]


def winograd_sepconv5(x, w, vertical, absval=False, dtype=torch.float64, partials=None):
    """The 5-tap convolution (pad 2) of x [B][C][H][W] with w [N][C][5] along W (1x5) or H (vertical, 5x1) as 1-D
    Winograd F(2,5), ragged edges padded with zero tiles; arguments as winograd_conv3x3 (the weight transform is
    computed in float64 and rounded once, as the kernel's packing does)."""
    BT, G, AT = _mats("f25", dtype, absval)
    if vertical:
        x = x.transpose(2, 3)
    B, C, H, W = x.shape
    tw = -(-W // 2)
    xp = torch.zeros(B, C, H, 2 * tw + 4, dtype=dtype)
    xp[..., 2:W + 2] = x.abs() if absval else x
    d = xp.unfold(3, 6, 2)                                            # [B, C, H, tw, 6]
    V = d @ BT.T
    U = ((w.abs() if absval else w).double() @ G.T).to(dtype)        # [N, C, 6]
    M = _accumulate(V, U, "bkhti,nki->bnhti", partials, dtype)
    Y = (M @ AT.T).reshape(B, -1, H, 2 * tw)[..., :W]
    return Y.transpose(2, 3) if vertical else Y


def direct_sepconv5_fp32(x, w, vertical):
    """The direct implicit GEMM of csrc/sepconv5.hip emulated in fp32: the 5 Cin products added term by term, zero
    outside the image."""
    B, Cin, H, W = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 2, 2) if vertical else (2, 2, 0, 0))
    emu = torch.zeros(B, w.shape[0], H, W)
    for c in range(Cin):
        for t in range(5):
            xs = xp[:, c, t:t + H, :] if vertical else xp[:, c, :, t:t + W]
            emu += w[:, c, t].view(1, -1, 1, 1) * xs.unsqueeze(1)
    return emu


def chunk_partials(K, splits):
    """Channel lists of a kernel's partial sums, chunks of 8 input channels: splits = [(kind, n)] applied in turn.
    ("slices", n): contiguous ranges of ceil(nchunk / n) chunks (F(2x2,3x3) K slices, F(4x4,3x3) ksplit uses
    floor(nchunk s / n) boundaries: ("ksplit", n)); ("interleave", g): chunk c to group c % g within each range."""
    nchunk = -(-K // 8)
    ranges = [list(range(nchunk))]
    for kind, n in splits:
        nxt = []
        for r in ranges:
            if kind == "slices":
                per = -(-len(r) // n)
                nxt += [r[i:i + per] for i in range(0, len(r), per)]
            elif kind == "ksplit":
                nxt += [r[len(r) * s // n:len(r) * (s + 1) // n] for s in range(n)]
            else:
                nxt += [r[g::n] for g in range(n)]
        ranges = nxt
    return [[k for c in r for k in range(8 * c, min(8 * c + 8, K))] for r in ranges]


# --------------------------------------------------------------------------- host dispatch mirror
def _atoi(env, name, default):
    v = env.get(name)
    if v is None:
        return default
    digits = ""
    for ch in v.strip():
        if ch.isdigit() or (ch in "+-" and not digits):
            digits += ch
        else:
            break
    try:
        return int(digits)
    except ValueError:
        return 0


def _cdiv(a, b):
    return -(-a // b)


def f23_kslices(B, K, N, H, W, env=None):
    """conv3x3.hip f23_kslices"""
    env = os.environ if env is None else env
    e = _atoi(env, "PCFA_CONV3X3_KSL", -1)
    if e == 0 or (H * W) % 4 != 0:
        return 1
    nchunk = _cdiv(K, 8)
    nwg = _cdiv(W, 16) * _cdiv(H, 8) * ((N + 31) // 32) * B
    want = e if e > 0 else min(256 // max(nwg, 1), nchunk // 2)
    if e < 0 and (B > 2 or H * W > 2048 or nwg > 128):
        want = 1
    if want < 2 or nchunk < 2:
        return 1
    want = min(want, nchunk)
    cper = _cdiv(nchunk, want)
    return _cdiv(nchunk, cper)


def f43_ksplit(B, K, N, H, W):
    """conv3x3_f43.hip pcfa_f43_ksplit"""
    nwg = _cdiv(W, 64) * _cdiv(H, 8) * _cdiv(N, 32) * B
    if nwg >= 192:
        return 1
    return max(min(256 // nwg, _cdiv(K, 8) // 2), 1)


def f43_packed_floats(K, N):
    return 36 * _cdiv(K, 8) * 8 * _cdiv(N, 32) * 32


def f43_supported(B, K, N, H, W):
    return W % 4 == 0 and W >= 8 and K * H * W < 0x7fffffff and B < 16384 and f43_packed_floats(K, N) < 0x7fffffff


def use_f43(B, K, N, H, W, env=None):
    """conv3x3.hip use_f43 (PCFA_CONV3X3_ALGO = f23 | f43 | r04)"""
    env = os.environ if env is None else env
    e = env.get("PCFA_CONV3X3_ALGO")
    forced = 0 if e is None else 4 if e[:1] == "r" else 43 if e[1:2] == "4" else 23
    if not f43_supported(B, K, N, H, W):
        return False
    if forced in (43, 23):
        return forced == 43
    if B == 1:
        px = H * W
        if px <= 2048 and f23_kslices(B, K, N, H, W, env) > 1:
            return False
        if px <= 4096 and K >= 176:
            return True
        if 4096 < px <= 16384 and K >= 384:
            return True
        if 16384 <= px < 100000 and K * N >= 15000:
            return True
    if forced != 4:
        return False
    if H < 24 or W < 64 or K < 16:
        return False
    ks = f43_ksplit(B, K, N, H, W)
    if ks > 1:
        return ks == 2 and K * N >= 192 * 256
    return H * W >= 100000


def conv3x3_workspace_bytes(B, K, N, H, W, env=None):
    """conv3x3.hip pcfa_conv3x3_workspace_bytes"""
    ksl = f23_kslices(B, K, N, H, W, env)
    sliced = ksl * B * N * H * W * 4 if ksl > 1 else 0
    f43 = 0
    if use_f43(B, K, N, H, W, env):
        ks = f43_ksplit(B, K, N, H, W)
        f43 = ks * B * N * H * W * 4 if ks > 1 else 0
    return max(f43, sliced)


def conv3x3_path(B, K, N, H, W, aligned=True, workspace=True, pair=None, env=None):
    """The kernel path pcfa_conv3x3_run (pair: (K2, N2) of pcfa_conv3x3_act_fwd_pair) takes for a shape: f43_direct,
    f43_split, f43_fallthrough (F(4x4,3x3) picked, x misaligned: the F(2x2,3x3) kernel runs), f23_ksliced, f23_ks2,
    f23_xcd, f23_mt2, f23_ring3, f23_plain, f23_plain_partial (K % 8 != 0) -- the F(2x2,3x3) labels of a fall-through
    are reported as its `sub` path."""
    env = os.environ if env is None else env
    if pair is None and use_f43(B, K, N, H, W, env):
        if aligned:
            return "f43_split" if f43_ksplit(B, K, N, H, W) > 1 else "f43_direct"
        return "f43_fallthrough"
    ksl = f23_kslices(B, K, N, H, W, env) if pair is None else 1
    if ksl > 1 and workspace:
        return "f23_ksliced"
    return f23_launch_path(B, K, N, H, W, pair, env)


def f23_launch_path(B, K, N, H, W, pair=None, env=None):
    """conv3x3.hip conv3x3_launch with ksl = 1"""
    env = os.environ if env is None else env
    mt = 2 if _atoi(env, "PCFA_CONV3X3_MT", 1) == 2 and pair is None else 1
    gx = _cdiv(W, 16) * _cdiv(H, 16 if mt == 2 else 8)
    gy = _cdiv(N, 64) * 2
    if pair is not None:
        gy += _cdiv(pair[1], 64) * 2
    nwg = gx * gy * B
    ks_env = _atoi(env, "PCFA_CONV3X3_KS", 0)
    if mt == 1 and pair is None and K % 16 == 0 and (ks_env == 2 if ks_env else nwg <= 256):
        return "f23_ks2"
    if _atoi(env, "PCFA_XCD_MAP", 1) != 0 and mt == 1 and gx * gy >= 1024:
        return "f23_xcd"
    if mt == 2:
        return "f23_mt2"
    if _atoi(env, "PCFA_CONV3X3_RING", 2) == 3:
        return "f23_ring3"
    return "f23_plain" if K % 8 == 0 else "f23_plain_partial"


def conv3x3_splits(path, B, K, N, H, W, env=None):
    """The kernel's partial-sum structure for chunk_partials and the `splits` count of the bound."""
    if path == "f23_ks2":
        return [("interleave", 2)], 2
    if path == "f23_ksliced":
        ksl = f23_kslices(B, K, N, H, W, env)
        return [("slices", ksl)], ksl
    if path.startswith("f43"):
        if path == "f43_fallthrough":
            return [], 1
        ks = f43_ksplit(B, K, N, H, W)
        six = _atoi(os.environ if env is None else env, "PCFA_F43_WAVES", 0) == 6
        return [("ksplit", ks)] + ([] if six else [("interleave", 2)]), ks
    return [], 1


def sepconv5_wino_wide(B, Cout, H, W, vertical):
    tiles = ((W // 64) * ((H + 1) // 2) if vertical else (W // 128) * H) * B
    return Cout % 64 == 0 and tiles * (Cout // 64) >= 200


def sepconv5_uses_winograd(B, Ca, Cb, Cout, H, W, vertical, enabled=True):
    """sepconv5_wino.hip sc5_wino_shape_ok"""
    Cin = Ca + Cb
    if not enabled:
        return False
    ks = 2 if sepconv5_wino_wide(B, Cout, H, W, vertical) else 4
    if Cout % 32 != 0 or Cin % (16 * ks) != 0 or Ca % 8 != 0:
        return False
    return W % (64 if vertical else 128) == 0 and B <= 65535 and H * W <= 1 << 30


def sepconv5_path(B, Ca, Cb, Cout, H, W, vertical, enabled=True, aligned=True, env=None):
    """wino_wide, wino_narrow (sepconv5_wino.hip), direct_split2, direct_fast, direct_slow (sepconv5.hip)"""
    env = os.environ if env is None else env
    if sepconv5_uses_winograd(B, Ca, Cb, Cout, H, W, vertical, enabled) and aligned:
        return "wino_wide" if sepconv5_wino_wide(B, Cout, H, W, vertical) else "wino_narrow"
    Cin = Ca + Cb
    fast = aligned and Cout % 4 == 0 and W % 4 == 0 and Cin % 32 == 0 and Cout >= 4 and W >= 4
    nwg = _cdiv(W, 64) * H * _cdiv(Cout, 64) * B
    ks_env = _atoi(env, "PCFA_SEPCONV_KS", 0)
    if fast and Cin % 64 == 0 and (ks_env == 2 if ks_env else nwg <= 320):
        return "direct_split2"
    return "direct_fast" if fast else "direct_slow"


def sepconv5_wino_groups(B, Cout, H, W, vertical):
    return 2 if sepconv5_wino_wide(B, Cout, H, W, vertical) else 4


def rel_l2_64(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def regions(H, W, m):
    """Named (row slice, column slice) groups of an output map for the statistical gate: edges, the ragged last tile
    (the rows / columns of the last tile row / column, which is partial when H or W is not a multiple of m) and the
    interior."""
    lr, lc = (math.ceil(H / m) - 1) * m, (math.ceil(W / m) - 1) * m
    return {"row0": (slice(0, 1), slice(None)), "rowN": (slice(H - 1, H), slice(None)),
            "col0": (slice(None), slice(0, 1)), "colN": (slice(None), slice(W - 1, W)),
            "last_tile": (slice(lr, H), slice(lc, W)), "interior": (slice(1, max(H - 1, 1)), slice(1, max(W - 1, 1)))}
