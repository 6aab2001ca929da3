"""The stride-2 convolutions (csrc/conv_strided.hip) for the float64 tests: a Python TRANSCRIPTION of the host rules
(which kernel configuration a shape runs, tiles, chunk counts, rows per workgroup, packed sizes -- no GPU, no ctypes),
the shape tables of tests/test_conv_strided_f64_gpu.py, and the references of each direction: the float64 result, the
bound's sum of absolute values and the fp32 emulation in the kernel's order of summation.

The transcription follows conv_strided.hip line by line; tests/test_conv_strided_f64_gpu.py and
tests/test_conv_strided_host_cpu.py check it against the library's host-only entry points.
"""
import functools
import itertools
import os

import torch
import torch.nn.functional as F

from tests.winograd import _atoi, _cdiv

INT_MAX = 0x7FFFFFFF
SLOPE = float(torch.tensor(0.1, dtype=torch.float32))   # the kernels take the slope as an fp32 number


def _rup(a, b):
    return _cdiv(a, b) * b


def _even(a):
    return a + (a & 1)


# --------------------------------------------------------------------------- host rules
def is_stem(Cin, k):
    return k == 7 and Cin == 3


def supported(Cin, N, k, H, W):
    """pcfa_conv_s2_supported"""
    if Cin < 1 or N < 1 or H < 2 or W < 4 or W % 4 != 0:
        return False
    if Cin * H * W > INT_MAX or N * H * W > INT_MAX:
        return False
    return is_stem(Cin, k) or k == 3


def bwd_supported(Cin, N, k, H, W):
    """pcfa_conv_s2_bwd_supported"""
    if not (k == 3 or is_stem(Cin, k)) or Cin < 1 or N < 1 or H < 2 or W < 8 or W % 8 != 0:
        return False
    return not (Cin * H * W > INT_MAX or N * H * W > INT_MAX)


def fwd_path(Cin, N, k, ds=False, env=None):
    """pcfa_conv_s2_fwd / pcfa_conv_s2_ds_fwd: StemCfg, Res3<WN, 1> or Res3<WN, 1, true> with WN = min(ceil(N / 32), 4)
    (the plain 3x3 honours the dev override PCFA_S2_WN)."""
    if not ds and is_stem(Cin, k):
        return "stem"
    assert k == 3, (Cin, k)
    nblk = _cdiv(N, 32)
    wn = min(nblk, 4)
    if not ds:
        wn = _atoi(os.environ if env is None else env, "PCFA_S2_WN", 0) or wn
    return ("ds_wn%d" if ds else "res_wn%d") % (wn if wn in (2, 3, 4) else 1)


def bwd_path(Cin, N, k, ds=False):
    """pcfa_conv_s2_bwd / pcfa_conv_s2_ds_bwd: the stem's own kernel, else S2BwdCfg<4,1>, <3,1>, <2,2>, <1,4> by
    ceil(Cin / 32) >= 4, 3, 2, 1."""
    if not ds and is_stem(Cin, k):
        return "stem_bwd"
    assert k == 3, (Cin, k)
    return ("ds_bwd_wn%d" if ds else "res_bwd_wn%d") % min(_cdiv(Cin, 32), 4)


FWD_LABELS = {"stem"} | {"res_wn%d" % i for i in (1, 2, 3, 4)}
DS_LABELS = {"ds_wn%d" % i for i in (1, 2, 3, 4)}
BWD_LABELS = {"stem_bwd"} | {"res_bwd_wn%d" % i for i in (1, 2, 3, 4)}
DS_BWD_LABELS = {"ds_bwd_wn%d" % i for i in (1, 2, 3, 4)}


def _wn(path):
    return int(path[-1])


def pixel_tile(path):
    """Pixels of one output row per workgroup: PXT = WP * MB * 32 output pixels (forward), PXC coarse pixels = 2 PXC
    columns of grad_x (backward)."""
    if path == "stem":
        return 128                                       # StemCfg: WN 2, WP 2, MB 2
    if path == "stem_bwd":
        return 64                                        # StemBwd::PXC = 16 MB
    return 32 * {1: 4, 2: 2, 3: 1, 4: 1}[_wn(path)]      # Res3<WN, 1> and S2BwdCfg<WN, WP> alike: WP = 4, 2, 1, 1


def channel_blocks(path):
    """32-channel blocks per workgroup (the stem's data gradient: its three channels in one 16-row tile)."""
    if path == "stem":
        return 2
    if path == "stem_bwd":
        return 1
    return _wn(path)


STEM_BWD_ROWS = 4   # StemBwd::TR coarse rows per workgroup


def chunks(path, Cin, N):
    """Chunks of the K loop.  Forward: one for the stem, else ceil(Cin / 4) padded to even; backward: ceil(N / 4)
    (the stem: ceil(N / 8)) padded to even -- two register sets of weights alternate."""
    if path == "stem":
        return 1
    if path == "stem_bwd":
        return _even(_cdiv(N, 8))
    if "bwd" in path:
        return _even(_cdiv(N, 4))
    return _even(_cdiv(Cin, 4))


def rows_per_workgroup(path, B, N, Ho, Wo, env=None):
    """fwd_t: as many rows as still leave >= 6 workgroups per CU, at most 16 (dev override PCFA_S2_RPW)."""
    env = os.environ if env is None else env
    tiles_x = _cdiv(Wo, pixel_tile(path))
    wn = channel_blocks(path)
    nby = _rup(_cdiv(N, 32), wn) // wn
    rpw = 1
    while rpw < 16 and tiles_x * _cdiv(Ho, rpw * 2) * nby * B >= 6 * 256:
        rpw *= 2
    e = _atoi(env, "PCFA_S2_RPW", 0)
    return e if e > 0 else rpw


def packed_floats(Cin, N, k):
    """pcfa_conv_s2_packed_floats: [block][chunk][step][lane]; the stem pads the blocks to 2 and has 3 * 4 * 7 steps, the
    3x3 pads them to 4 and has 2 * 9 steps per chunk of 4 channels."""
    if is_stem(Cin, k):
        return _rup(_cdiv(N, 32), 2) * 84 * 64
    if k == 3:
        return _rup(_cdiv(N, 32), 4) * _even(_cdiv(Cin, 4)) * 18 * 64
    return 0


def ds_packed_floats(Cin, N):
    """pcfa_conv_s2_ds_packed_floats: two more steps per chunk for the 1x1"""
    return _rup(_cdiv(N, 32), 4) * _even(_cdiv(Cin, 4)) * 20 * 64


def bwd_packed_floats(Cin, N, k):
    """pcfa_conv_s2_bwd_packed_floats"""
    if is_stem(Cin, k):
        return _even(_cdiv(N, 8)) * 32 * 64
    if k == 3:
        return _rup(_cdiv(Cin, 32), 4) * _even(_cdiv(N, 4)) * 18 * 64
    return 0


def ds_bwd_packed_floats(Cin, N):
    """pcfa_conv_s2_ds_bwd_packed_floats"""
    return _rup(_cdiv(Cin, 32), 4) * _even(_cdiv(N, 4)) * 20 * 64


def out_hw(k, H, W):
    return (H + 2 * (k // 2) - k) // 2 + 1, (W + 2 * (k // 2) - k) // 2 + 1


def regions(path, H, W, rpw=1):
    """Named (row slice, column slice) groups of the H x W output map of `path` (forward: the Ho x Wo output; backward:
    grad_x) for the statistical gate: first and last row and column, the ragged last pixel tile, the last row block
    (forward under rpw > 1; the stem's data gradient: its last 4 coarse rows), the interior, and for the gradients the
    four parity classes (y & 1, x & 1)."""
    px = pixel_tile(path) * (2 if "bwd" in path else 1)
    lc = (_cdiv(W, px) - 1) * px
    g = {"row0": (slice(0, 1), slice(None)), "rowN": (slice(H - 1, H), slice(None)),
         "col0": (slice(None), slice(0, 1)), "colN": (slice(None), slice(W - 1, W)),
         "last_tile": (slice(None), slice(lc, W)), "interior": (slice(1, max(H - 1, 1)), slice(1, max(W - 1, 1)))}
    rb = 2 * STEM_BWD_ROWS if path == "stem_bwd" else (rpw if "bwd" not in path else 1)
    if rb > 1:
        g["last_rows"] = (slice((_cdiv(H, rb) - 1) * rb, H), slice(None))
    if "bwd" in path:
        for a in (0, 1):
            for b in (0, 1):
                g["class%d%d" % (a, b)] = (slice(a, None, 2), slice(b, None, 2))
    return g


# --------------------------------------------------------------------------- the shape tables: (B, Cin, N, k, H, W)
FWD = [
    ((1, 3, 64, 7, 9, 264), "stem"),       # Wo = 132: two tiles of 128, the last with 4 pixels
    ((2, 3, 20, 7, 21, 72), "stem"),       # the second channel block is all padding
    ((2, 3, 96, 7, 6, 8), "stem"),         # nby = 2, the last group half empty
    ((1, 3, 1, 7, 2, 4), "stem"),          # the minimum
    ((1, 10, 24, 3, 9, 520), "res_wn1"),   # three tiles; 3 -> 4 chunks: one chunk is all padding
    ((1, 5, 32, 3, 7, 12), "res_wn1"),     # odd Cin
    ((1, 1, 8, 3, 2, 4), "res_wn1"),       # the minimum
    ((2, 16, 40, 3, 5, 136), "res_wn2"),   # ragged second block
    ((1, 64, 96, 3, 12, 72), "res_wn3"),   # RAFT 64 -> 96
    ((1, 7, 70, 3, 4, 40), "res_wn3"),     # ragged channels
    ((1, 128, 196, 3, 12, 40), "res_wn4"),  # PWC-Net conv6a: nby = 2, the last of 8 blocks empty
    ((1, 8, 128, 3, 6, 40), "res_wn4"),    # full blocks
]
DS = [(s, lab.replace("res", "ds")) for s, lab in FWD if s[3] == 3] + [((1, 96, 128, 3, 7, 40), "ds_wn4")]  # RAFT 96 -> 128 (four blocks), H odd
BWD = [
    ((1, 3, 64, 7, 9, 264), "stem_bwd"),   # three tiles of 64, odd H: the last coarse row has one fine row
    ((2, 3, 20, 7, 21, 72), "stem_bwd"),   # N % 8 != 0, 3 -> 4 chunks
    ((1, 3, 1, 7, 2, 8), "stem_bwd"),      # the minimum
    ((1, 10, 40, 3, 9, 264), "res_bwd_wn1"),
    ((1, 1, 1, 3, 2, 8), "res_bwd_wn1"),   # the minimum
    ((1, 5, 10, 3, 3, 16), "res_bwd_wn1"),  # padded chunk
    ((1, 64, 96, 3, 6, 136), "res_bwd_wn2"),
    ((2, 40, 10, 3, 5, 16), "res_bwd_wn2"),  # ragged block
    ((1, 96, 128, 3, 7, 72), "res_bwd_wn3"),
    ((1, 70, 6, 3, 4, 40), "res_bwd_wn3"),  # ragged block
    ((1, 128, 196, 3, 12, 40), "res_bwd_wn4"),
    ((1, 130, 6, 3, 3, 8), "res_bwd_wn4"),  # grid y = 2, the fifth block holds two channels
]
DS_BWD = [(s, lab.replace("res", "ds")) for s, lab in BWD if s[3] == 3]
RPW_SHAPE = (4, 4, 128, 3, 384, 256)       # res_wn4, tiles_x = 4, Ho = 192: 4 * 96 * 1 * 4 = 1536 workgroups at rpw 1 -> rpw 2


def host_rule_mismatches(lib):
    """Every (arguments, library's answer, mirror's answer) where the host-only entry points of `lib` disagree with the
    mirror, over a grid that holds every table shape and the 2^31 - 1 rule's two sides."""
    shapes = {s[1:] for t in (FWD, DS, BWD, DS_BWD) for s, _ in t} | {RPW_SHAPE[1:]}
    shapes |= set(itertools.product([1, 3, 4, 33, 97, 130], [1, 31, 64, 129, 196], [3, 5, 7], [1, 2, 9], [4, 8, 12, 18, 40]))
    shapes |= {(3, 64, 7, 0, 8), (0, 8, 3, 4, 8), (8, 0, 3, 4, 8), (8, 8, 3, 4, 0), (8, 8, 1, 4, 8),
               (4, 8, 3, 16384, 32768), (4, 8, 3, 16384, 32776), (3, 8, 7, 16384, 32768 + 8),   # Cin H W = 2^31 and around
               (1, 8, 3, 16384, 16384), (1, 9, 3, 16384, 16384), (1, 8, 3, 16383, 16384 + 8),   # N H W
               (3, 2, 7, 23170, 30888), (3, 2, 7, 23170, 30896)}                                   # 2147395440 / 2147951360
    bad = []
    for Cin, N, k, H, W in sorted(shapes):
        got = (bool(lib.pcfa_conv_s2_supported(Cin, N, k, H, W)), bool(lib.pcfa_conv_s2_bwd_supported(Cin, N, k, H, W)))
        exp = (supported(Cin, N, k, H, W), bwd_supported(Cin, N, k, H, W))
        if Cin >= 1 and N >= 1:
            got += (int(lib.pcfa_conv_s2_packed_floats(Cin, N, k)), int(lib.pcfa_conv_s2_bwd_packed_floats(Cin, N, k)),
                    int(lib.pcfa_conv_s2_ds_packed_floats(Cin, N)), int(lib.pcfa_conv_s2_ds_bwd_packed_floats(Cin, N)))
            exp += (packed_floats(Cin, N, k), bwd_packed_floats(Cin, N, k), ds_packed_floats(Cin, N),
                    ds_bwd_packed_floats(Cin, N))
        if got != exp:
            bad.append(((Cin, N, k, H, W), got, exp))
    return bad


def sid(s):
    return "x".join(map(str, s))


# --------------------------------------------------------------------------- references
def activate(y, act):
    if act == 1:
        return torch.relu(y)
    if act == 2:
        return torch.where(y > 0, y, y * torch.tensor(SLOPE, dtype=y.dtype))
    return y


@functools.lru_cache(maxsize=4)
def fwd_problem(B, Cin, N, k, H, W, ds=False, seed=0):
    """x, w, wd, bias, bias_d; per output (3x3 / 7x7, and the fused 1x1 under ds) without bias or activation: the
    float64 result, the sum of absolute values P and the fp32 emulation in the kernel's order -- chunk, channel pair (the
    stem: channel, row pair), row, tap, the two k of a step; the 1x1: channel by channel."""
    gen = torch.Generator().manual_seed(seed * 7919 + Cin * 131 + N * 17 + H * W + k)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(N, Cin, k, k, generator=gen) / (Cin * k * k) ** .5
    wd = torch.randn(N, Cin, 1, 1, generator=gen) / Cin ** .5
    b, bd = torch.randn(N, generator=gen), torch.randn(N, generator=gen)
    pad = k // 2
    Ho, Wo = out_hw(k, H, W)
    want = F.conv2d(x.double(), w.double(), stride=2, padding=pad)
    P = F.conv2d(x.double().abs(), w.double().abs(), stride=2, padding=pad)
    xp = F.pad(x, (pad, pad, pad, pad))

    def term(c, p, q):
        return w[:, c, p, q].view(1, N, 1, 1) * xp[:, c, p:p + 2 * Ho - 1:2, q:q + 2 * Wo - 1:2].unsqueeze(1)

    emu = torch.zeros(B, N, Ho, Wo)
    if is_stem(Cin, k):
        for c in range(3):
            for pp in range(4):
                for q in range(7):
                    for p in (2 * pp, 2 * pp + 1):
                        if p < 7:
                            emu = emu + term(c, p, q)
    else:
        for c0 in range(0, Cin, 2):
            for p in range(3):
                for q in range(3):
                    for c in range(c0, min(c0 + 2, Cin)):
                        emu = emu + term(c, p, q)
    outs = [(want, P, emu)]
    if ds:
        want_d = F.conv2d(x.double(), wd.double(), stride=2)
        P_d = F.conv2d(x.double().abs(), wd.double().abs(), stride=2)
        emu_d = torch.zeros(B, N, Ho, Wo)
        for c in range(Cin):
            emu_d = emu_d + wd[:, c, 0, 0].view(1, N, 1, 1) * x[:, c, ::2, ::2].unsqueeze(1)
        outs.append((want_d, P_d, emu_d))
    return x, w, wd, b, bd, outs


def grad_f64(g, w, H, W, gd=None, wd=None):
    """The data gradient of conv2d(stride=2, padding=k//2) [+ conv2d(1x1, stride=2)] as a transposed convolution whose
    output_padding returns H x W."""
    k = w.shape[-1]
    pad = k // 2
    Ho, Wo = g.shape[-2:]
    op = (H - ((Ho - 1) * 2 - 2 * pad + k), W - ((Wo - 1) * 2 - 2 * pad + k))
    dx = F.conv_transpose2d(g, w, stride=2, padding=pad, output_padding=op)
    if gd is not None:
        dx = dx + F.conv_transpose2d(gd, wd, stride=2, output_padding=(H - (2 * Ho - 1), W - (2 * Wo - 1)))
    return dx


@functools.lru_cache(maxsize=4)
def bwd_problem(B, Cin, N, k, H, W, ds=False, seed=0):
    """g, gd, w, wd; the float64 data gradient, P, and the fp32 emulation in the kernel's order: by parity class, chunk
    of 4 output channels, channel pair, p, q, the two k (then the pair's 1x1 steps into class (0, 0)); the stem: chunk of
    8, group of 4, the 16 taps (di, dj), the four k."""
    gen = torch.Generator().manual_seed(seed * 7919 + Cin * 131 + N * 17 + H * W + k + 1)
    Ho, Wo = out_hw(k, H, W)
    g, gd = torch.randn(B, N, Ho, Wo, generator=gen), torch.randn(B, N, Ho, Wo, generator=gen)
    w = torch.randn(N, Cin, k, k, generator=gen) / (N * k * k / 4) ** .5
    wd = torch.randn(N, Cin, 1, 1, generator=gen) / N ** .5
    d = lambda t: t.double()  # noqa: E731
    want = grad_f64(d(g), d(w), H, W, d(gd) if ds else None, d(wd) if ds else None)
    P = grad_f64(d(g).abs(), d(w).abs(), H, W, d(gd).abs() if ds else None, d(wd).abs() if ds else None)
    emu = torch.zeros(B, Cin, H, W)
    rows = (Ho, H // 2)   # coarse rows of class a: y = 2 i + a < H
    cls = {(a, b): torch.zeros(B, Cin, rows[a], Wo) for a in (0, 1) for b in (0, 1)}
    if is_stem(Cin, k):
        gp = F.pad(g, (1, 2, 1, 2))

        def tap(n, a, b, di, dj):   # dx[c][2 i + a][2 j + b] += g[n][i + di][j + dj] w[n][c][a + 3 - 2 di][b + 3 - 2 dj]
            p, q = a + 3 - 2 * di, b + 3 - 2 * dj
            if 0 <= p < 7 and 0 <= q < 7:
                cls[a, b] = cls[a, b] + w[n, :, p, q].view(1, Cin, 1, 1) * \
                    gp[:, n, 1 + di:1 + di + rows[a], 1 + dj:1 + dj + Wo].unsqueeze(1)

        for n0 in range(0, N, 4):
            for di in range(-1, 3):
                for dj in range(-1, 3):
                    for n in range(n0, min(n0 + 4, N)):
                        for a, b in cls:
                            tap(n, a, b, di, dj)
    else:
        gp = F.pad(g, (0, 1, 0, 1))
        for n4 in range(0, N, 4):
            for n0 in range(n4, min(n4 + 4, N), 2):
                for p in range(3):
                    for q in range(3):   # (p, q) feeds class (p != 1, q != 1) from g[i + (p == 0)][j + (q == 0)]
                        a, b, dp, dq = int(p != 1), int(q != 1), int(p == 0), int(q == 0)
                        for n in range(n0, min(n0 + 2, N)):
                            cls[a, b] = cls[a, b] + w[n, :, p, q].view(1, Cin, 1, 1) * \
                                gp[:, n, dp:dp + rows[a], dq:dq + Wo].unsqueeze(1)
            if ds:   # the chunk's 1x1 steps follow its 3x3 steps
                for n in range(n4, min(n4 + 4, N)):
                    cls[0, 0] = cls[0, 0] + wd[n, :, 0, 0].view(1, Cin, 1, 1) * gd[:, n].unsqueeze(1)
    for (a, b), t in cls.items():
        emu[:, :, a::2, b::2] = t
    return g, gd, w, wd, want, P, emu


def fwd_terms(Cin, k):
    return Cin * k * k + 1


def bwd_terms(Cin, N, k, ds=False):
    """The number of terms the bound allows an element of grad_x: 4 N for the 3x3 (class (1, 1) sums that many), N more
    under ds for the 1x1's share of class (0, 0); 16 N for the stem."""
    return 16 * N if is_stem(Cin, k) else 4 * N + (N if ds else 0)
