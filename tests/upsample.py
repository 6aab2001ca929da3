"""The upsamplers of csrc/upsample_ops.hip for the float64 tests: RAFT / GMA convex upsampling (pcfa_convex_upsample_fwd /
_bwd: convex_upsample_fwd_kernel, _bwd_kernel, _gflow_kernel), PWC-Net's bilinear upsampling (pcfa_upsample_bilinear_fwd /
_bwd) and FlowNet2's nearest upsampling (pcfa_upsample_nearest4_fwd / _bwd): float64 references, the kernels' arithmetic in
fp32 on the CPU (`emu`), inputs, case tables and the gates of tests/test_upsample_f64_gpu.py and
tests/test_upsample_host_cpu.py.  No GPU, no ctypes.  u, gamma, TINY as in tests/fenced.py; every bound carries the factor
SPARE = 1 + 2^-14 for second-order terms.

CONVEX UPSAMPLE.  flow [N][2][H][W], logits mask [N][9 * 64][H][W] (channel k 64 + i 8 + j), out [N][2][8H][8W]:
  p_k = softmax_k(x_k);  up_ck = 8 flow[c][h + k / 3 - 1][w + k % 3 - 1], zero outside the map;  out = sum_k p_k up_ck
  dp_k = sum_c g_c up_ck;  grad_mask_k = p_k (dp_k - sum_j p_j dp_j)
  T[c][k][h][w] = sum_ij p_k g_c;  grad_flow[c][y][x] = 8 sum_k T[c][k][y - k / 3 + 1][x - k % 3 + 1]
Reference: exactly that in float64 on the fp32 inputs.  Emulation: fp32 in the kernel's order -- max, exp(x - m), the sum in k
order, the division; the 9-term sums in k order; T over j in the thread, then over i; the 9-tap gather, times 8.
Softmax term.  d_k = m - x_k.  The fp32 subtraction errs by u d_k, which exp turns into a relative error; expf adds
C_EXP u; the sum of nine positive terms carries their weighted relative error, C_EXP u + u sum_j p_j d_j with
sum_j p_j d_j = H(p) - log s <= log 9 < 2.2, plus 8 u for its additions; the division u:
    |p^_k - p_k| <= p_k (2 C_EXP + d_k + 11.2) u.
C_EXP is the relative error of the device expf in units of u.  The HIP math API states 1 ulp, that is 2 u; the bound takes
C_EXP = 4, twice that, so (2 C_EXP + d_k + 10) u =: s_k holds with 2.8 u to spare.  It is consistent with the 2.43 u this
project measured for the whole device sigmoid (tests/gru_epilogue.py) and is not taken from the kernel under test.  Where
exp(-d_k) is below the normal range (d_k > 87.3) the result may be flushed: an absolute TINY per p_k (s >= 1, so the division
does not amplify it).  p_k = 0 exactly for x_k = -inf and for x_k - m overflowing to -inf; both references agree.
  forward    nine products and up to nine additions, gamma(10):  |out^ - out| <= SPARE sum_k (p_k (s_k + gamma(10)) + TINY)
             |up_k| + 12 TINY -- proportional to sum_k p_k |up_k|.
  grad_mask  a_k = sum_c |g_c up_ck| >= |dp_k| (dp_k: two roundings, gamma(2) a_k), D = sum_j p_j a_j; dot = sum p dp:
             |dot^ - dot| <= sum_j p_j (s_j + gamma(12)) a_j (+ TINY sum_j a_j); the subtraction and the product 2 u:
             |gm^_k - gm_k| <= SPARE [p_k (s_k + gamma(4)) (a_k + D) + p_k sum_j p_j (s_j + gamma(12)) a_j
                                      + TINY (a_k + D + sum_j a_j)] + 16 TINY -- proportional to p_k (|dp_k| + sum p |dp|),
             with a_k in place of |dp_k| because the two channels' products may cancel.
  grad_flow  chains of 9 (the product and 8 additions over j), 8 (over i) and 9 (the gather): gamma(26) with the factor 8
             exact:  |gf^ - gf| <= SPARE 8 sum over the 64 * 9 contributions (p (s + gamma(26)) + TINY) |g| + 4608 TINY.
Statistical gate: tests/gates.py against `emu`, overall, per 32 channels and per region: `border` (the ring of coarse
pixels whose taps leave the map), `interior`, `last_wg` (the columns of the last, partly dead, 64-column workgroup).
Shapes: W = 65, 70, 130 leave 1, 6, 2 live columns in the last workgroup; the dead columns' threads (w >= W, clamped to
W - 1) still take part in the LDS sum.  Logit classes per output pixel: `normal` N(0, 2); `peak40` one logit 40 above;
`tied` all nine equal; `saturated` one logit 120 above and one 95 below it (expf underflows, through the subnormals);
`minus_inf` some logits -inf; `huge` +-3e38 (x - m overflows to -inf).  Flow N(0, 3), every fifth pixel of magnitude 10^4.

BILINEAR UPSAMPLE (align_corners = False, times mul).  src = rscale (dst + 0.5) - 0.5 in fp32 with rscale = fp32(1 / f); the
compiler may or may not fuse the multiply-subtract, so positions() gives both roundings (they differ only for f = 3, 5, where
rscale is inexact).  From the fp32 position on everything is float64: clamp at 0, i1 = (int) src, i1p = i1 < size - 1,
l1 = src - i1 (exact in fp32 too), l0 = 1 - l1; out = mul (Ay x Ax^T) with the OH x H and OW x W tap matrices, and the exact
adjoint grad_in = mul (Ay^T g Ax).  A result must pass with the unfused or with the fused positions as reference; either
bound carries the term |delta src| |v1 - v0|, formed as the largest difference between the references of the four
(y, x) combinations of the two roundings and the one in use.
  forward   l0 (1), l0x v (1), the sum (1), l0y (1), its product (1), the sum (1), mul (1): gamma(7 + 2) |mul| P,
            P = Ay |x| Ax^T, + 9 TINY.
  backward  the kernel gathers over the window f y - (f + 1) / 2 - 1 .. f y + f + (f + 1) / 2 + 1 of L = f + 2 ((f + 1) / 2) + 3
            outputs per axis: the weights (2), two products (2), L additions per axis, mul (1):
            gamma(2 L + 5 + 2) |mul| S, S = Ay^T |g| Ax, + (2 L + 7) TINY.
The adjoint identity needs no mirror: |<y, g> - <x, gx>| in float64 on the kernel's own outputs is at most
sum |g| bound_fwd + sum |x| bound_bwd; a window that misses a contributing output fails it however small its weight.

NEAREST-4.  out = up4(x op s); grad_in = fp32(float64 sum of the 16 gradients) op s, both exact.

Kernel by kernel: convex_upsample_fwd_kernel, _bwd_kernel, _gflow_kernel -- every CONVEX_SHAPES case (W = 65, 70, 130: the
dead-column path; (1, 1, 1), (2, 1, 5): H = 1); upsample_bilinear_fwd_kernel, _bwd_kernel -- BILINEAR_SHAPES x FACTORS (f = 4
with W = 65, 129: the tail of the 256-thread blocks; f = 5, 8: the longest windows); upsample_nearest4_fwd_kernel,
_bwd_kernel -- NEAREST_SHAPES x div.
"""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as Fn

from tests.fenced import TINY, U, gamma
from tests.gates import gates as _gates

F32, F64 = torch.float32, torch.float64
SPARE = 1 + 2.0 ** -14
C_EXP = 4.0

# =========================================================================== convex upsample
CONVEX_SHAPES = ((1, 1, 1), (2, 1, 5), (1, 3, 63), (1, 2, 64), (2, 3, 65), (1, 7, 70), (1, 5, 130))
LOGIT_CLASSES = ("normal", "peak40", "tied", "saturated", "minus_inf", "huge")
CONVEX_GOUTS = ("random", "zero", "onehot")
MIN_PER_CLASS = 8
WILD_SHAPE = (2, 3, 65)


def _cgen(shape, salt):
    N, H, W = shape
    return torch.Generator().manual_seed(salt * 7919 + 131 * H + 17 * W + N)


def logit_class(shape):
    """The class index of every output pixel [N][8][8][H][W]."""
    N, H, W = shape
    coarse = torch.arange(N * H * W).view(N, 1, 1, H, W)
    sub = torch.arange(64).view(1, 8, 8, 1, 1)
    return (coarse * 65 + sub) % len(LOGIT_CLASSES)


@functools.lru_cache(maxsize=None)
def convex_inputs(shape):
    """(flow [N][2][H][W], mask [N][576][H][W]) fp32."""
    N, H, W = shape
    g = _cgen(shape, 1)
    flow = 3.0 * torch.randn(N, 2, H, W, generator=g)
    big = (torch.arange(H * W).view(1, 1, H, W) % 5 == 0).expand(N, 2, H, W)
    flow = torch.where(big, 1.0e4 * torch.randn(N, 2, H, W, generator=g), flow)
    x = 2.0 * torch.randn(N, 9, 8, 8, H, W, generator=g)
    cls = logit_class(shape).unsqueeze(1)
    ks = torch.randint(0, 9, (N, 1, 8, 8, H, W), generator=g)
    k2 = (ks + 1 + torch.randint(0, 8, (N, 1, 8, 8, H, W), generator=g)) % 9
    k = torch.arange(9).view(1, 9, 1, 1, 1, 1)
    star, second = k == ks, k == k2
    name = LOGIT_CLASSES.index
    x = torch.where((cls == name("peak40")) & star, x + 40.0, x)
    x = torch.where(cls == name("tied"), x[:, :1].expand_as(x), x)
    top = 120.0 + x.gather(1, ks)
    x = torch.where((cls == name("saturated")) & star, top, x)
    x = torch.where((cls == name("saturated")) & second, top - 95.0, x)
    drop = (torch.rand(N, 9, 8, 8, H, W, generator=g) < 0.4) & ~star
    x = torch.where((cls == name("minus_inf")) & (drop | second), torch.tensor(-math.inf), x)
    x = torch.where((cls == name("huge")) & star, torch.tensor(3.0e38), x)
    x = torch.where((cls == name("huge")) & second, torch.tensor(-3.0e38), x)
    return flow.contiguous(), x.reshape(N, 576, H, W).contiguous()


def convex_census(shape):
    N, H, W = shape
    flow, mask = convex_inputs(shape)
    x = mask.view(N, 9, 8, 8, H, W).double()
    cls = logit_class(shape)
    d = x.max(1).values.unsqueeze(1) - x
    out = {"class/" + c: int((cls == i).sum()) for i, c in enumerate(LOGIT_CLASSES)}
    out["tied"] = int((d == 0).all(1).sum())
    out["peak>=35"] = int(((d >= 35) & (d < 60)).sum(1).ge(8).sum())
    out["underflow"] = int(((d > 104) & (d < 1e30)).any(1).sum())
    out["subnormal"] = int(((d > 88) & (d < 103)).any(1).sum())
    out["-inf"] = int(torch.isinf(x).any(1).sum())
    out["overflow"] = int((d > 3.4e38).any(1).sum())
    out["flow>1e3"] = int((flow.abs() > 1e3).sum())
    out["live_in_last_wg"] = W - 64 * ((W - 1) // 64)
    out["dead_columns"] = 64 * (-(-W // 64)) - W
    return out


@functools.lru_cache(maxsize=None)
def convex_gout(shape, variant="random"):
    N, H, W = shape
    g = torch.randn(N, 2, 8 * H, 8 * W, generator=_cgen(shape, 2))
    if variant == "zero":
        g = torch.zeros_like(g)
    elif variant == "onehot":        # in the last live column of the last workgroup, next to the dead ones
        g = torch.zeros_like(g)
        g[N - 1, 1, 8 * (H - 1) + 3, 8 * (W - 1) + 5] = 1.0
    return g


def taps(flow, mut=None):
    """up [N][2][9][H][W] = 8 flow at the nine taps, zero outside, in flow's dtype."""
    N, _, H, W = flow.shape
    f8 = 8.0 * flow
    pad = Fn.pad(f8, (1, 1, 1, 1), mode="replicate") if mut == "clamp_border" else Fn.pad(f8, (1, 1, 1, 1))
    out = []
    for k in range(9):
        ky, kx = divmod(k, 3)
        if mut == "transpose":
            ky, kx = kx, ky
        out.append(pad[:, :, ky:ky + H, kx:kx + W])
    return torch.stack(out, 2)


def _sub(g, N, H, W):
    """[N][2][8H][8W] -> [N][2][i][j][H][W]."""
    return g.reshape(N, 2, H, 8, W, 8).permute(0, 1, 3, 5, 2, 4)


def _unsub(o, N, H, W):
    """[N][2][i][j][H][W] -> [N][2][8H][8W]."""
    return o.permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)


def _gather9(T):
    """sum_k T[n][c][k][y - k / 3 + 1][x - k % 3 + 1] in k order, zero outside."""
    N, C, _, H, W = T.shape
    Tp = Fn.pad(T, (1, 1, 1, 1))
    s = torch.zeros(N, C, H, W, dtype=T.dtype)
    for k in range(9):
        ky, kx = divmod(k, 3)
        s = s + Tp[:, :, k, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
    return s


def convex_ref(flow, mask, gout):
    """float64: out, grad_flow, grad_mask and their elementwise bounds."""
    N, _, H, W = flow.shape
    x = mask.double().view(N, 9, 8, 8, H, W)
    p = torch.softmax(x, 1)
    d = x.max(1, keepdim=True).values - x
    zero = torch.zeros((), dtype=F64)
    s = (2 * C_EXP + d + 10) * U
    ps = torch.where(p > 0, p * torch.where(torch.isfinite(s), s, zero), zero)          # p_k s_k, 0 where p_k = 0
    up = taps(flow.double())                                        # [N][2][9][H][W]
    upb = up.view(N, 2, 9, 1, 1, H, W)
    r = types.SimpleNamespace()
    r.out = _unsub((p.unsqueeze(1) * upb).sum(2), N, H, W)
    r.out_bound = SPARE * _unsub(((ps + p * gamma(10) + TINY).unsqueeze(1) * upb.abs()).sum(2), N, H, W) + 12 * TINY
    g = _sub(gout.double(), N, H, W)                                # [N][2][8][8][H][W]
    dp = (g.unsqueeze(2) * upb).sum(1)                              # [N][9][8][8][H][W]
    a = (g.unsqueeze(2) * upb).abs().sum(1)
    dot, D = (p * dp).sum(1, keepdim=True), (p * a).sum(1, keepdim=True)
    r.gm = (p * (dp - dot)).reshape(N, 576, H, W)
    inner = ((ps + p * gamma(12)) * a).sum(1, keepdim=True)
    r.gm_bound = (SPARE * ((ps + p * gamma(4)) * (a + D) + p * inner + TINY * (a + D + a.sum(1, keepdim=True))) + 16 * TINY).reshape(N, 576, H, W)
    T = (p.unsqueeze(1) * g.unsqueeze(2)).sum((3, 4))               # [N][2][9][H][W]
    A = ((ps + p * gamma(26) + TINY).unsqueeze(1) * g.abs().unsqueeze(2)).sum((3, 4))
    r.gf = 8.0 * _gather9(T)
    r.gf_bound = SPARE * 8.0 * _gather9(A) + 4608 * TINY
    return r


def _softmax32(x, mut=None):
    """softmax9 of the kernels: [N][9][...] fp32."""
    m = x[:, 0]
    for k in range(1, 9):
        m = torch.maximum(m, x[:, k])
    e = torch.exp(x if mut == "no_max" else x - m.unsqueeze(1))
    s = torch.zeros_like(m)
    for k in range(9):
        s = s + e[:, k]
    return e / s.unsqueeze(1)


def convex_emu(flow, mask, gout, mut=None):
    """fp32 in the kernels' order: (out, grad_flow, grad_mask)."""
    N, _, H, W = flow.shape
    p = _softmax32(mask.view(N, 9, 8, 8, H, W), mut)
    up = taps(flow, mut).view(N, 2, 9, 1, 1, H, W)
    o = torch.zeros(N, 2, 8, 8, H, W)
    for k in range(9):
        o = o + p[:, k].unsqueeze(1) * up[:, :, k]
    g = _sub(gout, N, H, W)
    dp = [g[:, 0] * up[:, 0, k] + g[:, 1] * up[:, 1, k] for k in range(9)]
    dot = torch.zeros(N, 8, 8, H, W)
    for k in range(9):
        dot = dot + p[:, k] * dp[k]
    gm = torch.stack([p[:, k] * (dp[k] if mut == "gm_no_dot" else dp[k] - dot) for k in range(9)], 1).reshape(N, 576, H, W)
    pg = p.unsqueeze(1) * g.unsqueeze(2)                            # [N][2][9][i][j][H][W]
    t = torch.zeros(N, 2, 9, 8, H, W)
    for j in range(8):
        t = t + pg[:, :, :, :, j]
    T = torch.zeros(N, 2, 9, H, W)
    for i in range(8):
        T = T + t[:, :, :, i]
    gf = _gather9(T)
    return _unsub(o, N, H, W), (gf if mut == "gflow_no8" else 8.0 * gf), gm


def convex_regions(shape):
    """name -> bool [H][W] over the coarse pixels."""
    N, H, W = shape
    h, w = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    border = ((h == 0) | (h == H - 1) | (w == 0) | (w == W - 1)).expand(H, W)
    last = (w >= 64 * ((W - 1) // 64)).expand(H, W) if W > 64 else torch.zeros(H, W, dtype=torch.bool)
    return {"border": border, "last_wg": last, "interior": ~border & ~last}


def _fine(m):
    return m.repeat_interleave(8, 0).repeat_interleave(8, 1)


@functools.lru_cache(maxsize=None)
def convex_case(shape, variant="random", wild=False):
    """Inputs, float64 results with bounds and the emulation of one case.  wild: three pixels' nine logits are -inf, +inf and
    NaN; the references are those of the logits with zeros there, gated on everything such a pixel does not feed."""
    N, H, W = shape
    flow, mask = convex_inputs(shape)
    c = types.SimpleNamespace(shape=shape, flow=flow, mask=mask, gout=convex_gout(shape, variant), poisoned=None)
    if wild:
        c.mask = mask.clone()
        clean = mask.clone()
        pix = torch.zeros(N, H, W, dtype=torch.bool)
        for (n, h, w, i, j), v in zip(((0, 0, 0, 2, 3), (N - 1, H // 2, 30, 7, 7), (N - 1, H - 1, W - 1, 0, 5)),
                                      (-math.inf, math.inf, math.nan)):
            ch = torch.arange(9) * 64 + i * 8 + j
            c.mask[n, ch, h, w], clean[n, ch, h, w], pix[n, h, w] = v, 0.0, True
        near = Fn.max_pool2d(pix.float().unsqueeze(1), 3, 1, 1).bool()                # the 3 x 3 neighbourhood [N][1][H][W]
        c.poisoned = types.SimpleNamespace(out=_fine_n(pix).unsqueeze(1), gm=pix.unsqueeze(1), gf=near)
        mask = clean
    c.ref = convex_ref(flow, mask, c.gout)
    c.emu = convex_emu(flow, mask, c.gout)
    return c


def _fine_n(m):
    return m.repeat_interleave(8, 1).repeat_interleave(8, 2)


def convex_check(c, got_out, got_gf, got_gm, record, prefix=""):
    """Both gates on the three results of one case: ((elem, stat) of out, of grad_flow, of grad_mask)."""
    N, H, W = c.shape
    reg = convex_regions(c.shape)
    res = []
    for name, got, want, bound, emu, fine in (("out_", got_out, c.ref.out, c.ref.out_bound, c.emu[0], True),
                                              ("gflow_", got_gf, c.ref.gf, c.ref.gf_bound, c.emu[1], False),
                                              ("gmask_", got_gm, c.ref.gm, c.ref.gm_bound, c.emu[2], False)):
        if got is None:
            res.append(None)
            continue
        if c.poisoned is not None:
            m = getattr(c.poisoned, {"out_": "out", "gflow_": "gf", "gmask_": "gm"}[name]).expand_as(got)
            got, emu = torch.where(m, want.float(), got), torch.where(m, want.float(), emu)
        extra = {k: (_fine(m) if fine else m).expand_as(want) for k, m in reg.items()}
        res.append(_gates(got, want, None, 0, emu, 0, record, prefix + name, regions=lambda *_: {}, bound=bound, extra=extra))
    return res


# =========================================================================== bilinear upsample
FACTORS = (1, 2, 3, 4, 5, 8)
BILINEAR_SHAPES = ((1, 1, 1), (3, 1, 9), (2, 6, 1), (2, 7, 5), (1, 5, 65), (4, 3, 129))
MULS = (20.0, 1.0, -0.5)
BILINEAR_GOUTS = ("random", "zero", "hot_nw", "hot_ne", "hot_sw", "hot_se", "hot_in")


def window(f):
    """(below, above): the backward's gather window f i - below .. f i + above."""
    return (f + 1) // 2 + 1, f + (f + 1) // 2 + 1


def positions(n_out, f, fused, mut=None):
    """src [n_out] fp32 before the clamp: rscale (dst + 0.5) - 0.5 with the product rounded (fused = False) or not."""
    rs = np.float32(1.0) / np.float32(f)
    t = torch.arange(n_out, dtype=F32) + 0.5
    if mut == "align_corners":
        return torch.arange(n_out, dtype=F32) * float(np.float32(max(n_out // f - 1, 0)) / np.float32(max(n_out - 1, 1)))
    if fused:
        return (t.double() * float(rs) - 0.5).float()          # the product of two fp32 values is exact in float64
    return t * torch.tensor(float(rs), dtype=F32) - 0.5


def bilin_taps(n_out, size, f, fused, dtype, mut=None):
    """bilin_tap for every output index: (i1, ip long, l0, l1 in dtype)."""
    src = positions(n_out, f, fused, mut)
    if mut != "no_clamp":
        src = torch.where(src < 0, torch.zeros(()), src)
    i1 = src.trunc().long()
    ip = (i1 < size - 1).long()
    l1 = src.to(dtype) - i1.to(dtype)
    return i1, ip, 1 - l1, l1


def tap_matrix(n_out, size, f, fused, mut=None):
    """A [n_out][size] float64: out = A in."""
    i1, ip, l0, l1 = bilin_taps(n_out, size, f, fused, F64, mut)
    A = torch.zeros(n_out, size, dtype=F64)
    r = torch.arange(n_out)
    A.index_put_((r, i1), l0, accumulate=True)
    A.index_put_((r, i1 + ip), l1, accumulate=True)
    return A


def bilinear_fwd_emu(x, f, mul, fused, mut=None):
    P, H, W = x.shape
    yi, yp, yl0, yl1 = bilin_taps(H * f, H, f, fused, F32, mut)
    xi, xp, xl0, xl1 = bilin_taps(W * f, W, f, fused, F32, mut)
    r0, r1 = x[:, yi], x[:, yi + yp]
    top = xl0 * r0[:, :, xi] + xl1 * r0[:, :, xi + xp]
    bot = xl0 * r1[:, :, xi] + xl1 * r1[:, :, xi + xp]
    return torch.tensor(mul, dtype=F32) * (yl0.view(-1, 1) * top + yl1.view(-1, 1) * bot)


def _axis_gather(g, size, f, fused, cut, mut):
    """sum over the window of w(O, i) g[..][O] along the last axis, in window order: [..][size] fp32."""
    n_out = size * f
    i1, ip, l0, l1 = bilin_taps(n_out, size, f, fused, F32, mut)
    below, above = window(f)
    i = torch.arange(size)
    lo, hi = (f * i - below + cut[0]).clamp_min(0), (f * i + above - cut[1]).clamp_max(n_out - 1)
    acc = torch.zeros(g.shape[:-1] + (size,))
    for k in range(below + above + 1):
        O = (lo + k).clamp_max(n_out - 1)
        w = torch.where(i1[O] == i, l0[O], torch.zeros(())) + torch.where(i1[O] + ip[O] == i, l1[O], torch.zeros(()))
        w = torch.where(lo + k <= hi, w, torch.zeros(()))
        acc = acc + w * g[..., O]
    return acc


def bilinear_bwd_emu(g, H, W, f, mul, fused, cut=((0, 0), (0, 0)), mut=None):
    """The gather of upsample_bilinear_bwd_kernel; cut = ((y below, y above), (x below, x above)) shortens the window."""
    r = _axis_gather(g, W, f, fused, cut[1], mut)                               # [P][OH][W]
    s = _axis_gather(r.transpose(1, 2), H, f, fused, cut[0], mut).transpose(1, 2)
    return torch.tensor(mul, dtype=F32) * s


@functools.lru_cache(maxsize=None)
def bilinear_inputs(shape, f):
    P, H, W = shape
    g = torch.Generator().manual_seed(1000 * f + 131 * H + 17 * W + P)
    return torch.randn(P, H, W, generator=g), torch.randn(P, H * f, W * f, generator=g)


def bilinear_gout(shape, f, variant):
    P, H, W = shape
    g = bilinear_inputs(shape, f)[1]
    if variant == "random":
        return g
    z = torch.zeros_like(g)
    OH, OW = H * f, W * f
    spot = {"hot_nw": (0, 0), "hot_ne": (0, OW - 1), "hot_sw": (OH - 1, 0), "hot_se": (OH - 1, OW - 1), "hot_in": (OH // 2, OW // 2)}
    if variant != "zero":
        z[P - 1][spot[variant]] = 1.0
    return z


@functools.lru_cache(maxsize=None)
def _matrices(shape, f):
    P, H, W = shape
    return {fu: (tap_matrix(H * f, H, f, fu), tap_matrix(W * f, W, f, fu)) for fu in (False, True)}


def bilinear_ref(shape, f, mul, variant="random"):
    """Per rounding of the positions (False: unfused, True: fused): out, its bound, grad_in, its bound (float64)."""
    P, H, W = shape
    x, _ = bilinear_inputs(shape, f)
    g = bilinear_gout(shape, f, variant)
    x64, g64, m = x.double(), g.double(), float(np.float32(mul))
    A = _matrices(shape, f)
    fw = {(a, b): m * (A[a][0] @ x64 @ A[b][1].T) for a in (False, True) for b in (False, True)}
    bw = {(a, b): m * (A[a][0].T @ g64 @ A[b][1]) for a in (False, True) for b in (False, True)}
    L = sum(window(f)) + 1
    out = {}
    for fu in (False, True):
        Ay, Ax = A[fu]
        dfw = torch.stack([(v - fw[fu, fu]).abs() for v in fw.values()]).max(0).values
        dbw = torch.stack([(v - bw[fu, fu]).abs() for v in bw.values()]).max(0).values
        out[fu] = types.SimpleNamespace(
            out=fw[fu, fu], out_bound=SPARE * (gamma(9) * abs(m) * (Ay @ x64.abs() @ Ax.T) + dfw) + 9 * TINY,
            gin=bw[fu, fu], gin_bound=SPARE * (gamma(2 * L + 7) * abs(m) * (Ay.T @ g64.abs() @ Ax) + dbw) + (2 * L + 7) * TINY)
    return out


def _either(record, prefix, got, refs, emus, what):
    """The gates with the unfused or with the fused positions as reference: (elem, stat, rounding that passed)."""
    err = None
    for fu in (False, True):
        r = refs[fu]
        want, bound = (r.out, r.out_bound) if what == "out" else (r.gin, r.gin_bound)
        notes = []                                   # only the rounding that passes is recorded
        try:
            e, s = _gates(got.unsqueeze(0), want.unsqueeze(0), None, 0, emus[fu].unsqueeze(0), 0, lambda *kv: notes.append(kv),
                          prefix, regions=lambda *_: {}, bound=bound.unsqueeze(0))
        except AssertionError as ex:
            err = err or ex
            continue
        for kv in notes:
            record(*kv)
        record(prefix + "positions", "fused" if fu else "unfused")
        return e, s, fu
    raise err


def bilinear_check_fwd(shape, f, mul, got, record, prefix="", emus=None):
    x, _ = bilinear_inputs(shape, f)
    emus = emus or {fu: bilinear_fwd_emu(x, f, mul, fu) for fu in (False, True)}
    return _either(record, prefix + "fwd_", got, bilinear_ref(shape, f, mul), emus, "out")


def bilinear_check_bwd(shape, f, mul, variant, got, record, prefix="", emus=None):
    P, H, W = shape
    g = bilinear_gout(shape, f, variant)
    emus = emus or {fu: bilinear_bwd_emu(g, H, W, f, mul, fu) for fu in (False, True)}
    if variant == "zero":
        assert bool((got == 0).all())
    return _either(record, prefix + variant + "_bwd_", got, bilinear_ref(shape, f, mul, variant), emus, "gin")


def adjoint_ratio(shape, f, mul, y, gx, fu_y, fu_g, variant="random"):
    """|<y, g> - <x, gx>| over its bound, from the kernel's own outputs."""
    x, _ = bilinear_inputs(shape, f)
    g = bilinear_gout(shape, f, variant)
    ref = bilinear_ref(shape, f, mul, variant)
    lhs = abs(float((y.double() * g.double()).sum() - (x.double() * gx.double()).sum()))
    rhs = float((g.double().abs() * ref[fu_y].out_bound).sum() + (x.double().abs() * ref[fu_g].gin_bound).sum())
    return lhs / rhs


# =========================================================================== nearest-4
NEAREST_SHAPES = ((1, 1, 1), (2, 3, 65), (3, 2, 5))
NEAREST_S = 20.0


def nearest4_case(shape, div):
    P, H, W = shape
    g = torch.Generator().manual_seed(H * W + int(div))
    x = torch.randn(P, H, W, generator=g) * 7
    gy = torch.randn(P, 4 * H, 4 * W, generator=g)
    up = torch.nn.Upsample(scale_factor=4, mode="nearest")
    y = up((x / NEAREST_S if div else x * NEAREST_S).unsqueeze(0))[0]
    s64 = gy.double().view(P, H, 4, W, 4).sum((2, 4)).float()
    return x, gy, y, (s64 / NEAREST_S if div else s64 * NEAREST_S)
