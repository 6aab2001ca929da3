"""The warps (csrc/warp_ops.hip: PWC-Net's and SpyNet's backward warp, forward and both backward forms) and FlowNet2's
Resample2d (csrc/flownet_ops.hip, csrc/resample2d_taps.hpp, the fixed-point backward of warp_ops.hip) for the float64
tests: the fp32 sample positions mirrored bit for bit, float64 references of everything after the position, a census of
where every pixel, channel and texel sits against the kernels' edges, flow builders that steer pixels there, the case
table and the gates of tests/test_warp_f64_gpu.py and tests/test_warp_host_cpu.py.  No GPU, no ctypes.

Positions are part of the contract: the kernels (warp_coord, spy_grid, spy_unnormalize, the Resample2d prologue) round
every step on its own, and so do the CPU fp32 tensor operations here:
  PWC-Net     f = fp32(flo fs); g = 2 (base + f); g = g / max(size - 1, 1); g = g - 1; pos = fmaf(g + 1, size, -1) / 2
  SpyNet      g = hor[x] + fp32(flo sx); g = clamp(g, -1, 1), NaN passed through; pos = fmaf(g + 1, size, -1) / 2
  Resample2d  pos = x + dx
The one fused step is (a size - 1) in float64, rounded once to fp32.  a = g + 1 is a multiple of 2^-24 (|g| >= 1/2: g is
one; |g| < 1/2: the sum lies in (1/2, 3/2) and is rounded to one), so a size - 1 is a multiple of 2^-24 too and exact in
float64 while |a| size + 1 < 2^29: fma_half asserts both on every finite case.

From the fp32 position on everything is float64: floor, the four weights (exact: position and floor are fp32 values),
tap validity, the mask sum, the blend, the scatter (scatter_add_) and the flow-gradient gather.  fp32 and float64 can
therefore not fall into different cells and every pixel is decided.  The mask decision compares the mask sum with the
fp32 threshold: build() asserts that no pixel's float64 mask sum lies within 2^-20 (relative) of the threshold unless
the fp32 mask sum is exact (equal to the float64 one: the weights that are multiples of 1/4 of the `threshold` cases and
their one-ulp neighbours) -- a condition on the inputs; the gates then leave out no pixel and no texel.

Every reference takes a dtype: float64 is the reference proper, float32 the plain fp32 implementation in the kernels' tap
and channel order (the `emu` of tests/gates.gates; tests/test_warp_host_cpu.py pushes it through every gate).  With
fixed = True the fp32 implementation adds its addends as the kernels do: rounded once to the call's unit, summed as
integers, converted once.

Gates: u, gamma, TINY of tests/fenced.py; elementwise |Y - Y64| <= bound, statistical as tests/gates.gates over
everything, per 32 channels and per census class of at least 256 elements.  n = the roundings one term goes through; the
two roundings of the weight's factors (ex = (x0 + 1) - ix, wx1 = ix - x0 and their y twins, each one subtraction) are the
`+ 2` spare every gate here carries.
  forward (PWC, SpyNet)   2 gamma(N_FWD + 2) P + (N_FWD + 2) TINY, P = sum over valid taps |x_t| w_t (times the mask)
      N_FWD = 5: w = ex ey (1), x_t w (1), three sums (3); the product with the 0/1 mask is exact
  forward (Resample2d)    the same with N_RS_FWD = 4: one term (1 - a)(1 - b) x is formed in double and rounded once (1),
      three fp32 sums (3).  alpha = xf - floor(xf) rounds only for xf < 0, where both neighbours are clamped to texel 0
      and the weights' sum, not their split, reaches the output.
  grad_x / grad_in1, fixed point   2 gamma(N_FIX + 2) S + k unit / 2 + (N_FIX + 2) TINY, S = sum |w g| over the addends
      of the texel, k their number (census), unit = 2^(floor(log2 max|grad_out|) - 40)
      N_FIX = 3: the weight product (1), the product with g (1), the finish's conversion (1; the integer sum is exact)
  grad_x / grad_in1, atomic        2 gamma(k + N_ATOMIC + 2) S + (..) TINY, N_ATOMIC = 2 (the two products), + k adds
  grad_flo (PWC, SpyNet)  2 gamma(n + 2) P + (n + 2) TINY, P = scale sum_c sum_taps |v w g|,
      scale = |fs| size / max(size - 1, 1) (PWC), |s| size / 2 where the clamp passes (SpyNet);
      n = n_gflo(C, G): tap_fma's product v w (1), one fma per tap and channel of the group (4 ceil(C / G)),
      flow_grad (PWC: the product with size / 2 and the division, 2; SpyNet: 1), the finish's G - 1 sums, the product
      with fs / sx / sy (1).  The spare 2 covers the one weight factor.
  grad_flow (Resample2d)  2 gamma(n + 2) P + u A + (n + 2) TINY, n = n_rs_gflow(C) = 2 + 4 C: gam gv (1), the product
      with the texel (1), four adds per channel into gdx / gdy.  gam = 1 - beta and 1 - gam are rounded absolutely
      (u / 2 each: beta = 2^-30 gives gam = 1.0f and 1 - gam = 0), so a weight is off by up to u absolutely:
      A = sum_c |gv| (|iTL| + |iTR| + |iBL| + |iBR|) is the unweighted sum of the corner products.
"""
import functools
import math
import types

import numpy as np
import torch

from tests.fenced import TINY, U, gamma
from tests.gates import gates as _gates

N_FWD, N_RS_FWD, N_FIX, N_ATOMIC = 5, 4, 3, 2
FIX_BITS = 40
FS = (1.0, 0.625, 5.0)
THR = float(np.float32(0.0001))     # PWC-Net's production mask threshold
WT, WWIN, WCH = 16, 32, 4           # the LDS window kernel's tile, window and channels per pass
BAND = 2.0 ** -20
F32, F64 = torch.float32, torch.float64


def f32(v):
    return float(np.float32(v))


def channel_groups(plane, C):
    g = 1
    while plane * g < 65536 and 2 * g <= C // 4 and g < 32:
        g *= 2
    return g


def n_gflo(C, G, spy):
    return 1 + 4 * -(-C // G) + (1 if spy else 2) + (G - 1) + 1


def n_rs_gflow(C):
    return 2 + 4 * C


def spy_scales(H, W):
    one = np.float32(1.0)
    return float(one / np.float32((W - 1.0) / 2.0)), float(one / np.float32((H - 1.0) / 2.0))


# --------------------------------------------------------------------------- positions (fp32, bit for bit)
def fma_half(a, size, strict=True):
    """fmaf(a, size, -1) / 2 of the fp32 tensor a: float64 product and sum (exact under the asserted condition), one
    rounding to fp32, an exact halving."""
    a64 = a.double()
    if strict:
        fin = a64[torch.isfinite(a64)]
        assert fin.numel() == a64.numel(), "non-finite grid value in a finite case"
        assert bool((fin * 2.0 ** 24 == (fin * 2.0 ** 24).round()).all()), "g + 1 is no multiple of 2^-24"
        assert float(fin.abs().max()) * size + 1 < 2.0 ** 29, "(g + 1) size - 1 does not fit 53 bits"
    return (a64 * size - 1.0).float() / 2.0


def _base(n, axis):
    t = torch.arange(n, dtype=F32)
    return t.view(1, 1, n) if axis == "x" else t.view(1, n, 1)


def pwc_axis(base, flo, fs, size, strict=True):
    g = 2.0 * (base + flo * torch.tensor(fs, dtype=F32))
    g = g / torch.full_like(g, float(max(size - 1, 1)))
    g = g - 1.0
    return fma_half(g + 1.0, size, strict)


def pwc_positions(flo, fs, strict=True):
    """(ix, iy) [B][H][W] fp32: warp_coord of meshgrid + fp32(flo fs)."""
    H, W = flo.shape[-2:]
    return pwc_axis(_base(W, "x"), flo[:, 0], fs, W, strict), pwc_axis(_base(H, "y"), flo[:, 1], fs, H, strict)


def spy_axis(lin, flo, s, size, strict=True):
    """(position, unclamped grid value g): spy_grid and spy_unnormalize."""
    g = lin + flo * torch.tensor(s, dtype=F32)
    gc = torch.where(g != g, g, g.clamp(-1.0, 1.0))
    return fma_half(gc + 1.0, size, strict), g


def spy_positions(flo, hor, ver, sx, sy, strict=True):
    H, W = flo.shape[-2:]
    ix, gx = spy_axis(hor.view(1, 1, W), flo[:, 0], sx, W, strict)
    iy, gy = spy_axis(ver.view(1, H, 1), flo[:, 1], sy, H, strict)
    return ix, iy, gx, gy


def rs_positions(flow):
    H, W = flow.shape[-2:]
    return _base(W, "x") + flow[:, 0], _base(H, "y") + flow[:, 1]


# --------------------------------------------------------------------------- the bilinear sample (warp_sample)
def _long(t):
    """tap_index: the floor clamped to +-1e8 before the conversion, NaN -> -1e8."""
    return torch.nan_to_num(t, nan=-1.0e8).clamp(-1.0e8, 1.0e8).long()


def sample(ix, iy, H, W, dtype=F64, mut=None):
    """warp_taps / warp_sample in `dtype` from the fp32 position: taps in the kernels' order nw, ne, sw, se."""
    ix, iy = ix.to(dtype), iy.to(dtype)
    fx, fy = ix.floor(), iy.floor()
    s = types.SimpleNamespace(x0=_long(fx), y0=_long(fy), wx1=ix - fx, wy1=iy - fy, ex=(fx + 1) - ix, ey=(fy + 1) - iy)
    s.w = [s.ex * s.ey, s.wx1 * s.ey, s.ex * s.wy1, s.wx1 * s.wy1]
    vx0, vy0 = (s.x0 >= 0) & (s.x0 < W), (s.y0 >= 0) & (s.y0 < H)
    vx1 = (s.x0 + 1 >= 0) & ((s.x0 + 1 <= W) if mut == "x1_le_W" else (s.x0 + 1 < W))
    vy1 = (s.y0 + 1 >= 0) & (s.y0 + 1 < H)
    s.vx0, s.vx1, s.vy0, s.vy1 = vx0, vx1, vy0, vy1
    s.valid = [vx0 & vy0, vx1 & vy0, vx0 & vy1, vx1 & vy1]
    offs = [s.y0 * W + s.x0, s.y0 * W + s.x0 + 1, (s.y0 + 1) * W + s.x0, (s.y0 + 1) * W + s.x0 + 1]
    s.off = [torch.where(v, o, torch.zeros_like(o)).clamp(0, H * W - 1) for v, o in zip(s.valid, offs)]
    zero = torch.zeros((), dtype=dtype)
    s.msum = torch.zeros_like(ix)
    for v, w in zip(s.valid, s.w):
        s.msum = s.msum + torch.where(v, w, zero)
    return s


def _active(s, thr, mut=None):
    t = torch.tensor(thr, dtype=F32).to(s.msum.dtype)
    return (s.msum > t) if mut == "mask_gt" else (s.msum >= t)


def _gather(xg, off):
    B, C, plane = xg.shape
    return xg.gather(2, off.reshape(B, 1, -1).expand(B, C, -1))


def warp_fwd(x, ix, iy, thr, dtype=F64, mut=None):
    """pwc_warp_fwd_kernel: (out, P) [B][C][H][W]."""
    B, C, H, W = x.shape
    s = sample(ix, iy, H, W, dtype, mut)
    xg = x.to(dtype).reshape(B, C, -1)
    v, P = torch.zeros_like(xg), torch.zeros_like(xg)
    for valid, w, off in zip(s.valid, s.w, s.off):
        t, ok, wt = _gather(xg, off), valid.reshape(B, 1, -1), w.reshape(B, 1, -1)
        v = torch.where(ok, _fma(t, wt.expand_as(t), v), v)      # `v += a * s.nw`, contracted
        P = torch.where(ok, P + t.abs() * wt, P)
    m = _active(s, thr, mut).to(dtype).reshape(B, 1, -1)
    return (v * m).reshape(B, C, H, W), (P * m).reshape(B, C, H, W)


def fix_shift(gout):
    m = float(gout.abs().max())
    return FIX_BITS - (math.frexp(m)[1] - 1) if m > 0 else FIX_BITS


def fix_unit(gout):
    return 2.0 ** -fix_shift(gout)


def _scatter(B, C, n, offs, addends, dtype, shift):
    """sum of the addends [B][C][pixels] at offs [B][pixels]: in `dtype`, or (shift given) rounded once to 2^-shift,
    summed as integers and converted once (fix_quantize / fix_to_float)."""
    acc = torch.zeros(B, C, n, dtype=torch.int64 if shift is not None else dtype)
    for off, a in zip(offs, addends):
        if shift is not None:
            a = (a.double() * 2.0 ** shift).round().long()
        acc.scatter_add_(2, off.reshape(B, 1, -1).expand(B, C, -1), a)
    if shift is not None:
        acc = (acc.double() * 2.0 ** -shift).float()
    return acc


def _fma(a, b, c):
    """fmaf(a, b, c) of fp32 tensors: the product is exact in float64, the sum is rounded there once before the rounding
    to fp32 (a double rounding that moves the result in about 2^-29 of the cases, and then by one ulp); float64: a b + c."""
    if c.dtype == F32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


# the taps' signs and weights in d out / d ix and d out / d iy (warp_scatter): (minus, weight's name)
_GIX = ((True, "ey"), (False, "ey"), (True, "wy1"), (False, "wy1"))
_GIY = ((True, "ex"), (True, "wx1"), (False, "ex"), (False, "wx1"))


def warp_bwd(x, ix, iy, gout, thr, scale, dtype=F64, fixed=False, spy_ok=None, mut=None, geom=None):
    """The backward of warp_fwd: (grad_x [B][C][H][W], grad_flo [B][2][H][W], bounds) with bounds = S, k, P (float64
    references only).  scale = (fs, fs) for PWC-Net, (sx, sy) with spy_ok = (okx, oky) for SpyNet.  The flow gradient
    is summed as the kernels do: per channel group in channel order, flow_grad, the groups in index order, the scale."""
    B, C, H, W = x.shape
    plane, spy = H * W, spy_ok is not None
    G = channel_groups(plane, C)
    s = sample(ix, iy, H, W, dtype, mut)
    act = _active(s, thr, mut).reshape(B, 1, -1)
    xg, g = x.to(dtype).reshape(B, C, -1), gout.to(dtype).reshape(B, C, -1)
    if mut == "drop_tail" and geom is not None and geom.tail.any():
        g = g.clone()
        g[:, C - 1] = 0
    zero = torch.zeros((), dtype=dtype)
    puts = [v.reshape(B, 1, -1) & act for v in s.valid]
    if mut == "drop_lx31" and geom is not None:
        lx = (s.x0 - geom.wx0).reshape(B, 1, -1)
        puts = [p & ~((lx + dx) == WWIN - 1) for p, dx in zip(puts, (0, 1, 0, 1))]
    adds = [torch.where(p, w.reshape(B, 1, -1) * g, zero) for p, w in zip(puts, s.w)]
    shift = fix_shift(gout) if fixed else None
    gx = _scatter(B, C, plane, s.off, adds, dtype, shift).reshape(B, C, H, W)
    vals = [_gather(xg, off) for off in s.off]
    parts = [[], []]
    for grp in range(G):
        gi = [torch.zeros(B, plane, dtype=dtype), torch.zeros(B, plane, dtype=dtype)]
        for c in range(grp, C, G):
            for t in range(4):
                ok = puts[t][:, 0] if mut != "drop_lx31" else (s.valid[t].reshape(B, -1) & act[:, 0])
                for axis, table in enumerate((_GIX, _GIY)):
                    minus, wname = table[t]
                    tv = vals[t][:, c] * getattr(s, wname).reshape(B, -1)
                    gi[axis] = torch.where(ok, _fma(-tv if minus else tv, g[:, c], gi[axis]), gi[axis])     # tap_fma
        for axis, size in enumerate((W, H)):
            if spy:
                keep = spy_ok[axis].reshape(B, -1) if mut != "spy_no_clamp_mask" else torch.ones(B, plane, dtype=torch.bool)
                parts[axis].append(torch.where(keep, 0.5 * size * gi[axis], zero))
            else:
                parts[axis].append(2.0 * ((0.5 * size * gi[axis]) / float(max(size - 1, 1))))
    gf = []
    for axis in range(2):
        tot = parts[axis][0]
        for p in parts[axis][1:]:
            tot = tot + p
        gf.append(tot * torch.tensor(scale[axis], dtype=F32).to(dtype))
    gf = torch.stack(gf, 1).reshape(B, 2, H, W)
    if dtype != F64:
        return gx, gf, None
    S = _scatter(B, C, plane, s.off, [a.abs() for a in adds], F64, None).reshape(B, C, H, W)
    k = _scatter(B, 1, plane, s.off, [p.to(F64) for p in puts], F64, None).reshape(B, 1, H, W)
    P = []
    for axis, (table, size) in enumerate(((_GIX, W), (_GIY, H))):
        acc = torch.zeros(B, plane, dtype=F64)
        for t in range(4):
            wt = getattr(s, table[t][1]).reshape(B, 1, -1)
            acc = acc + torch.where(puts[t], (vals[t] * wt * g).abs(), zero).sum(1)
        if spy:
            acc = acc * spy_ok[axis].reshape(B, -1).to(F64) * abs(scale[axis]) * 0.5 * size
        else:
            acc = acc * abs(f32(scale[axis])) * size / max(size - 1, 1)
        P.append(acc)
    return gx, gf, types.SimpleNamespace(S=S, k=k, P=torch.stack(P, 1).reshape(B, 2, H, W))


# --------------------------------------------------------------------------- Resample2d (resample2d_kernel.cu restated)
def rs_taps(xf, yf, h, w, dtype):
    """rs_taps: neighbours clamped one by one against (h, w), floor fractions."""
    xf, yf = xf.to(dtype), yf.to(dtype)
    fx, fy = xf.floor(), yf.floor()
    return (_long(fx).clamp(0, w - 1), _long(fx + 1).clamp(0, w - 1), _long(fy).clamp(0, h - 1), _long(fy + 1).clamp(0, h - 1),
            xf - fx, yf - fy)


def rs_bad(xf, yf):
    """Pixels whose position is not finite: their weights are NaN, the references give them no contribution."""
    return ~(torch.isfinite(xf) & torch.isfinite(yf))


def rs_fwd(in1, xf, yf, dtype=F64):
    """resample2d_fwd_kernel (bilinear): neighbours clamped against the OUTPUT size; (out, P) [B][C][H][W]."""
    B, C, iH, iW = in1.shape
    H, W = xf.shape[-2:]
    xL, xR, yT, yB, a, b = rs_taps(xf, yf, H, W, dtype)
    a, b = a.double().reshape(B, 1, -1), b.double().reshape(B, 1, -1)       # the kernel forms the weights in double
    img = in1.reshape(B, C, -1)
    v, P = torch.zeros(B, C, H * W, dtype=dtype), torch.zeros(B, C, H * W, dtype=F64)
    for yy, xx, wt in ((yT, xL, (1 - a) * (1 - b)), (yT, xR, a * (1 - b)), (yB, xL, (1 - a) * b), (yB, xR, a * b)):
        t = _gather(img, yy * iW + xx).double()
        v = v + (wt * t).to(dtype)                                            # each term rounded before it is added
        P = P + wt * t.abs()
    bad = rs_bad(xf, yf).reshape(B, 1, -1)                                    # (non-finite positions: not part of the reference)
    v, P = torch.where(bad, torch.zeros((), dtype=dtype), v), torch.where(bad, torch.zeros((), dtype=F64), P)
    return v.reshape(B, C, H, W), P.reshape(B, C, H, W)


def rs_bwd(in1, xf, yf, gout, dtype=F64, fixed=False, mut=None):
    """resample2d_bwd_pixel: grad_in1 [B][C][iH][iW] (neighbours clamped against the input size, truncation weights
    xf - (int)xf: negative for negative xf), grad_flow [B][2][H][W] (neighbours clamped against the flow size, floor
    fractions, the eight-term chains); bounds S, k, P, A for the float64 reference."""
    B, C, iH, iW = in1.shape
    H, W = xf.shape[-2:]
    xL, xR, yT, yB, _, _ = rs_taps(xf, yf, *((H, W) if mut == "rs_clamp_flow_size" else (iH, iW)), dtype)
    xd, yd = xf.to(dtype), yf.to(dtype)
    a1, b1 = (xd - (xd.floor() if mut == "rs_floor_weights" else xd.trunc())), (yd - (yd.floor() if mut == "rs_floor_weights" else yd.trunc()))
    a1, b1 = a1.reshape(B, 1, -1), b1.reshape(B, 1, -1)
    g = gout.to(dtype).reshape(B, C, -1)
    bad = rs_bad(xf, yf).reshape(B, 1, -1)
    zero = torch.zeros((), dtype=dtype)
    offs = [yT * iW + xL, yT * iW + xR, yB * iW + xL, yB * iW + xR]
    adds = [(1 - a1) * (1 - b1) * g, a1 * (1 - b1) * g, (1 - a1) * b1 * g, a1 * b1 * g]
    adds = [torch.where(bad, zero, a) for a in adds]
    g1 = _scatter(B, C, iH * iW, offs, adds, dtype, fix_shift(gout) if fixed else None).reshape(B, C, iH, iW)
    xL, xR, yT, yB, alpha, beta = rs_taps(xf, yf, H, W, dtype)
    img = in1.to(dtype).reshape(B, C, -1)
    iTL, iTR = _gather(img, yT * iW + xL), _gather(img, yT * iW + xR)
    iBL, iBR = _gather(img, yB * iW + xL), _gather(img, yB * iW + xR)
    gam_x, gam_y = (torch.where(bad[:, 0], zero, (1 - t).reshape(B, -1)) for t in (alpha, beta))
    g = torch.where(bad, zero, g)
    gdx, gdy = torch.zeros(B, H * W, dtype=dtype), torch.zeros(B, H * W, dtype=dtype)
    Px, Py, A = (torch.zeros(B, H * W, dtype=F64) for _ in range(3))
    for c in range(C):
        gv = g[:, c]
        # `gdx += gam_y * gv * iTR` as the compiler contracts it: the product of the first two factors, then one fused
        # multiply-add into the chain (where both neighbours are clamped to one texel the unfused chain cancels exactly
        # and the fused one leaves a residue of u |term|: both are plain fp32)
        gdx = _fma(gam_y * gv, iTR[:, c], gdx)
        gdx = _fma(-(gam_y * gv), iTL[:, c], gdx)
        gdx = _fma((1 - gam_y) * gv, iBR[:, c], gdx)
        gdx = _fma(-((1 - gam_y) * gv), iBL[:, c], gdx)
        gdy = _fma(gam_x * gv, iBL[:, c], gdy)
        gdy = _fma(-(gam_x * gv), iTL[:, c], gdy)
        gdy = _fma((1 - gam_x) * gv, iBR[:, c], gdy)
        gdy = _fma(-((1 - gam_x) * gv), iTR[:, c], gdy)
        if dtype == F64:
            top, bot = iTR[:, c].abs() + iTL[:, c].abs(), iBR[:, c].abs() + iBL[:, c].abs()
            left, right = iBL[:, c].abs() + iTL[:, c].abs(), iBR[:, c].abs() + iTR[:, c].abs()
            Px = Px + gv.abs() * (gam_y * top + (1 - gam_y) * bot)
            Py = Py + gv.abs() * (gam_x * left + (1 - gam_x) * right)
            A = A + gv.abs() * (top + bot)
    gflow = torch.stack([gdx, gdy], 1).reshape(B, 2, H, W)
    if dtype != F64:
        return g1, gflow, None
    S = _scatter(B, C, iH * iW, offs, [a.abs() for a in adds], F64, None).reshape(B, C, iH, iW)
    k = _scatter(B, 1, iH * iW, offs, [(~bad).to(F64)] * 4, F64, None).reshape(B, 1, iH, iW)
    return g1, gflow, types.SimpleNamespace(S=S, k=k, P=torch.stack([Px, Py], 1).reshape(B, 2, H, W),
                                            A=torch.stack([A, A], 1).reshape(B, 2, H, W))


# --------------------------------------------------------------------------- census
def window_geom(x0, y0, H, W, C):
    """The LDS window kernel's map of a plane (pwc_warp_bwd_det_lds_kernel): per pixel the window origin (the tile
    centre pixel's north-west tap - 15, clamped to [-1, max(size - 31, -1)]), the raw origin, and per channel whether
    it falls into a ragged G * 4 pass."""
    G = channel_groups(H * W, C)
    cy = (torch.arange(H) // WT * WT + WT // 2).clamp(max=H - 1).view(H, 1)
    cx = (torch.arange(W) // WT * WT + WT // 2).clamp(max=W - 1).view(1, W)
    raw_y, raw_x = y0[:, cy, cx] - (WWIN - WT) // 2 - WT // 2 + 1, x0[:, cy, cx] - (WWIN - WT) // 2 - WT // 2 + 1
    hi_y, hi_x = max(H - WWIN + 1, -1), max(W - WWIN + 1, -1)
    c = torch.arange(C)
    first = (c // G) // WCH * WCH * G + c % G          # the pass's first channel of this group
    tail = first + (WCH - 1) * G >= C                  # its last slot has no channel
    return types.SimpleNamespace(G=G, wy0=raw_y.clamp(-1, hi_y) if hi_y >= -1 else raw_y, wx0=raw_x.clamp(-1, hi_x),
                                 raw_y=raw_y, raw_x=raw_x, hi_y=hi_y, hi_x=hi_x, tail=tail, group=c % G)


def _axis_pattern(v0, v1, size, name):
    """Tap validity along one axis: in, lo (x0 = -1), hi (x0 = size - 1), out; size 1 has its own names."""
    if size == 1:
        return {"%s1_lo" % name: ~v0 & v1, "%s1_hi" % name: v0 & ~v1, "%s_out" % name: ~v0 & ~v1}
    return {"%s_in" % name: v0 & v1, "%s_lo" % name: ~v0 & v1, "%s_hi" % name: v0 & ~v1, "%s_out" % name: ~v0 & ~v1}


def pixel_classes(case, fs):
    """name -> bool [B][H][W] of one case at one flow scale."""
    r = ref(case, fs)
    B, C, H, W = case.shape
    out = {}
    if case.kind == "rs":
        xf, yf = r.pos
        xL, xR, yT, yB, _, _ = rs_taps(xf, yf, H, W, F64)
        out["rs/neg_x"], out["rs/neg_y"] = xf < 0, yf < 0
        out["rs/xL==xR"], out["rs/yT==yB"] = xL == xR, yT == yB
        out["rs/int_x"], out["rs/int_y"] = xf == xf.floor(), yf == yf.floor()
        if case.ishape[0] > H:
            out["rs/iH>H"] = torch.ones(B, H, W, dtype=torch.bool)
            out["rs/beyond_flow_size"] = (_long(xf.double().floor()) + 1 > W - 1) | (_long(yf.double().floor()) + 1 > H - 1)
        return out
    s = r.s
    px, py = _axis_pattern(s.vx0, s.vx1, W, "x"), _axis_pattern(s.vy0, s.vy1, H, "y")
    for nx, mx in px.items():
        for ny, my in py.items():
            if nx.endswith("out") or ny.endswith("out"):
                continue
            out["tap/%s,%s" % (nx, ny)] = mx & my
    out["tap/outside"] = px["x_out"] | py["y_out"]
    ix_int, iy_int = s.wx1 == 0, s.wy1 == 0
    out["int/x"], out["int/y"], out["int/xy"] = ix_int & ~iy_int, iy_int & ~ix_int, ix_int & iy_int
    if case.kind == "pwc":
        thr = torch.tensor(case.thr, dtype=F32).double()
        out["mask/above"], out["mask/on"], out["mask/below"] = s.msum > thr, s.msum == thr, s.msum < thr
    else:
        for name, g in (("x", r.grid[0]), ("y", r.grid[1])):
            g = g.expand(B, H, W)
            out["grid%s/in" % name], out["grid%s/lo" % name], out["grid%s/hi" % name] = (g > -1) & (g < 1), g < -1, g > 1
            out["grid%s/pm1" % name] = g.abs() == 1
    if H * W < 256:
        out["map/linear"] = torch.ones(B, H, W, dtype=torch.bool)
        return out
    out["map/window"] = torch.ones(B, H, W, dtype=torch.bool)
    gm = r.geom
    ly, lx = s.y0 - gm.wy0, s.x0 - gm.wx0
    cells = [((ly + dy >= 0) & (ly + dy < WWIN) & (lx + dx >= 0) & (lx + dx < WWIN)) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    n_in = sum(c.long() for c in cells)
    out["win/inside"], out["win/global"], out["win/straddle"] = n_in == 4, n_in == 0, (n_in > 0) & (n_in < 4)
    out["win/lx=31"] = ((lx == WWIN - 1) | (lx + 1 == WWIN - 1)) & (ly >= 0) & (ly < WWIN - 1)
    ys, xs = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    part_y, part_x = (ys // WT * WT + WT > H), (xs // WT * WT + WT > W)
    out["tile/full"] = (~part_y & ~part_x).expand(B, H, W)
    out["tile/partial_x"], out["tile/partial_y"] = (part_x & ~part_y).expand(B, H, W), (part_y & ~part_x).expand(B, H, W)
    out["tile/partial_xy"] = (part_x & part_y).expand(B, H, W)
    for name, raw, hi, size in (("y", gm.raw_y, gm.hi_y, H), ("x", gm.raw_x, gm.hi_x, W)):
        if size < WWIN:
            out["org%s/small" % name] = torch.ones(B, H, W, dtype=torch.bool)
        else:
            out["org%s/free" % name], out["org%s/lo" % name] = (raw >= -1) & (raw <= hi), raw < -1
            out["org%s/hi" % name] = raw > hi
    return out


def texel_classes(k):
    """name -> bool [B][1][h][w] from the texels' addend counts."""
    return {"k/0": k == 0, "k/1": k == 1, "k/2-4": (k >= 2) & (k <= 4), "k/5-16": (k >= 5) & (k <= 16), "k/>16": k > 16}


def channel_classes(case):
    B, C, H, W = case.shape
    gm = window_geom(torch.zeros(1, H, W, dtype=torch.long), torch.zeros(1, H, W, dtype=torch.long), H, W, C)
    out = {"chan/g%d" % g: gm.group == g for g in range(gm.G)}
    if H * W >= 256:
        out["chan/tail"] = gm.tail
    return out


def census(case, fs):
    """name -> count: pixels per class, channels per class, texels per addend count (the `one` gradient's backward)."""
    out = {n: int(m.sum()) for n, m in pixel_classes(case, fs).items()}
    if case.builder == "wild":
        out["poisoned"] = int(poisoned(case, fs)[0].sum())
    if case.kind != "rs":
        out.update({n: int(m.sum()) for n, m in channel_classes(case).items()})
        out["G"] = channel_groups(case.shape[2] * case.shape[3], case.shape[1])
    out.update({n: int(m.sum()) for n, m in texel_classes(ref_bwd(case, fs, "one").b.k).items()})
    return out


# --------------------------------------------------------------------------- flows
def _ulps(f0, n=16):
    up, dn, c = f0, f0, [f0]
    for _ in range(n):
        up, dn = torch.nextafter(up, torch.full_like(up, math.inf)), torch.nextafter(dn, torch.full_like(dn, -math.inf))
        c += [up, dn]
    return torch.stack(c)


def steer(pos, f0, target):
    """The flow within +-16 ulp of f0 whose mirrored position pos(flow) is nearest the target: (flow, exact hit)."""
    cand = _ulps(f0.float())
    d = (pos(cand).double() - target.double()).abs()
    best = d.argmin(0, keepdim=True)
    return cand.gather(0, best)[0], d.gather(0, best)[0] == 0


def _axis_fn(case, fs, axis):
    """(pos(flow) for candidate stacks [n][B][H][W], the float64 solve target -> flow) along one axis."""
    B, C, H, W = case.shape
    size = W if axis == 0 else H
    base = _base(size, "x" if axis == 0 else "y")
    if case.kind == "pwc":
        return (lambda f: pwc_axis(base, f, fs, size, False),
                lambda t: ((t + 0.5) * max(size - 1, 1) / size - base.double()) / f32(fs))
    if case.kind == "spy":
        lin = torch.linspace(-1.0, 1.0, size).view(base.shape)
        s = spy_scales(H, W)[axis]
        return (lambda f: spy_axis(lin, f, s, size, False)[0], lambda t: ((2 * t + 1) / size - 1 - lin.double()) / s)
    return (lambda f: base + f, lambda t: t - base.double())


def _steered(case, fs, targets):
    """flow [B][2][H][W] steering both axes to targets (tx, ty) [B][H][W], and the exact-hit masks."""
    fl, hits = [], []
    for axis, t in enumerate(targets):
        pos, solve = _axis_fn(case, fs, axis)
        f, hit = steer(pos, solve(t.double()).float(), t)
        fl.append(f)
        hits.append(hit)
    return torch.stack(fl, 1), hits


def _gen(case, fs, salt):
    B, C, H, W = case.shape
    return torch.Generator().manual_seed(salt * 7919 + int(fs * 1000) + 131 * H + 17 * W + C + B)


def flow_smooth(case, fs):
    B, C, H, W = case.shape
    amp = torch.tensor([min(3.0, float(W)), min(3.0, float(H))]).view(1, 2, 1, 1) / fs     # the scaled flow is the same at every fs
    coarse = amp * torch.randn(B, 2, 5, 7, generator=_gen(case, 1.0, 1))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).contiguous()


def flow_tearing(case, fs):
    B, C, H, W = case.shape
    return 40.0 * torch.randn(B, 2, H, W, generator=_gen(case, 1.0, 2)) / fs     # taps leave the window and the image


def flow_integer(case, fs):
    B, C, H, W = case.shape
    g = _gen(case, fs, 3)
    tx = torch.randint(-2, W + 2, (B, H, W), generator=g).double()
    ty = torch.randint(-2, H + 2, (B, H, W), generator=g).double()
    return _steered(case, fs, (tx, ty))[0]


QS = (2.0 ** -20, 0.25, 0.5)


def _edge_targets(size, pick, gen):
    opts = [-1.0 + q for q in QS] + [size - 1.0 - q for q in QS] + [-1.0, size - 1.0, size - 0.5, -1.0 - 2.0 ** -20]
    inner = torch.rand(pick.shape, generator=gen, dtype=F64) * max(size - 1, 0)
    return torch.where(pick < 10, torch.tensor(opts + [0.0], dtype=F64)[pick.clamp(max=10)], inner)


def flow_edges(case, fs):
    """-1 + q, size - 1 - q, -1, size - 1 (q = 2^-20, 1/4, 1/2), size - 1/2 (the last tap alone) and -1 - 2^-20 (just outside)
    along either axis, paired with each other and with positions inside."""
    B, C, H, W = case.shape
    g = _gen(case, fs, 4)
    i = torch.arange(B * H * W).reshape(B, H, W)
    i = i[:, torch.randperm(H, generator=g)][:, :, torch.randperm(W, generator=g)]
    return _steered(case, fs, (_edge_targets(W, i % 11, g), _edge_targets(H, (i // 3) % 11, g)))[0]


def flow_threshold(case, fs):
    """Positions whose weights are multiples of 1/4 and whose mask sum is the case's threshold t (1/4 or 1/2): one axis at
    -1 + t or size - 1 - t, the other on an integer inside; both axes at -1 + 1/2 (t = 1/4); a third of the pixels one
    ulp of the flow above, a third one below."""
    B, C, H, W = case.shape
    g = _gen(case, fs, 5)
    t = case.thr
    i = torch.arange(B * H * W).reshape(B, H, W)
    kind = (i // 3) % (5 if t == 0.25 else 4)
    inx = torch.randint(0, max(W - 1, 1), (B, H, W), generator=g).double()
    iny = torch.randint(0, max(H - 1, 1), (B, H, W), generator=g).double()
    tx = torch.where(kind == 0, torch.full_like(inx, -1.0 + t), torch.where(kind == 1, torch.full_like(inx, W - 1.0 - t), inx))
    ty = torch.where(kind == 2, torch.full_like(iny, -1.0 + t), torch.where(kind == 3, torch.full_like(iny, H - 1.0 - t), iny))
    tx = torch.where(kind == 4, torch.full_like(tx, -0.5), tx)
    ty = torch.where(kind == 4, torch.full_like(ty, -0.5), ty)
    flow, _ = _steered(case, fs, (tx, ty))
    side = (i % 3).unsqueeze(1).expand(B, 2, H, W)
    up = torch.nextafter(flow, torch.full_like(flow, math.inf))
    dn = torch.nextafter(flow, torch.full_like(flow, -math.inf))
    return torch.where(side == 1, up, torch.where(side == 2, dn, flow))


WILD = (math.inf, -math.inf, math.nan, 3.0e38, -3.0e38, 1.0e10, -1.0e10)


def wild_pixels(case):
    """(y, x, channel, value) of the poisoned flows: the first tile's centre pixel (it sets the window origin) and a
    handful of others, each value on either flow channel."""
    B, C, H, W = case.shape
    spots = [(min(WT // 2, H - 1), min(WT // 2, W - 1)), (0, 0), (H - 1, W - 1), (H // 2, W // 3), (H // 3, W // 2), (H - 1, 0),
             (0, W - 1), (H // 2, W - 1), (min(WT + WT // 2, H - 1), min(WT + WT // 2, W - 1)), (H // 4, W // 4), (H // 5, 2 * W // 3),
             (2 * H // 3, W // 5), (H // 2, W // 2), (1, 1)]
    return [(y, x, i % 2, WILD[i % len(WILD)]) for i, (y, x) in enumerate(spots)]


def flow_wild(case, fs):
    """smooth with +-inf, NaN, +-3e38 and +-1e10 in a handful of pixels' flows (both batches)."""
    flo = flow_smooth(case, fs).clone()
    for y, x, ch, v in wild_pixels(case):
        flo[:, ch, y, x] = v
    return flo


BUILDERS = {"smooth": flow_smooth, "wild": flow_wild, "tearing": flow_tearing, "integer": flow_integer, "edges": flow_edges,
            "threshold": flow_threshold}
RANDOM_BUILDERS = ("smooth", "tearing")


# --------------------------------------------------------------------------- the case table
def _case(kind, shape, builder, need, thr=None, ishape=None):
    B, C, H, W = shape
    thr = (THR if kind == "pwc" else -1.0) if thr is None else thr
    name = "%s-%s-%s" % (kind, "x".join(map(str, shape)), builder) + ("%g" % thr if builder == "threshold" else "") + \
        ("-in%dx%d" % ishape if ishape else "")
    return types.SimpleNamespace(kind=kind, shape=shape, builder=builder, thr=thr, need=need, name=name,
                                 ishape=ishape or (H, W), fs=FS if kind == "pwc" else (1.0,))


def _table():
    t = []
    lin = {"map/linear": 1}
    # linear kernel, G = 1, C below the 4-channel pass
    t.append(_case("pwc", (1, 5, 7, 9), "smooth", dict(lin, **{"tap/x_in,y_in": 20, "mask/above": 30, "chan/g0": 5, "k/2-4": 10})))
    t.append(_case("pwc", (1, 5, 7, 9), "integer", dict(lin, **{"int/xy": 10, "int/x": 5, "int/y": 5, "tap/outside": 3, "mask/below": 3})))
    t.append(_case("pwc", (1, 5, 7, 9), "edges", dict(lin, **{"tap/x_lo,y_in": 2, "tap/x_hi,y_in": 1, "tap/x_in,y_lo": 2, "tap/x_in,y_hi": 2,
                                                             "tap/x_lo,y_lo": 1, "tap/x_lo,y_hi": 1, "tap/x_hi,y_lo": 1})))
    # plane = 255: the largest linear plane; G = 2, batch 2
    t.append(_case("pwc", (2, 9, 15, 17), "tearing", dict(lin, **{"tap/outside": 100, "mask/below": 100, "chan/g1": 4, "G": 2, "k/1": 10})))
    t.append(_case("pwc", (2, 9, 15, 17), "integer", dict(lin, **{"int/xy": 100, "G": 2})))
    t.append(_case("pwc", (2, 9, 15, 17), "threshold", dict(lin, **{"mask/on": 25, "mask/above": 40, "mask/below": 40}), thr=0.25))
    # plane = 360: window kernel, G = 2, ragged pass tail, partial tiles both ways, H, W < 32
    win = {"map/window": 1}
    small = dict(win, **{"orgx/small": 1, "orgy/small": 1, "G": 2, "chan/tail": 3, "tile/full": 256, "tile/partial_x": 64,
                         "tile/partial_y": 32, "tile/partial_xy": 8})
    t.append(_case("pwc", (2, 11, 18, 20), "smooth", dict(small, **{"win/inside": 500, "k/2-4": 100})))
    t.append(_case("pwc", (2, 11, 18, 20), "tearing", dict(small, **{"tap/outside": 300, "k/1": 10})))
    t.append(_case("pwc", (2, 11, 18, 20), "integer", dict(small, **{"int/xy": 300, "int/x": 50, "int/y": 50, "win/straddle": 20})))
    t.append(_case("pwc", (2, 11, 18, 20), "edges", dict(small, **{"tap/x_lo,y_in": 8, "tap/x_hi,y_in": 8, "tap/x_in,y_lo": 8, "tap/x_in,y_hi": 8,
                                                                  "tap/x_lo,y_lo": 4, "tap/x_hi,y_hi": 4, "tap/x_lo,y_hi": 4, "tap/x_hi,y_lo": 4,
                                                                  "k/>16": 1})))
    t.append(_case("pwc", (2, 11, 18, 20), "threshold", dict(small, **{"mask/on": 36, "mask/above": 60, "mask/below": 60}), thr=0.5))
    # window origin clamped high and low, free; the four partial-tile kinds
    org = dict(win, **{"tile/full": 512, "tile/partial_x": 100, "tile/partial_y": 60, "tile/partial_xy": 6})
    t.append(_case("pwc", (1, 3, 50, 35), "smooth", dict(org, **{"orgy/free": 256, "orgy/lo": 256, "orgy/hi": 100, "orgx/lo": 256, "orgx/hi": 256,
                                                                 "win/inside": 1000})))
    t.append(_case("pwc", (1, 3, 50, 35), "tearing", dict(org, **{"win/global": 100, "win/straddle": 10, "win/inside": 100, "orgy/free": 100})))
    t.append(_case("pwc", (1, 3, 50, 35), "edges", dict(org, **{"tap/x_lo,y_lo": 4, "tap/x_hi,y_hi": 4, "win/global": 100, "k/>16": 1})))
    t.append(_case("pwc", (1, 3, 50, 35), "integer", dict(org, **{"int/xy": 500, "win/lx=31": 1})))
    # G = 4
    g4 = dict(win, **{"G": 4, "chan/g3": 4, "tile/full": 2048, "tile/partial_x": 256, "tile/partial_y": 512, "tile/partial_xy": 64})
    t.append(_case("pwc", (1, 16, 40, 72), "smooth", dict(g4, **{"orgx/free": 1000, "orgx/lo": 256, "orgx/hi": 256, "win/inside": 2500})))
    t.append(_case("pwc", (1, 16, 40, 72), "tearing", dict(g4, **{"win/global": 500, "win/straddle": 10, "tap/outside": 500})))
    t.append(_case("pwc", (1, 16, 40, 72), "threshold", dict(g4, **{"mask/on": 144, "mask/above": 300, "mask/below": 300}), thr=0.25))
    # size - 1 = 0 on both kernel maps
    t.append(_case("pwc", (1, 4, 1, 300), "smooth", dict(win, **{"tap/x_in,y1_lo": 50, "tap/x_in,y1_hi": 50, "orgy/small": 1})))
    t.append(_case("pwc", (1, 4, 1, 300), "integer", dict(win, **{"int/xy": 50, "tap/x_in,y1_hi": 30, "tap/outside": 30})))
    t.append(_case("pwc", (1, 4, 300, 1), "smooth", dict(win, **{"tap/x1_lo,y_in": 50, "tap/x1_hi,y_in": 50, "orgx/small": 1})))
    t.append(_case("pwc", (1, 4, 300, 1), "edges", dict(win, **{"tap/x1_lo,y_lo": 1, "tap/x1_hi,y_hi": 1, "tap/outside": 1})))
    t.append(_case("pwc", (1, 2, 1, 9), "smooth", dict(lin, **{"tap/x_in,y1_lo": 1, "tap/x_in,y1_hi": 1})))
    t.append(_case("pwc", (1, 2, 1, 9), "edges", dict(lin, **{"tap/outside": 1})))
    t.append(_case("pwc", (1, 2, 6, 1), "smooth", dict(lin, **{"tap/x1_lo,y_in": 1})))
    t.append(_case("pwc", (1, 2, 6, 1), "integer", dict(lin, **{"int/xy": 1, "tap/x1_hi,y_in": 1})))
    # SpyNet: the clamp
    t.append(_case("spy", (1, 5, 7, 9), "smooth", dict(lin, **{"gridx/in": 20, "gridx/lo": 1, "gridx/hi": 1, "gridy/lo": 1, "gridy/hi": 1})))
    t.append(_case("spy", (1, 5, 7, 9), "edges", dict(lin, **{"gridx/pm1": 2, "gridy/pm1": 2, "tap/x_lo,y_in": 2, "tap/x_hi,y_in": 1})))
    t.append(_case("spy", (2, 11, 18, 20), "tearing", dict(small, **{"gridx/lo": 100, "gridx/hi": 100, "gridy/lo": 100, "gridy/hi": 100,
                                                                    "gridx/in": 100, "k/>16": 4})))
    t.append(_case("spy", (2, 11, 18, 20), "integer", dict(small, **{"int/xy": 100, "gridx/in": 300})))
    t.append(_case("spy", (2, 11, 18, 20), "edges", dict(small, **{"gridx/pm1": 20, "gridy/pm1": 20, "tap/x_lo,y_lo": 4, "tap/x_hi,y_hi": 4})))
    t.append(_case("spy", (1, 3, 50, 35), "smooth", dict(org, **{"win/inside": 1000, "gridx/in": 1000, "orgy/free": 256})))
    t.append(_case("spy", (1, 3, 50, 35), "tearing", dict(org, **{"win/global": 100, "win/straddle": 10, "gridx/hi": 300})))
    t.append(_case("spy", (1, 16, 40, 72), "smooth", dict(g4, **{"win/inside": 2500, "gridy/in": 2000})))
    t.append(_case("spy", (1, 16, 40, 72), "tearing", dict(g4, **{"win/global": 300, "gridy/lo": 300})))
    # (size - 1) / 2 a power of two on both axes: the flow's division by it (the network on the CPU) and the product with
    # its fp32 reciprocal (ATen on the GPU, the kernels, the mirror) are the same operation
    t.append(_case("spy", (1, 5, 9, 17), "smooth", dict(lin, **{"gridx/in": 50, "gridy/in": 50})))
    t.append(_case("spy", (1, 5, 9, 17), "tearing", dict(lin, **{"gridx/lo": 10, "gridx/hi": 10, "gridy/lo": 10, "gridy/hi": 10})))
    t.append(_case("spy", (1, 3, 33, 17), "smooth", dict(win, **{"win/inside": 300, "tile/partial_xy": 1})))
    t.append(_case("spy", (1, 3, 33, 17), "tearing", dict(win, **{"gridx/lo": 50, "gridx/hi": 50, "gridy/lo": 50, "gridy/hi": 50})))
    # Resample2d
    rs = {"rs/neg_x": 1, "rs/neg_y": 1, "rs/xL==xR": 1, "rs/yT==yB": 1}
    t.append(_case("rs", (2, 3, 13, 27), "smooth", dict(rs, **{"k/2-4": 100})))
    t.append(_case("rs", (2, 3, 13, 27), "tearing", {"rs/neg_x": 100, "rs/neg_y": 100, "rs/xL==xR": 100, "rs/yT==yB": 100, "k/>16": 4}))
    t.append(_case("rs", (2, 3, 13, 27), "integer", {"rs/int_x": 300, "rs/int_y": 300, "rs/neg_x": 20, "rs/neg_y": 20, "rs/xL==xR": 20}))
    t.append(_case("rs", (1, 3, 33, 40), "smooth", dict(rs, **{"k/2-4": 300})))
    t.append(_case("rs", (1, 3, 33, 40), "tearing", {"rs/neg_x": 200, "rs/neg_y": 200, "k/>16": 4}))
    t.append(_case("rs", (1, 3, 13, 27), "tearing", {"rs/iH>H": 1, "rs/beyond_flow_size": 50, "rs/neg_x": 50}, ishape=(20, 31)))
    t.append(_case("rs", (1, 3, 13, 27), "integer", {"rs/iH>H": 1, "rs/beyond_flow_size": 20, "rs/int_x": 100}, ishape=(20, 31)))
    # out-of-range and non-finite flows on both kernel maps: every address stays in range (tap_index), the pixels whose
    # position is finite and the texels no other pixel reaches are gated like any other
    t.append(_case("pwc", (2, 9, 15, 17), "wild", dict(lin, **{"poisoned": 10})))
    t.append(_case("pwc", (2, 11, 18, 20), "wild", dict(small, **{"poisoned": 10})))
    t.append(_case("pwc", (1, 16, 40, 72), "wild", dict(g4, **{"poisoned": 10})))
    t.append(_case("spy", (1, 5, 7, 9), "wild", dict(lin, **{"poisoned": 1})))
    t.append(_case("spy", (1, 16, 40, 72), "wild", dict(g4, **{"poisoned": 2})))
    t.append(_case("rs", (2, 3, 13, 27), "wild", {"poisoned": 6}))
    t.append(_case("rs", (1, 3, 13, 27), "wild", {"poisoned": 3, "rs/iH>H": 1}, ishape=(20, 31)))
    return t


TABLE = _table()
CASES = {c.name: c for c in TABLE}
GOUTS = ("one", "tiny", "huge", "spike", "zero")


def cases(kind=None, window=None, random=None):
    out = [c for c in TABLE if kind is None or c.kind == kind]
    if window is not None:
        out = [c for c in out if (c.shape[2] * c.shape[3] >= 256) == window]
    if random is not None:
        out = [c for c in out if (c.builder in RANDOM_BUILDERS) == random]
    return out


# --------------------------------------------------------------------------- inputs and references, computed once
def _band(case, flo, fs):
    """Pixels whose float64 mask sum is within 2^-20 (relative) of the threshold although the fp32 sum is not exact."""
    B, C, H, W = case.shape
    ix, iy = pwc_positions(flo, fs, case.builder != "wild")
    m64, m32 = sample(ix, iy, H, W, F64).msum, sample(ix, iy, H, W, F32).msum
    t = torch.tensor(case.thr, dtype=F32).double()
    return ((m64 - t).abs() <= BAND * t) & (m32.double() != m64)


@functools.lru_cache(maxsize=None)
def _inputs(name, fs):
    case = CASES[name]
    B, C, H, W = case.shape
    iH, iW = case.ishape
    x = torch.randn(B, C, iH, iW, generator=_gen(case, fs, 11))
    flo = BUILDERS[case.builder](case, fs).float().contiguous()
    if case.kind == "pwc":
        for _ in range(6):
            band = _band(case, flo, fs)
            if not bool(band.any()):
                break
            flo = torch.where(band.unsqueeze(1), flo + 2.0 ** -10, flo)     # nudge and re-check
        assert not bool(_band(case, flo, fs).any()), "a mask sum within 2^-20 of the threshold"
    return x, flo


def inputs(case, fs=1.0):
    return _inputs(case.name, fs)


def spy_args(case):
    B, C, H, W = case.shape
    return (torch.linspace(-1.0, 1.0, W), torch.linspace(-1.0, 1.0, H)) + spy_scales(H, W)


@functools.lru_cache(maxsize=None)
def _ref(name, fs):
    case = CASES[name]
    B, C, H, W = case.shape
    x, flo = inputs(case, fs)
    r = types.SimpleNamespace(x=x, flo=flo, spy_ok=None, scale=(fs, fs))
    if case.kind == "rs":
        r.pos = rs_positions(flo)
        r.out, r.P = rs_fwd(x, *r.pos)
        r.emu = rs_fwd(x, *r.pos, dtype=F32)[0]
        return r
    if case.kind == "pwc":
        r.pos = pwc_positions(flo, fs, case.builder != "wild")
    else:
        hor, ver, sx, sy = spy_args(case)
        ix, iy, gx, gy = spy_positions(flo, hor, ver, sx, sy, case.builder != "wild")
        r.pos, r.grid, r.scale = (ix, iy), (gx, gy), (sx, sy)
        r.spy_ok = ((gx >= -1) & (gx <= 1), (gy >= -1) & (gy <= 1))
    r.s = sample(*r.pos, H, W)
    r.geom = window_geom(r.s.x0, r.s.y0, H, W, C)
    r.out, r.P = warp_fwd(x, *r.pos, case.thr)
    r.emu = warp_fwd(x, *r.pos, case.thr, dtype=F32)[0]
    return r


def ref(case, fs=1.0):
    return _ref(case.name, fs)


@functools.lru_cache(maxsize=None)
def _gout(name, variant):
    case = CASES[name]
    B, C, H, W = case.shape
    g = torch.randn(B, C, H, W, generator=_gen(case, 0.0, 12))
    if variant == "tiny":
        g = g * 1e-9
    elif variant == "huge":
        g = g * 1e9
    elif variant == "spike":      # one element 2^30 times the rest: most addends fall below the call's unit
        g.view(-1)[g.numel() // 2] = 2.0 ** 30
    elif variant == "zero":
        g = torch.zeros_like(g)
    return g


def gout(case, variant="one"):
    return _gout(case.name, variant)


def fp32_bwd(case, fs, variant, fixed, mut=None):
    """The plain fp32 backward of one case: (grad_x, grad_flo)."""
    r = ref(case, fs)
    if case.kind == "rs":
        return rs_bwd(r.x, *r.pos, gout(case, variant), F32, fixed, mut)[:2]
    return warp_bwd(r.x, *r.pos, gout(case, variant), case.thr, r.scale, F32, fixed, r.spy_ok, mut, r.geom)[:2]


def fp32_fwd(case, fs, mut=None):
    r = ref(case, fs)
    return rs_fwd(r.x, *r.pos, dtype=F32)[0] if case.kind == "rs" else warp_fwd(r.x, *r.pos, case.thr, F32, mut)[0]


@functools.lru_cache(maxsize=None)
def _ref_bwd(name, fs, variant):
    case = CASES[name]
    r = ref(case, fs)
    g = gout(case, variant)
    if case.kind == "rs":
        gx, gf, b = rs_bwd(r.x, *r.pos, g)
    else:
        gx, gf, b = warp_bwd(r.x, *r.pos, g, case.thr, r.scale, F64, False, r.spy_ok)
    return types.SimpleNamespace(gx=gx, gf=gf, b=b, unit=fix_unit(g),
                                 emu={fixed: fp32_bwd(case, fs, variant, fixed) for fixed in (True, False)})


def ref_bwd(case, fs=1.0, variant="one"):
    return _ref_bwd(case.name, fs, variant)


# --------------------------------------------------------------------------- gates
def _none(H, W, m):
    return {}


def poisoned(case, fs=1.0):
    """(pixels [B][H][W], texels [B][1][iH][iW]) that a poisoned flow decides: what they hold is recorded, not asserted.
    PWC-Net: a flow that is not finite or beyond 1e9 leaves every tap outside the image (tap_index) -- no texel.  SpyNet:
    the clamp brings every value but NaN back to the border, a legitimate position; NaN leaves every tap outside.
    Resample2d: a finite position is clamped to a legitimate one; a non-finite one has NaN weights on the clamped texels."""
    r = ref(case, fs)
    B, C, H, W = case.shape
    iH, iW = case.ishape
    tex = torch.zeros(B, 1, iH * iW, dtype=torch.bool)
    if case.kind == "pwc":
        pix = ~(torch.isfinite(r.flo).all(1) & (r.flo.abs() < 1.0e9).all(1))
    elif case.kind == "spy":
        pix = torch.isnan(r.flo).any(1)
    else:
        pix = rs_bad(*r.pos)
        xL, xR, yT, yB, _, _ = rs_taps(*r.pos, iH, iW, F64)
        for off in (yT * iW + xL, yT * iW + xR, yB * iW + xL, yB * iW + xR):
            tex.scatter_reduce_(2, off.reshape(B, 1, -1), pix.reshape(B, 1, -1), "amax")
    return pix, tex.reshape(B, 1, iH, iW)


def _same_bits(record, prefix, got, emu):
    """Recorded, not asserted: the share of elements whose bits are those of the fp32 implementation on the CPU."""
    record(prefix + "bits_of_fp32_model", "%.4f" % float((got.contiguous().view(torch.int32) == emu.contiguous().view(torch.int32)).double().mean()))


def _leave_out(got, emu, mask):
    return torch.where(mask.expand_as(got), emu.to(got.dtype), got)


def _pixel_groups(case, fs, C):
    B = case.shape[0]
    out = {n: m.unsqueeze(1).expand(B, C, *m.shape[1:]) for n, m in pixel_classes(case, fs).items() if n not in ("map/linear", "map/window")}
    return out


def check_fwd(case, fs, got, record, prefix="fwd_"):
    """The forward of one case against float64: (elementwise ratio, statistical ratio)."""
    r = ref(case, fs)
    n = N_RS_FWD if case.kind == "rs" else N_FWD
    extra = _pixel_groups(case, fs, case.shape[1])
    if case.kind != "rs":
        B, C, H, W = case.shape
        extra.update({nm: m.view(1, C, 1, 1).expand(B, C, H, W) for nm, m in channel_classes(case).items()})
    if case.builder == "wild":
        got = _leave_out(got, r.emu, poisoned(case, fs)[0].unsqueeze(1))
    _same_bits(record, prefix, got, r.emu)
    return _gates(got, r.out, r.P, n, r.emu, 0, record, prefix, regions=_none, extra=extra)


def bound_gx(b, unit, fixed):
    if fixed:
        return 2 * gamma(N_FIX + 2) * b.S + b.k * unit / 2 + (N_FIX + 2) * TINY
    n = b.k + N_ATOMIC + 2
    return 2 * gamma(n) * b.S + n * TINY


def bound_fwd(P, n=N_FWD):
    return 2 * gamma(n + 2) * P + (n + 2) * TINY


def bound_gflo(b, C, H, W, kind):
    if kind == "rs":
        n = n_rs_gflow(C)
        return 2 * gamma(n + 2) * b.P + U * b.A + (n + 2) * TINY
    n = n_gflo(C, channel_groups(H * W, C), kind == "spy")
    return 2 * gamma(n + 2) * b.P + (n + 2) * TINY


def bound_gf(case, b):
    B, C, H, W = case.shape
    return bound_gflo(b, C, H, W, case.kind)


def spynet_reference(x, flo, hor, ver, gout):
    """SpyNet's warp of any fp32 inputs in float64 from the mirrored positions, with the elementwise bounds of its three
    results: ((out, bound), (grad_x, bound of the fixed-point scatter), (grad_flo, bound))."""
    B, C, H, W = x.shape
    sx, sy = spy_scales(H, W)
    ix, iy, gx, gy = spy_positions(flo, hor, ver, sx, sy)
    ok = ((gx >= -1) & (gx <= 1), (gy >= -1) & (gy <= 1))
    out, P = warp_fwd(x, ix, iy, -1.0)
    g1, g2, b = warp_bwd(x, ix, iy, gout, -1.0, (sx, sy), spy_ok=ok)
    return (out, bound_fwd(P)), (g1, bound_gx(b, fix_unit(gout), True)), (g2, bound_gflo(b, C, H, W, "spy"))


def resample2d_reference(x, flow, gout):
    """Resample2d's backward of any fp32 inputs in float64 (input of the flow's size): ((grad_in1, bound of the
    fixed-point scatter), (grad_flow, bound))."""
    B, C, H, W = x.shape
    g1, g2, b = rs_bwd(x, *rs_positions(flow), gout)
    return (g1, bound_gx(b, fix_unit(gout), True)), (g2, bound_gflo(b, C, H, W, "rs"))


def check_bwd(case, fs, variant, got_gx, got_gf, fixed, record, prefix="bwd_"):
    """Both gradients of one case against float64: ((elem, stat) of grad_x, (elem, stat) of grad_flo)."""
    r = ref_bwd(case, fs, variant)
    B, C, H, W = case.shape
    iH, iW = case.ishape
    emu_gx, emu_gf = r.emu[fixed]
    if case.builder == "wild":
        pix, tex = poisoned(case, fs)
        got_gx, got_gf = _leave_out(got_gx, emu_gx, tex), _leave_out(got_gf, emu_gf, pix.unsqueeze(1))
    _same_bits(record, prefix + "gx_", got_gx, emu_gx)
    _same_bits(record, prefix + "gf_", got_gf, emu_gf)
    if variant == "zero":
        assert bool((got_gx == 0).all()) and bool((got_gf == 0).all()), "zero grad_out must give exact zeros"
    ex = {n: m.expand(B, C, iH, iW) for n, m in texel_classes(r.b.k).items()}
    if case.kind != "rs":
        ex.update({nm: m.view(1, C, 1, 1).expand(B, C, H, W) for nm, m in channel_classes(case).items()})
    a = _gates(got_gx, r.gx, None, 0, emu_gx, 0, record, prefix + "gx_", regions=_none, bound=bound_gx(r.b, r.unit, fixed), extra=ex)
    b = _gates(got_gf, r.gf, None, 0, emu_gf, 0, record, prefix + "gf_", regions=_none, bound=bound_gf(case, r.b),
               extra=_pixel_groups(case, fs, 2))
    return a, b
