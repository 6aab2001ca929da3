"""The PWC-Net and FlowNetC cost volumes and ChannelNorm for the float64 tests (csrc/spatial_corr.hip: pcfa_spatial_corr_fwd /
_bwd, pcfa_cost_volume9_fwd / _bwd; csrc/flownet_ops.hip: pcfa_flownet_corr_fwd / _bwd, pcfa_channelnorm_fwd / _bwd): mirrors
of the host's dispatch plans, the float64 references, the kernels' own arithmetic on the CPU (`emu`), the bounds, the seeded
inputs, the case tables and the gates of tests/test_costvol_f64_gpu.py and tests/test_costvol_host_cpu.py.  No GPU, no ctypes.

Plans.  scorr_plan restates plan_fwd (label t<TH>x<TW>_ns<slices>_r<rounds>), scorr_bwd_plan the backward's launch geometry,
sc_is_fast the fast-path predicate of the entry points, fcorr_plan fc_make_params / fc_is_flownetc and the fast kernels' tiling.

References (float64, plain torch, shift-and-multiply over the displacement grid, from the formulas in the two files' headers).
  sampler   out[b][ph][pw][h][w] = sum_{c,i,j} in1[b][c][u + i dilH][v + j dilW] in2[b][c][u + i dilH + sU][v + j dilW + sV],
            u = h dH - padH, v = w dW - padW, sU = (ph - (patchH - 1) / 2) dil_patchH, sV likewise; a term with either
            operand outside the image is dropped (both images are zero-padded, so it is a product with 0).  Its gradients are
            the same loops as scatters: gin1[.., y1, x1] += g in2[.., y2, x2], gin2[.., y2, x2] += g in1[.., y1, x1].
  fused     out = leaky(scale corr); backward: the sampler's gradients of g scale m, m = fwd_out > 0 ? 1 : slope, from the
            fwd_out tensor the call is GIVEN (+0, -0 and negative values take the slope).
  FlowNet   out[b][tj D + ti][y][x] = 1 / (k k C) sum_{c, |j|,|i| <= (k-1)/2} in1[c][y1 + j][x1 + i] in2[c][y2 + j][x2 + i],
            y1 = y s1 + md - pad, y2 = y1 + (tj - md / s2) s2 (0 outside the image), D = 2 (md / s2) + 1; gradients (s1 = 1) as
            scatters of the same terms.
  ChannelNorm  out = sqrt(sum_c x^2); backward gin = dy x / (norm + 1e-9), norm the tensor the call is given.

Emulation (fp32, the kernel's order; products rounded, then added -- the kernels may contract to FMAs, which only errs less).
  sampler fast forward   channel c of a round goes to slice (c - c0) mod ns; a slice adds its channels in order, the rounds
                         follow in order in the same accumulator; the slices are added in slice order; then scale, then
                         LeakyReLU.
  sampler fast backward  taps t = fl(fl(g gscale) slope?) first; gin1 adds its 81 taps in (ey, ex) order; gin2 adds plane
                         80 - e at tap e (the same order seen from the other image).
  sampler generic        forward c, i, j; backward ph, pw, i, j.
  FlowNet fast           forward channels in order, then / C; backward 441 taps in (tj, ti) order, then / C.
  FlowNet generic        forward j, i, c, then / (k k C); backward displacement, then output row and column ascending.
  ChannelNorm            channels in order, sqrt; fl(g x) in fp32, the division in double, rounded to fp32.

Bounds (u = 2^-24, gamma(m) = m u / (1 - m u), TINY = 2^-126).  A sum of n products accumulated in fp32 in ANY order: every
product passes through at most n roundings (its own and at most n - 1 additions; the sliced forward's depth, C / ns + ns, is
below that), so |fl(sum) - sum| <= gamma(n) sum |a||b| (Higham 3.1, 4.2); an FMA drops a rounding.  k further roundings (the
scale, the slope, the / C) multiply by (1 + d)^k: gamma(n + k).  LeakyReLU with |slope| <= 1 is a contraction (|l(a) - l(b)|
<= |a - b|), so the forward's bound is that of scale corr whatever the sign; an operation whose result falls below the normal
range may be flushed: TINY each.
  sampler forward   gamma(C kH kW + k) |scale| sum |in1||in2| + (C kH kW + k) TINY; k = 0 for the plain sampler (scale = slope =
                    1: no operation), 2 for the fused one.
  sampler backward  gamma(npatch kH kW + k) sum |g scale m| |x| + (..) TINY, npatch = patchH patchW (81), k = 0 / 2: the taps
                    are fl(fl(g scale) m).
  FlowNet forward   gamma(k k C + 1) sum |in1||in2| / (k k C) + (..) TINY; backward gamma(L + 1) sum |g||x| / (k k C) + (..)
                    TINY with L the number of live taps of the element (gradient inside the output and partner inside the
                    image), counted by the reference itself on all-ones operands.
  ChannelNorm fwd   r = fl(sum x^2) = S (1 + t), |t| <= gamma(C + 1) (all terms positive); sqrt(1 + t) - 1 is within
                    |t| / 2 (1 + |t|); the correctly rounded sqrtf adds u:  SPARE (gamma(C + 1) / 2 + u) sqrt(S) + TINY.  The
                    inputs are asserted to be 0 or of magnitude in [2^-60, 2^63], so that no square under- or overflows.
  ChannelNorm bwd   one fp32 product (u), a double-precision sum and division (3 2^-53), the rounding to fp32 (u):
                    SPARE 2 u |want| + 2 TINY.
No tolerance is taken from a GPU run.  The statistical gate is that of tests/gates.py against `emu`.

Inputs, three variants per case.  `random`: N(0, 1) times a per-channel power of two in [1/4, 4].  `integer`: operands in
{-4..4}, gradient in {-2..2}, scale a power of two, slope 0.5 or 0.125 (FlowNet: k k C a power of two): every partial sum is an
integer multiple of scale slope below 2^24 of them (exact_ok asserts n max|a| max|b| < 2^24), so every fp32 operation is exact
in any order and the gate is equality with the float64 result, with no tolerance (+0 and -0 compare equal: the kernels'
accumulators start at +0).  `onehot`: in1 (forward) or the gradient (backward) is 2 at one element and 0 elsewhere, the other
operands are distinct integers +-(1 + index) (< 2^22): one product per output, exact; the element sits in turn at the image
corners, on both sides of the tile seams in x and y, and at the last channel / plane of a group (onehot_positions).  For the
fused backward fwd_out is fp32(reference forward) with +0, -0, 2^-126 and -2^-126 planted (plant) in every one of the 81 planes
at the first and last columns of the backward's 32-wide tiles and at the halo columns that grad_in2's taps read shifted.
"""
import functools
import itertools
import types

import torch
import torch.nn.functional as Fn

from tests.fenced import TINY, U, gamma
from tests.gates import gates as _gates

F32, F64 = torch.float32, torch.float64
SPARE = 1 + 2.0 ** -14
SC_LDS_BUDGET = 144 * 1024
SPECIALS = (0.0, -0.0, 2.0 ** -126, -2.0 ** -126)


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------- the host's plans
def scorr_plan(B, C, H, W):
    """plan_fwd and launch_fwd (spatial_corr.hip:219-263) and the kernel's staging split (:72-78, :103)."""
    tiles = ((4, 32, 2), (2, 32, 4), (2, 16, 8))
    k = 2
    for i, (th, tw, _) in enumerate(tiles):
        if cdiv(H, th) * cdiv(W, tw) * B >= 200:
            k = i
            break
    th, tw, ns = tiles[k]
    while ns > 1 and C // ns < 4:
        ns >>= 1
    pcf = th * tw + (th + 8) * (tw + 8)
    crmax = SC_LDS_BUDGET // (pcf * 4)
    rounds = cdiv(C, crmax)
    cr = cdiv(cdiv(C, rounds), ns) * ns
    clipped = cr > crmax
    if clipped:
        cr = crmax // ns * ns
    sizes = [min(cr, C - c0) for c0 in range(0, C, cr)]
    stage, red = cr * pcf * 4, (ns * 81 * th * tw * 4 if ns > 1 else 0)
    threads = (tw // 4) * th * 9 * ns
    ppc = th * (tw // 4) + (th + 8) * ((tw + 8) // 4)
    tiles_x = cdiv(W, tw)
    ntiles = tiles_x * cdiv(H, th)
    return types.SimpleNamespace(th=th, tw=tw, ns=ns, crmax=crmax, cr=cr, clipped=clipped, rounds=len(sizes), sizes=sizes,
                                 lds=max(stage, red), threads=threads, ppc=ppc, lanes=threads // ppc, tiles_x=tiles_x,
                                 ntiles=ntiles, dead=ntiles % 8 != 0, grid=8 * cdiv(ntiles, 8) * B,
                                 label="t%dx%d_ns%d_r%d" % (th, tw, ns, len(sizes)))


def scorr_bwd_plan(B, C, H, W, bth=2):
    """scorr9_backward (spatial_corr.hip:450-469): 32-wide tiles of bth rows, 32-channel groups, both gradients in z."""
    tiles_x = cdiv(W, 32)
    ntiles = tiles_x * cdiv(H, bth)
    groups = cdiv(C, 32)
    nz = 2 * B * groups
    return types.SimpleNamespace(bth=bth, tiles_x=tiles_x, ntiles=ntiles, groups=groups, tail=C % 32, nz=nz,
                                 dead=ntiles % 8 != 0, grid=8 * cdiv(ntiles, 8) * nz, label="b%dx32_g%d%s" % (
                                     bth, groups, "_tail%d" % (C % 32) if C % 32 else ""))


def sampler(k=(1, 1), patch=(9, 9), pad=(0, 0), dil=(1, 1), dil_patch=(1, 1), stride=(1, 1)):
    return types.SimpleNamespace(k=k, patch=patch, pad=pad, dil=dil, dil_patch=dil_patch, stride=stride)


FAST = sampler()


def sc_args(p):
    """The sixteen integers after (B, C, iH, iW) of pcfa_spatial_corr_fwd / _bwd."""
    return p.k + p.patch + p.pad + p.dil + p.dil_patch + p.stride


def sc_out_size(H, W, p):
    """make_params (spatial_corr.hip:559-571): (oH, oW), or None where the call is refused."""
    every = p.k + p.patch + p.dil + p.dil_patch + p.stride
    if H < 1 or W < 1 or min(every) < 1 or min(p.pad) < 0:
        return None
    nH = H + 2 * p.pad[0] - ((p.k[0] - 1) * p.dil[0] + 1)
    nW = W + 2 * p.pad[1] - ((p.k[1] - 1) * p.dil[1] + 1)
    if nH < 0 or nW < 0:
        return None
    return nH // p.stride[0] + 1, nW // p.stride[1] + 1


def sc_is_fast(p, W, aligned=True):
    """is_fast(p, 9) && aligned (spatial_corr.hip:573-576, :600-602, :625-628): every operand 16-byte aligned."""
    return (p.k == (1, 1) and p.stride == (1, 1) and p.pad == (0, 0) and p.dil_patch == (1, 1) and p.patch == (9, 9)
            and W % 4 == 0 and aligned)


def flownet(pad=20, k=1, md=20, s1=1, s2=2):
    return types.SimpleNamespace(pad=pad, k=k, md=md, s1=s1, s2=s2)


def fc_args(f):
    return (f.pad, f.k, f.md, f.s1, f.s2)


def fcorr_plan(B, C, H, W, f, aligned=True):
    """fc_make_params, fc_is_flownetc and the launches (flownet_ops.hip:33-45, :121-127, :481-485, :503-517).  aligned: in1,
    in2 (and out, on the forward) 16-byte aligned; the backward's gradients are free.  None where the call is refused."""
    if min(B, C, H, W) < 1 or f.pad < 0 or f.k < 1 or f.k % 2 == 0 or f.md < 0 or f.s1 < 1 or f.s2 < 1:
        return None
    kr = (f.k - 1) // 2
    nH, nW = H + 2 * f.pad - 2 * (kr + f.md), W + 2 * f.pad - 2 * (kr + f.md)
    if nH < 1 or nW < 1:
        return None
    drad = f.md // f.s2
    fast = (f.k, f.s1, f.s2, f.md, f.pad) == (1, 1, 2, 20, 20) and W % 4 == 0 and aligned
    return types.SimpleNamespace(oH=cdiv(nH, f.s1), oW=cdiv(nW, f.s1), drad=drad, dsize=2 * drad + 1, kr=kr,
                                 nelems=f.k * f.k * C, label="fast" if fast else "generic", tiles_x=cdiv(W, 32),
                                 tiles_y=cdiv(H, 8), row_groups=7, chunks=cdiv(C, 8), tail=C % 8, pow2=C & (C - 1) == 0,
                                 divide="reciprocal" if C & (C - 1) == 0 else "division")


# --------------------------------------------------------------------------- the sampler: reference and generic emulation
def _sc_geom(H, W, p):
    oH, oW = sc_out_size(H, W, p)
    MH, MW = p.pad[0] + p.patch[0] * p.dil_patch[0] + 1, p.pad[1] + p.patch[1] * p.dil_patch[1] + 1

    def rows(i, sU):
        s = MH - p.pad[0] + i * p.dil[0] + sU
        return slice(s, s + (oH - 1) * p.stride[0] + 1, p.stride[0])

    def cols(j, sV):
        s = MW - p.pad[1] + j * p.dil[1] + sV
        return slice(s, s + (oW - 1) * p.stride[1] + 1, p.stride[1])

    shifts = [(ph, pw, (ph - (p.patch[0] - 1) // 2) * p.dil_patch[0], (pw - (p.patch[1] - 1) // 2) * p.dil_patch[1])
              for ph in range(p.patch[0]) for pw in range(p.patch[1])]
    taps = list(itertools.product(range(p.k[0]), range(p.k[1])))
    return oH, oW, MH, MW, rows, cols, shifts, taps


def _zpad(x, MH, MW):
    return Fn.pad(x, (MW, MW, MH, MH))


def sc_fwd(in1, in2, p, dtype=F64):
    """[B][patchH][patchW][oH][oW].  float64: the reference (channels with an all-zero in1 are skipped: their terms are
    exact zeros).  float32: the generic kernel's order, per output c, i, j."""
    B, C, H, W = in1.shape
    oH, oW, MH, MW, rows, cols, shifts, taps = _sc_geom(H, W, p)
    a, b = in1.to(dtype), in2.to(dtype)
    if dtype == F64:
        nz = (a != 0).flatten(2).any(2).any(0)
        a, b = a[:, nz], b[:, nz]
    a, b = _zpad(a, MH, MW), _zpad(b, MH, MW)
    out = torch.zeros(B, p.patch[0], p.patch[1], oH, oW, dtype=dtype)
    for ph, pw, sU, sV in shifts:
        o = out[:, ph, pw]
        if dtype == F64:
            for i, j in taps:
                o += (a[:, :, rows(i, 0), cols(j, 0)] * b[:, :, rows(i, sU), cols(j, sV)]).sum(1)
        else:
            for c in range(a.shape[1]):
                for i, j in taps:
                    o += a[:, c, rows(i, 0), cols(j, 0)] * b[:, c, rows(i, sU), cols(j, sV)]
    return out


def sc_bwd(in1, in2, g, p, dtype=F64, reverse2=False, mut=None):
    """(gin1, gin2) of g [B][patchH][patchW][oH][oW]: per element the taps are added in (ph, pw, i, j) order -- the generic
    kernels' and the fast gin1's; reverse2: gin2 in descending plane order, the fast kernel's.  float64: the reference
    (all-zero planes of g are skipped)."""
    B, C, H, W = in1.shape
    oH, oW, MH, MW, rows, cols, shifts, taps = _sc_geom(H, W, p)
    a, b, g = _zpad(in1.to(dtype), MH, MW), _zpad(in2.to(dtype), MH, MW), g.to(dtype)
    g1, g2 = torch.zeros_like(a), torch.zeros_like(b)
    live = [s for s in shifts if dtype != F64 or bool((g[:, s[0], s[1]] != 0).any())]
    for ph, pw, sU, sV in live:
        gp = g[:, ph, pw].unsqueeze(1)
        for i, j in taps:
            g1[:, :, rows(i, 0), cols(j, 0)] += gp * b[:, :, rows(i, sU), cols(j, sV)]
    for ph, pw, sU, sV in (live[::-1] if reverse2 else live):
        gp = g[:, ph, pw].unsqueeze(1)
        if mut == "not_mirrored":
            sU, sV = -sU, -sV
        for i, j in taps:
            g2[:, :, rows(i, sU), cols(j, sV)] += gp * a[:, :, rows(i, 0), cols(j, 0)]
    crop = (slice(None), slice(None), slice(MH, MH + H), slice(MW, MW + W))
    return g1[crop].contiguous(), g2[crop].contiguous()


def leaky(x, slope):
    return torch.where(x > 0, x, x * slope)


def taps64(g, fwd_out, scale, slope):
    """g scale m in float64, m = fwd_out > 0 ? 1 : slope (fwd_out None: the plain sampler, m = 1)."""
    t = g.double() * scale
    return t if fwd_out is None else torch.where(fwd_out.view_as(g) > 0, t, t * slope)


def sc_ref_fwd(in1, in2, p, scale=1.0, slope=1.0, fused=False, with_bound=True):
    """(out64, bound)."""
    C = in1.shape[1]
    n, k = C * p.k[0] * p.k[1], 2 if fused else 0
    v = sc_fwd(in1, in2, p) * scale
    want = leaky(v, slope) if fused else v
    if not with_bound:
        return want, None
    P = sc_fwd(in1.abs(), in2.abs(), p)
    return want, gamma(n + k) * abs(scale) * P + (n + k) * TINY


def sc_ref_bwd(in1, in2, g, p, fwd_out=None, scale=1.0, slope=1.0, with_bound=True):
    """((gin1, gin2), (bound1, bound2))."""
    t = taps64(g, fwd_out, scale, slope)
    n, k = p.patch[0] * p.patch[1] * p.k[0] * p.k[1], 0 if fwd_out is None else 2
    want = sc_bwd(in1, in2, t, p)
    if not with_bound:
        return want, None
    P = sc_bwd(in1.abs(), in2.abs(), t.abs(), p)
    return want, tuple(gamma(n + k) * q + (n + k) * TINY for q in P)


# --------------------------------------------------------------------------- the sampler's fast kernels in fp32
def sc_emu_fwd_fast(in1, in2, plan, scale=1.0, slope=1.0, mut=None):
    B, C, H, W = in1.shape
    b = Fn.pad(in2, (4, 4, 4, 4)).contiguous()
    if mut == "halo_shift":                     # the halo column x = -1 staged from x = 0
        b[:, :, :, 3] = b[:, :, :, 4]
    sb, sc_, sh, _ = b.stride()
    win = b.as_strided((B, C, 9, 9, H, W), (sb, sc_, sh, 1, sh, 1))
    acc = torch.zeros(plan.ns, B, 9, 9, H, W)
    for c0 in range(0, C, plan.cr):
        for c in range(c0, min(c0 + plan.cr, C)):
            acc[(c - c0) % plan.ns] += in1[:, c, None, None] * win[:, c]
    tot = acc[0]
    for s in range(1, plan.ns - (1 if mut == "drop_slice" else 0)):
        tot = tot + acc[s]
    tot = tot * torch.tensor(scale, dtype=F32)
    return leaky(tot, torch.tensor(slope, dtype=F32)) if slope != 1.0 else tot


def sc_emu_taps(g, fwd_out, scale, slope, mut=None):
    t = g * torch.tensor(scale, dtype=F32)
    if fwd_out is None:
        return t
    f = fwd_out.view_as(g)
    return torch.where((f >= 0) if mut == "mask_ge" else (f > 0), t, t * torch.tensor(slope, dtype=F32))


def sc_emu_bwd_fast(in1, in2, g, fwd_out=None, scale=1.0, slope=1.0, mut=None):
    return sc_bwd(in1, in2, sc_emu_taps(g, fwd_out, scale, slope, mut), FAST, F32, reverse2=True, mut=mut)


# --------------------------------------------------------------------------- FlowNet correlation
def _fc_geom(H, W, f, pl):
    M = f.pad + pl.kr + 1
    base = M + f.md - f.pad

    def rows(j, d=0):
        s = base + j + d
        return slice(s, s + (pl.oH - 1) * f.s1 + 1, f.s1)

    def cols(i, d=0):
        s = base + i + d
        return slice(s, s + (pl.oW - 1) * f.s1 + 1, f.s1)

    disp = [(tj * pl.dsize + ti, (tj - pl.drad) * f.s2, (ti - pl.drad) * f.s2)
            for tj in range(pl.dsize) for ti in range(pl.dsize)]
    return M, rows, cols, disp


def fc_fwd(in1, in2, f, dtype=F64, divide=True):
    """[B][D D][oH][oW].  float32: per output j, i, c -- the generic kernel's order and, at k = 1, the fast kernel's."""
    B, C, H, W = in1.shape
    pl = fcorr_plan(B, C, H, W, f)
    M, rows, cols, disp = _fc_geom(H, W, f, pl)
    a, b = _zpad(in1.to(dtype), M, M), _zpad(in2.to(dtype), M, M)
    out = torch.zeros(B, pl.dsize ** 2, pl.oH, pl.oW, dtype=dtype)
    kk = range(-pl.kr, pl.kr + 1)
    for tc, dy, dx in disp:
        o = out[:, tc]
        for j in kk:
            for i in kk:
                if dtype == F64:
                    o += (a[:, :, rows(j), cols(i)] * b[:, :, rows(j, dy), cols(i, dx)]).sum(1)
                else:
                    for c in range(C):
                        o += a[:, c, rows(j), cols(i)] * b[:, c, rows(j, dy), cols(i, dx)]
    return out / torch.tensor(float(pl.nelems), dtype=dtype) if divide else out


def fc_bwd(in1, in2, g, f, dtype=F64, divide=True):
    """(gin1, gin2), stride1 = 1: per element the taps in displacement order, then output row and column ascending."""
    B, C, H, W = in1.shape
    assert f.s1 == 1
    pl = fcorr_plan(B, C, H, W, f)
    M, rows, cols, disp = _fc_geom(H, W, f, pl)
    a, b, g = _zpad(in1.to(dtype), M, M), _zpad(in2.to(dtype), M, M), g.to(dtype)
    g1, g2 = torch.zeros_like(a), torch.zeros_like(b)
    kk = range(pl.kr, -pl.kr - 1, -1)
    for tc, dy, dx in disp:
        gp = g[:, tc].unsqueeze(1)
        if dtype == F64 and not bool((gp != 0).any()):
            continue
        for j in kk:
            for i in kk:
                g1[:, :, rows(j), cols(i)] += gp * b[:, :, rows(j, dy), cols(i, dx)]
                g2[:, :, rows(j, dy), cols(i, dx)] += gp * a[:, :, rows(j), cols(i)]
    crop = (slice(None), slice(None), slice(M, M + H), slice(M, M + W))
    n = torch.tensor(float(pl.nelems), dtype=dtype)
    return tuple((t[crop] / n if divide else t[crop]).contiguous() for t in (g1, g2))


def fc_ref_fwd(in1, in2, f):
    n = fcorr_plan(*in1.shape, f).nelems
    P = fc_fwd(in1.abs(), in2.abs(), f)
    return fc_fwd(in1, in2, f), gamma(n + 1) * P + (n + 1) * TINY


def fc_ref_bwd(in1, in2, g, f):
    one = torch.ones_like(in1)
    live = fc_bwd(one, one, torch.ones_like(g), f, divide=False)
    P = fc_bwd(in1.abs(), in2.abs(), g.abs(), f)
    return fc_bwd(in1, in2, g, f), tuple(gamma(L + 1) * q + (L + 1) * TINY for L, q in zip(live, P))


def fc_emu_fwd(in1, in2, f):
    return fc_fwd(in1, in2, f, F32)


def fc_emu_bwd(in1, in2, g, f):
    return fc_bwd(in1, in2, g, f, F32)


# --------------------------------------------------------------------------- ChannelNorm
def cn_ref_fwd(x):
    S = (x.double() ** 2).sum(1, keepdim=True)
    C = x.shape[1]
    return S.sqrt(), SPARE * (gamma(C + 1) / 2 + U) * S.sqrt() + TINY


def cn_ref_bwd(x, norm, dy):
    want = dy.double() * x.double() / (norm.double() + 1e-9)
    return want, SPARE * 2 * U * want.abs() + 2 * TINY


def cn_emu_fwd(x):
    r = torch.zeros_like(x[:, :1])
    for c in range(x.shape[1]):
        r = r + x[:, c:c + 1] * x[:, c:c + 1]
    return r.sqrt()


def cn_emu_bwd(x, norm, dy, mut=None):
    return ((dy * x).double() / (norm.double() + (0.0 if mut == "no_eps" else 1e-9))).float()


# --------------------------------------------------------------------------- case tables
def _sc(shape, label, why):
    return types.SimpleNamespace(shape=shape, label=label, why=why, name="x".join(map(str, shape)))


SC_TABLE = [
    _sc((1, 3, 1, 4), "t2x16_ns1_r1", "one tile, mostly dead rows"),
    _sc((2, 5, 7, 36), "t2x16_ns1_r1", "odd H; last x tile one quad wide; 12 tiles, not a multiple of 8"),
    _sc((1, 9, 3, 20), "t2x16_ns2_r1", "ns 2"),
    _sc((1, 19, 5, 44), "t2x16_ns4_r1", "ns 4"),
    _sc((1, 37, 6, 20), "t2x16_ns8_r1", "ns 8; cr 40 > C; channel tail of the backward's 32-group"),
    _sc((1, 137, 4, 16), "t2x16_ns8_r2", "two rounds, 72 + 65"),
    _sc((1, 270, 3, 12), "t2x16_ns8_r3", "the cr > crmax branch: 128, 128, 14"),
    _sc((1, 196, 6, 20), "t2x16_ns8_r2", "KITTI level 6: 104 + 92"),
    _sc((1, 3, 49, 252), "t2x32_ns1_r1", "direct-store epilogue on 2x32"),
    _sc((2, 64, 48, 160), "t2x32_ns4_r1", "two pairs per closure, level 2"),
    _sc((1, 81, 49, 252), "t2x32_ns4_r2", "44 + 37; ragged rows; last tile 28 wide"),
    _sc((1, 7, 57, 436), "t4x32_ns1_r1", "H = 14 * 4 + 1; last tile 20 wide; direct-store epilogue on 4x32"),
    _sc((4, 64, 48, 160), "t4x32_ns2_r2", "four pairs per closure: 32 + 32"),
    _sc((1, 61, 57, 436), "t4x32_ns2_r2", "uneven rounds on 4x32: 32 + 29"),
]
SC_CASES = {c.name: c for c in SC_TABLE}
SC_SIZES = {"1x137x4x16": [72, 65], "1x270x3x12": [128, 128, 14], "1x196x6x20": [104, 92], "1x81x49x252": [44, 37],
            "4x64x48x160": [32, 32], "1x61x57x436": [32, 29], "1x37x6x20": [37]}
SC_TALL = ("2x5x7x36", "1x37x6x20")             # run once more on the 4-row backward tile (PCFA_SC_BTH=4)
SC_WILD = "1x19x5x44"


def _gen(name, shape, p, route, why, shift=(0, 0)):
    """route: `generic`, or `fast` made generic by `shift` floats on (in1, in2)."""
    return types.SimpleNamespace(name=name, shape=shape, p=p, route=route, why=why, shift=shift)


_RECT = sampler(k=(3, 1), patch=(5, 3), pad=(1, 0), dil=(1, 2), dil_patch=(2, 1), stride=(1, 2))
_RECT_T = sampler(**{k: v[::-1] for k, v in vars(_RECT).items()})
SC_GENERIC = [
    _gen("rect", (2, 3, 9, 11), _RECT, "params", "every H/W pair differs"),
    _gen("rect_t", (2, 3, 9, 11), _RECT_T, "params", "its transpose"),
    _gen("patch9_w7", (1, 4, 5, 7), FAST, "w%4", "the fast parameters with W % 4 != 0"),
    _gen("patch9_in1_shifted", (1, 4, 5, 8), FAST, "shift", "W % 4 == 0, in1 one float off", (1, 0)),
    _gen("patch9_in2_shifted", (1, 4, 5, 8), FAST, "shift", "W % 4 == 0, in2 one float off", (0, 1)),
    _gen("even_patch", (2, 3, 9, 11), sampler(k=(1, 3), patch=(4, 6), pad=(0, 2), dil=(1, 1), dil_patch=(1, 2), stride=(2, 1)),
         "params", "an even patch size: the centre is (patch - 1) / 2 rounded down"),
]


def _fc(shape, why):
    return types.SimpleNamespace(shape=shape, why=why, name="x".join(map(str, shape)))


FC_FAST = [
    _fc((1, 8, 8, 32), "one tile"),
    _fc((2, 19, 13, 36), "tail of 3 channels, ragged tile, division branch"),
    _fc((1, 1, 1, 4), "the smallest"),
    _fc((1, 9, 45, 68), "H, W > 40: all 441 displacements meet real data, the 48x72 halo fully inside somewhere"),
    _fc((1, 16, 9, 64), "reciprocal branch, two x tiles"),
]
FC_SHAPE = (2, 6, 12, 14)


def _fg(name, f, route, shape=FC_SHAPE, shift=0, backward=True):
    return types.SimpleNamespace(name=name, f=f, route=route, shape=shape, shift=shift, backward=backward)


FC_GENERIC = [_fg("p%d_k%d_md%d_s%d_%d" % t, flownet(*t), "params")
              for t in [(4, 1, 4, 1, 2), (5, 3, 4, 1, 2), (3, 3, 2, 1, 1), (2, 1, 4, 1, 2), (6, 1, 4, 1, 2), (20, 1, 20, 1, 4)]] + [
    _fg("pad_lt_md_s2_3", flownet(3, 3, 4, 1, 3), "params"),
    _fg("stride1_2", flownet(4, 1, 4, 2, 2), "stride1", backward=False),
    _fg("fast_w14", flownet(), "w%4"),
    _fg("fast_in1_shifted", flownet(), "shift", (2, 6, 12, 16), 1),
]
CN_TABLE = [(2, 3, 5, 7), (1, 2, 1, 1), (1, 64, 3, 5), (3, 1, 4, 4)]


# --------------------------------------------------------------------------- inputs
def _seed(shape, salt):
    return torch.Generator().manual_seed(salt + sum(s * 131 ** i for i, s in enumerate(shape)) % (2 ** 31))


def _distinct(shape, start=1):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=F64)
    return ((i + start) * (1 - 2 * (i % 2))).float().view(shape)


def int_consts(idx):
    """(scale, slope) of the integer and one-hot variants: powers of two."""
    return (0.25, 0.5) if idx % 2 == 0 else (0.5, 0.125)


def exact_ok(n, *operands):
    """n products of the operands' magnitudes stay below 2^24: every partial sum is exact in fp32."""
    m = n
    for t in operands:
        m *= float(t.abs().max())
    return m < 2 ** 24


@functools.lru_cache(maxsize=None)
def operands(shape, gshape, variant, salt=0):
    """(in1, in2, g) of the `random` and `integer` variants."""
    gen = _seed(shape, salt)
    C = shape[1]
    if variant == "random":
        sc = (2.0 ** (torch.randperm(C, generator=gen).double() * 4 / max(C - 1, 1) - 2)).float().view(1, C, 1, 1)
        return (torch.randn(shape, generator=gen) * sc, torch.randn(shape, generator=gen) * sc,
                torch.randn(gshape, generator=gen))
    assert variant == "integer"
    return (torch.randint(-4, 5, shape, generator=gen).float(), torch.randint(-4, 5, shape, generator=gen).float(),
            torch.randint(-2, 3, gshape, generator=gen).float())


def onehot_positions(shape, th, tw, nplanes, group):
    """(b, c, plane, y, x): the corners, both sides of the first and last tile seams in y and x, the last channel / plane of
    a group -- clipped to the tensor, duplicates dropped."""
    B, C, H, W = shape
    xs = [0, W - 1] + [x for x in (tw - 1, tw, (W - 1) // tw * tw - 1, (W - 1) // tw * tw) if 0 <= x < W]
    ys = [0, H - 1] + [y for y in (th - 1, th, (H - 1) // th * th - 1, (H - 1) // th * th) if 0 <= y < H]
    pos = [(0, 0, 0, 0, 0), (B - 1, C - 1, nplanes - 1, H - 1, W - 1), (0, min(group, C) - 1, 8, 0, W - 1),
           (B - 1, C - 1 - (C - 1) % group, nplanes - 9, H - 1, 0)]
    for k, (y, x) in enumerate(zip(ys[2:], xs[2:])):
        pos.append((k % B, (k * 7 + group - 1) % C, (40 + 10 * k) % nplanes, y, x))
    for k, x in enumerate(xs[2 + len(ys[2:]):]):
        pos.append((k % B, C // 2, (4 + 9 * k) % nplanes, H // 2, x))
    for k, y in enumerate(ys[2 + len(xs[2:]):]):
        pos.append((k % B, C // 2, (36 + k) % nplanes, y, W // 2))
    return list(dict.fromkeys(pos))


def onehot_in1(shape, pos):
    """(in1, in2): in1 = 2 at pos, in2 distinct integers."""
    a = torch.zeros(shape)
    a[pos[0], pos[1], pos[3], pos[4]] = 2.0
    return a, _distinct(shape)


def onehot_g(shape, gshape, pos):
    """(in1, in2, g): g = 2 at (b, plane, y, x), in1 and in2 distinct integers."""
    g = torch.zeros(gshape)
    g.view(gshape[0], -1, gshape[-2], gshape[-1])[pos[0], pos[2], min(pos[3], gshape[-2] - 1), min(pos[4], gshape[-1] - 1)] = 2.0
    return _distinct(shape), _distinct(shape, 3), g


def plant_columns(W):
    """First and last columns of the backward's 32-wide tiles and the halo columns read shifted by grad_in2's taps."""
    cols = set(range(0, 4)) | set(range(W - 4, W))
    for x0 in range(32, W, 32):
        cols |= set(range(x0 - 4, x0 + 4))
    return sorted(c for c in cols if 0 <= c < W)


def plant(fwd_out):
    """fwd_out [B][81][H][W] with the four special values at known places of every plane; returns (tensor, mask)."""
    f = fwd_out.clone()
    B, D, H, W = f.shape
    where = torch.zeros_like(f, dtype=torch.bool)
    sp = torch.tensor(SPECIALS)
    for d in range(D):
        for x in plant_columns(W):
            y = (d + x) % H
            f[:, d, y, x] = sp[(d + x // 2 + y) % 4]
            where[:, d, y, x] = True
    return f, where


CN_RUNS = [(s, True) for s in CN_TABLE] + [((1, 2, 1, 1), False)]     # the one-pixel case holds its two special pixels in turn


@functools.lru_cache(maxsize=None)
def cn_inputs(shape, huge=True):
    """(x, dy): one pixel of magnitude 1e18 (the last) and one all-zero pixel (the first: norm 0, gradient exactly 0); where
    the tensor has a single pixel, `huge` says which of the two it is."""
    gen = _seed(shape, 5)
    x = torch.randn(shape, generator=gen)
    x = torch.where(x.abs() < 2.0 ** -60, torch.full_like(x, 0.5), x)
    B, C, H, W = shape
    single = B * H * W == 1
    if huge:
        x[B - 1, :, H - 1, W - 1] = 1.0e18 * torch.sign(x[B - 1, :, H - 1, W - 1] + 0.5)
    if not (single and huge):
        x[0, :, 0, 0] = 0.0
    nz = x[x != 0].abs()
    assert nz.numel() == 0 or (float(nz.min()) >= 2.0 ** -60 and float(nz.max()) <= 2.0 ** 63)
    return x, torch.randn(B, 1, H, W, generator=gen)


# --------------------------------------------------------------------------- gates
def _none(H, W, m):
    return {}


def _as4(t):
    return t.reshape(t.shape[0], -1, t.shape[-2], t.shape[-1])


def gate(got, want, bound, emu, record, prefix, keep=None):
    """Both gates of tests/gates.py; keep: elements gated (the others are replaced by the reference: the wild case)."""
    got, want, bound, emu = _as4(got), _as4(want), _as4(bound), _as4(emu)
    if keep is not None:
        keep = _as4(keep)
        got, emu = torch.where(keep, got, want.float()), torch.where(keep, emu, want.float())
    return _gates(got, want, None, 0, emu, 0, record, prefix, regions=_none, bound=bound)


def exact(got, want, record, prefix):
    """Equality with the float64 result (+0 == -0); records and returns the number of mismatches, which must be 0."""
    w = want.float()
    assert bool((w.double() == want).all()), "the float64 result is not an fp32 number: the variant is not exact"
    bad = int((~(got.view_as(w) == w)).sum())
    record(prefix + "bit_mismatches", bad)
    assert bad == 0, (prefix, bad, "first at", (~(got.view_as(w) == w)).nonzero()[0].tolist())
    return bad


# --------------------------------------------------------------------------- one case's operands, references and emulation
def sc_lookup(key):
    """(shape, parameters, fast?) of a sampler case of either table."""
    if key in SC_CASES:
        return SC_CASES[key].shape, FAST, True
    case = next(c for c in SC_GENERIC if c.name == key)
    return case.shape, case.p, False


def sc_consts(key, variant):
    """(scale, slope) of the fused calls: PWC-Net's 1 / C and 0.1 on `random`, powers of two on the exact variants."""
    shape, _, _ = sc_lookup(key)
    return (1.0 / shape[1], 0.1) if variant == "random" else int_consts(sum(shape))


def _f32(x):
    return float(torch.tensor(x, dtype=F32))


@functools.lru_cache(maxsize=None)
def sc_data(key, variant):
    """Operands, float64 references and bounds of the `random` / `integer` variant of a case, computed once."""
    shape, p, fast = sc_lookup(key)
    B, C, H, W = shape
    oH, oW = sc_out_size(H, W, p)
    rnd = variant == "random"
    d = types.SimpleNamespace(key=key, variant=variant, shape=shape, p=p, fast=fast, rnd=rnd,
                              gshape=(B, p.patch[0], p.patch[1], oH, oW))
    d.in1, d.in2, d.g = operands(shape, d.gshape, variant)
    scale, slope = sc_consts(key, variant)
    d.scale, d.slope = _f32(scale), _f32(slope)                 # what the kernel receives
    n, nb = C * p.k[0] * p.k[1], p.patch[0] * p.patch[1] * p.k[0] * p.k[1]
    if not rnd:
        assert exact_ok(n, d.in1, d.in2) and exact_ok(nb, d.g, d.in1) and exact_ok(nb, d.g, d.in2)
    v = sc_fwd(d.in1, d.in2, p)
    P = sc_fwd(d.in1.abs(), d.in2.abs(), p) if rnd else None
    d.fwd = {"plain": (v, gamma(n) * P + n * TINY if rnd else None)}
    (w1, w2), Pb = sc_ref_bwd(d.in1, d.in2, d.g, p, with_bound=rnd)
    d.bwd = {"plain": ((w1, w2), Pb)}
    if fast:
        d.fwd["fused"] = (leaky(v * d.scale, d.slope), gamma(n + 2) * d.scale * P + (n + 2) * TINY if rnd else None)
        d.fwd_out, d.planted = plant(d.fwd["fused"][0].float().view(B, 81, H, W))
        want, _ = sc_ref_bwd(d.in1, d.in2, d.g, p, d.fwd_out, d.scale, d.slope, with_bound=False)
        # |g scale m| <= |scale| |g|: the plain bound's sum |g||x| times |scale|, with the two further roundings
        bnd = tuple((q - nb * TINY) / gamma(nb) * gamma(nb + 2) * d.scale + (nb + 2) * TINY for q in Pb) if rnd else None
        d.bwd["fused"] = (want, bnd)
    return d


def sc_emulate(d, mut=None):
    """{fwd: {form: out}, bwd: {form: (gin1, gin2)}} in fp32 in the order of the kernel the case runs on."""
    res = {"fwd": {}, "bwd": {}}
    if d.fast:
        plan = scorr_plan(*d.shape)
        res["fwd"]["plain"] = sc_emu_fwd_fast(d.in1, d.in2, plan, mut=mut)
        res["fwd"]["fused"] = sc_emu_fwd_fast(d.in1, d.in2, plan, d.scale, d.slope, mut=mut)
        res["bwd"]["plain"] = sc_emu_bwd_fast(d.in1, d.in2, d.g, mut=mut)
        res["bwd"]["fused"] = sc_emu_bwd_fast(d.in1, d.in2, d.g, d.fwd_out, d.scale, d.slope, mut=mut)
    else:
        res["fwd"]["plain"] = sc_fwd(d.in1, d.in2, d.p, F32)
        res["bwd"]["plain"] = sc_bwd(d.in1, d.in2, d.g, d.p, F32)
    return res


@functools.lru_cache(maxsize=None)
def sc_emulation(key, variant):
    return sc_emulate(sc_data(key, variant))


def sc_check(d, got, record, prefix="", keep=None, emu=None):
    """Gates every result in `got` (the layout of sc_emulate): both gates on `random`, equality on `integer`.  keep: the
    same layout of masks.  Returns the largest (elementwise, statistical) ratios."""
    worst = [0.0, 0.0]
    emu = emu or (sc_emulation(d.key, d.variant) if d.rnd else None)
    for form, out in got["fwd"].items():
        want, bound = d.fwd[form]
        tag = "%s%s_%s_fwd_" % (prefix, d.variant, form)
        if d.rnd:
            r = gate(out.view_as(want), want, bound, emu["fwd"][form], record, tag, None if keep is None else keep["fwd"])
            worst = [max(a, b) for a, b in zip(worst, r)]
        else:
            exact(out, want, record, tag)
    for form, outs in got["bwd"].items():
        wants, bounds = d.bwd[form]
        for i in range(2):
            tag = "%s%s_%s_gin%d_" % (prefix, d.variant, form, i + 1)
            if d.rnd:
                r = gate(outs[i], wants[i], bounds[i], emu["bwd"][form][i], record, tag,
                         None if keep is None else keep["bwd"][i])
                worst = [max(a, b) for a, b in zip(worst, r)]
            else:
                exact(outs[i], wants[i], record, tag)
    return tuple(worst)


def sc_positions(key):
    """The one-hot positions of a sampler case: the forward's tile seams and the backward's (2 x 32; 4 x 32 when tall)."""
    shape, p, fast = sc_lookup(key)
    nplanes = p.patch[0] * p.patch[1]
    if not fast:
        return onehot_positions(shape, shape[2], shape[3], nplanes, 32)
    plan = scorr_plan(*shape)
    pos = onehot_positions(shape, plan.th, plan.tw, nplanes, 32) + onehot_positions(shape, 2, 32, nplanes, 32)
    return list(dict.fromkeys(pos))


def sc_onehot(key, pos, fwd_out=None):
    """One position: the forward's (in1, in2) with in1 one-hot, the backward's (in1, in2, g) with g one-hot, and their
    float64 results {fwd: {form: out}, bwd: {form: (gin1, gin2)}}.  fwd_out: the tensor the fused backward is given."""
    shape, p, fast = sc_lookup(key)
    B, C, H, W = shape
    oH, oW = sc_out_size(H, W, p)
    gshape = (B, p.patch[0], p.patch[1], oH, oW)
    scale, slope = sc_consts(key, "onehot")
    o = types.SimpleNamespace(key=key, variant="onehot", rnd=False, fast=fast, p=p, shape=shape, gshape=gshape,
                              scale=_f32(scale), slope=_f32(slope), fwd_out=fwd_out)
    o.f_in1, o.f_in2 = onehot_in1(shape, pos)
    o.in1, o.in2, o.g = onehot_g(shape, gshape, pos)
    assert exact_ok(1, o.f_in1, o.f_in2) and exact_ok(1, o.g, o.in1) and exact_ok(1, o.g, o.in2)
    v = sc_fwd(o.f_in1, o.f_in2, p)
    o.fwd = {"plain": (v, None)}
    o.bwd = {"plain": sc_ref_bwd(o.in1, o.in2, o.g, p, with_bound=False)}
    if fast:
        o.fwd["fused"] = (leaky(v * o.scale, o.slope), None)
        o.bwd["fused"] = sc_ref_bwd(o.in1, o.in2, o.g, p, fwd_out, o.scale, o.slope, with_bound=False)
    return o


def sc_emulate_onehot(o, mut=None):
    res = {"fwd": {}, "bwd": {}}
    if o.fast:
        plan = scorr_plan(*o.shape)
        res["fwd"]["plain"] = sc_emu_fwd_fast(o.f_in1, o.f_in2, plan, mut=mut)
        res["fwd"]["fused"] = sc_emu_fwd_fast(o.f_in1, o.f_in2, plan, o.scale, o.slope, mut=mut)
        res["bwd"]["plain"] = sc_emu_bwd_fast(o.in1, o.in2, o.g, mut=mut)
        res["bwd"]["fused"] = sc_emu_bwd_fast(o.in1, o.in2, o.g, o.fwd_out, o.scale, o.slope, mut=mut)
    else:
        res["fwd"]["plain"] = sc_fwd(o.f_in1, o.f_in2, o.p, F32)
        res["bwd"]["plain"] = sc_bwd(o.in1, o.in2, o.g, o.p, F32)
    return res


# FlowNet correlation -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fc_data(shape, fargs, variant):
    f = flownet(*fargs)
    pl = fcorr_plan(*shape, f)
    d = types.SimpleNamespace(shape=shape, f=f, variant=variant, rnd=variant == "random", plan=pl,
                              gshape=(shape[0], pl.dsize ** 2, pl.oH, pl.oW), backward=f.s1 == 1)
    d.in1, d.in2, d.g = operands(shape, d.gshape, variant, salt=9)
    if d.rnd:
        d.fwd = fc_ref_fwd(d.in1, d.in2, f)
        d.bwd = fc_ref_bwd(d.in1, d.in2, d.g, f) if d.backward else None
    else:
        assert pl.nelems & (pl.nelems - 1) == 0, "the exact variants need k k C a power of two"
        assert exact_ok(pl.nelems, d.in1, d.in2) and exact_ok(pl.dsize ** 2 * f.k ** 2, d.g, d.in1)
        d.fwd = (fc_fwd(d.in1, d.in2, f), None)
        d.bwd = (fc_bwd(d.in1, d.in2, d.g, f), None) if d.backward else None
    return d


def fc_emulate(d, mut=None):
    res = {"fwd": fc_emu_fwd(d.in1, d.in2, d.f)}
    if d.backward:
        g = d.g.flip(1) if mut == "planes_flipped" else d.g
        res["bwd"] = fc_emu_bwd(d.in1, d.in2, g, d.f)
    return res


@functools.lru_cache(maxsize=None)
def fc_emulation(shape, fargs):
    return fc_emulate(fc_data(shape, fargs, "random"))


def fc_check(d, got, record, prefix="", emu=None):
    worst = [0.0, 0.0]
    emu = emu or (fc_emulation(d.shape, fc_args(d.f)) if d.rnd else None)
    items = [("fwd_", got["fwd"], d.fwd[0], d.fwd[1], emu["fwd"] if d.rnd else None)]
    if "bwd" in got:
        items += [("gin%d_" % (i + 1), got["bwd"][i], d.bwd[0][i], d.bwd[1][i] if d.rnd else None,
                   emu["bwd"][i] if d.rnd else None) for i in range(2)]
    for name, out, want, bound, e in items:
        tag = "%s%s_%s" % (prefix, d.variant, name)
        if d.rnd:
            worst = [max(a, b) for a, b in zip(worst, gate(out, want, bound, e, record, tag))]
        else:
            exact(out, want, record, tag)
    return tuple(worst)


def fc_onehot(shape, fargs, pos):
    f = flownet(*fargs)
    pl = fcorr_plan(*shape, f)
    assert pl.nelems & (pl.nelems - 1) == 0
    gshape = (shape[0], pl.dsize ** 2, pl.oH, pl.oW)
    o = types.SimpleNamespace(shape=shape, f=f, variant="onehot", rnd=False, plan=pl, gshape=gshape, backward=f.s1 == 1)
    o.f_in1, o.f_in2 = onehot_in1(shape, pos)
    o.in1, o.in2, o.g = onehot_g(shape, gshape, pos)
    assert exact_ok(1, o.f_in1, o.f_in2) and exact_ok(1, o.g, o.in1) and exact_ok(1, o.g, o.in2)
    o.fwd = (fc_fwd(o.f_in1, o.f_in2, f), None)
    o.bwd = (fc_bwd(o.in1, o.in2, o.g, f), None)
    return o


def fc_positions(shape, dsize):
    return onehot_positions(shape, 8, 32, dsize ** 2, 8)


# ChannelNorm ---------------------------------------------------------------------------------------------------------------
def cn_check(shape, huge, got_norm, got_gin, record, prefix=""):
    """Both gates on the forward and the backward; the backward's norm operand is fp32(reference norm)."""
    x, dy = cn_inputs(shape, huge)
    want, bound = cn_ref_fwd(x)
    norm = want.float()
    r1 = gate(got_norm.view_as(want), want, bound, cn_emu_fwd(x), record, prefix + "fwd_")
    wg, bg = cn_ref_bwd(x, norm, dy)
    r2 = gate(got_gin, wg, bg, cn_emu_bwd(x, norm, dy), record, prefix + "bwd_")
    if bool((x[0, :, 0, 0] == 0).all()):
        assert bool((got_gin[0, :, 0, 0] == 0).all()) and float(got_norm.flatten()[0]) == 0.0, "the all-zero pixel"
    return max(r1[0], r2[0]), max(r1[1], r2[1])
