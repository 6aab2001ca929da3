"""The four fused SepConvGRU epilogues of the sepconv5 kernels (csrc/sepconv5.hpp GruEpi modes 1-4, include/pcfa_hip.h
pcfa_sepconv5_gru_*) stated once in float64, with an elementwise bound and an fp32 emulation for every output; shared by
tests/test_gru_epilogue_host_cpu.py and tests/test_gru_epilogue_f64_gpu.py.

  gates_fwd  (1): [zc | rc] = conv_zr([h | rest]) + add_zr;  z = sigmoid(zc), r = sigmoid(rc), rh = r h
  update_fwd (2): qc = conv_q([rh | rest]) + add_q;  q = tanh(qc), hnew = (1 - z) h + z q
  gates_bwd  (3): [drh | d_rest] = conv_q'(dqc);  dzr = [dz (1 - z) z | ((drh h)(1 - r)) r],  dh = drh r + dh_in
  update_bwd (4): [ddh | d_rest] += conv_zr'(dzr);  g = dh_acc + ddh;  dz = g q - g h, dqc = (g z)(1 - q q), dh = g (1 - z)
conv' = the data gradient: the same operator with the flipped, transposed weight.  The same expressions evaluate in
float64 (`want`) and in fp32 on the kernel's emulated convolution (`emu`: wg.winograd_sepconv5 with the kernel's K groups,
wg.direct_sepconv5_fp32), so the two differ by rounding alone.

Elementwise bound.  E = 2 gamma(n + 2) P + (n + 2) 2^-126 is the convolution's bound (tests/winograd.py: n = Cin + 10
Winograd, 5 Cin + 2 direct; P from the absolute values); a tensor added before the activation (add_zr, add_q, dh_acc)
costs one more rounding and enters P with its magnitude.  E passes through the epilogue with Lipschitz constants -- 1/4
for the sigmoid, 1 for tanh, and the absolute value of every exact operand that multiplies (|h| for rh, |z| for hnew,
|h (1 - r) r| for dzr[:, C:], |q - h| for dz, ...) -- and the k fp32 operations of the expression itself add gamma(k) times
the sum of its absolute terms (k per output: tests/winograd.py).  The device sigmoid (expf, add, divide) and tanhf add
c u |want|; dzr[:, :C] of mode 3 holds no convolution and gets the gamma(k) term only; d_rest keeps the plain bound E.

c_sigmoid, c_tanh.  Measured on an MI355X from the un-fused elementwise kernels pcfa_gru_gates_fwd / pcfa_gru_update_fwd
(gru_math.hip, whose expressions the epilogues copy) on `activation_grid()` -- 2^20 pre-activations over [-30, 30], half
of them in [-2, 2] -- against float64 of the same fp32 argument, in units of u |f64|:
    sigmoid: max 2.43 -> C_SIGMOID = 5        tanhf: max 2.36 -> C_TANH = 5
(twice the measured maximum, rounded up: the grid is finite).  test_activation_constants measures them again.  Against
E / 4 this term is small at every shape of CASES: E / 4 >= gamma(54) P / 2 with P of order 1, i.e. some 1.6e-6, where
c u = 5 * 6e-8 = 3e-7 of a value that is at most 1.
"""
import functools
import types

import torch
import torch.nn.functional as F

from tests import winograd as wg
from tests.fenced import TINY, U, gamma

MEASURED_SIGMOID, MEASURED_TANH = 2.43, 2.36     # units of u |f64| (rounded up in the last digit)
C_SIGMOID, C_TANH = 5, 5

ENTRIES = ("gates_fwd", "update_fwd", "gates_bwd", "update_bwd")
LABELS = ("wino_wide", "wino_narrow", "direct_split2", "direct_fast", "direct_slow")
CASES = [  # (B, C, Cr, H, W) and the pairs (entry point, path) a case is in the table for
    (1, 128, 32, 100, 128),   # update_fwd wide Winograd; everything direct_fast
    (1, 64, 64, 100, 128),    # gates_bwd / update_bwd wide Winograd
    (1, 128, 64, 50, 128),    # narrow Winograd backward; direct_split2
    (2, 32, 32, 9, 128),      # narrow Winograd forward; batch 2; odd H; Cout = 32
    (1, 64, 32, 9, 68),       # branch-free direct with a partial last pixel tile
    (1, 32, 8, 90, 68),       # direct_slow forward: Cin % 8 == 0 but not % 32
    (2, 32, 12, 7, 13),       # direct_slow everywhere: W % 4 != 0, Cr % 32 != 0, batch 2
]
SATURATED = (30.0, -30.0, 100.0, -100.0)


def op_shape(entry, C, Cr):
    """(Ca, Cb, Cout) of the convolution an entry point launches"""
    return {"gates_fwd": (C, Cr, 2 * C), "update_fwd": (C, Cr, C), "gates_bwd": (C, 0, C + Cr),
            "update_bwd": (2 * C, 0, C + Cr)}[entry]


def path(entry, B, C, Cr, H, W, vertical, enabled=True, env=None):
    Ca, Cb, Cout = op_shape(entry, C, Cr)
    return wg.sepconv5_path(B, Ca, Cb, Cout, H, W, vertical, enabled=enabled, env={} if env is None else env)


def run_shape(case, vertical):
    """The 5x1 runs of the first two cases take H = 101 -- an odd row pair on the wide tile too -- where that keeps
    every label of the case."""
    B, C, Cr, H, W = case
    if vertical and case in CASES[:2]:
        odd = (B, C, Cr, H + 1, W)
        if all(path(e, *odd, 1, on) == path(e, *case, 1, on) for e in ENTRIES for on in (True, False)):
            return odd
    return case


def activation_grid():
    """2^20 fp32 pre-activations over [-30, 30], half of them in [-2, 2]"""
    n = 1 << 19
    return torch.cat([torch.linspace(-30, 30, n, dtype=torch.float64), torch.linspace(-2, 2, n, dtype=torch.float64)]).float()


def units_of_u(got, want64):
    """max |got - want| / (u |want|) (0 where both are 0)"""
    err = (got.double() - want64).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / (U * want64.abs())).max())


# --------------------------------------------------------------------------- the four epilogues, in the operands' dtype
def sigmoid(x):
    return 1 / (1 + torch.exp(-x))   # as gru_math.hip sigmoidf_


def epi_gates_fwd(pre, h):
    C = h.shape[1]
    z, r = sigmoid(pre[:, :C]), sigmoid(pre[:, C:])
    return z, r, r * h


def epi_update_fwd(pre, z, h):
    q = torch.tanh(pre)
    return q, (1 - z) * h + z * q


def epi_gates_bwd(drh, z, r, h, dz, dh_in):
    dzc = dz * (1 - z) * z
    drc = (drh * h) * (1 - r) * r
    dh = drh * r
    return torch.cat([dzc, drc], 1), dh if dh_in is None else dh + dh_in


def epi_update_bwd(g, z, q, h):
    return g * q - g * h, (g * z) * (1 - q * q), g * (1 - z)


# --------------------------------------------------------------------------- the convolution: float64, |.|, emulated fp32
def bwd_weight(wt):
    """the operator of the data gradient of a Conv2d weight [Cout'][Cin'][5]: flipped and transposed"""
    return wt.transpose(0, 1).flip(-1)


def conv_f64(x, weff, vertical):
    return F.conv2d(x.double(), weff.double().unsqueeze(-1 if vertical else -2), padding=(2, 0) if vertical else (0, 2))


def conv_abs(x, weff, vertical, wino):
    if wino:
        return wg.winograd_sepconv5(x.double(), weff.double(), vertical, absval=True)
    return conv_f64(x.abs(), weff.abs(), vertical)


def conv_fp32(x, weff, vertical, wino, groups):
    if wino:
        return wg.winograd_sepconv5(x, weff, vertical, dtype=torch.float32,
                                    partials=wg.chunk_partials(x.shape[1], [("interleave", groups)]))
    return wg.direct_sepconv5_fp32(x, weff, vertical)


def conv_terms(Cin, wino):
    return Cin + 10 if wino else 5 * Cin + 2


def conv_bound(P, n):
    return 2 * gamma(n + 2) * P + (n + 2) * TINY


# --------------------------------------------------------------------------- inputs and problems (cached per shape)
def _saturate(t, gen):
    sel = torch.rand(t.shape, generator=gen) < 0.01
    vals = torch.tensor(SATURATED)[torch.randint(0, 4, t.shape, generator=gen)]
    return torch.where(sel, vals, t)


@functools.lru_cache(maxsize=2)
def inputs(B, C, Cr, H, W, vertical):
    gen = torch.Generator().manual_seed(C * 31 + Cr * 7 + H * W + vertical)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    Cin, s = C + Cr, (B, C, H, W)
    d = types.SimpleNamespace()
    d.h, d.rest = torch.tanh(rnd(*s)), rnd(B, Cr, H, W)
    d.w_zr, d.w_q = rnd(2 * C, Cin, 5) / (5 * Cin) ** .5, rnd(C, Cin, 5) / (5 * Cin) ** .5
    d.add_zr, d.add_q = _saturate(rnd(B, 2 * C, H, W), gen), _saturate(rnd(*s), gen)
    d.z, d.r, d.q = torch.sigmoid(rnd(*s)), torch.sigmoid(rnd(*s)), torch.tanh(rnd(*s))
    d.rh = d.r * d.h
    d.dz, d.dqc, d.dh_in, d.dh_acc, d.dzr = rnd(*s), rnd(*s), rnd(*s), rnd(*s), rnd(B, 2 * C, H, W)
    d.prev_rest = rnd(B, Cr, H, W)
    return d


def operand(d, entry):
    """(the convolution's input, the Conv2d weight it belongs to, data gradient?)"""
    return {"gates_fwd": (lambda: (torch.cat([d.h, d.rest], 1), d.w_zr, False)),
            "update_fwd": (lambda: (torch.cat([d.rh, d.rest], 1), d.w_q, False)),
            "gates_bwd": (lambda: (d.dqc, d.w_q, True)),
            "update_bwd": (lambda: (d.dzr, d.w_zr, True))}[entry]()


@functools.lru_cache(maxsize=2)
def _conv_f64_cached(B, C, Cr, H, W, vertical, entry):
    x, wt, backward = operand(inputs(B, C, Cr, H, W, vertical), entry)
    return conv_f64(x, bwd_weight(wt) if backward else wt, vertical)


@functools.lru_cache(maxsize=2)
def problem(B, C, Cr, H, W, vertical, entry, wino, groups):
    """{output: (want float64, elementwise bound, fp32 emulation)} of one entry point on one path, and
    {output: mask of the elements whose addend is saturated} (modes 1 and 2).  gates_bwd: `dh` with dh_in, `dh_null`
    without; `d_rest` written, `d_rest_acc` accumulated onto prev_rest.  update_bwd: d_rest always accumulates."""
    d = inputs(B, C, Cr, H, W, vertical)
    x, wt, backward = operand(d, entry)
    weff = bwd_weight(wt) if backward else wt
    y64 = _conv_f64_cached(B, C, Cr, H, W, vertical, entry)
    P = conv_abs(x, weff, vertical, wino)
    y32 = conv_fp32(x, weff, vertical, wino, groups)
    n = conv_terms(x.shape[1], wino)
    f8 = lambda t: t.double()  # noqa: E731
    g = gamma
    outs, sat = {}, {}
    if entry == "gates_fwd":
        E = conv_bound(P + f8(d.add_zr).abs(), n + 1)
        z, r, rh = epi_gates_fwd(y64 + f8(d.add_zr), f8(d.h))
        ez, er, erh = epi_gates_fwd(y32 + d.add_zr, d.h)
        bz, br = (0.25 * E[:, lo:lo + C] * (1 + C_SIGMOID * U) + C_SIGMOID * U * s + TINY for lo, s in ((0, z), (C, r)))
        outs = {"z": (z, bz, ez), "r": (r, br, er),
                "rh": (rh, f8(d.h).abs() * br * (1 + g(1)) + g(1) * rh.abs() + TINY, erh)}
        sz, sr = d.add_zr[:, :C].abs() >= 30, d.add_zr[:, C:].abs() >= 30
        sat = {"z": sz, "r": sr, "rh": sr}
    elif entry == "update_fwd":
        E = conv_bound(P + f8(d.add_q).abs(), n + 1)
        z, h = f8(d.z), f8(d.h)
        q, hnew = epi_update_fwd(y64 + f8(d.add_q), z, h)
        eq, ehnew = epi_update_fwd(y32 + d.add_q, d.z, d.h)
        bq = E * (1 + C_TANH * U) + C_TANH * U * q.abs() + TINY
        outs = {"q": (q, bq, eq),
                "hnew": (hnew, z * bq * (1 + g(4)) + g(4) * (((1 - z) * h).abs() + (z * q).abs()) + TINY, ehnew)}
        sq = d.add_q.abs() >= 30
        sat = {"q": sq, "hnew": sq}
    elif entry == "gates_bwd":
        E = conv_bound(P[:, :C], n)
        z, r, h, dz, dh_in, drh = f8(d.z), f8(d.r), f8(d.h), f8(d.dz), f8(d.dh_in), y64[:, :C]
        dzr, dh = epi_gates_bwd(drh, z, r, h, dz, dh_in)
        _, dh0 = epi_gates_bwd(drh, z, r, h, dz, None)
        edzr, edh = epi_gates_bwd(y32[:, :C], d.z, d.r, d.h, d.dz, d.dh_in)
        _, edh0 = epi_gates_bwd(y32[:, :C], d.z, d.r, d.h, d.dz, None)
        bzr = torch.cat([g(3) * dzr[:, :C].abs() + TINY,
                         (h * (1 - r) * r).abs() * E * (1 + g(4)) + g(4) * dzr[:, C:].abs() + TINY], 1)
        prev = f8(d.prev_rest)
        outs = {"dzr": (dzr, bzr, edzr),
                "dh": (dh, r * E * (1 + g(2)) + g(2) * (dh_in.abs() + dh0.abs()) + TINY, edh),
                "dh_null": (dh0, r * E * (1 + g(1)) + g(1) * dh0.abs() + TINY, edh0),
                "d_rest": (y64[:, C:], conv_bound(P[:, C:], n), y32[:, C:]),
                "d_rest_acc": (y64[:, C:] + prev, conv_bound(P[:, C:] + prev.abs(), n), y32[:, C:] + d.prev_rest)}
    else:
        acc = f8(d.dh_acc)
        E = conv_bound(P[:, :C] + acc.abs(), n + 1)
        z, q, h, gg = f8(d.z), f8(d.q), f8(d.h), acc + y64[:, :C]
        dz, dqc, dh = epi_update_bwd(gg, z, q, h)
        edz, edqc, edh = epi_update_bwd(d.dh_acc + y32[:, :C], d.z, d.q, d.h)
        prev = f8(d.prev_rest)
        outs = {"dz": (dz, (q - h).abs() * E + g(3) * ((gg * q).abs() + (gg * h).abs() + (q.abs() + h.abs()) * E) + TINY, edz),
                "dqc": (dqc, (z * (1 - q * q)).abs() * E + g(4) * (gg.abs() + E) * z * (1 + q * q) + TINY, edqc),
                "dh": (dh, (1 - z) * E * (1 + g(2)) + g(2) * dh.abs() + TINY, edh),
                "d_rest": (y64[:, C:] + prev, conv_bound(P[:, C:] + prev.abs(), n), y32[:, C:] + d.prev_rest)}
    return outs, sat


def saturated_exact(add, sigmoid_):
    """(mask, value) of the elements an fp32 activation must give exactly: the convolution moves a pre-activation by a
    few units at most, so tanh is +-1 at every saturated addend; the sigmoid is 1 from +30 on (1 - 1e-11 rounds to 1)
    and 0 at -100 (expf overflows: 1 / inf), while at -30 it is a normal number of order 1e-13."""
    if sigmoid_:
        return (add >= 30) | (add <= -100), (add > 0).float()
    return add.abs() >= 30, torch.sign(add)


def groups_of(W):
    """regions(H, W, m) for gates(): the Winograd pairs' groups plus the columns of the ragged last 64-pixel tile"""
    def regions(H, W_, m):
        r = wg.regions(H, W_, m)
        if W_ % 64:
            r["px_tile"] = (slice(None), slice(W_ // 64 * 64, W_))
        return r
    return regions


# --------------------------------------------------------------------------- the whole step, as pcfa_amd/ops/gru.py chains it
def step(conv, h, rest, halves, go, rest_relu=0):
    """One SepConvGRU update and its backward in the dtype of the arguments: halves = ((w_zr, p_zr, w_q, p_q) of the 1x5
    half-step, (..) of the 5x1 one), weights [.][C + Cr][5]; conv(x, weff, vertical, Ca) -> the 5-tap convolution.
    Forward modes 1 -> 2 per half; backward: the un-fused update backward of the last half, then modes 3 -> 4 -> 3 and the
    plain data gradient of the first z|r convolution.  Returns (out, dh, d_rest, dp_zr1, dp_q1, dp_zr2, dp_q2)."""
    C = h.shape[1]
    saved = []
    for v, (w_zr, p_zr, w_q, p_q) in enumerate(halves):
        z, r, rh = epi_gates_fwd(conv(torch.cat([h, rest], 1), w_zr, v, C) + p_zr, h)
        q, hnew = epi_update_fwd(conv(torch.cat([rh, rest], 1), w_q, v, C) + p_q, z, h)
        saved.append((z, r, q, h))
        h = hnew
    (z0, r0, q0, h0), (z1, r1, q1, h1) = saved
    (w_zr0, _, w_q0, _), (w_zr1, _, w_q1, _) = halves
    dz1, dqc1, dh1 = epi_update_bwd(go, z1, q1, h1)
    o = conv(dqc1, bwd_weight(w_q1), 1, C)
    dzr1, dh1 = epi_gates_bwd(o[:, :C], z1, r1, h1, dz1, dh1)
    d_rest = o[:, C:]
    o = conv(dzr1, bwd_weight(w_zr1), 1, 2 * C)
    dz0, dqc0, dh0 = epi_update_bwd(dh1 + o[:, :C], z0, q0, h0)
    d_rest = d_rest + o[:, C:]
    o = conv(dqc0, bwd_weight(w_q0), 0, C)
    dzr0, dh0 = epi_gates_bwd(o[:, :C], z0, r0, h0, dz0, dh0)
    d_rest = d_rest + o[:, C:]
    o = conv(dzr0, bwd_weight(w_zr0), 0, 2 * C)
    dh0, d_rest = dh0 + o[:, :C], d_rest + o[:, C:]
    if rest_relu:
        d_rest = torch.cat([d_rest[:, :rest_relu] * (rest[:, :rest_relu] > 0), d_rest[:, rest_relu:]], 1)
    return h, dh0, d_rest, dzr0, dqc0, dzr1, dqc1


def step_conv_f64(x, weff, vertical, Ca):
    return conv_f64(x, weff, vertical)


def step_conv_fp32(enabled):
    """the emulated convolution on the path the host picks for each launch of the step"""
    def conv(x, weff, vertical, Ca):
        B, Cin, H, W = x.shape
        Cout = weff.shape[0]
        wino = wg.sepconv5_uses_winograd(B, Ca, Cin - Ca, Cout, H, W, vertical, enabled)
        return conv_fp32(x, weff, vertical, wino, wg.sepconv5_wino_groups(B, Cout, H, W, vertical))
    return conv
