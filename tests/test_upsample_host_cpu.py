"""The references, emulations, inputs and gates of tests/upsample.py on the CPU (no GPU).

Every convex case holds every logit class with at least its minimum count and the live / dead columns it is listed for; the
fp32 emulations pass every gate against float64 on every case and variant (the worst ratios are printed, pytest -s, and
recorded as junit properties); the references agree with torch autograd of the oracle's convex_upsample and of F.interpolate in
float64; and one-line faults in the emulations each fail a gate.  Shortening the bilinear backward's window by one output
changes nothing (the kernel's window has that much slack on either side: an equivalent mutant, shown bit for bit); the
window is therefore shortened until the first bit changes, and that fails.
"""
import pytest
import torch
import torch.nn.functional as Fn

from tests import upsample as up

torch.set_num_threads(min(16, torch.get_num_threads()))
WORST = {}


def _quiet(*_):
    pass


def _note(entry, res):
    w = WORST.setdefault(entry, [0.0, 0.0])
    w[0], w[1] = max(w[0], res[0]), max(w[1], res[1])
    print("%-22s emulation elementwise %.3g, statistical %.3g; worst so far %.3g / %.3g" % ((entry,) + tuple(res[:2]) + tuple(w)))


# --------------------------------------------------------------------------- convex
@pytest.mark.parametrize("shape", up.CONVEX_SHAPES, ids=str)
def test_convex_census(shape):
    N, H, W = shape
    got = up.convex_census(shape)
    for c in up.LOGIT_CLASSES:
        assert got["class/" + c] >= up.MIN_PER_CLASS, (c, got)
    for k in ("tied", "peak>=35", "underflow", "subnormal", "-inf", "overflow"):
        assert got[k] >= up.MIN_PER_CLASS, (k, got)
    assert got["flow>1e3"] >= 1
    assert got["live_in_last_wg"] == {1: 1, 5: 5, 63: 63, 64: 64, 65: 1, 70: 6, 130: 2}[W]
    assert (got["dead_columns"] > 0) == (W % 64 != 0)
    assert 576 * N * H * W * 4 <= 12 * 2 ** 20
    reg = up.convex_regions(shape)
    assert bool((reg["border"] | reg["last_wg"] | reg["interior"]).all())
    if W > 64:
        assert int(reg["last_wg"].sum()) == H * got["live_in_last_wg"]


@pytest.mark.parametrize("shape", up.CONVEX_SHAPES, ids=str)
def test_convex_emulation_passes_the_gates(record_property, shape):
    for variant in up.CONVEX_GOUTS:
        c = up.convex_case(shape, variant)
        a, b, d = up.convex_check(c, *c.emu, record_property, variant + "_")
        if variant == "random":
            _note("convex_out", a)
        _note("convex_grad_flow", b)
        _note("convex_grad_mask", d)
        if variant == "zero":
            assert bool((c.emu[1] == 0).all()) and bool((c.emu[2] == 0).all())


def test_convex_wild_case_keeps_its_references_finite():
    c = up.convex_case(up.WILD_SHAPE, "random", True)
    assert int(c.poisoned.gm.sum()) == 3 and int(c.poisoned.out.sum()) == 3 * 64
    assert not bool(torch.isfinite(c.mask).all())
    for t in (c.ref.out, c.ref.gf, c.ref.gm, c.ref.out_bound, c.ref.gf_bound, c.ref.gm_bound) + tuple(c.emu):
        assert bool(torch.isfinite(t).all())
    up.convex_check(c, *c.emu, _quiet)


def test_convex_reference_is_the_oracles_autograd(oracle_ops):
    N, H, W = 2, 3, 65
    g = torch.Generator().manual_seed(3)
    flow = (3 * torch.randn(N, 2, H, W, generator=g)).float()
    mask = (2 * torch.randn(N, 576, H, W, generator=g)).float()
    gout = torch.randn(N, 2, 8 * H, 8 * W, generator=g)
    r = up.convex_ref(flow, mask, gout)
    f64, m64 = flow.double().requires_grad_(), mask.double().requires_grad_()
    out = oracle_ops.convex_upsample(f64, m64)
    gf, gm = torch.autograd.grad(out, (f64, m64), gout.double())
    for a, b in ((out.detach(), r.out), (gf, r.gf), (gm, r.gm)):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    # and the emulation is an fp32 implementation of the same thing
    e = up.convex_emu(flow, mask, gout)
    for a, b, bound in zip(e, (r.out, r.gf, r.gm), (r.out_bound, r.gf_bound, r.gm_bound)):
        assert float(((a.double() - b).abs() / bound).max()) <= 1


@pytest.mark.parametrize("mut,which", [("no_max", 0), ("clamp_border", 0), ("clamp_border", 2), ("transpose", 0), ("transpose", 2),
                                       ("gflow_no8", 1), ("gm_no_dot", 2)])
@pytest.mark.parametrize("shape", [(2, 1, 5), (2, 3, 65)], ids=str)
def test_convex_faults_fail(shape, mut, which):
    c = up.convex_case(shape)
    bad = up.convex_emu(c.flow, c.mask, c.gout, mut)
    got = [None, None, None]
    got[which] = bad[which]
    assert not torch.equal(bad[which].view(torch.int32), c.emu[which].view(torch.int32))
    with pytest.raises(AssertionError):
        up.convex_check(c, *got, _quiet)


# --------------------------------------------------------------------------- bilinear
BIL = [(s, f) for s in up.BILINEAR_SHAPES for f in up.FACTORS]


@pytest.mark.parametrize("shape,f", BIL, ids=str)
def test_bilinear_emulation_passes_the_gates(record_property, shape, f):
    P, H, W = shape
    x, _ = up.bilinear_inputs(shape, f)
    for mul in up.MULS:
        for fu in (False, True):
            y = up.bilinear_fwd_emu(x, f, mul, fu)
            res = up.bilinear_check_fwd(shape, f, mul, y, record_property, "mul%g_" % mul)
            _note("bilinear_fwd", res)
            for variant in (up.BILINEAR_GOUTS if mul == up.MULS[0] else ("random",)):
                gx = up.bilinear_bwd_emu(up.bilinear_gout(shape, f, variant), H, W, f, mul, fu)
                rb = up.bilinear_check_bwd(shape, f, mul, variant, gx, record_property, "mul%g_" % mul)
                _note("bilinear_bwd", rb)
                if variant == "random":
                    a = up.adjoint_ratio(shape, f, mul, y, gx, res[2], rb[2])
                    record_property("mul%g_adjoint_ratio" % mul, "%.3g" % a)
                    assert a <= 1, a


def test_positions_differ_only_where_rscale_is_inexact():
    for f in up.FACTORS:
        a, b = up.positions(129 * f, f, False), up.positions(129 * f, f, True)
        if f in (1, 2, 4, 8):
            assert torch.equal(a, b)
            assert torch.equal(a.double(), (torch.arange(129 * f).double() + 0.5) / f - 0.5)
        else:
            assert not torch.equal(a, b)
        assert float((a.double() - ((torch.arange(129 * f).double() + 0.5) / f - 0.5)).abs().max()) <= 129 * 2.0 ** -22


@pytest.mark.parametrize("shape,f", BIL, ids=str)
def test_bilinear_reference_is_interpolates_autograd(shape, f):
    P, H, W = shape
    x, g = up.bilinear_inputs(shape, f)
    x64 = x.double().unsqueeze(0).requires_grad_()
    y = 20.0 * Fn.interpolate(x64, scale_factor=f, mode="bilinear", align_corners=False)
    (gx,) = torch.autograd.grad(y, x64, g.double().unsqueeze(0))
    r = up.bilinear_ref(shape, f, 20.0)
    tol = 1e-12 if f in (1, 2, 4, 8) else 2.0 ** -21 * max(H, W)          # the positions' fp32 rounding times a slope
    for fu in (False, True):
        assert float((y.detach()[0] - r[fu].out).abs().max()) <= tol * 20 * 2 * float(x.abs().max())
        assert float((gx[0] - r[fu].gin).abs().max()) <= tol * 20 * 2 * float(g.abs().max()) * (f + 1) ** 2


@pytest.mark.parametrize("mut", ["align_corners", "no_clamp"])
@pytest.mark.parametrize("f", [2, 3, 5])
def test_bilinear_position_faults_fail(mut, f):
    shape = (2, 7, 5)
    P, H, W = shape
    x, g = up.bilinear_inputs(shape, f)
    with pytest.raises(AssertionError):
        up.bilinear_check_fwd(shape, f, 20.0, up.bilinear_fwd_emu(x, f, 20.0, False, mut), _quiet)
    with pytest.raises(AssertionError):
        up.bilinear_check_bwd(shape, f, 20.0, "random", up.bilinear_bwd_emu(g, H, W, f, 20.0, False, mut=mut), _quiet)


@pytest.mark.parametrize("f", [5, 8])
@pytest.mark.parametrize("side", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["y_below", "y_above", "x_below", "x_above"])
def test_bilinear_short_window_fails(f, side):
    shape = (2, 7, 5)
    P, H, W = shape
    x, g = up.bilinear_inputs(shape, f)
    y = up.bilinear_fwd_emu(x, f, 20.0, False)
    good = up.bilinear_bwd_emu(g, H, W, f, 20.0, False)

    def cut(n):
        c = [[0, 0], [0, 0]]
        c[side[0]][side[1]] = n
        return up.bilinear_bwd_emu(g, H, W, f, 20.0, False, cut=c)

    n = 1
    assert torch.equal(cut(1).view(torch.int32), good.view(torch.int32)), "one output short is no equivalent mutant any more"
    while torch.equal(cut(n).view(torch.int32), good.view(torch.int32)):
        n += 1
        assert n < 3 * f
    bad = cut(n)
    with pytest.raises(AssertionError):
        up.bilinear_check_bwd(shape, f, 20.0, "random", bad, _quiet)
    assert up.adjoint_ratio(shape, f, 20.0, y, good, False, False) <= 1 < up.adjoint_ratio(shape, f, 20.0, y, bad, False, False)


# --------------------------------------------------------------------------- nearest-4
@pytest.mark.parametrize("shape", up.NEAREST_SHAPES, ids=str)
def test_nearest4_expression(shape):
    for div in (0, 1):
        x, gy, y, gx = up.nearest4_case(shape, div)
        P, H, W = shape
        assert y.shape == (P, 4 * H, 4 * W) and gx.shape == x.shape
        assert torch.equal(y[:, ::4, ::4], x / 20.0 if div else x * 20.0) and torch.equal(y[:, 3::4, 3::4], y[:, ::4, ::4])
