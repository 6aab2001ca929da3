"""The plan mirrors, float64 references, kernel-order emulations, inputs and gates of tests/costvol.py on the CPU (no GPU).

Every table case reaches the plan it is listed for, and the tables reach every plan label, slice count, round shape, generic
trigger and ChannelNorm case; lanes >= 1 everywhere; the exact variants meet their exactness condition (asserted where they are
built) and the planted fwd_out covers every plane and the seam columns; the emulation passes both gates against float64 on
every case and variant (the worst ratios are printed, pytest -s, and recorded as junit properties); one-line faults in the
emulation fail the equality gate and the elementwise gate; the references agree with autograd of a direct loop formulation.
"""
import ctypes
import itertools

import pytest
import torch

from pcfa_amd import _hip
from tests import costvol as cv
from tests.fenced import PCFA_ERR_INVALID_ARG

torch.set_num_threads(min(16, torch.get_num_threads()))
F64 = torch.float64
WORST = {}


def _quiet(*_):
    pass


def _note(entry, res):
    w = WORST.setdefault(entry, [0.0, 0.0])
    w[0], w[1] = max(w[0], res[0]), max(w[1], res[1])
    print("%-16s emulation elementwise %.3g, statistical %.3g; worst so far %.3g / %.3g" % ((entry,) + tuple(res) + tuple(w)))


# --------------------------------------------------------------------------- the plans
@pytest.mark.parametrize("case", cv.SC_TABLE, ids=lambda c: c.name)
def test_sampler_cases_reach_their_plans(record_property, case):
    p = cv.scorr_plan(*case.shape)
    record_property("path", p.label)
    assert p.label == case.label
    assert p.lanes >= 1 and p.threads <= 576 and p.lds <= 160 * 1024 and p.cr % p.ns == 0 and p.cr <= p.crmax
    assert sum(p.sizes) == case.shape[1] and p.sizes == cv.SC_SIZES.get(case.name, [case.shape[1]])
    assert cv.sc_is_fast(cv.FAST, case.shape[3]) and cv.sc_out_size(case.shape[2], case.shape[3], cv.FAST) == case.shape[2:]
    n = case.shape[0] * case.shape[1] * case.shape[2] * case.shape[3]
    assert 81 * n <= 160e6 and case.shape[0] * 81 * case.shape[2] * case.shape[3] * 4 <= 10 * 2 ** 20


def test_sampler_table_covers_the_plans():
    plans = {c.name: cv.scorr_plan(*c.shape) for c in cv.SC_TABLE}
    by_tile = {}
    for p in plans.values():
        by_tile.setdefault((p.th, p.tw), set()).add((p.ns, p.rounds))
    assert {t: {ns for ns, _ in v} for t, v in by_tile.items()} == {(2, 16): {1, 2, 4, 8}, (2, 32): {1, 4}, (4, 32): {1, 2}}
    assert all(any(r > 1 for _, r in v) and any(r == 1 for _, r in v) for v in by_tile.values())
    assert [n for n, p in plans.items() if p.clipped] == ["1x270x3x12"]
    assert {p.dead for p in plans.values()} == {True, False}
    assert any(p.sizes[0] != p.sizes[-1] for p in plans.values()) and any(p.cr > sum(p.sizes) for p in plans.values())
    # the three combinations no test ran before
    assert plans["2x64x48x160"].label == "t2x32_ns4_r1" and plans["4x64x48x160"].label == "t4x32_ns2_r2"
    assert plans["1x270x3x12"].sizes == [128, 128, 14]
    # level 2 at KITTI size with two and four pairs per closure: 120 then 240 workgroups, and 240 on the 4-row tile
    assert cv.cdiv(48, 4) * cv.cdiv(160, 32) * 2 == 120 and cv.cdiv(48, 2) * cv.cdiv(160, 32) * 2 == 240
    bw = [cv.scorr_bwd_plan(*c.shape) for c in cv.SC_TABLE]
    assert {q.tail for q in bw} >= {3, 5, 9, 19, 37 % 32, 61 % 32, 0, 81 % 32, 270 % 32}
    assert {q.groups for q in bw} >= {1, 2, 3, 5, 7, 9} and {q.dead for q in bw} == {True, False}
    tall = [cv.scorr_bwd_plan(*cv.SC_CASES[n].shape, bth=4) for n in cv.SC_TALL]
    assert [q.label for q in tall] == ["b4x32_g1_tail5", "b4x32_g2_tail5"] and all(q.ntiles % 8 for q in tall)
    assert cv.SC_WILD in cv.SC_CASES


def test_generic_sampler_cases_leave_the_fast_path():
    assert {c.route for c in cv.SC_GENERIC} == {"params", "w%4", "shift"}
    for c in cv.SC_GENERIC:
        aligned = c.shift == (0, 0)
        assert not cv.sc_is_fast(c.p, c.shape[3], aligned), c.name
        if c.route != "params":             # only the one trigger keeps them off the fast path
            assert cv.sc_is_fast(c.p, c.shape[3] // 4 * 4, True)
        assert cv.sc_out_size(c.shape[2], c.shape[3], c.p) is not None
    rect = [c.p for c in cv.SC_GENERIC if c.route == "params"]
    for field in ("k", "patch", "pad", "dil", "dil_patch", "stride"):
        assert any(getattr(p, field)[0] != getattr(p, field)[1] for p in rect), field
    assert any(p.patch[0] % 2 == 0 and p.patch[1] % 2 == 0 for p in rect)
    assert cv.sc_out_size(2, 9, cv.sampler(k=(3, 1), pad=(0, 0))) is None          # the kernel taller than the padded image


def test_out_size_is_the_mirrors():
    """pcfa_spatial_corr_out_size and pcfa_flownet_corr_out_size are host functions."""
    lib = _hip.load()
    oh, ow, oc = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    for c in cv.SC_GENERIC + [cv._gen(s.name, s.shape, cv.FAST, "fast", "") for s in cv.SC_TABLE]:
        H, W, p = c.shape[2], c.shape[3], c.p
        assert lib.pcfa_spatial_corr_out_size(H, W, *p.k, *p.pad, *p.dil, *p.stride, ctypes.byref(oh), ctypes.byref(ow)) == 0
        assert (oh.value, ow.value) == cv.sc_out_size(H, W, p), c.name
    assert lib.pcfa_spatial_corr_out_size(2, 9, 3, 1, 0, 0, 1, 1, 1, 1, ctypes.byref(oh), ctypes.byref(ow)) == PCFA_ERR_INVALID_ARG
    for shape, f in [(c.shape, c.f) for c in cv.FC_GENERIC] + [(c.shape, cv.flownet()) for c in cv.FC_FAST]:
        pl = cv.fcorr_plan(*shape, f)
        assert lib.pcfa_flownet_corr_out_size(shape[2], shape[3], *cv.fc_args(f), ctypes.byref(oc), ctypes.byref(oh),
                                              ctypes.byref(ow)) == 0
        assert (oc.value, oh.value, ow.value) == (pl.dsize ** 2, pl.oH, pl.oW)
    for bad in (cv.flownet(0, 2, 4, 1, 2), cv.flownet(0, 1, 20, 1, 2)):      # even kernel_size; an empty output
        assert cv.fcorr_plan(1, 4, 8, 8, bad) is None
        assert lib.pcfa_flownet_corr_out_size(8, 8, *cv.fc_args(bad), None, None, None) == PCFA_ERR_INVALID_ARG


def test_flownet_and_channelnorm_tables_cover_the_paths():
    fast = [cv.fcorr_plan(*c.shape, cv.flownet()) for c in cv.FC_FAST]
    assert {p.label for p in fast} == {"fast"} and {p.divide for p in fast} == {"reciprocal", "division"}
    assert {p.tail for p in fast} >= {0, 1, 3} and any(p.tiles_x > 1 for p in fast) and any(p.tiles_y > 1 for p in fast)
    assert all((p.oH, p.oW, p.dsize) == (c.shape[2], c.shape[3], 21) for p, c in zip(fast, cv.FC_FAST))
    assert any(c.shape[2] > 40 and c.shape[3] > 40 for c in cv.FC_FAST)
    # shifted gradients stay on the fast path, a shifted in1 / out or W % 4 != 0 leaves it
    assert cv.fcorr_plan(1, 8, 8, 32, cv.flownet(), aligned=False).label == "generic"
    gen = {c.name: cv.fcorr_plan(*c.shape, c.f, aligned=c.shift == 0) for c in cv.FC_GENERIC}
    assert {p.label for p in gen.values()} == {"generic"} and {c.route for c in cv.FC_GENERIC} == {"params", "stride1", "w%4", "shift"}
    assert cv.fcorr_plan(*cv.FC_GENERIC[-1].shape, cv.flownet()).label == "fast"
    f = cv.flownet(3, 3, 4, 1, 3)
    assert f.pad < f.md and f.md % f.s2 != 0 and gen["pad_lt_md_s2_3"].dsize == 3
    assert [c.backward for c in cv.FC_GENERIC if c.f.s1 != 1] == [False]
    assert cv.CN_TABLE == [(2, 3, 5, 7), (1, 2, 1, 1), (1, 64, 3, 5), (3, 1, 4, 4)]
    zero, big = 0, 0
    for shape, huge in cv.CN_RUNS:
        x, _ = cv.cn_inputs(shape, huge)
        zero, big = zero + bool((x[0, :, 0, 0] == 0).all()), big + (float(x.abs().max()) > 0.99e18)
    assert zero == big == len(cv.CN_TABLE)


# --------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("case", cv.SC_TABLE, ids=lambda c: c.name)
def test_exact_variants_and_planted_masks(case):
    d = cv.sc_data(case.name, "integer")          # asserts exact_ok
    B, C, H, W = case.shape
    assert float(d.in1.abs().max()) <= 4 and float(d.g.abs().max()) <= 2 and bool((d.in1 == d.in1.round()).all())
    for v in (d.scale, d.slope):
        assert v in (0.5, 0.25, 0.125)
    f, where = d.fwd_out, d.planted
    assert bool(where.flatten(2).any(2).all()), "a plane without a planted value"
    cols = cv.plant_columns(W)
    assert {0, W - 1} <= set(cols) and all({x0 - 4, x0 - 1, x0, x0 + 3} & set(range(W)) <= set(cols) for x0 in range(32, W, 32))
    bits = f[where].view(torch.int32)
    want = torch.tensor(cv.SPECIALS).view(torch.int32)
    assert set(bits.tolist()) == set(want.tolist()), "not all of +0, -0, +-2^-126 planted"
    assert bool((d.g.view_as(f)[where & (f == 0)] != 0).any()), "no planted zero meets a nonzero gradient"
    pos = cv.sc_positions(case.name)
    assert {(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)} <= {(p[3], p[4]) for p in pos} and len(pos) <= 16
    p = cv.scorr_plan(*case.shape)
    if W > p.tw:
        assert {p.tw - 1, p.tw} <= {q[4] for q in pos}
    if H > p.th:
        assert {p.th - 1, p.th} <= {q[3] for q in pos}
    assert any(q[1] == min(32, C) - 1 for q in pos)


# --------------------------------------------------------------------------- the emulation passes the gates
@pytest.mark.parametrize("case", cv.SC_TABLE, ids=lambda c: c.name)
def test_sampler_fast_emulation_passes_the_gates(record_property, case):
    for variant in ("random", "integer"):
        d = cv.sc_data(case.name, variant)
        _note("scorr_fast", cv.sc_check(d, cv.sc_emulate(d), record_property))
    fo = cv.sc_data(case.name, "integer").fwd_out
    every = cv.sc_positions(case.name)
    if d.in1.numel() > 500000:              # the emulation walks every channel and tap: corners and one seam pair here,
        every = every[:4] + every[-2:]      # every position on the smaller cases (and, on the GPU, on all of them)
    for k, pos in enumerate(every):
        o = cv.sc_onehot(case.name, pos, fo)
        cv.sc_check(o, cv.sc_emulate_onehot(o), record_property, "pos%d_" % k)


@pytest.mark.parametrize("case", cv.SC_GENERIC, ids=lambda c: c.name)
def test_sampler_generic_emulation_passes_the_gates(record_property, case):
    for variant in ("random", "integer"):
        d = cv.sc_data(case.name, variant)
        _note("scorr_generic", cv.sc_check(d, cv.sc_emulate(d), record_property))
    for k, pos in enumerate(cv.sc_positions(case.name)):
        o = cv.sc_onehot(case.name, pos)
        cv.sc_check(o, cv.sc_emulate_onehot(o), record_property, "pos%d_" % k)


FC_ALL = [(c.name, c.shape, cv.fc_args(cv.flownet())) for c in cv.FC_FAST] + [(c.name, c.shape, cv.fc_args(c.f)) for c in cv.FC_GENERIC]


@pytest.mark.parametrize("name,shape,fargs", FC_ALL, ids=[t[0] for t in FC_ALL])
def test_flownet_emulation_passes_the_gates(record_property, name, shape, fargs):
    d = cv.fc_data(shape, fargs, "random")
    _note("fcorr", cv.fc_check(d, cv.fc_emulate(d), record_property))
    if d.plan.nelems & (d.plan.nelems - 1) == 0 and d.backward:
        e = cv.fc_data(shape, fargs, "integer")
        cv.fc_check(e, cv.fc_emulate(e), record_property)
        for k, pos in enumerate(cv.fc_positions(shape, d.plan.dsize)):
            o = cv.fc_onehot(shape, fargs, pos)
            got = {"fwd": cv.fc_fwd(o.f_in1, o.f_in2, o.f, torch.float32), "bwd": cv.fc_bwd(o.in1, o.in2, o.g, o.f, torch.float32)}
            cv.fc_check(o, got, record_property, "pos%d_" % k)


@pytest.mark.parametrize("shape,huge", cv.CN_RUNS, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_channelnorm_emulation_passes_the_gates(record_property, shape, huge):
    x, dy = cv.cn_inputs(shape, huge)
    norm = cv.cn_ref_fwd(x)[0].float()
    _note("channelnorm", cv.cn_check(shape, huge, cv.cn_emu_fwd(x), cv.cn_emu_bwd(x, norm, dy), record_property))
    if bool((x[0, :, 0, 0] == 0).all()):
        with pytest.raises(AssertionError):        # the 1e-9 left out: 0 / 0 at the all-zero pixel
            cv.cn_check(shape, huge, cv.cn_emu_fwd(x), cv.cn_emu_bwd(x, norm, dy, "no_eps"), _quiet)


# --------------------------------------------------------------------------- one-line faults each fail both gates
MUTANTS = [("halo_shift", "1x3x1x4", "fwd"), ("drop_slice", "1x9x3x20", "fwd"), ("not_mirrored", "1x3x1x4", "bwd"),
           ("mask_ge", "1x3x1x4", "bwd")]


@pytest.mark.parametrize("mut,name,side", MUTANTS)
def test_faults_fail_the_equality_and_the_elementwise_gate(mut, name, side):
    """Each on the smallest case where it applies: one tile (a halo column, the mirrored taps, the mask) and the first
    case with two channel slices."""
    for variant in ("integer", "random"):
        d = cv.sc_data(name, variant)
        good, bad = cv.sc_emulate(d), cv.sc_emulate(d, mut)
        cv.sc_check(d, good, _quiet)
        changed = {k: v for k, v in bad[side].items() if mut != "mask_ge" or k == "fused"}
        with pytest.raises(AssertionError) as err:
            cv.sc_check(d, {"fwd": {}, "bwd": {}, side: changed}, _quiet, emu=good)
        if variant == "random":
            assert "elementwise" in str(err.value), "the statistical gate alone caught it"


def test_a_wrong_flownet_displacement_fails():
    d = cv.fc_data((1, 8, 8, 32), cv.fc_args(cv.flownet()), "integer")
    with pytest.raises(AssertionError):
        cv.fc_check(d, cv.fc_emulate(d, "planes_flipped"), _quiet)


# --------------------------------------------------------------------------- the references against a direct formulation
def _direct_sampler(a, b, p):
    B, C, H, W = a.shape
    oH, oW = cv.sc_out_size(H, W, p)
    rows = []
    for n, ph, pw, h, w in itertools.product(range(B), range(p.patch[0]), range(p.patch[1]), range(oH), range(oW)):
        sU, sV = (ph - (p.patch[0] - 1) // 2) * p.dil_patch[0], (pw - (p.patch[1] - 1) // 2) * p.dil_patch[1]
        s = a.new_zeros(())
        for i, j in itertools.product(range(p.k[0]), range(p.k[1])):
            y1, x1 = h * p.stride[0] - p.pad[0] + i * p.dil[0], w * p.stride[1] - p.pad[1] + j * p.dil[1]
            y2, x2 = y1 + sU, x1 + sV
            if 0 <= y1 < H and 0 <= x1 < W and 0 <= y2 < H and 0 <= x2 < W:
                s = s + (a[n, :, y1, x1] * b[n, :, y2, x2]).sum()
        rows.append(s)
    return torch.stack(rows).view(B, p.patch[0], p.patch[1], oH, oW)


@pytest.mark.parametrize("shape,p", [((1, 2, 4, 5), cv._RECT), ((2, 2, 5, 4), cv._RECT_T), ((1, 2, 3, 4), cv.FAST),
                                     ((1, 1, 4, 6), cv.SC_GENERIC[-1].p)])
def test_sampler_reference_is_autograd_of_the_loops(shape, p):
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(shape, generator=gen, dtype=F64).requires_grad_()
    b = torch.randn(shape, generator=gen, dtype=F64).requires_grad_()
    out = _direct_sampler(a, b, p)
    g = torch.randn(out.shape, generator=gen, dtype=F64)
    ga, gb = torch.autograd.grad(out, (a, b), g, retain_graph=True)
    assert torch.allclose(cv.sc_fwd(a.detach(), b.detach(), p), out.detach(), rtol=1e-13, atol=1e-13)
    w1, w2 = cv.sc_bwd(a.detach(), b.detach(), g, p)
    assert torch.allclose(w1, ga, rtol=1e-13, atol=1e-13) and torch.allclose(w2, gb, rtol=1e-13, atol=1e-13)
    # the fused form: autograd of leaky(scale corr) away from 0
    fo = torch.nn.functional.leaky_relu(0.37 * out, 0.1)
    fa, fb = torch.autograd.grad(fo, (a, b), g)
    (f1, f2), _ = cv.sc_ref_bwd(a.detach(), b.detach(), g, p, fo.detach(), 0.37, 0.1, with_bound=False)
    assert torch.allclose(f1, fa, rtol=1e-13, atol=1e-13) and torch.allclose(f2, fb, rtol=1e-13, atol=1e-13)


def _direct_flownet(a, b, f):
    B, C, H, W = a.shape
    pl = cv.fcorr_plan(B, C, H, W, f)

    def at(t, n, y, x):
        return t[n, :, y, x] if 0 <= y < H and 0 <= x < W else t.new_zeros(C)

    rows = []
    for n, tj, ti, y, x in itertools.product(range(B), range(pl.dsize), range(pl.dsize), range(pl.oH), range(pl.oW)):
        y1, x1 = y * f.s1 + f.md - f.pad, x * f.s1 + f.md - f.pad
        y2, x2 = y1 + (tj - pl.drad) * f.s2, x1 + (ti - pl.drad) * f.s2
        s = a.new_zeros(())
        for j, i in itertools.product(range(-pl.kr, pl.kr + 1), repeat=2):
            s = s + (at(a, n, y1 + j, x1 + i) * at(b, n, y2 + j, x2 + i)).sum()
        rows.append(s / (f.k * f.k * C))
    return torch.stack(rows).view(B, pl.dsize ** 2, pl.oH, pl.oW)


@pytest.mark.parametrize("shape,fargs", [((1, 2, 5, 6), (3, 3, 4, 1, 3)), ((2, 3, 4, 5), (2, 1, 2, 1, 2)), ((1, 2, 6, 7), (4, 1, 4, 2, 2))])
def test_flownet_reference_is_autograd_of_the_loops(shape, fargs):
    f = cv.flownet(*fargs)
    gen = torch.Generator().manual_seed(4)
    a = torch.randn(shape, generator=gen, dtype=F64).requires_grad_()
    b = torch.randn(shape, generator=gen, dtype=F64).requires_grad_()
    out = _direct_flownet(a, b, f)
    assert torch.allclose(cv.fc_fwd(a.detach(), b.detach(), f), out.detach(), rtol=1e-13, atol=1e-13)
    if f.s1 == 1:
        g = torch.randn(out.shape, generator=gen, dtype=F64)
        ga, gb = torch.autograd.grad(out, (a, b), g)
        w1, w2 = cv.fc_bwd(a.detach(), b.detach(), g, f)
        assert torch.allclose(w1, ga, rtol=1e-13, atol=1e-13) and torch.allclose(w2, gb, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 64, 3, 5)])
def test_channelnorm_reference_is_autograd(shape):
    x, dy = cv.cn_inputs(shape)
    x = x.double()
    x[0, :, 0, 0] = 1.0                       # sqrt is not differentiable at the all-zero pixel
    x.requires_grad_()
    norm = (x * x).sum(1, keepdim=True).sqrt()
    (gx,) = torch.autograd.grad(norm, x, dy.double())
    assert torch.allclose(cv.cn_ref_fwd(x.detach())[0], norm.detach(), rtol=1e-14, atol=0)
    want, _ = cv.cn_ref_bwd(x.detach(), norm.detach(), dy)
    assert torch.allclose(want, gx, rtol=1e-8, atol=0)         # the reference's + 1e-9 in the denominator
