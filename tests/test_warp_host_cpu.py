"""The position mirrors, the float64 references, the census and the gates of tests/warp.py on the CPU (no GPU).

Every table case reaches the census classes it lists with at least its minimum count, and the band condition on the mask
sum holds (asserted where the inputs are built); the plain fp32 implementation passes every gate against float64 on every
case, flow scale and grad_out variant (the worst ratios are printed, pytest -s, and recorded as junit properties); on the
random-flow cases the fp32 implementation agrees per element, within the same elementwise bounds, with the oracle's
pwc_warp and resample2d and with nets.spynet.backward_warp under autograd -- the position mirrors are the reference's
positions; and one-line faults in the fp32 implementation each fail a gate (floor weights in Resample2d's grad_in1 change
nothing but rounding: shown to be an equivalent mutant, a clamp against the wrong size stands in for it).
"""
import pytest
import torch

from tests import warp as wp

torch.set_num_threads(min(16, torch.get_num_threads()))
IDS = [c.name for c in wp.TABLE]
NEAR = 2.0 ** -18     # cross-check only: pixels this close to an integer position are left out (ATen's scalar remainder)
WORST = {}


def _quiet(*_):
    pass


def _note(entry, res):
    w = WORST.setdefault(entry, [0.0, 0.0])
    w[0], w[1] = max(w[0], res[0]), max(w[1], res[1])
    print("%-14s plain fp32 elementwise %.3g, statistical %.3g; worst so far %.3g / %.3g" % ((entry,) + tuple(res) + tuple(w)))


@pytest.mark.parametrize("case", wp.TABLE, ids=IDS)
def test_cases_reach_their_classes(case):
    """A condition on the table, not a measurement: every listed class at every flow scale, and the band condition
    (asserted by wp.inputs)."""
    for fs in case.fs:
        got = wp.census(case, fs)
        short = {k: (got.get(k, 0), v) for k, v in case.need.items() if got.get(k, 0) < v}
        assert not short, (case.name, fs, short)


def test_table_covers_the_kernel_maps():
    names = {(c.kind, c.shape[2] * c.shape[3] >= 256) for c in wp.TABLE}
    assert names >= {("pwc", False), ("pwc", True), ("spy", False), ("spy", True)}
    assert {wp.channel_groups(c.shape[2] * c.shape[3], c.shape[1]) for c in wp.cases("pwc")} == {1, 2, 4}
    assert any(c.ishape != c.shape[2:] for c in wp.cases("rs"))
    assert {c.thr for c in wp.cases("pwc")} == {wp.THR, 0.25, 0.5}


def test_fused_step_condition_is_checked():
    with pytest.raises(AssertionError):
        wp.fma_half(torch.tensor([2.0 ** 25]), 300)
    with pytest.raises(AssertionError):
        wp.fma_half(torch.tensor([2.0 ** -30]), 9)
    with pytest.raises(AssertionError):
        wp.fma_half(torch.tensor([float("nan")]), 9)


@pytest.mark.parametrize("case", wp.TABLE, ids=IDS)
def test_fp32_passes_the_gates(record_property, case):
    det = case.ishape == case.shape[2:]          # the fixed-point Resample2d backward takes in1 of the flow's size
    for fs in case.fs:
        _note(case.kind + "_fwd", wp.check_fwd(case, fs, wp.fp32_fwd(case, fs), record_property, "fs%g_fwd_" % fs))
        for variant in wp.GOUTS:
            for fixed in ((True, False) if variant in ("one", "zero") else (True,)):
                if fixed and not det:
                    continue
                gx, gf = wp.fp32_bwd(case, fs, variant, fixed)
                a, b = wp.check_bwd(case, fs, variant, gx, gf, fixed, record_property,
                                    "fs%g_%s_%s_" % (fs, variant, "fix" if fixed else "atomic"))
                _note(case.kind + ("_gx_fix" if fixed else "_gx_atomic"), a)
                _note(case.kind + "_gflo", b)


# --------------------------------------------------------------------------- the mirrors are the reference's positions
def _near(pos):
    ix, iy = (p.double() for p in pos)
    return ((ix - ix.round()).abs() < NEAR) | ((iy - iy.round()).abs() < NEAR)


def _ratio(got, want, bound, keep):
    r = (got.double() - want).abs() / bound
    return float(torch.where(keep.expand_as(r), r, torch.zeros_like(r)).max())


def _cross(case, fs, out, gx, gf):
    """out, grad_x, grad_flo of the reference implementation within the elementwise bounds of the float64 references,
    on every pixel not within 2^-18 of an integer position and every texel no such pixel reaches."""
    r, rb = wp.ref(case, fs), wp.ref_bwd(case, fs, "one")
    B, C, H, W = case.shape
    iH, iW = case.ishape
    near = _near(r.pos)
    assert float(near.double().mean()) <= 0.01, "more than 1 % of the pixels next to an integer position"
    keep = ~near.unsqueeze(1)
    n = wp.N_RS_FWD if case.kind == "rs" else wp.N_FWD
    assert _ratio(out, r.out, 2 * wp.gamma(n + 2) * r.P + (n + 2) * wp.TINY, keep) <= 1
    assert _ratio(gf, rb.gf, wp.bound_gf(case, rb.b), keep) <= 1
    touched = torch.zeros(B, 1, iH, iW, dtype=torch.bool)
    for b, y, x in near.nonzero().tolist():
        py, px = int(r.pos[1][b, y, x].floor()), int(r.pos[0][b, y, x].floor())
        touched[b, 0, max(py - 1, 0):py + 3, max(px - 1, 0):px + 3] = True
        if case.kind == "rs":      # clamped neighbours
            touched[b, 0, min(max(py, 0), iH - 1), :] = True
    assert _ratio(gx, rb.gx, wp.bound_gx(rb.b, rb.unit, False), ~touched) <= 1


@pytest.mark.parametrize("case", wp.cases("pwc", random=True), ids=lambda c: c.name)
def test_pwc_positions_are_the_oracles(oracle_ops, case):
    for fs in case.fs:
        x, flo = (t.clone().requires_grad_() for t in wp.inputs(case, fs))
        out = oracle_ops.pwc_warp(x, flo, mask_threshold=case.thr, flow_scale=fs)
        gx, gf = torch.autograd.grad(out, (x, flo), wp.gout(case))
        _cross(case, fs, out.detach(), gx, gf)


def _pow2(n):
    return n & (n - 1) == 0


# the network divides the flow by (size - 1) / 2; ATen's GPU division by a scalar, the kernels and the mirror multiply by
# the fp32 reciprocal.  On the CPU the two are the same operation only where (size - 1) / 2 is a power of two.
SPY_EXACT = [c for c in wp.cases("spy", random=True) if _pow2((c.shape[2] - 1) // 2) and _pow2((c.shape[3] - 1) // 2)
             and c.shape[2] % 2 and c.shape[3] % 2]


@pytest.mark.parametrize("case", SPY_EXACT, ids=lambda c: c.name)
def test_spynet_positions_are_the_networks(case):
    from pcfa_amd.nets.spynet import backward_warp
    assert len(SPY_EXACT) >= 4 and {c.shape[2] * c.shape[3] >= 256 for c in SPY_EXACT} == {False, True}
    x, flo = (t.clone().requires_grad_() for t in wp.inputs(case))
    out = backward_warp(x, flo)
    gx, gf = torch.autograd.grad(out, (x, flo), wp.gout(case))
    _cross(case, 1.0, out.detach(), gx, gf)


@pytest.mark.parametrize("case", wp.cases("rs", random=True), ids=lambda c: c.name)
def test_resample2d_is_the_oracles(oracle_ops, case):
    x, flow = wp.inputs(case)
    out = oracle_ops.resample2d_forward(x, flow)
    g1, g2 = oracle_ops.resample2d_backward(x, flow, wp.gout(case))
    _cross(case, 1.0, out, g1, g2)


# --------------------------------------------------------------------------- the gates bite
def _fails(check):
    try:
        check()
    except AssertionError:
        return True
    return False


def _mut_fwd(mut, cases):
    return sum(_fails(lambda: wp.check_fwd(c, fs, wp.fp32_fwd(c, fs, mut), _quiet)) for c in cases for fs in c.fs)


def _mut_bwd(mut, cases, fixed=True):
    return sum(_fails(lambda: wp.check_bwd(c, fs, "one", *wp.fp32_bwd(c, fs, "one", fixed, mut), fixed, _quiet))
               for c in cases for fs in c.fs)


def test_mutation_mask_greater_than():
    """`>` for `>=` at the mask: the pixels exactly on the threshold."""
    assert _mut_fwd("mask_gt", [c for c in wp.cases("pwc") if c.builder == "threshold"]) >= 1
    assert _mut_bwd("mask_gt", [c for c in wp.cases("pwc") if c.builder == "threshold"]) >= 1


def test_mutation_east_tap_one_past_the_row():
    """`x0 + 1 <= W` for `< W`: the east taps at x0 = W - 1 read the next row."""
    assert _mut_fwd("x1_le_W", [c for c in wp.cases("pwc") if c.builder == "edges"]) >= 1
    assert _mut_bwd("x1_le_W", [c for c in wp.cases("spy") if c.builder == "edges"]) >= 1


def test_mutation_ragged_pass_drops_its_last_channel():
    assert _mut_bwd("drop_tail", [c for c in wp.cases(window=True) if c.kind != "rs" and c.shape[1] % 4]) >= 1


def test_floor_weights_in_grad_in1_are_an_equivalent_mutant():
    """Floor fractions in place of the truncation fractions xf - (int)xf change grad_in1 by rounding only, so no gate can
    fail on them: the two differ for xf < 0 alone, and there both neighbours are clamped to texel 0, which receives
    (1 - a) + a = 1 times the y weight whatever a is (the same along y).  Asserted in float64 on every Resample2d case;
    the fault that does move grad_in1 -- neighbours clamped against the flow's size -- fails the gates."""
    for c in wp.cases("rs"):
        r = wp.ref(c)
        want = wp.ref_bwd(c).gx
        got = wp.rs_bwd(r.x, *r.pos, wp.gout(c), mut="rs_floor_weights")[0]
        assert float((got - want).abs().max()) <= 1e-13 * float(wp.ref_bwd(c).b.S.max())
    assert any(bool((r.pos[0] < 0).any()) and bool((r.pos[1] < 0).any()) for r in map(wp.ref, wp.cases("rs")))
    assert _mut_bwd("rs_floor_weights", wp.cases("rs")) == 0
    assert _mut_bwd("rs_clamp_flow_size", [c for c in wp.cases("rs") if c.ishape != c.shape[2:]], fixed=False) >= 1


def test_mutation_spynet_clamp_mask_omitted():
    assert _mut_bwd("spy_no_clamp_mask", wp.cases("spy")) >= 1


def test_mutation_scatter_drops_window_column_31():
    assert _mut_bwd("drop_lx31", [c for c in wp.cases(window=True) if c.kind != "rs"]) >= 1


def test_gates_catch_one_texel():
    """One wrong texel of a 40 x 72 plane (invisible to a global rel_l2 < 2e-5) fails the elementwise gate."""
    case = wp.CASES["pwc-1x16x40x72-smooth"]
    gx, gf = wp.fp32_bwd(case, 1.0, "one", True)
    gx = gx.clone()
    gx[0, 7, 20, 36] *= 1 + 2.0 ** -14
    with pytest.raises(AssertionError):
        wp.check_bwd(case, 1.0, "one", gx, gf, True, _quiet)
