"""The references, emulations, case tables and bounds of tests/test_lbfgs_f64_gpu.py and tests/test_attack_math_f64_gpu.py
(tests/optim.py) on the CPU (no GPU).

Every case reaches the classes its name promises (the census); the float64 substitutions are the two-loop recursion; the
fp32 emulations -- and, where there is one, a second fp32 implementation that shares only the formula with the emulation --
pass every gate against float64; and each of the seven one-line faults of optim.MUTANTS, put into the emulation, fails a gate
on a named case while agreeing with the emulation up to the place where it bites.  So a kernel that misses a gate is wrong and
not merely differently rounded, and a kernel with one of these faults cannot pass.
"""
import numpy as np
import pytest
import torch

from oracle import ops as oracle_ops
from tests import optim as op
from tests.fenced import TINY, U, gamma

torch.set_num_threads(min(16, torch.get_num_threads()))
F32, F64 = torch.float32, torch.float64
CASE = {c.name: c for c in op.GRAM_CASES}
LOOP = {c.name: c for c in op.LOOP_CASES}


# --------------------------------------------------------------------------- L-BFGS, Gram form
def test_gram_sizes_reach_their_classes():
    seen = {c.name: op.gram_census(c) for c in op.GRAM_CASES}
    assert {"nblk3", "last_block_ok1_false", "padded"} <= seen["rows_to_128"]          # ld4 = 1025: 512 + 512 + 1
    assert "ld4_is_1" in seen["smallest_n4"] and "padded" not in seen["smallest_n4"]
    assert "padded" in seen["smallest_n5"] and "nblk1" in seen["smallest_n8"]
    assert "last_block_full" in seen["block_edges_2048"] and "nblk1" in seen["block_edges_2048"]
    assert {"last_block_ok1_false", "nblk2"} <= seen["block_edges_3072"]
    assert {"nblk293", "reduce_second_trip", "final_second_trip", "padded"} <= seen["many_blocks"]
    assert all("reduce_second_trip" not in s for n, s in seen.items() if n != "many_blocks")
    assert 128 * 128 * 8 + 4 * 128 * 8 == 135168


def test_rows_to_128_reaches_every_m():
    steps, reached = op.gram_trajectory(CASE["rows_to_128"], "indep")
    assert {"m%d" % m for m in range(129)} <= reached
    assert {"prefetch_rem%d" % r for r in range(4)} <= reached and "staged16" in reached and "second_lane_row" in reached
    assert {"rejected_at_empty", "rejected_at_partial", "wrap", "first_nonzero"} <= reached
    assert [s.m for s in steps if not s.accepted] == [0, 4, 62, 127]


def test_workload_cap_wraps_30_times():
    steps, reached = op.gram_trajectory(CASE["workload_cap"], "corr")
    assert steps[-1].header == (30, 100, 1, 101) and "second_lane_row" in reached


def test_small_rings_reach_their_classes():
    steps, reached = op.gram_trajectory(CASE["reject_on_full"], "indep")
    assert "rejected_at_full" in reached and steps[7].header == (2, 5, 0, 6) and steps[8].header == (3, 5, 1, 6)
    for name, m in (("second_row_edge_64", 64), ("second_row_edge_65", 65)):
        steps, reached = op.gram_trajectory(CASE[name], "indep")
        assert steps[-1].m == m and steps[-1].header[0] == 80 - m and ("second_lane_row" in reached) == (m == 65)
    steps, reached = op.gram_trajectory(CASE["smallest_n4"], "indep")
    assert [s.header[:2] for s in steps] == [(0, 1), (1, 1), (0, 1), (1, 1)]            # a two-row ring


@pytest.mark.parametrize("kind", op.KINDS)
def test_substitutions_equal_two_loop(kind):
    """d64 of the textbook recursion = cg g + sum cS_k s_k + cY_k y_k with the float64 coefficients of optim.substitute"""
    for name in ("block_edges_2048", "second_row_edge_65"):
        case = CASE[name]
        steps, _ = op.gram_trajectory(case, kind)
        book = op.RefBook(case.cap)
        for st, (grad, _, _) in zip(steps, op.feed_inputs(case, kind)):
            book.update(st.s32.double(), st.y32.double())
            m = st.m
            d = st.c64[0] * grad[:case.n].double()
            for k, (s, y) in enumerate(book.kept):
                d = d + st.c64[1 + k] * s + st.c64[1 + m + k] * y
            assert op.rel_l2(d, st.d64) < 1e-9, (name, st.feed, op.rel_l2(d, st.d64))


def _plain_two_loop(case, kind):
    """torch.optim.LBFGS's own fp32 operations on the kept pairs, per feed: shares nothing with GramEmu but the formula"""
    book, out = [], []
    H = np.float32(1)
    for grad, g_prev, d in op.feed_inputs(case, kind):
        s, y = (d * np.float32(op.T_STEP))[:case.n], (grad - g_prev)[:case.n]
        ys = np.float32(float((y * s).sum()))
        if ys > 1e-10:
            book = (book + [(s, y, np.float32(1) / ys)])[-case.cap:]
            H = ys / np.float32(float((y * y).sum()))
        if book:
            out.append(op.two_loop_f32(grad[:case.n], [(s_, y_) for s_, y_, _ in book], [r for _, _, r in book], H)[0])
        else:
            out.append(-grad[:case.n] * H)
    return out


@pytest.mark.parametrize("kind", op.KINDS)
@pytest.mark.parametrize("case", op.GRAM_CASES, ids=lambda c: c.name)
def test_gram_emulation_passes_the_gates(record_property, case, kind):
    steps, _ = op.gram_trajectory(case, kind)
    plain = _plain_two_loop(case, kind)
    worst = [0.0, 0.0, 0.0, 0.0]
    for st, pl in zip(steps, plain):
        ehdr, eH, eys, eyy = st.emu
        assert ehdr == st.header, st.feed       # the kernel's bookkeeping = torch's
        if st.accepted:      # H = fp32(ys) / fp32(yy) of the fp32 sums: their two bounds and the division
            assert abs(eH - st.H) <= (gamma(op.DOT_DEPTH) * (st.ys_abs / st.ys64 + 1) + 3 * U) * st.H
        assert abs(eys - st.ys64) <= gamma(op.DOT_DEPTH) * st.ys_abs
        assert abs(eyy - st.yy64) <= gamma(op.DOT_DEPTH) * st.yy_abs
        assert bool((st.bound > 0).all()) and bool(torch.isfinite(st.bound).all())
        e = op.elem_ratio(st.dE, st.d64, st.bound)
        ep, sp = op.elem_ratio(pl, st.d64, st.bound), op.stat_ratio(pl, st.d64, st.dE)
        worst = [max(a, b) for a, b in zip(worst, (e, ep, sp, op.rel_l2(st.dE, st.d64)))]
        assert e <= 1 and ep <= 1 and sp <= 1, (st.feed, st.m, e, ep, sp)
    for k, v in zip(("emu_elem_ratio", "torch_elem_ratio", "torch_stat_ratio", "emu_rel_l2"), worst):
        record_property(k, "%.3g" % v)
    assert worst[3] < 1e-6          # the statistical gate is a few 1e-6 at the most


def _first_failure(case, kind, mutant):
    good, _ = op.gram_trajectory(case, kind)
    bad, _ = op.gram_trajectory(case, kind, mutant)
    for g, b in zip(good, bad):
        if op.stat_ratio(b.dE, g.d64, g.dE) > 1 or op.elem_ratio(b.dE, g.d64, g.bound) > 1:
            return g, [torch.equal(x.dE, y.dE) for x, y in zip(good[:g.feed], bad[:g.feed])]
    return None, None


def test_mutant_rows_from_64_dropped():
    st, same = _first_failure(CASE["second_row_edge_65"], "indep", "drop_rows_ge_64")
    assert st is not None and st.m == 65 and all(same)           # bites at the first m > 64, nowhere before
    assert _first_failure(CASE["second_row_edge_64"], "indep", "drop_rows_ge_64")[0] is None


@pytest.mark.parametrize("kind", op.KINDS)
def test_mutant_lower_triangle(kind):
    st, same = _first_failure(CASE["block_edges_2048"], kind, "lower_triangle")
    assert st is not None and st.m == 2 and all(same)            # one pair has no off-diagonal


@pytest.mark.parametrize("kind", op.KINDS)
def test_mutant_ring_off_by_one(kind):
    st, same = _first_failure(CASE["block_edges_3072"], kind, "ring_off_by_one")
    assert st is not None and st.header[0] + st.m > 6 and all(same)      # the first feed whose live rows wrap the 6-row ring


def test_mutant_second_trip_of_the_block_sum():
    st, _ = _first_failure(CASE["many_blocks"], "indep", "drop_second_trip")
    assert st is not None
    assert _first_failure(CASE["block_edges_3072"], "indep", "drop_second_trip")[0] is None


# --------------------------------------------------------------------------- L-BFGS, two-loop form
def test_loop_cases_reach_their_classes():
    seen = {c.name: op.loop_census(c) for c in op.LOOP_CASES}
    assert {"n4_second_trip", "tail3", "m_many", "ring_wraps"} <= seen["grid_stride"]
    assert all("n4_zero" in seen["tail_only_n%d_m%d" % (n, m)] for n in (1, 2, 3) for m in (1, 2))
    assert {"tail%d" % t for t in range(4)} <= set().union(*seen.values())
    assert "m1" in seen["one_pair"] and "m1" in seen["tail_only_n2_m1"]
    assert {"full_ring", "ring_wraps"} <= seen["full_ring"]
    assert 1049779 // 4 == 262444 > op.RED_THREADS_TOTAL and 1049779 % 4 == 3


@pytest.mark.parametrize("case", op.LOOP_CASES, ids=lambda c: c.name)
def test_two_loop_emulation_passes_the_gates(record_property, case):
    d64, dE, bound, (g, pairs, ro, H) = op.loop_reference(case)
    d2 = op.two_loop_f32(g, pairs, ro, H, None, True)[0]
    e, e2, s2 = op.elem_ratio(dE, d64, bound), op.elem_ratio(d2, d64, bound), op.stat_ratio(d2, d64, dE)
    record_property("emu_elem_ratio", "%.3g" % e)
    record_property("second_elem_ratio", "%.3g" % e2)
    record_property("second_stat_ratio", "%.3g" % s2)
    record_property("emu_rel_l2", "%.3g" % op.rel_l2(dE, d64))
    assert e <= 1 and e2 <= 1 and s2 <= 1, (e, e2, s2)


@pytest.mark.parametrize("name,mutant", [("grid_stride", "drop_tail"), ("tail_only_n3_m1", "drop_tail"),
                                         ("tail_only_n7", "drop_tail"), ("grid_stride", "drop_second_trip")])
def test_two_loop_mutants_fail(name, mutant):
    d64, dE, bound, (g, pairs, ro, H) = op.loop_reference(LOOP[name])
    bad = op.two_loop_f32(g, pairs, ro, H, mutant)[0]
    assert op.elem_ratio(bad, d64, bound) > 1
    # drop_tail has no statistical gate: 3 elements of a million do not move the norm, fewer than 256 are no statistic
    if mutant == "drop_second_trip":
        assert op.stat_ratio(bad, d64, dE) > 1
        assert torch.equal(op.two_loop_f32(*op.loop_inputs(LOOP["full_ring"]), mutant)[0], op.loop_reference(LOOP["full_ring"])[1])


@pytest.mark.parametrize("n", op.PAIR_NS)
def test_pair_sums_within_the_depth_bound(n):
    g, g_prev, d = op.pair_inputs(n)
    y, s = g - g_prev, d * np.float32(op.T_STEP)
    for a, b in ((y, s), (y, y)):
        want, mag = float(a.double() @ b.double()), float((a.double() * b.double()).abs().sum())
        assert abs(float(torch.dot(a, b)) - want) <= gamma(op.pair_depth(n)) * mag


# --------------------------------------------------------------------------- reductions and the loss
def test_loss_cases_reach_their_classes():
    seen = {c.name: op.loss_census(c) for c in op.LOSS_CASES}
    every = set().union(*seen.values())
    assert {"pix_second_trip", "pred_crop"} <= seen["crop_436"] and 436 * 1024 == 446464
    assert "pred_channels_last" in seen["channels_last"] and "target_expanded" in seen["expanded_target"]
    assert {"delta_second_trip", "n1_ne_n2"} <= seen["long_delta2"] and "bwd_delta_second_trip" in seen["big_delta"]
    assert {"regime_above", "regime_below", "regime_tie", "flow3d", "aee_nan"} <= every
    assert "bwd_flow_second_trip" in seen["bwd_second_trip"] and "bwd_flow_second_trip" not in seen["crop_436"]
    for c in op.LOSS_CASES:
        op.loss_case(c.name)                            # asserts the 1000 x condition of the regime
    assert op.red_depth(446464) == 26 and op.red_depth(7) == 25


def test_one_hot_sums_are_exact_and_see_every_element():
    for N in (op.ONE_HOT_N, 436 * 1024):
        for at in op.RED_ONE_HOT_AT:
            x = torch.zeros(N)
            x[at] = 2.0 ** -3
            assert float(op.strided_sum32(x * x)) == 2.0 ** -6
            dropped = float(op.strided_sum32(x * x, "drop_second_trip"))
            assert (dropped == 0.0) == (at in (262144, -1)), (N, at)        # the fault is seen exactly past the first trip


@pytest.mark.parametrize("f_type", op.F_TYPES)
@pytest.mark.parametrize("case", op.LOSS_CASES, ids=lambda c: c.name)
def test_loss_emulation_passes_the_gates(record_property, case, f_type):
    name = case.name
    po, to, d1, d2, bound = op.loss_case(name)
    b = op.loss_bounds(name, f_type)
    emu = op.loss_fwd_emu(name, f_type)
    for gl in op.GRAD_LOSSES:
        ref, gp, ga, gb = op.loss_ref64(oracle_ops, name, f_type, gl)
        if gl == 1.0:
            r = {"sim": abs(float(emu[1]) - ref["sim"]) / b["sim"], "msq": abs(float(emu[2]) - ref["msq"]) / b["msq"],
                 "loss": abs(float(emu[0]) - ref["loss"]) / op.loss_total_bound(b, ref)}
            for k, v in r.items():
                record_property(k + "_ratio", "%.3g" % v)
                assert v <= 1, (k, v)
            for k, i in (("pt", 3), ("pp", 4), ("tt", 5)):
                assert abs(float(emu[i]) - b["sums"][k]) <= gamma(b["D"] + 2 + op.TERM_R[k]) * b["abs"][k]
        egp, ega, egb = op.loss_bwd_emu(name, f_type, gl, emu)
        egp = egp[0] if po.dims3 else egp
        nan = torch.isnan(gp)
        assert torch.equal(torch.isnan(egp), nan) and bool(torch.isfinite(egp[~nan]).all())
        assert bool(nan.any()) == (f_type == "aee" and case.equal_pixels > 0)
        bd = op.flow_grad_bound(name, f_type, gp, gl)
        assert float(((egp.double() - gp).abs() / bd)[~nan].max()) <= 1
        for e_, g_ in ((ega, ga), (egb, gb)):
            if case.regime == "below":
                assert float(e_.abs().max()) == 0.0 and float(g_.abs().max()) == 0.0
            else:
                assert float(((e_.double() - g_).abs() / (gamma(4) * g_.abs() + TINY)).max()) <= 1


def test_tie_is_half_and_the_mutant_is_not():
    po, to, d1, d2, bound = op.loss_case("tie")
    emu = op.loss_fwd_emu("tie", "mse")
    assert float(emu[2]) == 0.25 and float(emu[6]) == 0.0
    ref, _, ga, gb = op.loss_ref64(oracle_ops, "tie", "mse")
    assert ref["arg"] == 0.0
    full = op.MU / (d1.numel() + d2.numel()) * 2 * d1.double()
    assert torch.allclose(ga, 0.5 * full, rtol=1e-12, atol=0)           # float64 autograd of torch.max at the tie: half
    _, ega, _ = op.loss_bwd_emu("tie", "mse", 1.0, emu)
    _, bad, _ = op.loss_bwd_emu("tie", "mse", 1.0, emu, "sel_one_at_tie")
    gate = lambda x: float(((x.double() - ga).abs() / (gamma(4) * ga.abs() + TINY)).max())   # noqa: E731
    assert gate(ega) <= 1 < gate(bad)


def test_mutant_second_trip_of_a_reduction():
    """crop_436: 184,320 of 446,464 pixels are second-trip elements; the value gate of every sum sees them missing"""
    b = op.loss_bounds("crop_436", "aee")
    ref, _, _, _ = op.loss_ref64(oracle_ops, "crop_436", "aee")
    bad = op.loss_fwd_emu("crop_436", "aee", "drop_second_trip")
    assert abs(float(bad[1]) - ref["sim"]) > b["sim"]
    b = op.loss_bounds("long_delta2", "mse")
    ref, _, _, _ = op.loss_ref64(oracle_ops, "long_delta2", "mse")
    assert abs(float(op.loss_fwd_emu("long_delta2", "mse", "drop_second_trip")[2]) - ref["msq"]) > b["msq"]


# --------------------------------------------------------------------------- element-wise kernels
def test_ew_shapes_reach_their_classes():
    seen = [op.ew_census(s) for s in op.EW_SHAPES]
    assert seen[0] == {"total_second_trip", "sample_one_trip"} and seen[1] == {"total_second_trip", "sample_second_trip"}
    assert seen[2] == seen[3] == {"total_one_trip", "sample_one_trip"}


@pytest.mark.parametrize("shape", op.EW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clipping_is_exact_and_the_edges_occur(shape):
    big = int(np.prod(shape)) > 1000
    for with_delta in (False, True):
        image, delta, go = op.clip_inputs(shape, with_delta)
        x = image + delta if with_delta else image
        assert torch.equal((x * 64).round(), x * 64) and float(x.min()) >= -0.5 and float(x.max()) <= 1.5
        n0, n1 = op.edge_census(x)
        assert min(n0, n1) >= (64 if big else 1), (n0, n1)
        for scale in (1.0, 255.0):
            assert torch.equal(op.box_fwd(image, delta, False, 0., scale, F32), op.box_fwd(image, delta, False, 0., scale, F64).float())
            gi, gd = op.box_bwd(image, delta, go, False, 0., scale, F32)
            wi, wd = op.box_bwd(image, delta, go, False, 0., scale, F64)
            assert torch.equal(gi, wi.float()) and torch.equal(gd, wd.float())
            assert torch.equal(wi.float().double(), wi) and torch.equal(wd.float().double(), wd)       # nothing was rounded
            # float64 autograd of the reference's own expression agrees, pass-through at exactly 0 and 1 included
            xi = image.double().requires_grad_(True)
            dl = delta.double().requires_grad_(True) if with_delta else None
            oracle_ops.box_transform(xi, dl, False, 0., scale).backward(go.double())
            assert torch.equal(xi.grad, wi) and (dl is None or torch.equal(dl.grad, wd))
            on_edge = (x == 0) | (x == 1)
            assert torch.equal(wi[on_edge], (go.double() * scale)[on_edge])
            bad, _ = op.box_bwd(image, delta, go, False, 0., scale, F32, "exclusive_mask")
            assert not torch.equal(bad, wi.float())
        w = x                                           # extract_deltas, clipping
        img = op.clip_inputs(shape, True)[0]
        assert torch.equal(op.deltas_fwd(w, img, False, 0., F32), op.deltas_fwd(w, img, False, 0., F64).float())
        assert torch.equal(op.deltas_bwd(w, go, False, 0., F32), op.deltas_bwd(w, go, False, 0., F64).float())
        assert not torch.equal(op.deltas_bwd(w, go, False, 0., F32, "exclusive_mask"), op.deltas_bwd(w, go, False, 0., F64).float())


@pytest.mark.parametrize("shape", op.EW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_joint_is_exact_and_both_clamps_sit_on_edges(shape):
    nd, imax, imin, go = op.joint_inputs(shape)
    a = nd + imax
    b = a.clamp(0, 1) - imax + imin
    need = 64 if int(np.prod(shape)) > 1000 else 1
    assert min(op.edge_census(a) + op.edge_census(b)) >= need, (op.edge_census(a), op.edge_census(b))
    both = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
    assert int(both.sum()) >= need
    assert torch.equal(op.joint_fwd(nd, imax, imin, F32), op.joint_fwd(nd, imax, imin, F64).float())
    want = op.joint_bwd(nd, imax, imin, go, F64)
    assert torch.equal(op.joint_bwd(nd, imax, imin, go, F32), want.float())
    x = nd.double().requires_grad_(True)
    oracle_ops.extract_deltas_joint(x, imax.double(), imin.double())[0].backward(go.double())
    assert torch.equal(x.grad, want)
    assert torch.equal(want[both], go.double()[both])                   # pass-through where both clamps sit on an edge
    assert not torch.equal(op.joint_bwd(nd, imax, imin, go, F32, "exclusive_mask"), want.float())


@pytest.mark.parametrize("shape", op.EW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_change_of_variables_emulation_passes_the_gates(record_property, shape):
    worst = {}
    for with_delta in (False, True):
        image, delta, go, cls = op.cov_inputs(shape, with_delta)
        x = image + delta if with_delta else image
        ax = x.abs()
        assert bool(((ax <= 4) | (ax >= 12)).all()) and bool(torch.isinf(x).any()) and bool((ax <= 4).any())
        e_t = op.tanh_error(x)
        assert 0 < e_t < 4 * U
        for eps in (0.0, 1e-7):
            for scale in (1.0, 255.0):
                want = op.box_fwd(image, delta, True, eps, scale, F64)
                got = op.box_fwd(image, delta, True, eps, scale, F32)
                assert bool(torch.isfinite(got).all())
                op.fold(worst, "fwd", op.worst_ratio(got, want, 2e-7 * scale))
                gi, gd = op.box_bwd(image, delta, go, True, eps, scale, F32)
                wi, wd = op.box_bwd(image, delta, go, True, eps, scale, F64)
                k = op.box_k_c(eps, F64)[0]
                bi = op.cov_grad_bound(x, go * scale, k, wi, e_t)
                bd = bi.sum(0, keepdim=True) + gamma(shape[0]) * wi.abs().sum(0, keepdim=True)
                op.fold(worst, "grad", op.worst_ratio(gi, wi, bi))
                op.fold(worst, "grad_delta", op.worst_ratio(gd, wd, bd))
                assert float(gi[(ax >= 12)].abs().max()) == 0.0
                xi = image.double().requires_grad_(True)
                oracle_ops.box_transform(xi, None if delta is None else delta.double(), True, eps, scale).backward(go.double())
                assert float((xi.grad - wi).abs().max()) <= 1e-12 * scale * float(go.abs().max())
    for k_, v in worst.items():
        record_property(k_ + "_ratio", "%.3g" % v)
    assert set(worst) == {"fwd", "grad", "grad_delta"}


def test_no_gate_passes_on_a_nan():
    """worst_ratio and fold, which every folded gate goes through: a NaN in the output, or inf - inf, is a failure"""
    want, bound = torch.zeros(5, dtype=F64), torch.ones(5, dtype=F64)
    got = torch.zeros(5)
    assert op.worst_ratio(got, want, bound) == 0.0
    got[3] = float("nan")
    assert op.worst_ratio(got, want, bound) == float("inf") and op.elem_ratio(got, want, bound) == float("inf")
    assert op.worst_ratio(torch.full((5,), float("inf")), want + float("inf"), bound) == float("inf")
    for bad in (float("nan"), float("inf"), 1.5):
        with pytest.raises(AssertionError):
            op.fold({}, "x", bad)
    w = {}
    op.fold(w, "x", 0.25)
    op.fold(w, "x", 0.125)
    assert w == {"x": 0.25}
