"""Host side of `--step_norm l2` (attack_FGSM.pgd_l2_attack_step, FgsmAttack._l2_step) on the CPU port, whose operator
table has no `pgd_l2_step`: the flags, the torch statement, the loop's fallback and its budget, the graph key, the claim
that the default makes the calls it made before -- and the checks of tests/pgd_cases.py that have to hold BEFORE
tests/test_pgd_l2_step_gpu.py judges the kernel with them: the census of the case table, the properties on an fp32 CPU
model of the stated sequence over six chained steps, and the two wrong models."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from pcfa_amd import attack_FGSM, ops
from pcfa_amd.helper_functions import logging, parsing_file
from tests import closure_util, pgd_cases
from tests.pgd_cases import SETTINGS, SMALL

torch.set_num_threads(min(16, torch.get_num_threads()))


def _max_threads():
    from pcfa_amd import _hip
    return _hip.load().pcfa_pgd_l2_max_threads()       # a host function: no GPU needed


@pytest.fixture(autouse=True)
def _cpu_port(oracle_ops, monkeypatch):
    monkeypatch.setenv("PCFA_USE_CPU", "1")
    with ops.override_for_testing(oracle_ops):
        yield


def _cli(**kw):
    base = dict(net="SpyNet", weights="random:1234", dataset="Synthetic", dataset_stage="evaluation", small_run=False,
                synthetic_size="64x64", synthetic_pairs=2, dstype="final", output_folder="experiment_data",
                small_save=False, save_frequency=1, no_save=True, unregistered_artifacts=True, joint_perturbation=False,
                steps=2, target="zero", custom_target_path="", loss="mse", epsilon=0.00025, pairs_in_flight=1)
    base.update(kw)
    return Namespace(**base)


def _spynet_pair(seed=0):
    from pcfa_amd.helper_functions.datasets import synthetic_pair
    i1, i2, flow = synthetic_pair(seed, 64, 64)
    return i1[None], i2[None], flow[None]


# ---- flags ---------------------------------------------------------------------------------------------------------------
def test_parser_defaults_choices_and_help():
    parser = parsing_file.create_parser(stage="training", attack_type="fgsm")
    args = parser.parse_args([])
    assert args.step_norm == "sign" and args.delta_bound == 0.005
    args = parser.parse_args(["--step_norm", "l2", "--delta_bound", "0.003"])
    assert args.step_norm == "l2" and args.delta_bound == 0.003
    with pytest.raises(SystemExit):
        parser.parse_args(["--step_norm", "linf"])
    helps = {a.dest: a.help for a in parser._actions}
    assert "NEW" in helps["step_norm"] and "NEW" in helps["delta_bound"]
    # PCFA's own --delta_bound is the flag it was
    pcfa = parsing_file.create_parser(stage="training", attack_type="pcfa")
    assert pcfa.parse_args([]).delta_bound == 0.005 and not hasattr(pcfa.parse_args([]), "step_norm")


# ---- the case table and the models, before the GPU is judged by them --------------------------------------------------------
def test_census_both_branches_occur_and_none_is_marginal():
    counts, margin = pgd_cases.census()
    assert counts["s = 1"] >= 8 and counts["s < 1"] >= 8 and counts["a = 0"] >= 8, counts
    assert margin > 1e-3, margin            # no case sits so close to r == b that fp32 and float64 could take different branches
    active = {(e, b): pgd_cases.statement64(*pgd_cases.table(1025), e, b, 0)["s"] < 1 for e, b in SETTINGS}
    assert set(active.values()) == {True, False}, active


def _torch_step(tab, eps, bound, joint):
    t = [torch.from_numpy(a) for a in tab]
    return attack_FGSM.pgd_l2_attack_step(t[0], t[1], t[2], t[3], t[4], t[5], eps, bound, common_perturb=bool(joint))


@pytest.mark.parametrize("kind", pgd_cases.KINDS)
def test_torch_statement_equals_the_fp32_model_bitwise(kind):
    """attack_FGSM.pgd_l2_attack_step on the CPU is the stated sequence: the same bits as tests/pgd_cases.model32 given the
    same a and s (the sums differ in order only), the same scalars to double rounding."""
    for n in (5, 257, 1025):
        for eps, bound in SETTINGS:
            for joint in (0, 1):
                tab = pgd_cases.table(n, kind)
                p1, p2, d1, d2, (G, a, E, s) = _torch_step(tab, eps, bound, joint)
                m = pgd_cases.model32(*tab, eps, bound, joint, a=a, s=s)
                for got, want in zip((p1, p2, d1, d2), m[:4]):
                    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), (n, kind, eps, joint)
                free = pgd_cases.model32(*tab, eps, bound, joint)[4]
                assert (a, s) == (free[1], free[3])
                for got, want in ((G, free[0]), (E, free[2])):
                    assert (math.isnan(got) and math.isnan(want)) or got == want or abs(got - want) <= 2e-13 * abs(want)


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("gscale", [1.0, 1e-6])
def test_properties_of_the_fp32_model_over_six_chained_steps(gscale, joint):
    """0 <= x <= 1, d == x - img bitwise and the budget b (1 + 2u) + 2u (pgd_cases.budget: derived, not measured) on the
    fp32 CPU model of the stated sequence, for every size and setting, gradients of 1e6 N(0,1) and of N(0,1), six steps
    from the table's iterates with the gradients rotated between steps."""
    worst = 0.0
    for n in SMALL + (4 * 1024 + 5,):
        for eps, bound in SETTINGS:
            x1, x2, g1, g2, i1, i2 = pgd_cases.table(n, "mixed", gscale)
            cap = pgd_cases.budget(bound)
            for k in range(6):
                x1, x2, d1, d2, _ = pgd_cases.model32(x1, x2, np.roll(g1, k), np.roll(g2, 2 * k), i1, i2, eps, bound, joint)
                assert x1.min() >= 0 and x1.max() <= 1 and x2.min() >= 0 and x2.max() <= 1
                assert np.array_equal((x1 - i1).view(np.int32), d1.view(np.int32))
                assert np.array_equal((x2 - i2).view(np.int32), d2.view(np.int32))
                r = pgd_cases.norm64(d1, d2)
                assert r <= cap, (n, eps, bound, k, r, cap)
                if r > pgd_cases.f32(bound):
                    worst = max(worst, (r - pgd_cases.f32(bound)) / (cap - pgd_cases.f32(bound)))
    assert worst < 1.0


def test_the_fp32_model_meets_the_element_bound_and_the_wrong_models_do_not():
    """The stated fp32 sequence stays inside the float64 statement's element bound on every case; a model that forms G from
    g1 alone leaves it.  A model that contracts x - a g into one rounding cannot leave a bound of this kind (pgd_cases: it
    is the better-rounded result), so it is shown to differ from the stated sequence in its bits instead: the comparison the
    GPU test makes with the a and s read back."""
    broken_g = contracted = 0
    for n in SMALL:
        for kind in pgd_cases.KINDS:
            for eps, bound in SETTINGS:
                for joint in (0, 1):
                    tab = pgd_cases.table(n, kind)
                    ref = pgd_cases.statement64(*tab, eps, bound, joint)
                    bnd = pgd_cases.bounds(ref, pgd_cases.sum_depth(n, _max_threads()))
                    good = pgd_cases.model32(*tab, eps, bound, joint)
                    assert (good[4][3] < 1) == (ref["s"] < 1)
                    for name, got, b in zip(("x1", "x2", "d1", "d2"), good[:4], bnd):
                        assert pgd_cases.worst_excess(got, ref[name], b) <= 1.0, (name, n, kind, eps, bound, joint)
                    if kind != "mixed" or n < 255:
                        continue
                    wrong = pgd_cases.model32(*tab, eps, bound, joint, g_from_g1=True)
                    if not joint:        # (under `joint` g1 == g2: half of G scales a by sqrt(2) all the same)
                        assert wrong[4][1] != good[4][1]
                    worst = max(pgd_cases.worst_excess(got, ref[name], b)
                                for name, got, b in zip(("x1", "x2", "d1", "d2"), wrong[:4], bnd))
                    assert worst > 1.0, (n, eps, bound, joint, worst)
                    broken_g += 1
                    fma = pgd_cases.model32(*tab, eps, bound, joint, contract=True)
                    differs = sum(int((g.view(np.int32) != w.view(np.int32)).sum()) for g, w in zip(fma[:4], good[:4]))
                    assert differs > 0, (n, eps, bound, joint)
                    contracted += 1
    assert broken_g == contracted == 4 * len(SETTINGS) * 2


# ---- the loop --------------------------------------------------------------------------------------------------------------
class _Counting:
    """An operator table that counts the calls of the two step kernels and hands everything else through."""

    def __init__(self, inner, steps):
        self._inner, self.calls = inner, {"fgsm_step": 0, "pgd_l2_step": 0}
        for name in steps:
            setattr(self, name, self._counted(name))

    def _counted(self, name):
        def step(x1, x2, g1, g2, image1, image2, d1, d2, epsilon, *rest):
            self.calls[name] += 1
            with torch.no_grad():
                if name == "fgsm_step":
                    p1, p2 = attack_FGSM.fgsm_attack_step(x1, x2, epsilon, g1, g2, clipping=True,
                                                          common_perturb=bool(rest[0]))
                    q1, q2 = p1 - image1, p2 - image2
                else:
                    p1, p2, q1, q2, _ = attack_FGSM.pgd_l2_attack_step(x1, x2, g1, g2, image1, image2, epsilon, rest[0],
                                                                       common_perturb=bool(rest[1]))
                x1.copy_(p1), x2.copy_(p2), d1.copy_(q1), d2.copy_(q2)
        return step

    def __getattr__(self, name):
        return getattr(self._inner, name)


def test_fallback_runs_the_torch_statement_and_every_row_is_inside_the_budget(oracle_ops, monkeypatch):
    assert not hasattr(oracle_ops, "pgd_l2_step")
    calls = []
    real = attack_FGSM.pgd_l2_attack_step
    monkeypatch.setattr(attack_FGSM, "pgd_l2_attack_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    dev = torch.device("cpu")
    model = closure_util.load_model("SpyNet", False, dev)
    for joint in (False, True):
        del calls[:]
        args = _cli(step_norm="l2", epsilon=0.002, delta_bound=0.003, steps=4, joint_perturbation=joint)
        cap = pgd_cases.budget(0.003)
        st = attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, args)
        for _ in range(args.steps):
            st.step()
            assert pgd_cases.norm64(st.delta1.numpy().ravel(), st.delta2.numpy().ravel()) <= cap    # the iterate, in float64
        assert len(calls) == 4 and len(st.history) == 4
        rows = [h["l2_delta-avg"] for h in st.history]
        assert all(0 < r <= cap for r in rows), (rows, cap)              # every history row is inside the budget
        # a step of length epsilon (less what the box clips), then the cap
        assert 0.001 < rows[0] <= 0.002 * (1 + 1e-3) and rows[-1] == pytest.approx(0.003, rel=1e-3)
        got = attack_FGSM.fgsm_attack(model, *_spynet_pair(), dev, True, args)
        assert got["l2_delta-avg"] == rows[-1] and got["history"] == st.history
    assert logging.SINK.params["delta_bound"] == 0.003
    st = attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, args)
    assert st.graphed is None and not st.has_step_kernel and st.step_norm == "l2"


def test_default_args_call_the_signed_step_only(oracle_ops):
    dev = torch.device("cpu")
    model = closure_util.load_model("SpyNet", False, dev)
    table = _Counting(oracle_ops, ("fgsm_step", "pgd_l2_step"))
    with ops.override_for_testing(table):
        st = attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli(steps=3))     # no step_norm, no delta_bound
        assert st.step_norm == "sign" and st.has_step_kernel
        for _ in range(3):
            st.step()
        assert table.calls == {"fgsm_step": 3, "pgd_l2_step": 0} and st.step_launches == 3
        l2 = attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli(steps=2, step_norm="l2", delta_bound=0.005))
        l2.step()
        assert table.calls == {"fgsm_step": 3, "pgd_l2_step": 1}
    plain = attack_FGSM.fgsm_attack(model, *_spynet_pair(), dev, True, _cli(steps=3))
    assert plain["l2_delta-avg"] == st.result()["l2_delta-avg"]


def test_graph_key_names_the_step_rule_and_keeps_the_lane_last():
    dev = torch.device("cpu")
    model = closure_util.load_model("SpyNet", False, dev)
    sign = attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli())
    l2 = attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli(step_norm="l2", delta_bound=0.005))
    other = attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli(step_norm="l2", delta_bound=0.004))
    assert sign.graph_key != l2.graph_key != other.graph_key and len({sign.graph_key, l2.graph_key, other.graph_key}) == 3
    assert sign.graph_key[-1] == l2.graph_key[-1] == 0 and sign.graph_key[-2] == l2.graph_key[-2] == "cpu"
    assert l2.graph_key[-4:-2] == ("l2", 0.005) and sign.graph_key[-4:-2] == ("sign", None)
    with ops.core.lane(3):
        assert attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli(step_norm="l2", delta_bound=0.005)).graph_key[-1] == 3
    with pytest.raises(ValueError, match="step_norm"):
        attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli(step_norm="linf"))
    with pytest.raises(ValueError, match="positive"):
        attack_FGSM.FgsmAttack(model, *_spynet_pair(), 0, dev, True, _cli(step_norm="l2", delta_bound=0.0))
