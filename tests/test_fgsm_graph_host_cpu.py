"""Host side of the I-FGSM product loop on the CPU port (oracle operator table, which has no `fgsm_step`): the flag, the
refusal of lanes without a GPU, the torch fallback with its history, `steps == 0`, and the census of the step kernel's
crafted cases (tests/fgsm_cases.py; the kernel itself: tests/test_fgsm_step_gpu.py).  The per-lane LRU of the graph cache:
tests/test_graph_sets_cpu.py."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from pcfa_amd import attack_FGSM, ops
from pcfa_amd.helper_functions import logging, losses, ownutilities, parsing_file, targets
from tests import closure_util, fgsm_cases


@pytest.fixture(autouse=True)
def _cpu_port(oracle_ops, monkeypatch):
    monkeypatch.setenv("PCFA_USE_CPU", "1")     # the CPU port, also where a GPU is visible (select_device)
    torch.set_num_threads(8)
    with ops.override_for_testing(oracle_ops):
        yield


def _cli(**kw):
    base = dict(net="SpyNet", weights="random:1234", dataset="Synthetic", dataset_stage="evaluation", small_run=False,
                synthetic_size="64x64", synthetic_pairs=2, dstype="final", output_folder="experiment_data",
                small_save=False, save_frequency=1, no_save=True, unregistered_artifacts=True, joint_perturbation=False,
                steps=2, target="zero", custom_target_path="", loss="mse", epsilon=0.00025, pairs_in_flight=1)
    base.update(kw)
    return Namespace(**base)


def _old_fgsm_attack(model, image1, image2, flow, device, has_gt, args):
    """The per-pair loop as the package ran it before FgsmAttack existed (two fresh leaves per iteration, metrics after
    the last one): what `fgsm_attack` has to keep returning."""
    image1, image2, flow = image1.to(device), image2.to(device), flow.to(device)
    if not ownutilities.model_takes_unit_input(args.net):
        image1, image2 = image1 / 255., image2 / 255.
    padder, [image1, image2] = ownutilities.preprocess_img(args.net, image1, image2)
    nw1 = image1.clone().detach().requires_grad_(True)
    nw2 = image2.clone().detach().requires_grad_(True)

    def predict(a, b):
        out = ownutilities.compute_flow(model, "scaled_input_model", a, b, test_mode=True)
        [out] = ownutilities.postprocess_flow(args.net, padder, out)
        return out

    flow_pred = predict(nw1, nw2)
    flow_pred_init = flow_pred.detach().clone()
    target = targets.get_target(args.target, flow_pred_init, custom_target_path=args.custom_target_path,
                                device=device).to(device)
    res = {"aee_pred-tgt": logging.calc_metrics_const(target, flow_pred_init)}
    delta1 = delta2 = torch.zeros_like(image1)
    for _ in range(args.steps):
        loss = losses.get_loss(args.loss, flow_pred, target)
        model.zero_grad()
        loss.backward()
        nw1, nw2 = attack_FGSM.fgsm_attack_step(nw1, nw2, args.epsilon, nw1.grad.data, nw2.grad.data, clipping=True,
                                                common_perturb=args.joint_perturbation)
        delta1 = torch.clamp(nw1, 0., 1.) - image1
        delta2 = torch.clamp(nw2, 0., 1.) - image2
        nw1 = nw1.detach().requires_grad_(True)
        nw2 = nw2.detach().requires_grad_(True)
        flow_pred = predict(nw1, nw2)
    aee_adv_tgt, aee_adv_pred = logging.calc_metrics_adv(flow_pred.detach(), target, flow_pred_init)
    l2_1, l2_2, l2_12 = logging.calc_delta_metrics(delta1.detach(), delta2.detach())
    res.update({"aee_predadv-tgt": aee_adv_tgt, "aee_pred-predadv": aee_adv_pred, "l2_delta1": l2_1,
                "l2_delta2": l2_2, "l2_delta-avg": l2_12})
    if has_gt:
        res["aee_predadv-gt"] = logging.calc_metrics_adv_gt(flow_pred.detach(), flow)
    return res


def _spynet_pair(seed=0):
    from pcfa_amd.helper_functions.datasets import synthetic_pair
    i1, i2, flow = synthetic_pair(seed, 64, 64)
    return i1[None], i2[None], flow[None]


def test_parser_has_pairs_in_flight():
    parser = parsing_file.create_parser(stage="training", attack_type="fgsm")
    assert parser.parse_args([]).pairs_in_flight == 1
    assert parser.parse_args(["--pairs_in_flight", "3"]).pairs_in_flight == 3


def test_lanes_need_a_gpu():
    with pytest.raises(ValueError, match="--pairs_in_flight needs a GPU"):
        attack_FGSM.attack(_cli(pairs_in_flight=2))


@pytest.mark.parametrize("joint", [False, True])
def test_torch_fallback_returns_todays_values_with_a_history(oracle_ops, joint):
    assert not hasattr(oracle_ops, "fgsm_step")
    args = _cli(joint_perturbation=joint, steps=3)
    dev = torch.device("cpu")
    model = closure_util.load_model("SpyNet", False, dev)
    pair = _spynet_pair()
    want = _old_fgsm_attack(model, *pair, dev, True, args)
    got = attack_FGSM.fgsm_attack(model, *pair, dev, True, args)
    history = got.pop("history")
    assert got == want                                          # the same keys, the same floats
    assert len(history) == 3 and set(history[0]) == set(attack_FGSM.HISTORY_KEYS)
    assert {k: history[-1][k] for k in history[-1]} == {k: want[k] for k in history[-1]}
    assert history[0]["l2_delta-avg"] < history[1]["l2_delta-avg"] < history[2]["l2_delta-avg"] <= 3 * args.epsilon
    st = attack_FGSM.FgsmAttack(model, *pair, 0, dev, True, args)
    assert st.graphed is None and not st.has_step_kernel and st.step_launches == 0
    # and the history went to the metric sink under the reference's names, one record per iteration
    logged = [r for r in logging.SINK.records if r[0] == "l2_delta-avg"]
    assert [r[1] for r in logged[-3:]] == [h["l2_delta-avg"] for h in history]


def test_zero_steps_returns_what_eager_returned():
    args = _cli(steps=0)
    dev = torch.device("cpu")
    model = closure_util.load_model("SpyNet", False, dev)
    pair = _spynet_pair(1)
    want = _old_fgsm_attack(model, *pair, dev, True, args)
    got = attack_FGSM.fgsm_attack(model, *pair, dev, True, args)
    assert got.pop("history") == []
    assert got == want and got["l2_delta-avg"] == 0.0


def test_census_of_the_crafted_step_cases():
    """Every class occurs in both modes, and the classes mean what they say on the torch reference (CPU)."""
    x1, x2, g1, g2, i1, i2 = (torch.from_numpy(a) for a in fgsm_cases.crafted())
    eps32 = float(fgsm_cases.EPS32)
    for joint in (0, 1):
        counts, masks = fgsm_cases.census(joint)
        assert all(counts[c] >= 1 for c in fgsm_cases.CLASSES), (joint, counts)
        p1, p2, d1, d2 = fgsm_cases.torch_reference(x1, x2, g1, g2, i1, i2, fgsm_cases.EPSILON, joint)
        for which, (x, p, d, img) in enumerate(((x1, p1, d1, i1), (x2, p2, d2, i2))):
            m = {c: torch.from_numpy(v) for c, v in masks[which].items()}
            assert bool(torch.isnan(p[m["NaN kept"]]).all()) and bool(torch.isnan(d[m["NaN kept"]]).all())
            assert torch.equal(p[m["unmoved by sign 0"]], x[m["unmoved by sign 0"]])
            assert bool((p[m["clamped at 0"]] == 0).all()) and bool((p[m["clamped at 1"]] == 1).all())
            assert torch.equal(p[m["moved by +eps"]], x[m["moved by +eps"]] + eps32)
            assert torch.equal(p[m["moved by -eps"]], x[m["moved by -eps"]] - eps32)
            ok = ~torch.isnan(p)
            assert torch.equal(d[ok], p[ok] - img[ok])
        covered = sum(masks[0][c].astype(int) for c in fgsm_cases.CLASSES)
        assert covered.min() >= 1                               # every element falls into a class
    # the joint mode's own corners: inf - inf and the half of the smallest subnormal move nothing
    s = (0.5 * (g1 + g2)).sign()
    pairs = list(zip(g1.tolist(), g2.tolist()))
    n_x = len(fgsm_cases.X_VALUES)
    for a, b in ((np.inf, -np.inf), (float(fgsm_cases.SUB), 0.0), (0.0, -float(fgsm_cases.SUB))):
        k = pairs.index((a, b))
        assert bool((s[k:k + n_x] == 0).all())
    k = pairs.index((float(fgsm_cases.BIG), float(fgsm_cases.BIG)))
    assert bool((s[k:k + n_x] == 1).all()) and bool(torch.isinf(g1[k] + g2[k]))
