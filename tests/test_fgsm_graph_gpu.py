"""attack_FGSM.FgsmAttack on the MI355X: the captured loop (forward graph, loss + backward graph, one step kernel per
iteration, metrics in a device buffer) against the eager loop written out below from public pieces -- bit for bit, since
both run the same deterministic kernels in the same order -- and what the product loop needs around it: graph reuse,
pairs in flight, no host traffic per iteration, artefacts."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from pcfa_amd import attack_FGSM, attack_PCFA, graphed
from pcfa_amd.helper_functions import datasets, logging, losses, ownutilities, targets
from tests import closure_util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SIZES = {"RAFT": (128, 160), "PWCNet": (64, 96)}      # the sizes of the closure tests


def _args(net, joint=False, loss="aee", steps=3, **kw):
    base = dict(net=net, weights="random:%d" % closure_util.WEIGHT_SEED, dataset="Synthetic", dataset_stage="evaluation",
                small_run=False, synthetic_size="%dx%d" % SIZES[net], synthetic_pairs=2, dstype="final",
                output_folder="experiment_data", small_save=False, save_frequency=1, no_save=True,
                unregistered_artifacts=True, joint_perturbation=joint, steps=steps, epsilon=0.00025, target="zero",
                custom_target_path="", loss=loss, pairs_in_flight=1)
    base.update(kw)
    return Namespace(**base)


def _pair(net, seed):
    """(image1, image2, flow) as the synthetic loader hands them over: [1,3,H,W] in 0..255 and [1,2,H,W]."""
    h, w = SIZES[net]
    i1, i2, flow = datasets.synthetic_pair(seed, h, w)
    return i1[None], i2[None], flow[None]


def _model(net):
    return closure_util.load_model(net, False, DEV)


def eager_reference(model, image1, image2, flow_gt, args):
    """attack_FGSM.py:150-247 iteration by iteration in eager torch + the package's public helpers; the metrics of every
    iteration as the reference logs them (:199-241)."""
    image1, image2, flow_gt = image1.to(DEV), image2.to(DEV), flow_gt.to(DEV)
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
    flow_init = flow_pred.detach().clone()
    target = targets.get_target(args.target, flow_init, custom_target_path=args.custom_target_path, device=DEV).to(DEV)
    result = {"aee_pred-tgt": logging.calc_metrics_const(target, flow_init)}
    history = []
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
        aee_adv_tgt, aee_adv_pred = logging.calc_metrics_adv(flow_pred.detach(), target, flow_init)
        l2_1, l2_2, l2_12 = logging.calc_delta_metrics(delta1.detach(), delta2.detach())
        history.append({"aee_predadv-tgt": aee_adv_tgt, "aee_pred-predadv": aee_adv_pred,
                        "aee_predadv-gt": logging.calc_metrics_adv_gt(flow_pred.detach(), flow_gt), "l2_delta1": l2_1,
                        "l2_delta2": l2_2, "l2_delta-avg": l2_12})
    result.update(history[-1])
    return {"delta1": delta1.detach(), "delta2": delta2.detach(), "flow": flow_pred.detach(), "history": history,
            "result": result}


def _run(model, pair, args, batch=0, **kw):
    st = attack_FGSM.FgsmAttack(model, pair[0], pair[1], pair[2], batch, DEV, True, args, **kw)
    for _ in range(args.steps):
        st.step()
    return st


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_equal_runs(st, want):
    """want: a dict of eager_reference or another FgsmAttack."""
    if not isinstance(want, dict):
        want = {"delta1": want.delta1, "delta2": want.delta2, "flow": want.flow_pred, "history": want.history,
                "result": want.result()}
    for name, got, ref in (("delta1", st.delta1, want["delta1"]), ("delta2", st.delta2, want["delta2"]),
                           ("flow", st.flow_pred, want["flow"])):
        assert _same_bits(got, ref), "%s: %d of %d elements differ" % (name, int((got != ref).sum()), ref.numel())
    assert len(st.history) == len(want["history"]) > 0
    for i, (got, ref) in enumerate(zip(st.history, want["history"])):
        assert got == ref, (i, got, ref)                      # floats compared exactly, names included
    assert st.result() == want["result"]


@pytest.mark.parametrize("loss", ["aee", "mse"])
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("net", ["RAFT", "PWCNet"])
def test_graph_loop_equals_eager_bitwise(net, joint, loss):
    args = _args(net, joint, loss)
    model, pair = _model(net), _pair(net, 3)
    want = eager_reference(model, *pair, args)
    st = _run(model, pair, args, use_graph=True, reuse_graphs=False)
    assert st.graphed is not None, "capture failed: the eager loop ran"
    assert st.step_launches == args.steps
    assert (st.graphed.forwards, st.graphed.backwards) == (args.steps + 1, args.steps)
    assert float(st.delta1.abs().max()) > 0                    # the images moved
    _assert_equal_runs(st, want)


def test_eager_loop_of_the_class_equals_the_reference_loop(monkeypatch):
    """PCFA_HIP_GRAPH=0: the class's eager loop (step kernel, no graphs) gives the same bits."""
    monkeypatch.setenv("PCFA_HIP_GRAPH", "0")
    args = _args("PWCNet", True, "aee")
    model, pair = _model("PWCNet"), _pair("PWCNet", 4)
    st = _run(model, pair, args)
    assert st.graphed is None and st.step_launches == args.steps
    _assert_equal_runs(st, eager_reference(model, *pair, args))


def test_second_pair_reuses_the_graphs(monkeypatch):
    captures = []
    init = graphed.SplitGraphedStep.__init__
    monkeypatch.setattr(graphed.SplitGraphedStep, "__init__",
                        lambda self, *a, **k: (captures.append(1), init(self, *a, **k))[1])
    args = _args("RAFT", False, "aee", steps=2, epsilon=0.0003)   # an epsilon no other test uses: a key of its own
    model, a, b = _model("RAFT"), _pair("RAFT", 5), _pair("RAFT", 6)
    first = _run(model, a, args, use_graph=True, reuse_graphs=True)
    assert len(captures) == 1 and not first.graphs_reused
    kept = model._pcfa_fgsm_graphs[first.graph_key]
    assert kept.captures == 1 and kept.pairs == 1 and kept.graphed is first.graphed
    first_delta, first_result = first.delta1.clone(), first.result()
    second = _run(model, b, args, batch=1, use_graph=True, reuse_graphs=True)
    assert second.graphs_reused and len(captures) == 1 and kept.captures == 1 and kept.pairs == 2
    assert second.graphed is kept.graphed
    assert first.retired and first.graphed is None
    with pytest.raises(RuntimeError, match="retired"):
        first.step()
    assert _same_bits(first.delta1, first_delta) and first.result() == first_result   # its results stay readable
    fresh = _run(model, b, args, batch=1, use_graph=True, reuse_graphs=False)
    assert len(captures) == 2 and not fresh.graphs_reused
    _assert_equal_runs(second, fresh)
    assert "_pcfa_pair_graphs" not in model.__dict__ or first.graph_key not in model._pcfa_pair_graphs   # PCFA's cache: untouched


def test_two_pairs_in_flight_equal_their_solo_runs():
    args = _args("RAFT", False, "aee")
    model, pairs = _model("RAFT"), [_pair("RAFT", 7), _pair("RAFT", 8)]
    solo = [_run(model, p, args, batch=k, use_graph=True, reuse_graphs=False) for k, p in enumerate(pairs)]
    # `step()` does not wait for the GPU, and a lane is ONE stream-ordered sequence of launches (its scratch buffers are
    # shared by everything the lane runs): the solo runs, lane 0 on the default stream, have to be finished before lane 0
    # goes on on its run stream -- as they are in the driver, which reads every pair's result before the next group starts
    torch.cuda.synchronize()
    flight = attack_PCFA.PairsInFlight(
        lambda k: attack_FGSM.FgsmAttack(model, pairs[k][0], pairs[k][1], pairs[k][2], k, DEV, True, args, use_graph=True),
        2, DEV)
    flight.run(args.steps)
    for k in range(2):
        assert flight.attacks[k].graphed is not None and flight.attacks[k].graph_key[-1] == k
        _assert_equal_runs(solo[k], eager_reference(model, *pairs[k], args))
        _assert_equal_runs(flight.attacks[k], solo[k])


def test_driver_pairs_in_flight_returns_the_same_dict():
    one = attack_FGSM.attack(_args("RAFT", False, "mse", steps=2, synthetic_pairs=3, pairs_in_flight=1))
    two = attack_FGSM.attack(_args("RAFT", False, "mse", steps=2, synthetic_pairs=3, pairs_in_flight=2))
    assert one["pairs"] == two["pairs"] == 3
    assert one == two


def test_no_host_traffic_per_iteration(monkeypatch):
    counts = {}

    def counted(owner, name):
        fn = getattr(owner, name)

        def wrapper(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a, **k)
        monkeypatch.setattr(owner, name, wrapper)
    counted(torch.cuda, "synchronize")
    counted(torch.Tensor, "item")
    counted(torch.Tensor, "tolist")
    counted(torch.Tensor, "cpu")
    model, pair = _model("PWCNet"), _pair("PWCNet", 9)
    _run(model, pair, _args("PWCNet", False, "aee", steps=1), use_graph=True, reuse_graphs=False)   # one-time work (weight packs)
    seen = {}
    for steps in (2, 4):
        counts.clear()
        st = _run(model, pair, _args("PWCNet", False, "aee", steps=steps), use_graph=True, reuse_graphs=False)
        assert st.graphed is not None
        assert len(st.history) == steps and st.result()["l2_delta-avg"] > 0
        assert st.step_launches == steps
        seen[steps] = dict(counts)
    assert seen[2] == seen[4], seen
    assert seen[4]["tolist"] == 1                              # the history is read back once


def test_artefacts(tmp_path):
    args = _args("PWCNet", False, "aee", steps=2, synthetic_pairs=1, no_save=False, output_folder=str(tmp_path))
    model = _model("PWCNet")
    folder = attack_FGSM._output_folder(args, "")
    pair = _pair("PWCNet", 0)
    st = _run(model, pair, args, use_graph=True, reuse_graphs=False)
    st.save(folder)
    names = sorted(os.listdir(folder))
    assert names == sorted("00000_%s.npy" % n for n in ("delta1_final", "delta2_final", "image1", "image2", "target",
                                                         "flow_pred_final", "flow_pred_init", "flow_gt"))
    assert np.array_equal(np.load(os.path.join(folder, "00000_delta1_final.npy")), st.delta1.cpu().numpy())
    # the driver: the same eight files with an output folder, nothing at all with --no_save
    out = tmp_path / "driver"
    attack_FGSM.attack(_args("PWCNet", False, "aee", steps=2, synthetic_pairs=1, no_save=False, output_folder=str(out)))
    written = [f for _, _, files in os.walk(str(out)) for f in files]
    assert sorted(written) == names
    quiet = tmp_path / "quiet"
    attack_FGSM.attack(_args("PWCNet", False, "aee", steps=2, synthetic_pairs=1, no_save=True, output_folder=str(quiet)))
    assert not quiet.exists()
