"""attack_PCFA.PairBatch: B independent per-pair attacks whose closure is one forward and backward at batch B.

What can be exact is exact: B = 1 against PairAttack (every bit), the element-wise variable transforms, the per-item
loss / metric kernels (tests/test_loss_items_gpu.py) and the optimiser (tests/test_lbfgs_items_gpu.py).  What remains is
the network at batch B against batch 1, whose kernels round differently; it is held to the project's own bar for batch-1
against batch-2 closures (tests/test_gpu_parity.py::test_universal_cosim_two_ranks_on_gpu_equals_single_process: loss
1e-5 relative, gradient 1e-2 relative L2) and, for a flow, to 1e-4 of its largest value
(test_pwcnet_batch_of_pairs_matches_single_pairs).  The measured distances are junit properties."""
import pytest
import torch

import bench
from pcfa_amd import attack_PCFA
from pcfa_amd.helper_functions import datasets, logging
from tests import closure_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEEDS = (11, 12)          # as the pairs-in-flight tests
BATCHES = (3, 5)          # the pairs' dataset indices: every item logs under its own batch * steps + step
CASES = {"raft": ("RAFT", 128, 160, "change_of_variables", False),
         "raft_joint": ("RAFT", 128, 160, "clipping", True),
         "pwcnet": ("PWCNet", 128, 192, "change_of_variables", False)}


def _model(net, box, config=None):
    model = closure_util.load_model(net, box == "change_of_variables", DEV, config=config)
    for name in ("_pcfa_pair_graphs", "_pcfa_pair_batch_graphs"):
        if hasattr(model, name):
            getattr(model, name).clear()
    return model


def _args(case, target="zero", steps=1):
    net, _, _, box, joint = CASES[case]
    return bench.attack_args(net, box, joint=joint, target=target, steps=steps)


def _pair(case, seed):
    _, h, w, _, _ = CASES[case]
    i1, i2, _ = datasets.synthetic_pair(seed, h, w)
    return i1[None], i2[None]


def _batch(model, case, args, graph, seeds=SEEDS):
    pairs = [(BATCHES[k],) + _pair(case, seed) + (None,) for k, seed in enumerate(seeds)]
    return attack_PCFA.PairBatch(model, pairs, attack_PCFA.EPS_BOX, DEV, False, attack_PCFA.default_mu(args), args,
                                 use_graph=graph)


def _solo(model, case, args, graph, k, seed):
    i1, i2 = _pair(case, seed)
    return attack_PCFA.PairAttack(model, i1, i2, None, BATCHES[k], attack_PCFA.EPS_BOX, DEV, False,
                                  attack_PCFA.default_mu(args), args, use_graph=graph, reuse_graphs=False)


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _flat_grads(params, b=None):
    return torch.cat([(p.grad if b is None else p.grad[b]).detach().reshape(-1) for p in params]).clone()


# ---- (a) B = 1 is PairAttack, bit for bit ------------------------------------------------------------------------------
def test_one_item_equals_pair_attack():
    model, args = _model("RAFT", "change_of_variables"), _args("raft", steps=2)
    pb = _batch(model, "raft", args, True, seeds=SEEDS[:1])
    solo = _solo(model, "raft", args, True, 0, SEEDS[0])
    assert pb.graphed is not None and solo.graphed is not None
    for _ in range(2):
        got, want = pb.step(), solo.step()
        assert tuple(got[0]) == tuple(want)
    assert torch.equal(pb.delta1, solo.delta1) and torch.equal(pb.delta2, solo.delta2)
    assert torch.equal(pb.flow_pred, solo.flow_pred)
    assert pb.result(0) == solo.result()
    assert torch.equal(pb.rec[0].delta1_min, solo.delta1_min) and torch.equal(pb.rec[0].flow_pred_min, solo.flow_pred_min)
    assert pb.closures == solo.closures == 20


# ---- (b) every item's loss and gradient against the solo closure at the same variables ---------------------------------
def _closure_distances(model, case, graph):
    args = _args(case)
    pb = _batch(model, case, args, graph)
    solos = [_solo(model, case, args, graph, k, seed) for k, seed in enumerate(SEEDS)]
    assert (pb.graphed is not None) == graph
    g = torch.Generator().manual_seed(5)
    out = []
    for moved in (False, True):
        if moved:   # N(0, 0.05^2) on every variable: the penalty becomes active
            with torch.no_grad():
                for i, p in enumerate(pb.params):
                    p.add_((torch.randn(p.shape, generator=g) * 0.05).to(DEV))
                    for k, solo in enumerate(solos):
                        solo.params[i].copy_(p[k:k + 1])
        losses = pb.closure().detach().clone()
        for k, solo in enumerate(solos):
            want = float(solo.closure())
            got_g, want_g = _flat_grads(pb.params, k), _flat_grads(solo.params)
            out.append((moved, k, abs(float(losses[k]) - want) / abs(want), _rel_l2(got_g, want_g)))
        if moved:   # the penalty is live: its share of the loss (and of the gradient) is not zero
            with torch.no_grad():
                d1, d2 = pb.current_deltas()
            assert float(attack_PCFA.losses.two_norm_avg_delta(d1[0], d2[0])) > args.delta_bound
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_item_closures_match_solo_closures_raft(graph, record_property):
    _check_closures("raft", graph, record_property)


@pytest.mark.parametrize("case", ["raft_joint", "pwcnet"])
def test_item_closures_match_solo_closures(case, record_property):
    _check_closures(case, True, record_property)


def _check_closures(case, graph, record_property):
    net, _, _, box, _ = CASES[case]
    for moved, k, dl, dg in _closure_distances(_model(net, box), case, graph):
        tag = "%s_item%d" % ("moved" if moved else "initial", k)
        record_property("loss_rel_" + tag, dl)
        record_property("grad_rel_l2_" + tag, dg)
        print("%s %s %s: loss rel %.3e, grad rel-L2 %.3e" % (case, "graph" if graph else "eager", tag, dl, dg))
        assert dl <= 1e-5, (tag, dl)
        assert dg < 1e-2, (tag, dg)


# ---- (c) no cross-talk --------------------------------------------------------------------------------------------------
def test_item_bits_do_not_depend_on_the_batch_mate():
    """Default RAFT has no fixed-point scatter (one shift per call) on the closure's path: item 0's loss and gradient
    bits are the same whatever pair sits next to it."""
    model, args = _model("RAFT", "change_of_variables"), _args("raft")
    seen = []
    for mate in (12, 13):
        pb = _batch(model, "raft", args, False, seeds=(11, mate))
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for p in pb.params:
                p[0].add_((torch.randn(p[0].shape, generator=g) * 0.05).to(DEV))
        seen.append((pb.closure()[0].clone(), _flat_grads(pb.params, 0)))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    assert seen[0][1].abs().max() > 0


# ---- (d) two steps with each item's own target ----------------------------------------------------------------------------
def _reference_rule(history, bound):
    """attack_PCFA.py:226-243 of the reference, written out: -> index of the recorded iterate."""
    below, best, l2_min, aee_min = False, None, float("inf"), float("inf")
    for i, (aee, _, l2) in enumerate(history):
        update = False
        if not below:
            if l2 < l2_min or (l2 == l2_min and aee < aee_min):
                update = True
                if l2 <= bound:
                    below = True
        elif l2 <= bound and aee < aee_min:
            update = True
        if update:
            best, l2_min, aee_min = i, l2, aee
    return best


@pytest.mark.parametrize("case", list(CASES))
def test_two_steps_with_own_targets(case, record_property):
    net, _, _, box, _ = CASES[case]
    steps = 2
    model, args = _model(net, box), _args(case, target="neg_flow", steps=steps)
    first_record = len(logging.SINK.records)
    pb = _batch(model, case, args, True)
    assert pb.graphed is not None
    history, deltas = [], []
    for _ in range(steps):
        history.append(pb.step())
        deltas.append(pb.delta1.clone())
    records = logging.SINK.records[first_record:]
    for k, seed in enumerate(SEEDS):
        solo = _solo(model, case, args, False, k, seed)
        # the item's target is the negative of ITS unattacked flow, which is the solo pair's up to batch-2 rounding
        assert torch.equal(pb.target[k], -pb.flow_pred_init[k])
        scale = float(solo.flow_pred_init.abs().max())
        assert float((pb.flow_pred_init[k:k + 1] - solo.flow_pred_init).abs().max()) <= 1e-4 * scale
        # the item's final variables (and its target) in a solo attack of that pair
        with torch.no_grad():
            for p, q in zip(pb.params, solo.params):
                q.copy_(p[k:k + 1])
            solo.target.copy_(pb.target[k:k + 1])
            (d1, d2), flow = solo._repredict_body()
        assert torch.equal(pb.delta1[k:k + 1], d1) and torch.equal(pb.delta2[k:k + 1], d2)
        dflow = float((pb.flow_pred[k:k + 1] - flow).abs().max()) / float(flow.abs().max())
        aee, _ = logging.calc_metrics_adv(flow, solo.target, solo.flow_pred_init)
        _, _, l2 = logging.calc_delta_metrics(d1, d2)
        r = pb.rec[k]
        record_property("flow_rel_max_item%d" % k, dflow)
        record_property("aee_adv_tgt_rel_item%d" % k, abs(r.aee_adv_tgt - aee) / aee)
        print("%s item %d: flow %.3e of max|flow|, aee_adv_tgt rel %.3e" % (case, k, dflow, abs(r.aee_adv_tgt - aee) / aee))
        assert dflow <= 1e-4
        assert abs(r.aee_adv_tgt - aee) <= 1e-5 * aee
        assert abs(r.l2_delta12 - l2) <= 1e-5 * l2
        # the best-iterate record against the per-step values, and those against what was logged under the item's steps
        mine = [h[k] for h in history]
        best = _reference_rule(mine, args.delta_bound)
        assert best is not None
        assert (r.aee_adv_tgt_min_val, r.aee_adv_pred_min_val, r.delta12_min_val) == mine[best]
        assert torch.equal(r.delta1_min, deltas[best][k:k + 1])
        assert pb.result(k)[4:6] + pb.result(k)[8:] == mine[-1][:2] + (mine[-1][2],) + mine[best][:2] + (mine[best][2],)
        for s in range(steps):
            at = BATCHES[k] * steps + s
            logged = {key: v for key, v, step in records if step == at}
            assert logged["batch"] == BATCHES[k] and logged["steps"] == s
            assert (logged["aee_predadv-tgt"], logged["aee_pred-predadv"], logged["l2_delta-avg"]) == mine[s]


# ---- the graph sets: a cache of their own, keyed by B ---------------------------------------------------------------------
def test_graph_sets_are_reused_per_shape_and_item_count():
    model, args = _model("RAFT", "change_of_variables"), _args("raft")
    first = _batch(model, "raft", args, True)
    assert not first.graphs_reused and list(model._pcfa_pair_batch_graphs) == [first.graph_key]
    assert first.graph_key[-1] == 2 and not getattr(model, "_pcfa_pair_graphs", {})      # PCFA's pair cache untouched
    want = first.step()
    second = _batch(model, "raft", args, True)                   # the same pairs again on the adopted graphs
    assert second.graphs_reused and first.retired and second.graphed is not None
    assert second.step() == want
    with pytest.raises(RuntimeError):
        first.step()
    one = _batch(model, "raft", args, True, seeds=SEEDS[:1])     # another B: a set of its own
    assert not one.graphs_reused and len(model._pcfa_pair_batch_graphs) == 2
    model._pcfa_pair_batch_graphs.clear()


def test_driver_rows_keep_the_pairs_indices(monkeypatch):
    """attack_l2 --pairs_per_closure 2 on three synthetic pairs: a PairBatch of two and a flushed single pair.  The rows
    go to gather_rows under the pairs' own indices, and the pair attacked alone has exactly the row of
    --pairs_per_closure 1."""
    from pcfa_amd import sharding
    seen = []
    gather = sharding.gather_rows
    monkeypatch.setattr(sharding, "gather_rows", lambda rows, **kw: seen.append(list(rows)) or gather(rows, **kw))
    base = dict(net="RAFT", steps=1, synthetic_pairs=3, synthetic_size="128x160", pairs_in_flight=1)
    one = attack_PCFA.attack_l2(closure_util.cli_args(pairs_per_closure=1, **base))
    two = attack_PCFA.attack_l2(closure_util.cli_args(pairs_per_closure=2, **base))
    assert one["pairs"] == two["pairs"] == 3
    rows1, rows2 = ({r[0]: r for r in rows} for rows in seen)
    assert sorted(rows1) == sorted(rows2) == [0, 1, 2] and all(len(r) == 13 for r in rows2.values())
    assert rows2[2] == rows1[2]
    assert all(v == v for r in (rows2[0], rows2[1]) for v in r[5:])     # (the columns that never depend on ground truth)
