"""attack_FGSM.FgsmAttack with `--step_norm l2` on the MI355X: the captured loop (forward graph, loss + backward graph, the
three launches of ops.pgd_l2_step between them) against the class's eager loop bit for bit, two lanes against their solo
runs, the budget on every iterate, graph reuse, and no host traffic per iteration.  epsilon = 0.002 under a bound of 0.003:
the first step stays inside the budget, from the second on the projection is active."""
from argparse import Namespace

import pytest
import torch

from pcfa_amd import attack_FGSM, attack_PCFA, graphed, hip_ops
from pcfa_amd.helper_functions import datasets
from tests import closure_util, pgd_cases
from tests.pgd_cases import U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SIZES = {"RAFT": (128, 160), "PWCNet": (128, 192)}
EPSILON, BOUND = 0.002, 0.003
# for the extra check that the first row is a step of length epsilon: a history row is the fp32 metric of the perturbation
# (losses.two_norm_avg_delta: two fp32 sums of squares, their sum, a root, a quotient), fewer than 32 roundings in its
# longest chain at these sizes, half of them under the root.  The budget itself is asserted on the rows without it.
ROW_SLACK = 1 + 16 * U


def _args(net, joint=False, steps=3, **kw):
    base = dict(net=net, weights="random:%d" % closure_util.WEIGHT_SEED, dataset="Synthetic", dataset_stage="evaluation",
                small_run=False, synthetic_size="%dx%d" % SIZES[net], synthetic_pairs=2, dstype="final",
                output_folder="experiment_data", small_save=False, save_frequency=1, no_save=True,
                unregistered_artifacts=True, joint_perturbation=joint, steps=steps, epsilon=EPSILON, target="zero",
                custom_target_path="", loss="aee", pairs_in_flight=1, step_norm="l2", delta_bound=BOUND)
    base.update(kw)
    return Namespace(**base)


def _pair(net, seed):
    h, w = SIZES[net]
    i1, i2, flow = datasets.synthetic_pair(seed, h, w)
    return i1[None], i2[None], flow[None]


def _model(net):
    return closure_util.load_model(net, False, DEV)


def _run(model, pair, args, batch=0, scalars=None, **kw):
    st = attack_FGSM.FgsmAttack(model, pair[0], pair[1], pair[2], batch, DEV, True, args, **kw)
    for _ in range(args.steps):
        st.step()
        if scalars is not None:          # (G, a, E, s) of this step and the float64 norm of what it left: host reads of the TEST
            scalars.append(hip_ops.pgd_l2_workspace(DEV)[:4].tolist()
                           + [pgd_cases.norm64(st.delta1.cpu().numpy().ravel(), st.delta2.cpu().numpy().ravel())])
    return st


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_equal_runs(st, want):
    for name in ("x1", "x2", "delta1", "delta2", "flow_pred"):
        got, ref = getattr(st, name).detach(), getattr(want, name).detach()
        assert _same_bits(got, ref), "%s: %d of %d elements differ" % (name, int((got != ref).sum()), ref.numel())
    n = st.steps_done
    assert n == want.steps_done > 0 and _same_bits(st._hist[:n], want._hist[:n])      # the history buffer itself
    assert st.history == want.history and st.result() == want.result()


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("net", ["RAFT", "PWCNet"])
def test_graph_loop_equals_eager_loop_bitwise_inside_the_budget(net, joint):
    args = _args(net, joint)
    model, pair = _model(net), _pair(net, 3)
    eager = _run(model, pair, args, use_graph=False)
    assert eager.graphed is None and eager.step_launches == args.steps
    scalars = []
    st = _run(model, pair, args, scalars=scalars, use_graph=True, reuse_graphs=False)
    assert st.graphed is not None, "capture failed: the eager loop ran"
    assert st.step_launches == args.steps and st.step_norm == "l2"
    assert (st.graphed.forwards, st.graphed.backwards) == (args.steps + 1, args.steps)
    _assert_equal_runs(st, eager)
    cap = pgd_cases.budget(BOUND)
    print("G, a, E, s, norm64 per step:", scalars)
    assert scalars[0][3] == 1.0                                 # one step of length epsilon < bound: no projection
    assert any(row[3] < 1.0 for row in scalars[1:])            # ... then the projection is active
    for G, a, E, s, norm in scalars:
        assert 0 < a and 0 < G and norm <= cap, (G, a, E, s, norm, cap)
    rows = [h["l2_delta-avg"] for h in st.history]
    assert len(rows) == args.steps and all(0 < r <= cap for r in rows), (rows, cap)      # every row inside the budget
    assert rows[0] <= pgd_cases.f32(EPSILON) * ROW_SLACK       # the step has averaged L2 length epsilon; the box only clips
    for x in (st.x1.detach(), st.x2.detach()):
        assert float(x.min()) >= 0 and float(x.max()) <= 1


def test_two_lanes_equal_their_solo_runs():
    args = _args("RAFT")
    model, pairs = _model("RAFT"), [_pair("RAFT", 7), _pair("RAFT", 8)]
    solo = [_run(model, p, args, batch=k, use_graph=True, reuse_graphs=False) for k, p in enumerate(pairs)]
    torch.cuda.synchronize()            # lane 0 is one stream-ordered sequence: finished before it goes on on its run stream
    flight = attack_PCFA.PairsInFlight(
        lambda k: attack_FGSM.FgsmAttack(model, pairs[k][0], pairs[k][1], pairs[k][2], k, DEV, True, args, use_graph=True),
        2, DEV)
    flight.run(args.steps)
    for k in range(2):
        assert flight.attacks[k].graphed is not None and flight.attacks[k].graph_key[-1] == k
        assert flight.attacks[k].graph_key[-4:-2] == ("l2", BOUND)
        _assert_equal_runs(flight.attacks[k], solo[k])
    assert not _same_bits(solo[0].delta1, solo[1].delta1)


def test_second_pair_adopts_the_graphs_and_a_sign_attack_gets_its_own(monkeypatch):
    captures = []
    init = graphed.SplitGraphedStep.__init__
    monkeypatch.setattr(graphed.SplitGraphedStep, "__init__",
                        lambda self, *a, **k: (captures.append(1), init(self, *a, **k))[1])
    args = _args("PWCNet", steps=2, epsilon=0.0021)               # an epsilon no other test uses: a key of its own
    model, a, b = _model("PWCNet"), _pair("PWCNet", 5), _pair("PWCNet", 6)
    first = _run(model, a, args, use_graph=True, reuse_graphs=True)
    assert len(captures) == 1 and not first.graphs_reused
    kept = model._pcfa_fgsm_graphs[first.graph_key]
    second = _run(model, b, args, batch=1, use_graph=True, reuse_graphs=True)
    assert second.graphs_reused and len(captures) == 1 and kept.pairs == 2 and second.graphed is kept.graphed
    assert first.retired
    fresh = _run(model, b, args, batch=1, use_graph=True, reuse_graphs=False)
    assert len(captures) == 2
    _assert_equal_runs(second, fresh)
    sign_args = _args("PWCNet", steps=2, epsilon=0.0021, step_norm="sign")
    sign = _run(model, b, sign_args, batch=2, use_graph=True, reuse_graphs=True)
    assert len(captures) == 3 and not sign.graphs_reused and sign.graph_key != second.graph_key
    assert not second.retired and set(model._pcfa_fgsm_graphs) >= {second.graph_key, sign.graph_key}
    assert not _same_bits(sign.delta1, second.delta1)           # a signed step is another step


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
    _run(model, pair, _args("PWCNet", steps=1), use_graph=True, reuse_graphs=False)   # one-time work (weight packs, workspace)
    seen, allocated = {}, {}
    for steps in (2, 4):
        counts.clear()
        st = attack_FGSM.FgsmAttack(model, *pair, 0, DEV, True, _args("PWCNet", steps=steps), use_graph=True,
                                    reuse_graphs=False)
        assert st.graphed is not None
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(steps):
            st.step()
        allocated[steps] = torch.cuda.memory_stats()["allocation.all.allocated"] - before
        assert len(st.history) == steps and st.step_launches == steps
        seen[steps] = dict(counts)
    assert seen[2] == seen[4], seen
    assert seen[4]["tolist"] == 1                              # the history is read back once
    assert allocated[2] == allocated[4], allocated            # iterations do not allocate: twice as many, no more blocks
