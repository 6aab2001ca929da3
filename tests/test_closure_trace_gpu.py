"""The closure digest trace on the GPU (pcfa_amd.trace.ClosureTrace, PairAttack(trace=...), --trace_digests): tracing does
not change what the closure computes, two evaluations and graph against eager leave equal tables, a one-bit change in one
operator's output is named exactly, two lanes in flight equal solo with their whole history, the files round-trip through
the command line, and without a trace a step launches what it launched before the feature existed.

RAFT at 128x160 and PWC-Net at 128x192 with seeded random weights: the sizes of the other closure tests.

(The first run of these tests on the MI355X named a real defect: at 128x192 PWC-Net's pyramid layer conv6aa sees a 4x6 map,
ops.conv_s2 served W % 4 == 0 only, so that one layer ran as a library convolution -- and four evaluations of one closure at
the same variables left four different digests in its record, every earlier record equal.  nets/pwcnet.py now pads such a
map to the next multiple of 4 and runs it on ops.conv_s2 like every other size.)"""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pcfa_amd import attack_PCFA, graph_sets, ops
from pcfa_amd import config as pcfa_config
from pcfa_amd.helper_functions import datasets
from pcfa_amd.trace import GRAD, ClosureTrace, diff_paths
from tests import closure_util
from tests.util import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = {"RAFT": (128, 160), "PWCNet": (128, 192)}


def pair_attack(net, seed, trace=None, use_graph=False, reuse_graphs=False, steps=1):
    """PairAttack on one synthetic pair, as pcfa_attack builds it (change of variables, zero target, AEE)."""
    import bench
    dev = torch.device(DEV)
    model = closure_util.load_model(net, True, dev)
    args = bench.attack_args(net, steps=steps)
    i1, i2, _ = datasets.synthetic_pair(seed, *SIZES[net])
    return attack_PCFA.PairAttack(model, i1[None], i2[None], None, 0, attack_PCFA.EPS_BOX, dev, False,
                                  attack_PCFA.default_mu(args), args, use_graph=use_graph, reuse_graphs=reuse_graphs,
                                  trace=trace)


def nudge(st, seed=7):
    """Move the variables off the initial point, in place (the graphs' static addresses stay)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in st.params:
            p.add_((0.02 * torch.randn(p.shape, generator=g)).to(p.device))


def new_trace(net, **kw):
    return ClosureTrace(closure_util.load_model(net, True, torch.device(DEV)), DEV, max_closures=kw.pop("max_closures", 4), **kw)


def evaluate(st):
    loss = st.closure()
    torch.cuda.synchronize()
    return loss.detach().clone(), [p.grad.detach().clone() for p in st.params]


_EAGER = {}


def eager(net):
    """One untraced and two traced eager closure evaluations of `net` at the same variables, computed once: loss and
    gradients of each, the table after each traced evaluation, the names."""
    if net not in _EAGER:
        plain = pair_attack(net, 3)
        nudge(plain)
        out = {"plain": evaluate(plain)}
        trace = new_trace(net)
        st = pair_attack(net, 3, trace=trace)
        nudge(st)
        out["traced"] = evaluate(st)
        out["table"], out["names"] = trace.table()
        out["traced2"] = evaluate(st)
        out["table2"], _ = trace.table()
        out["history"] = trace.history()
        trace.close()
        _EAGER[net] = out
    return _EAGER[net]


def describe(a, b, names):
    return ClosureTrace.first_difference((np.asarray(a)[None], names), (np.asarray(b)[None], names))


@pytest.mark.parametrize("net", ["RAFT", "PWCNet"])
def test_tracing_does_not_perturb_the_closure(net):
    if net == "RAFT":    # the batched motion-encoder backward is what the default build runs: the hooks sit on its outputs too
        assert pcfa_config.cfg(closure_util.load_model(net, True, torch.device(DEV))).motion_bwd == "batched"
    e = eager(net)
    (loss0, grads0), (loss1, grads1) = e["plain"], e["traced"]
    assert torch.equal(loss0, loss1)
    assert len(grads0) == len(grads1) == 2 and all(torch.equal(a, b) for a, b in zip(grads0, grads1))
    names = e["names"]
    assert len(names) > 100 and sum(n.endswith(GRAD) for n in names) > 40
    assert names[-3:] == ["closure loss"] + ["closure grad of variable %d %s" % (i, tuple(grads0[i].shape)) for i in (0, 1)]
    outputs = [r for r, n in enumerate(names) if not n.endswith(GRAD)]
    assert (e["table"][outputs, 1] != 0).sum() > len(outputs) // 2        # the rows were written
    assert not ops._lane_tables                             # no lane keeps a table of its own after its pass


@pytest.mark.parametrize("net", ["RAFT", "PWCNet"])
def test_two_eager_evaluations_give_equal_tables(net):
    e = eager(net)
    assert torch.equal(e["traced"][0], e["traced2"][0])
    assert np.array_equal(e["table"], e["table2"]), describe(e["table"], e["table2"], e["names"])
    digests, names, steps = e["history"]
    assert digests.shape == (2, len(names), 4) and np.array_equal(digests[0], e["table"]) and list(steps) == [0, 0]


@pytest.mark.parametrize("net", ["RAFT", "PWCNet"])
def test_graph_replay_leaves_the_eager_table(net):
    e = eager(net)
    model = closure_util.load_model(net, True, torch.device(DEV))
    sets = graph_sets.cache(model, "pair-graph")
    before = dict(sets)
    trace = new_trace(net)
    st = pair_attack(net, 3, trace=trace, use_graph=True, reuse_graphs=None)
    assert st.graphed is not None and not st.graphs_reused
    assert dict(sets) == before                     # a traced attack leaves no graph set behind
    assert trace.passes == 3 and trace.kept == 0    # two warm-up passes and the capture; none of them is kept
    nudge(st)
    loss, grads = evaluate(st)
    table, names = trace.table()
    trace.close()
    assert names == e["names"]
    assert np.array_equal(table, e["table"]), describe(e["table"], table, names)     # (names the operator if it fails)
    assert torch.equal(loss, e["traced"][0]) and all(torch.equal(a, b) for a, b in zip(grads, e["traced"][1]))
    assert trace.kept == 1 and np.array_equal(trace.history()[0][0], table)


class FlipOneBit:
    """The operator table with ONE call changed: the k-th call of `name` after arm() gets the lowest mantissa bit of one
    element in the middle of its (first) output flipped."""

    def __init__(self, name, k):
        self.name, self.k, self.count, self.flipped = name, k, None, None
        self.table = ops.active()

    def arm(self):
        self.count = 0

    def __getattr__(self, attr_name):
        attr = getattr(self.table, attr_name)
        if attr_name != self.name:
            return attr

        def wrapped(*args, **kw):
            out = attr(*args, **kw)
            if self.count is not None:
                if self.count == self.k:
                    t = out[0] if isinstance(out, (tuple, list)) else out
                    at = tuple(s // 2 for s in t.shape)
                    t.data.view(torch.int32)[at] ^= 1
                    self.flipped = tuple(t.shape)
                self.count += 1
            return out
        return wrapped


@pytest.mark.parametrize("net,name,k", [("RAFT", "conv3x3", 7), ("PWCNet", "pwc_warp", 1)])
def test_first_difference_names_the_operator_whose_output_changed(net, name, k):
    e = eager(net)
    flip = FlipOneBit(name, k)
    trace = new_trace(net)
    with ops.override_for_testing(flip):
        st = pair_attack(net, 3, trace=trace)
        nudge(st)
        flip.arm()
        evaluate(st)
    table, names = trace.table()
    trace.close()
    assert names == e["names"] and flip.flipped is not None
    calls = [r for r, n in enumerate(names) if " ops.%s out0 " % name in n and not n.endswith(GRAD)]
    want = calls[k]
    d = ClosureTrace.first_difference((e["table"][None], names), (table[None], names))
    assert d is not None and d["kind"] == "bits" and d["closure"] == 0
    assert (d["record"], d["name"]) == (want, names[want]), d
    assert names[want].endswith(str(flip.flipped))
    assert abs(d["a"][0] - d["b"][0]) == 1 and d["inf"][0] == d["inf"][1]   # one lowest bit: the plain sum moved by one
    # every record computed before it is equal, bit for bit
    order = ClosureTrace.computed_order(names)
    earlier = order[:order.index(want)]
    assert len(earlier) >= k and np.array_equal(e["table"][earlier], table[earlier])


def test_two_lanes_in_flight_equal_solo_history_included(tmp_path):
    net, seeds, steps = "RAFT", (11, 12), 2
    dev = torch.device(DEV)
    traces = []

    def make(k):
        traces.append(new_trace(net, max_closures=32))
        return pair_attack(net, seeds[k], trace=traces[-1], use_graph=True, steps=steps)
    flight = attack_PCFA.PairsInFlight(make, 2, dev)
    assert all(st.graphed is not None for st in flight.attacks)
    last = flight.run(steps)
    for k, tr in enumerate(traces):
        tr.save(str(tmp_path / ("flight%d.npz" % k)))
        tr.close()
    for k, seed in enumerate(seeds):
        tr = new_trace(net, max_closures=32)
        solo = pair_attack(net, seed, trace=tr, use_graph=True, steps=steps)
        for _ in range(steps):
            solo_last = solo.step()
        tr.save(str(tmp_path / ("solo%d.npz" % k)))
        tr.close()
        a = flight.attacks[k]
        assert tuple(last[k]) == tuple(solo_last) and a.closures == solo.closures == tr.kept
        fa, fb = (ClosureTrace.load(str(tmp_path / (n % k))) for n in ("flight%d.npz", "solo%d.npz"))
        assert fa["names"] == fb["names"] and list(fa["steps"]) == list(fb["steps"]) == [0] * 10 + [1] * (a.closures - 10)
        assert fa["digests"].shape == (a.closures, len(fa["names"]), 4)
        assert np.array_equal(fa["digests"], fb["digests"]), ClosureTrace.first_difference(fa, fb)
        assert not np.array_equal(fa["digests"][0], fa["digests"][1])        # (the closures are not copies of each other)
        del solo


def _cli(*argv):
    p = subprocess.run([sys.executable, "-m", "pcfa_amd.trace"] + list(argv), cwd=REPO, capture_output=True, text=True)
    return p.returncode, p.stdout.strip()


def test_trace_digests_flag_round_trip(tmp_path):
    folders = [str(tmp_path / run) for run in ("a", "b")]
    for folder in folders:
        res = attack_PCFA.attack_l2(closure_util.cli_args(net="RAFT", steps=1, synthetic_pairs=2, synthetic_size="128x160",
                                                          pairs_in_flight=1, pairs_per_closure=1, trace_digests=folder))
        assert res["pairs"] == 2
        assert sorted(os.listdir(folder)) == ["00000_trace.npz", "00001_trace.npz"]
    assert diff_paths(folders[0], folders[1]) is None
    assert _cli("diff", folders[0], folders[1]) == (0, "null")
    one = ClosureTrace.load(os.path.join(folders[0], "00000_trace.npz"))
    two = ClosureTrace.load(os.path.join(folders[0], "00001_trace.npz"))
    assert one["digests"].shape[0] == 10 and one["names"] == two["names"]
    assert not np.array_equal(one["digests"], two["digests"])                  # two pairs, two trajectories
    victim = os.path.join(folders[1], "00001_trace.npz")
    digests = two["digests"].copy()
    digests[4, 30, 0] += np.uint64(1)
    np.savez(victim, digests=digests, names=np.array(two["names"]), steps=two["steps"])
    code, out = _cli("diff", folders[0], folders[1])
    d = json.loads(out)
    assert code == 1 and d["file"] == "00001_trace.npz"
    assert (d["closure"], d["step"], d["record"], d["name"]) == (4, 0, 30, two["names"][30])


# One step() of an untraced, graphed RAFT PairAttack at 128x160 (seed 5), as the call spy saw it on the commit BEFORE this
# feature (measured there, not on this code): the closure is replayed, so these are the optimiser's and the metrics' launches.
PARENT_STEP_CALLS = 6
PARENT_STEP_COUNTS = {"pcfa_avg_epe": 2, "pcfa_sum_squares": 4}


def test_without_a_trace_a_step_launches_what_it_did_before():
    model = closure_util.load_model("RAFT", True, torch.device(DEV))
    sets = graph_sets.cache(model, "pair-graph")
    sets.clear()
    st = pair_attack("RAFT", 5, use_graph=True)
    assert st.graphed is not None and st.trace is None
    seen = []

    def spy(name, args, invoke):
        seen.append(name)
        return invoke(name, *args)
    ops.core.set_call_spy(spy)
    try:
        st.step()
    finally:
        ops.core.set_call_spy(None)
    torch.cuda.synchronize()
    print("entry points of one step: %d %s" % (len(seen), json.dumps(collections.Counter(seen), sort_keys=True)))
    assert "pcfa_digest_words" not in seen
    assert len(seen) == PARENT_STEP_CALLS
    assert dict(collections.Counter(seen)) == PARENT_STEP_COUNTS
