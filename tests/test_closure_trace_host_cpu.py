"""Host logic of the closure digest trace (pcfa_amd.trace.ClosureTrace): row assignment, the replay-stability and capacity
checks, first_difference, the .npz round trip with the command line's exit codes, the parser flag and the refused flag
combinations.  The digest kernel is replaced by a numpy stand-in through the documented digest_fn= argument and the
operator table by a two-function table: no GPU."""
import json
import os
import subprocess
import sys
import types
from argparse import Namespace

import numpy as np
import pytest
import torch

from pcfa_amd import attack_PCFA, ops
from pcfa_amd.helper_functions import parsing_file
from pcfa_amd.trace import ClosureTrace, diff_paths
from tests.util import REPO

M64 = (1 << 64) - 1


def digest_np(words, index0=0):
    """The four sums of csrc/digest.hpp over uint32 words, in Python integers."""
    s = m = nan = inf = 0
    for k, w in enumerate(int(v) for v in words):
        z = ((index0 + k) * 0x9E3779B97F4A7C15) & M64
        z ^= z >> 32
        z = (z * 0xD6E8FEB86659FD93) & M64
        z ^= z >> 32
        s = (s + w) & M64
        m = (m + w * (z | 1)) & M64
        nan += (w & 0x7FFFFFFF) > 0x7F800000
        inf += (w & 0x7FFFFFFF) == 0x7F800000
    return [s, m, nan, inf]


def stand_in(t, out_row, workspace):
    words = t.detach().contiguous().float().view(torch.int32).numpy().view(np.uint32).ravel()
    out_row.copy_(torch.from_numpy(np.array(digest_np(words), dtype=np.uint64)))


def table_ops():
    """A two-operator table: one output that carries gradient, one pair of outputs of which the second does not."""
    t = types.SimpleNamespace()
    t.double = lambda x: x * 2.0
    t.split = lambda x: (x + 1.0, x.detach() * 3.0)
    t.CONSTANT = 7
    return t


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 3)
        self.act = torch.nn.ReLU()

    def forward(self, x, swap=False, extra=0):
        y = ops.get().double(x)
        y = self.act(self.lin(y)) if not swap else self.lin(self.act(y))
        a, b = ops.get().split(y)
        for _ in range(extra):
            a = ops.get().double(a)
        return (a * b).sum()


def one_pass(trace, net, x, **kw):
    x.grad = None
    with trace.recording():
        loss = net(x, **kw)
        loss.backward()
    return loss


def test_rows_follow_forward_order_and_gradients_sit_next_to_their_outputs():
    torch.manual_seed(0)
    net, x = Net(), torch.randn(2, 3, requires_grad=True)
    with ops.override_for_testing(table_ops()):
        trace = ClosureTrace(net, "cpu", capacity=32, max_closures=4, digest_fn=stand_in)
        assert ops.get().CONSTANT == 7
        one_pass(trace, net, x)
        assert ops.get() is ops.active()          # the lane's own table is gone with the pass
    assert trace.names == [
        "0000 ops.double out0 (2, 3)", "0000 ops.double out0 (2, 3) <- grad",
        "0001 module.lin out0 (2, 3)", "0001 module.lin out0 (2, 3) <- grad",
        "0002 module.act out0 (2, 3)", "0002 module.act out0 (2, 3) <- grad",
        "0003 ops.split out0 (2, 3)", "0003 ops.split out0 (2, 3) <- grad",
        "0003 ops.split out1 (2, 3)", None]       # no gradient arrives at a detached output: its row stays unnamed
    digests, names = trace.table()
    assert names == [n for n in trace.names if n is not None] and digests.shape == (9, 4) and digests.dtype == np.uint64
    # every row holds the digest of exactly the tensor it names: recompute the closure by hand
    x2 = x.detach().clone().requires_grad_()
    y = x2 * 2.0
    z = net.lin(y)
    r = net.act(z)
    a, b = r + 1.0, r.detach() * 3.0
    for t_ in (y, z, r, a):
        t_.retain_grad()
    (a * b).sum().backward()
    want = [y, y.grad, z, z.grad, r, r.grad, a, a.grad, b]
    for row, t_ in enumerate(want):
        words = t_.detach().contiguous().view(torch.int32).numpy().view(np.uint32).ravel()
        assert [int(v) for v in digests[row]] == digest_np(words), names[row]
    # a second pass at the same point gives the same table, and tracing leaves the gradient alone
    g1 = x.grad.clone()
    with ops.override_for_testing(table_ops()):
        one_pass(trace, net, x)
    assert np.array_equal(trace.table()[0], digests) and torch.equal(x.grad, g1) and torch.equal(x.grad, x2.grad)
    assert trace.passes == 2
    trace.close()
    assert not net.lin._forward_hooks and not net.act._forward_hooks


def test_a_pass_that_names_a_row_differently_raises():
    net, x = Net(), torch.randn(2, 3, requires_grad=True)
    with ops.override_for_testing(table_ops()):
        trace = ClosureTrace(net, "cpu", capacity=32, max_closures=4, digest_fn=stand_in)
        one_pass(trace, net, x)
        with pytest.raises(RuntimeError, match=r"row 2 is '0001 module\.act out0 \(2, 3\)' in this pass and "
                                               r"'0001 module\.lin out0 \(2, 3\)' in the first one"):
            one_pass(trace, net, x, swap=True)
        assert ops.get() is ops.active()
        with pytest.raises(RuntimeError, match="not replay-stable"):      # more records than the first pass
            one_pass(trace, net, x, extra=1)
        one_pass(trace, net, x)                                          # the recorder is usable after a refusal


def test_capacity_overflow_raises_on_the_host():
    net, x = Net(), torch.randn(2, 3, requires_grad=True)
    with ops.override_for_testing(table_ops()):
        trace = ClosureTrace(net, "cpu", capacity=8, max_closures=1, digest_fn=stand_in)
        with pytest.raises(RuntimeError, match="more than 8 rows"):
            one_pass(trace, net, x)
        trace = ClosureTrace(net, "cpu", capacity=10, max_closures=1, digest_fn=stand_in)
        one_pass(trace, net, x)
        trace.keep(0)
        with pytest.raises(RuntimeError, match="max_closures=1"):
            trace.keep(1)


def test_a_lane_without_a_trace_passes_straight_through():
    net, x = Net(), torch.randn(2, 3, requires_grad=True)
    with ops.override_for_testing(table_ops()):
        trace = ClosureTrace(net, "cpu", capacity=32, max_closures=1, digest_fn=stand_in)
        with ops.core.lane(3):
            with trace.recording():
                assert ops.get() is not ops.active()
                with ops.core.lane(0):
                    assert ops.get() is ops.active()       # another lane's caller, while lane 3 records
                    net(x)                                 # ... and that lane's modules leave nothing in lane 3's trace
                assert trace._pass.records == 0
                net(x).backward()
        assert len(trace.names) == 10


def _trace(values, names, steps=None):
    t = {"digests": np.array(values, dtype=np.uint64), "names": list(names)}
    if steps is not None:
        t["steps"] = np.array(steps)
    return t


def test_first_difference_on_hand_made_arrays():
    names = ["0000 ops.a out0 (1,)", "0000 ops.a out0 (1,) <- grad", "0001 ops.b out0 (1,)"]
    base = [[[1, 2, 0, 0], [3, 4, 0, 0], [5, 6, 0, 0]], [[7, 8, 0, 0], [9, 10, 0, 0], [11, 12, 1, 2]]]
    a = _trace(base, names, steps=[0, 0])
    assert ClosureTrace.first_difference(a, _trace(base, names)) is None
    other = [[list(r) for r in c] for c in base]
    other[1][1] = [9, 2 ** 64 - 1, 0, 0]       # closure 1, record 1
    d = ClosureTrace.first_difference(a, _trace(other, names))
    assert d == {"kind": "bits", "closure": 1, "step": 0, "record": 1, "name": names[1], "a": [9, 10, 0, 0],
                 "b": [9, 2 ** 64 - 1, 0, 0], "nan": [0, 0], "inf": [0, 0]}
    # ... and the output of a later call in the same closure: every output was computed before any gradient, so that one
    # is where the difference arose
    other[1][2][2:] = [0, 3]
    d = ClosureTrace.first_difference(a, _trace(other, names))
    assert (d["closure"], d["record"], d["name"], d["nan"], d["inf"]) == (1, 2, names[2], [1, 0], [2, 3])
    # among gradients the one of the LATER output comes first (the backward pass runs from the last output to the first)
    names4 = names + ["0001 ops.b out0 (1,) <- grad"]
    base4 = [c + [[13, 14, 0, 0]] for c in base]
    other = [[list(r) for r in c] for c in base4]
    other[0][1][0] = other[0][3][0] = 99
    d = ClosureTrace.first_difference(_trace(base4, names4), _trace(other, names4))
    assert (d["closure"], d["step"], d["record"], d["name"]) == (0, None, 3, names4[3])
    # an earlier closure comes before everything in a later one
    other[0] = [list(r) for r in base4[0]]
    other[0][1][0], other[1][0][0] = 99, 98
    d = ClosureTrace.first_difference(_trace(base4, names4), _trace(other, names4))
    assert (d["closure"], d["record"]) == (0, 1)
    # structural: a name, the number of records, the number of closures
    renamed = names[:1] + ["0000 ops.a out0 (2,) <- grad"] + names[2:]
    d = ClosureTrace.first_difference(a, _trace(base, renamed))
    assert d["kind"] == "names" and d["record"] == 1 and (d["a"], d["b"]) == (names[1], renamed[1]) and d["nan"] is None
    d = ClosureTrace.first_difference(a, _trace([c[:2] for c in base], names[:2]))
    assert d["kind"] == "records" and d["record"] == 2 and d["name"] == names[2] and (d["a"], d["b"]) == (3, 2)
    d = ClosureTrace.first_difference(a, _trace(base[:1], names))
    assert d["kind"] == "closures" and d["closure"] == 1 and (d["a"], d["b"]) == (2, 1)
    assert set(d) == {"kind", "closure", "step", "record", "name", "a", "b", "nan", "inf"}


def _cli(*argv):
    p = subprocess.run([sys.executable, "-m", "pcfa_amd.trace"] + list(argv), cwd=REPO, capture_output=True, text=True)
    return p.returncode, p.stdout.strip()


def test_npz_round_trip_and_command_line(tmp_path):
    torch.manual_seed(1)
    net, x = Net(), torch.randn(2, 3, requires_grad=True)
    folders = []
    for run in ("a", "b"):
        with ops.override_for_testing(table_ops()):
            trace = ClosureTrace(net, "cpu", capacity=32, max_closures=4, digest_fn=stand_in)
            for j in range(3):
                with torch.no_grad():
                    x.copy_(torch.full((2, 3), 0.25 * (j + 1)))
                one_pass(trace, net, x)
                trace.keep(j, step=j // 2)
        folders.append(str(tmp_path / run))
        trace.save(os.path.join(folders[-1], "00000_trace.npz"))
        trace.save(os.path.join(folders[-1], "00001_trace.npz"))
    fa, fb = (os.path.join(f, "00001_trace.npz") for f in folders)
    z = np.load(fa)
    assert sorted(z.files) == ["digests", "names", "steps"]
    assert z["digests"].dtype == np.uint64 and z["digests"].shape == (3, 9, 4) and list(z["steps"]) == [0, 0, 1]
    got = ClosureTrace.load(fa)
    assert got["names"] == [n for n in trace.names if n is not None]
    assert np.array_equal(got["digests"], trace.history()[0]) and not np.array_equal(got["digests"][0], got["digests"][1])
    assert _cli("diff", fa, fb) == (0, "null")
    assert _cli("diff", folders[0], folders[1]) == (0, "null")
    # one array entry altered on disk: the command names the closure and the record
    digests = got["digests"].copy()
    digests[2, 4, 1] ^= np.uint64(1)
    np.savez(fb, digests=digests, names=np.array(got["names"]), steps=got["steps"])
    code, out = _cli("diff", fa, fb)
    d = json.loads(out)
    assert code == 1 and (d["closure"], d["step"], d["record"], d["name"]) == (2, 1, 4, got["names"][4])
    code, out = _cli("diff", folders[0], folders[1])
    d = json.loads(out)
    assert code == 1 and d["file"] == "00001_trace.npz" and (d["closure"], d["record"]) == (2, 4)
    assert diff_paths(folders[0], folders[1]) == d
    os.remove(os.path.join(folders[0], "00000_trace.npz"))
    code, out = _cli("diff", folders[0], folders[1])
    assert code == 1 and json.loads(out)["kind"] == "files"
    assert _cli("diff", fa)[0] == 2


def test_parser_has_trace_digests():
    parser = parsing_file.create_parser(stage='training', attack_type='pcfa')
    assert parser.parse_args([]).trace_digests == ''
    assert parser.parse_args(["--trace_digests", "out/traces"]).trace_digests == "out/traces"
    assert "NEW" in next(a.help for a in parser._actions if "--trace_digests" in a.option_strings)


def _args(**kw):
    base = dict(net="RAFT", steps=2, joint_perturbation=False, universal_perturbation=False,
                boxconstraint="change_of_variables", delta_bound=0.005, mu=-1., target="zero", custom_target_path="",
                loss="aee", save_frequency=1, small_save=False, no_save=True, output_folder="experiment_data",
                pairs_in_flight=1, pairs_per_closure=1, batch_size=1, epochs=1, trace_digests="traces")
    base.update(kw)
    return Namespace(**base)


def test_refused_flag_combinations(monkeypatch):
    def unreachable(*a, **kw):
        raise AssertionError("the flags are refused before anything is loaded")
    monkeypatch.setattr(attack_PCFA, "_load_model", unreachable)
    loader = [(torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 64, 96), None, None)] * 2
    with pytest.raises(ValueError, match="--trace_digests.*--pairs_per_closure"):
        attack_PCFA.attack_l2(_args(pairs_per_closure=2), loader, False)
    with pytest.raises(ValueError, match="--trace_digests.*--universal_perturbation"):
        attack_PCFA.attack_l2_universal(_args(universal_perturbation=True, boxconstraint="clipping"), loader, False)
    with pytest.raises(ValueError, match="--trace_digests.*--universal_perturbation"):
        attack_PCFA.attack_l2(_args(universal_perturbation=True), loader, False)
