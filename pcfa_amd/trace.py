"""Closure digest trace: which operator's bits differ first between two runs of an attack, and in which closure evaluation.

    trace = ClosureTrace(model, device)
    st = attack_PCFA.PairAttack(..., trace=trace)      # or: attack_PCFA.py --trace_digests DIR
    ... st.step() ...
    trace.save("00000_trace.npz")
    python -m pcfa_amd.trace diff A B                   # two files or two folders: one JSON line, exit code 0 / 1

While a pass is open (`with trace.recording():` -- the attack opens one around every closure body) every call of the
operator table and every leaf module of the model leaves one RECORD per floating output: the output's digest
(ops.tensor_digest: four exact 64-bit sums over its bits, csrc/digest.hpp) and, where the output requires grad, the digest
of the gradient arriving at it.  A digest is one or two kernel launches on the current stream into the record's own row of
a device table, with the record's own scratch: no allocation, no read-back, no library reduction, so the launches are
captured with the closure and every replay of the graph refills the table.  `keep(j)` files the table as closure
evaluation j (device to device); `table()` / `save()` are the only reads.

Rows are assigned at forward time, in call order: record k owns rows 2k (output) and 2k + 1 (its gradient), so a row does not
depend on the order in which autograd fires hooks.  The names are fixed by the first pass; a later pass that names a row
differently raises, because such a closure is not replay-stable.  The two runs to compare may be two processes, two
machines, graph against eager, or in flight against solo: `first_difference` walks closure by closure, record by record
in the order things were computed (outputs in call order, then gradients from the last output back to the first), so the
record it names is where the difference arose: an operator whose inputs' records are all equal.
"""
import contextlib
import json
import os
import sys
import weakref

import numpy as np
import torch

from . import ops

_UNTRACED = ("tensor_digest", "digest_workspace_words")
GRAD = " <- grad"     # what the name of a gradient's record ends in
FINAL = "closure grad of variable"   # what the records of the variables' own gradients (PairAttack) begin with


class _Pass:
    def __init__(self):
        self.calls = 0      # operator / module calls seen: the counter in front of every name
        self.records = 0    # records made (two rows each)


class _TracedTable:
    """The operator table with every call recorded: forwards to ops.active() -- the same kernels in the same order, a
    proxy, not another implementation -- and hands what comes back to the trace."""

    def __init__(self, trace):
        self._trace = weakref.ref(trace)

    def __getattr__(self, name):
        attr = getattr(ops.active(), name)
        if not callable(attr) or isinstance(attr, type) or name in _UNTRACED:
            return attr
        trace = self._trace

        def wrapped(*args, **kw):
            out = attr(*args, **kw)
            tr = trace()
            if tr is not None:
                tr._watch("ops." + name, out)
            return out
        return wrapped


class ClosureTrace:
    """Recorder of one attack's closure evaluations (module docstring).

    model: its leaf modules are hooked (removed by `close()`); device: where table, scratch and history live.
    capacity: rows of the table (two per record); max_closures: closure evaluations `keep` can file.
    digest_fn(tensor, out_row, workspace): what writes a record (default: the operator table's tensor_digest, GPU only) --
    a stand-in lets the host logic run without a GPU."""

    def __init__(self, model, device, capacity=4096, max_closures=256, digest_fn=None):
        self.device = torch.device(device)
        self.capacity, self.max_closures = int(capacity), int(max_closures)
        if digest_fn is None:
            self._digest = ops.active().tensor_digest
            ws_words = ops.active().digest_workspace_words()
        else:
            self._digest, ws_words = digest_fn, 1
        # (allocated as int64 and viewed: the same bits, and every fill / copy kernel exists for int64)
        self._table = torch.zeros((self.capacity, 4), dtype=torch.int64, device=self.device).view(torch.uint64)
        # one scratch per row: records made on different streams (Config.overlap_encoders' side stream, the streams backward
        # nodes run on) never share one
        self._ws = torch.zeros((self.capacity, ws_words), dtype=torch.int64, device=self.device)
        self._history = torch.zeros((self.max_closures, self.capacity, 4), dtype=torch.int64,
                                    device=self.device).view(torch.uint64)
        self.names = None          # row -> name (None: a gradient row of an output that needs none), fixed by the first pass
        self.passes = 0
        self.kept = 0              # closure evaluations filed
        self.steps = {}            # history slot -> the attack step it belongs to
        self._pass = None
        self._names_now = None
        self._lane = 0
        self._proxy = _TracedTable(self)
        self._hooks = []
        me = weakref.ref(self)

        def module_hook(name):
            def hook(_mod, _inp, out):
                tr = me()
                if tr is not None and tr._pass is not None and ops.core.current_lane() == tr._lane:
                    tr._watch("module." + name, out)
            return hook
        if model is not None:
            for name, mod in model.named_modules():
                if not list(mod.children()):
                    self._hooks.append(mod.register_forward_hook(module_hook(name)))

    def close(self):
        """Take the hooks off the model (the recorded data stays readable)."""
        for h in self._hooks:
            h.remove()
        self._hooks = []

    # ---- recording ---------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def recording(self):
        """One pass: the operator calls of the caller's lane and the model's leaf modules are recorded until the block
        ends.  Nothing in here reads from the device."""
        if self._pass is not None:
            raise RuntimeError("ClosureTrace: a pass is already open")
        self._lane = ops.core.current_lane()
        self._pass = _Pass()
        self._names_now = [] if self.names is None else None
        prev = ops.set_lane_table(self._lane, self._proxy)
        try:
            yield self
            self._end_pass()
        finally:
            ops.set_lane_table(self._lane, prev)
            self._pass = None
            self._names_now = None

    def _end_pass(self):
        rows = 2 * self._pass.records
        if self.names is None:
            self.names = self._names_now
        elif rows != len(self.names):
            raise RuntimeError("ClosureTrace: this pass made %d records, the first one %d: the closure is not replay-stable "
                               "(first name without a partner: %r)"
                               % (rows // 2, len(self.names) // 2, self.names[rows] if rows < len(self.names) else None))
        self.passes += 1

    def _row(self, row, name):
        """Claim `row` under `name`: fixed by the first pass, checked by every later one."""
        if row >= self.capacity:
            raise RuntimeError("ClosureTrace: more than %d rows (%d records) in one closure: raise capacity"
                               % (self.capacity, self.capacity // 2))
        if self._names_now is not None:
            while len(self._names_now) <= row:
                self._names_now.append(None)
            self._names_now[row] = name
        elif row >= len(self.names) or self.names[row] != name:
            raise RuntimeError("ClosureTrace: row %d is %r in this pass and %r in the first one: the closure is not "
                               "replay-stable" % (row, name, self.names[row] if row < len(self.names) else None))

    def _write(self, row, t):
        self._digest(t, self._table[row], self._ws[row])

    def _grad_hook(self, row):
        # closes over the trace and the row: autograd calls it on a thread of its own, where no thread-local exists
        def hook(grad):
            if grad is not None:     # (an output nobody used hands None to its hook: the row keeps its zeros)
                self._write(row, grad)
        return hook

    def record(self, name, t):
        """One record under `name` for tensor t inside an open pass: its digest and, if it requires grad, its gradient's."""
        p = self._pass
        k = p.records
        self._row(2 * k, name)
        self._row(2 * k + 1, name + GRAD if t.requires_grad else None)
        p.records += 1
        self._write(2 * k, t.detach())
        if t.requires_grad:
            t.register_hook(self._grad_hook(2 * k + 1))

    def _watch(self, name, out):
        p = self._pass
        if p is None:
            return
        outs = out if isinstance(out, (tuple, list)) else (out,)
        for j, t in enumerate(outs):
            if torch.is_tensor(t) and t.is_floating_point() and t.numel() > 0:
                self.record("%04d %s out%d %s" % (p.calls, name, j, tuple(t.shape)), t)
        p.calls += 1

    # ---- reading -----------------------------------------------------------------------------------------------------
    def _used(self):
        return [r for r, n in enumerate(self.names or ()) if n is not None]

    def table(self):
        """(digests uint64 [records][4], names) of the rows in use as the last pass -- or the last replay of a graph that
        captured one -- left them: one device-to-host copy."""
        used = self._used()
        host = self._table[:len(self.names or ())].cpu().numpy()
        return host[used], [self.names[r] for r in used]

    def keep(self, j, step=None):
        """File the table as closure evaluation j: device to device, on the current stream."""
        if not 0 <= j < self.max_closures:
            raise RuntimeError("ClosureTrace: closure evaluation %d does not fit max_closures=%d" % (j, self.max_closures))
        n = len(self.names or ())
        self._history[j, :n].copy_(self._table[:n])
        self.kept = max(self.kept, j + 1)
        if step is not None:
            self.steps[j] = int(step)

    def history(self):
        """(digests uint64 [closures kept][records][4], names, step of every closure or -1)."""
        used = self._used()
        host = self._history[:self.kept, :len(self.names or ())].cpu().numpy()
        steps = np.array([self.steps.get(j, -1) for j in range(self.kept)], dtype=np.int64)
        return host[:, used], [self.names[r] for r in used], steps

    def save(self, path):
        """One .npz: `digests` uint64 [closures][records][4], `names`, and `steps` (the attack step of every closure)."""
        digests, names, steps = self.history()
        folder = os.path.dirname(os.path.abspath(path))
        os.makedirs(folder, exist_ok=True)
        with open(path, "wb") as f:
            np.savez(f, digests=digests, names=np.array(names, dtype=np.str_), steps=steps)

    @staticmethod
    def load(path):
        with np.load(path, allow_pickle=False) as z:
            out = {"digests": z["digests"], "names": [str(n) for n in z["names"]]}
            if "steps" in z.files:
                out["steps"] = z["steps"]
        return out

    @staticmethod
    def computed_order(names):
        """The records of a closure in the order they were computed: the outputs in call order, then the gradients from the
        last output back to the first, then the variables' own gradients -- walking it, the first record that differs is where a difference arose, not where
        it arrived."""
        grads = [r for r, n in enumerate(names) if n.endswith(GRAD)]
        final = [r for r, n in enumerate(names) if n.startswith(FINAL)]      # the variables' gradients: the backward's end
        return [r for r, n in enumerate(names) if not n.endswith(GRAD) and not n.startswith(FINAL)] + grads[::-1] + final

    @staticmethod
    def first_difference(a, b):
        """First difference between two traces (what `load` / `history` return, or a file name): None, or
        {"closure", "step", "record", "name", "a", "b", "nan", "inf"} -- for differing bits `a` / `b` are the two digests and
        `nan` / `inf` the two counts of each; a name or count mismatch is a STRUCTURAL difference (`kind`: "names",
        "records" or "closures"; `a` / `b` then hold the two names or counts, `nan` / `inf` None)."""
        a, b = (ClosureTrace._as_trace(t) for t in (a, b))
        da, db = np.asarray(a["digests"], dtype=np.uint64), np.asarray(b["digests"], dtype=np.uint64)
        na, nb = list(a["names"]), list(b["names"])
        steps = a.get("steps")

        def step_of(c):
            return int(steps[c]) if steps is not None and c < len(steps) and steps[c] >= 0 else None

        def structural(kind, closure, record, name, va, vb):
            return {"kind": kind, "closure": closure, "step": None if closure is None else step_of(closure),
                    "record": record, "name": name, "a": va, "b": vb, "nan": None, "inf": None}
        for r, (x, y) in enumerate(zip(na, nb)):
            if x != y:
                return structural("names", None, r, x, x, y)
        if len(na) != len(nb):
            r = min(len(na), len(nb))
            return structural("records", None, r, nb[r] if len(na) < len(nb) else na[r], len(na), len(nb))
        order = np.array(ClosureTrace.computed_order(na), dtype=np.int64)
        for c in range(min(len(da), len(db))):
            rows = order[np.nonzero((da[c][order] != db[c][order]).any(axis=1))[0]] if len(order) else ()
            if len(rows):
                r = int(rows[0])
                va, vb = [int(v) for v in da[c, r]], [int(v) for v in db[c, r]]
                return {"kind": "bits", "closure": c, "step": step_of(c), "record": r, "name": na[r], "a": va, "b": vb,
                        "nan": [va[2], vb[2]], "inf": [va[3], vb[3]]}
        if len(da) != len(db):
            return structural("closures", min(len(da), len(db)), None, None, len(da), len(db))
        return None

    @staticmethod
    def _as_trace(t):
        if isinstance(t, (str, os.PathLike)):
            return ClosureTrace.load(t)
        if isinstance(t, tuple):
            return dict(zip(("digests", "names", "steps"), t))
        return t


def diff_paths(a, b):
    """first_difference of two trace files, or of the equally named *_trace.npz files of two folders (the first file that
    differs, with its name under "file"; a file only one folder has is a structural difference)."""
    if os.path.isdir(a) != os.path.isdir(b):
        raise ValueError("diff: two files or two folders")
    if not os.path.isdir(a):
        return ClosureTrace.first_difference(a, b)
    fa, fb = (sorted(f for f in os.listdir(d) if f.endswith("_trace.npz")) for d in (a, b))
    for name in sorted(set(fa) | set(fb)):
        if name not in fa or name not in fb:
            return {"kind": "files", "file": name, "closure": None, "step": None, "record": None, "name": None,
                    "a": name in fa, "b": name in fb, "nan": None, "inf": None}
        d = ClosureTrace.first_difference(os.path.join(a, name), os.path.join(b, name))
        if d is not None:
            return dict(d, file=name)
    return None


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 3 or argv[0] != "diff":
        sys.stderr.write("usage: python -m pcfa_amd.trace diff A B    (two .npz traces, or two folders of them)\n")
        return 2
    d = diff_paths(argv[1], argv[2])
    print(json.dumps(d))
    return 0 if d is None else 1


if __name__ == "__main__":
    sys.exit(main())
