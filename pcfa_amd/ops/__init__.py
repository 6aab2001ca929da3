"""Operator table used by the networks and the attack loop.

The package ships exactly one implementation, :mod:`pcfa_amd.ops.hip` (HIP
kernels through the C-ABI; the operators live in the sibling modules corr, conv,
gru, gma, pwc, flownet, attack_math, artefacts, ingest, with core / profiling underneath;
``pcfa_amd.hip_ops`` is an alias of the same module).  It raises on non-GPU tensors and when
libpcfa_hip.so is missing -- there is no CPU fallback.

`override_for_testing` exists so that the test-suite can drive the *host*
logic (attack schedule, sharding, model plumbing) on a GPU-less machine by
injecting the CPU oracle from outside the package; nothing in pcfa_amd calls it.

`set_lane_table` is the product's own hook: the closure digest trace (pcfa_amd.trace) hands the callers of ONE lane a
recording proxy over the table while its pass is open; every other lane, and every lane outside a pass, gets the table
itself.
"""
import contextlib

from . import hip as _hip_ops

_active = _hip_ops
_lane_tables = {}   # lane -> the table that lane's callers get instead of _active (set_lane_table); empty unless tracing


def get():
    if _lane_tables:
        table = _lane_tables.get(_hip_ops.current_lane())
        if table is not None:
            return table
    return _active


def active():
    """The process-wide table, whatever the caller's lane: what a lane's own table (set_lane_table) forwards to."""
    return _active


def set_lane_table(lane, table):
    """Hand the callers of ONE lane (ops.core.current_lane(): a host thread, or the stream a backward node runs on) `table`
    instead of the process-wide one; None takes it back.  Returns what the lane had before.  This is how
    pcfa_amd.trace.ClosureTrace sees the operator calls of its own closure -- a proxy that forwards every call to
    `active()` and digests what comes back -- while other lanes' closures, running on other threads of the same process, go
    straight through.  The table is process-global and lanes are threads, hence the routing by lane."""
    prev = _lane_tables.get(lane)
    if table is None:
        _lane_tables.pop(lane, None)
    else:
        _lane_tables[lane] = table
    return prev


@contextlib.contextmanager
def override_for_testing(ops_module):
    global _active
    prev = _active
    _active = ops_module
    try:
        yield ops_module
    finally:
        _active = prev
