"""The two gates of the float64 kernel tests and the small buffer helpers they go with, shared by
tests/test_winograd_f64_gpu.py, tests/test_conv_strided_f64_gpu.py and tests/test_gru_epilogue_f64_gpu.py.

Elementwise: |Y - Y64| <= 2 gamma(n + 2) P + (n + 2) 2^-126.  Statistical: rel_l2(Y, Y64) <= 3 max(rel_l2(E, Y64), u), E the
same sum accumulated in fp32 on the CPU in the kernel's order, globally, per named group of the output map (`regions`)
and per 32-channel block; groups of fewer than 256 elements are left to the elementwise gate.  A caller whose
output is more than a sum (the fused GRU epilogues, tests/gru_epilogue.py) passes its own elementwise `bound` in place of
the formula, and further groups (`extra`: name -> index of the output, a boolean mask for instance) for the statistical gate.
"""
import torch

from tests import winograd as wg
from tests.fenced import TINY, U, gamma


def dense_stride(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= s
    return tuple(reversed(st))


def unchanged(f):
    return torch.equal(f.buf.view(torch.int32), f.bits0)


def gates(got, want, P, n, emu, m, record, prefix="", regions=None, bound=None, extra=None):
    """(elementwise ratio, statistical ratio) over every group; records both and returns them.  regions(H, W, m): the
    named (row slice, column slice) groups of the output map (default: the Winograd tiles' of tests/winograd.py).
    bound: the elementwise bound itself (P and n are then unused); extra: {name: index} of further groups."""
    got = got.double()
    if bound is None:
        bound = 2 * gamma(n + 2) * P + (n + 2) * TINY
    elem = float(((got - want).abs() / bound).max())
    groups = {"all": (slice(None), slice(None))}
    H, W = want.shape[-2:]
    groups.update((regions or wg.regions)(H, W, m))
    stat, worst = 0.0, ""
    views = [(name, (slice(None), slice(None)) + sl) for name, sl in groups.items()]
    views += [("ch%d" % c, (slice(None), slice(c, c + 32))) for c in range(0, want.shape[1], 32)]
    views += list((extra or {}).items())
    for name, idx in views:
        w_, g_, e_ = want[idx], got[idx], emu[idx]
        if w_.numel() < 256 or float(w_.norm()) == 0.0:
            continue
        r = wg.rel_l2_64(g_, w_) / (3 * max(wg.rel_l2_64(e_, w_), U))
        if r > stat:
            stat, worst = r, name
    record(prefix + "elem_ratio", "%.3g" % elem)
    record(prefix + "stat_ratio", "%.3g" % stat)
    record(prefix + "stat_worst_group", worst)
    assert elem <= 1, ("elementwise", elem)
    assert stat <= 1, ("statistical", stat, worst)
    return elem, stat
