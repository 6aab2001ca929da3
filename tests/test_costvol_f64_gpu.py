"""The PWC-Net and FlowNetC cost volumes and ChannelNorm through the C-ABI on fenced buffers (tests/fenced.py), against float64:
pcfa_spatial_corr_fwd / _bwd, pcfa_cost_volume9_fwd / _bwd (csrc/spatial_corr.hip), pcfa_flownet_corr_fwd / _bwd and
pcfa_channelnorm_fwd / _bwd (csrc/flownet_ops.hip).  The plan mirrors, references, emulations, inputs, case tables and gates are
those of tests/costvol.py (every bound is derived in its docstring); tests/test_costvol_host_cpu.py shows on the CPU that the
cases reach their paths and that the kernels' arithmetic passes every gate.

Inputs sit between NaN; outputs are pre-filled with a sentinel NaN.  Each call checks (_twice of tests/test_warp_f64_gpu.py):
the status; every input and every fence bit-unchanged; no sentinel or non-finite value left in an output; a second call from
the same state gives identical bits (none of these kernels uses atomics).  The plan label, the ratios with their worst group
and the number of mismatches of every exact variant are recorded as junit properties.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from pcfa_amd import _hip
from tests import costvol as cv
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, SENTINEL, Fenced, stream
from tests.gates import dense_stride, unchanged
from tests.test_warp_f64_gpu import _bits, _twice

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC_ENV = ("PCFA_SC_TILE", "PCFA_SC_NS", "PCFA_SC_CR", "PCFA_SC_BTH", "PCFA_SC_DBG")


def _lib():
    return _hip.load()


def _in(t, shift=0):
    return Fenced(t.shape, dense_stride(t.shape), NAN_BITS, shift).write(t)


def _out(shape, shift=0):
    return Fenced(tuple(shape), dense_stride(tuple(shape)), SENTINEL, shift)


def _flat(gshape):
    return (gshape[0], gshape[1] * gshape[2], gshape[3], gshape[4])


# --------------------------------------------------------------------------- one call of every sampler entry point
def sc_forward(in1, in2, p, gshape, fused=None, shift=(0, 0, 0), decided=None):
    """fused: (scale, slope) -> pcfa_cost_volume9_fwd, else pcfa_spatial_corr_fwd; shift: floats off on (in1, in2, out)."""
    lib = _lib()
    B, C, H, W = in1.shape
    f1, f2, fo = _in(in1, shift[0]), _in(in2, shift[1]), _out(_flat(gshape), shift[2])
    if fused:
        call = lambda: lib.pcfa_cost_volume9_fwd(f1.ptr(), f2.ptr(), fo.ptr(), B, C, H, W, fused[0], fused[1], stream())   # noqa: E731
    else:
        call = lambda: lib.pcfa_spatial_corr_fwd(f1.ptr(), f2.ptr(), fo.ptr(), B, C, H, W, *cv.sc_args(p), stream())   # noqa: E731
    return _twice(call, [fo], [f1, f2], decided=decided)[0].view(gshape)


def sc_backward(in1, in2, g, p, fused=None, fwd_out=None, shift=(0, 0, 0, 0, 0), decided=None):
    lib = _lib()
    B, C, H, W = in1.shape
    f1, f2, fg = _in(in1, shift[0]), _in(in2, shift[1]), _in(g.reshape(_flat(g.shape)), shift[2])
    o1, o2 = _out(in1.shape, shift[3]), _out(in1.shape, shift[4])
    if fused:
        ff = _in(fwd_out)
        call = lambda: lib.pcfa_cost_volume9_bwd(f1.ptr(), f2.ptr(), ff.ptr(), fg.ptr(), o1.ptr(), o2.ptr(), B, C, H, W,   # noqa: E731
                                                 fused[0], fused[1], stream())
        return tuple(_twice(call, [o1, o2], [f1, f2, fg, ff], decided=decided))
    call = lambda: lib.pcfa_spatial_corr_bwd(f1.ptr(), f2.ptr(), fg.ptr(), o1.ptr(), o2.ptr(), B, C, H, W, *cv.sc_args(p), stream())   # noqa: E731
    return tuple(_twice(call, [o1, o2], [f1, f2, fg], decided=decided))


def sc_run(d, shift=(0, 0), forward=True):
    """Every call of one data set (tests/costvol.py: sc_data or sc_onehot), in the layout of cv.sc_emulate."""
    got = {"fwd": {}, "bwd": {}}
    a, b = getattr(d, "f_in1", d.in1), getattr(d, "f_in2", d.in2)
    if forward:
        got["fwd"]["plain"] = sc_forward(a, b, d.p, d.gshape, shift=shift + (0,))
    got["bwd"]["plain"] = sc_backward(d.in1, d.in2, d.g, d.p, shift=shift + (0, 0, 0))
    if d.fast:
        assert shift == (0, 0)
        if forward:
            got["fwd"]["fused"] = sc_forward(a, b, d.p, d.gshape, (d.scale, d.slope))
        got["bwd"]["fused"] = sc_backward(d.in1, d.in2, d.g, d.p, (d.scale, d.slope), d.fwd_out)
    return got


def _sc_case(record, key, shift=(0, 0)):
    worst = (0.0, 0.0)
    fo = None
    for variant in ("random", "integer"):
        d = cv.sc_data(key, variant)
        r = cv.sc_check(d, sc_run(d, shift), record)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        fo = getattr(d, "fwd_out", None)
    for k, pos in enumerate(cv.sc_positions(key)):
        o = cv.sc_onehot(key, pos, fo)
        cv.sc_check(o, sc_run(o, shift), record, "pos%d_" % k)
    record("worst_elem_ratio", "%.3g" % worst[0])
    record("worst_stat_ratio", "%.3g" % worst[1])


@pytest.mark.parametrize("case", cv.SC_TABLE, ids=lambda c: c.name)
def test_scorr_fast(record_property, case):
    """pcfa_spatial_corr_fwd / _bwd (scale 1, slope 1) and pcfa_cost_volume9_fwd / _bwd (1 / C and 0.1 on `random`, powers of
    two on `integer` and `onehot`, the backward on the planted fwd_out) on the plan the case is in the table for."""
    assert all(os.environ.get(k) is None for k in SC_ENV)
    p = cv.scorr_plan(*case.shape)
    assert p.label == case.label and cv.sc_is_fast(cv.FAST, case.shape[3])
    record_property("path", "scorr9_fwd_kernel<%d,%d> %s%s" % (p.th, p.tw, p.label, " (cr > crmax)" if p.clipped else ""))
    record_property("backward_path", "scorr9_bwd_kernel<2> " + cv.scorr_bwd_plan(*case.shape).label)
    _sc_case(record_property, case.name)


@pytest.mark.parametrize("case", cv.SC_GENERIC, ids=lambda c: c.name)
def test_scorr_generic(record_property, case):
    """scorr_fwd_generic_kernel and scorr_bwd_generic_kernel<1, 2>: rectangular parameter sets, and the fast parameters kept
    off the fast path by W % 4 != 0 or an operand one float off a 16-byte boundary."""
    assert not cv.sc_is_fast(case.p, case.shape[3], case.shift == (0, 0))
    record_property("path", "generic: " + case.route)
    oh, ow = ctypes.c_int(-7), ctypes.c_int(-7)
    H, W, p = case.shape[2], case.shape[3], case.p
    assert _lib().pcfa_spatial_corr_out_size(H, W, *p.k, *p.pad, *p.dil, *p.stride, ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oh.value, ow.value) == cv.sc_out_size(H, W, p)
    _sc_case(record_property, case.name, case.shift)


def test_scorr_refusals():
    """pcfa_cost_volume9_* refuses W % 4 != 0 and any operand off a 16-byte boundary; null pointers, zero sizes and a kernel
    larger than the padded image are invalid arguments; a refused call writes nothing."""
    lib = _lib()
    s = stream()
    for shape in ((1, 4, 5, 7), (1, 4, 5, 8)):
        B, C, H, W = shape
        gshape = (B, 81, H, W)
        a, b, g = cv.operands(shape, gshape, "random")
        fixed = [_in(a), _in(b), _in(g), _in(g), _out(gshape), _out(shape), _out(shape)]
        moved = [_in(a, 1), _in(b, 2), _in(g, 3), _in(g, 1), _out(gshape, 2), _out(shape, 3), _out(shape, 1)]
        every = fixed + moved

        def refused(status, want):
            torch.cuda.synchronize()
            assert status == want, (status, want)
            assert all(unchanged(f) for f in every), "a refused call touched a buffer"

        def fwd(sel=(), **kw):
            i1, i2, _, _, o, _, _ = [(moved if k in sel else fixed)[k].ptr() for k in range(7)]
            i1, i2, o = kw.get("i1", i1), kw.get("i2", i2), kw.get("o", o)
            return lib.pcfa_cost_volume9_fwd(i1, i2, o, kw.get("B", B), kw.get("C", C), kw.get("H", H), kw.get("W", W), 0.25, 0.1, s)

        def bwd(sel=(), **kw):
            ptrs = [(moved if k in sel else fixed)[k].ptr() for k in range(7)]
            i1, i2, ff, gg, _, g1, g2 = [kw.get("p%d" % k, q) for k, q in enumerate(ptrs)]
            return lib.pcfa_cost_volume9_bwd(i1, i2, ff, gg, g1, g2, kw.get("B", B), kw.get("C", C), kw.get("H", H), kw.get("W", W),
                                             0.25, 0.1, s)

        if W % 4:
            refused(fwd(), PCFA_ERR_UNSUPPORTED)
            refused(bwd(), PCFA_ERR_UNSUPPORTED)
            continue
        for k in (0, 1, 4):
            refused(fwd((k,)), PCFA_ERR_UNSUPPORTED)
        for k in (0, 1, 2, 3, 5, 6):
            refused(bwd((k,)), PCFA_ERR_UNSUPPORTED)
        for k in ("i1", "i2", "o"):
            refused(fwd(**{k: None}), PCFA_ERR_INVALID_ARG)
        for k in range(7):
            if k != 4:
                refused(bwd(**{"p%d" % k: None}), PCFA_ERR_INVALID_ARG)
        for k in "BCHW":
            refused(fwd(**{k: 0}), PCFA_ERR_INVALID_ARG)
            refused(bwd(**{k: 0}), PCFA_ERR_INVALID_ARG)
        p = [q.ptr() for q in fixed]
        args = cv.sc_args(cv.FAST)
        big = cv.sc_args(cv.sampler(k=(7, 1)))             # 7 rows of kernel on 5 rows of image, pad 0
        assert cv.sc_out_size(H, W, cv.sampler(k=(7, 1))) is None
        refused(lib.pcfa_spatial_corr_fwd(p[0], p[1], p[4], B, C, H, W, *big, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_spatial_corr_bwd(p[0], p[1], p[3], p[5], p[6], B, C, H, W, *big, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_spatial_corr_fwd(None, p[1], p[4], B, C, H, W, *args, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_spatial_corr_fwd(p[0], p[1], None, B, C, H, W, *args, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_spatial_corr_bwd(p[0], p[1], None, p[5], p[6], B, C, H, W, *args, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_spatial_corr_bwd(p[0], p[1], p[3], p[5], None, B, C, H, W, *args, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_spatial_corr_fwd(p[0], p[1], p[4], B, 0, H, W, *args, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_spatial_corr_bwd(p[0], p[1], p[3], p[5], p[6], B, C, 0, W, *args, s), PCFA_ERR_INVALID_ARG)
        zero_stride = args[:10] + (0, 1)
        refused(lib.pcfa_spatial_corr_fwd(p[0], p[1], p[4], B, C, H, W, *zero_stride, s), PCFA_ERR_INVALID_ARG)


# --------------------------------------------------------------------------- the 4-row backward tile, in a process of its own
def _tall_runs():
    return [(name, variant) for name in cv.SC_TALL for variant in ("random", "integer")]


def _child(path):
    """Runs in a fresh process with PCFA_SC_BTH=4 (read once per process): the backward of both SC_TALL cases, plain and
    fused, through the same per-call checks."""
    assert os.environ.get("PCFA_SC_BTH") == "4"
    res = {}
    for name, variant in _tall_runs():
        d = cv.sc_data(name, variant)
        res[name, variant] = sc_run(d, forward=False)["bwd"]
    torch.save(res, path)


def test_scorr_tall_backward_tile(record_property):
    """scorr9_bwd_kernel<4> (kept for tuning, PCFA_SC_BTH=4) on two cases, gated like the 2-row tile."""
    assert os.environ.get("PCFA_SC_BTH") is None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "res.pt")
        env = dict(os.environ, PCFA_SC_BTH="4", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        try:
            r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                               ["-c", "import sys; from tests import test_costvol_f64_gpu as t; t._child(sys.argv[1])", path],
                               cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as ex:      # a hang: the child has been killed, the card is suspect
            pytest.exit("the PCFA_SC_BTH=4 child hung and was killed after %g s: nothing more is started on the GPU\n%s"
                        % (ex.timeout, (ex.stderr or "")[-3000:]), returncode=1)
        if r.returncode < 0 or r.returncode in (134, 139):
            pytest.exit("the PCFA_SC_BTH=4 child ended abnormally (%d): nothing more is started on the GPU\n%s"
                        % (r.returncode, r.stderr[-3000:]), returncode=1)
        assert r.returncode == 0, r.stderr[-3000:]
        theirs = torch.load(path)
    assert sorted(theirs) == sorted(_tall_runs())
    for (name, variant), bwd in theirs.items():
        q = cv.scorr_bwd_plan(*cv.SC_CASES[name].shape, bth=4)
        record_property(name + "_path", "scorr9_bwd_kernel<4> " + q.label)
        cv.sc_check(cv.sc_data(name, variant), {"fwd": {}, "bwd": bwd}, record_property, name + "_tall_")


# --------------------------------------------------------------------------- NaN and infinities in in1
def _counts(v):
    return "%d: %d nan, %d inf, %d finite" % (v.numel(), int(v.isnan().sum()), int(v.isinf().sum()), int(torch.isfinite(v).sum()))


def test_scorr_wild(record_property):
    """One NaN, one +inf and one -inf in in1.  An element of in1 meets only the outputs of its own pixel (all 81 planes) and,
    in grad_in2, its own channel within the 9 x 9 window around it; grad_in1 does not read in1.  Every other output passes
    the gates; what the touched ones hold is recorded -- among them the outputs whose poisoned tap has its partner outside the
    image: the header drops such terms, the fast kernel multiplies by a staged zero (NaN), the generic one skips them."""
    name = cv.SC_WILD
    d = cv.sc_data(name, "random")
    B, C, H, W = d.shape
    poison = [(2, 1, 2, float("nan")), (7, 2, 17, float("inf")), (C - 1, H - 1, W - 1, float("-inf"))]
    in1 = d.in1.clone()
    keep_f = torch.ones(d.gshape, dtype=torch.bool)
    keep_2 = torch.ones(d.shape, dtype=torch.bool)
    for c, y, x, v in poison:
        in1[0, c, y, x] = v
        keep_f[:, :, :, y, x] = False
        keep_2[0, c, max(y - 4, 0):y + 5, max(x - 4, 0):x + 5] = False
    keep_1 = torch.ones(d.shape, dtype=torch.bool)
    assert int((~keep_f).sum()) == 3 * 81
    keep = {"fwd": keep_f, "bwd": (keep_1, keep_2)}
    flat = keep_f.view(cv._as4(keep_f).shape)
    got = {"fwd": {}, "bwd": {}}
    for form, fused in (("plain", None), ("fused", (d.scale, d.slope))):
        got["fwd"][form] = sc_forward(in1, d.in2, d.p, d.gshape, fused, decided=[flat])
        got["bwd"][form] = sc_backward(in1, d.in2, d.g, d.p, fused, d.fwd_out if fused else None, decided=[keep_1, keep_2])
    cv.sc_check(d, got, record_property, "wild_", keep)
    generic = sc_forward(in1, d.in2, d.p, d.gshape, shift=(0, 1, 0), decided=[flat])
    cv.sc_check(d, {"fwd": {"plain": generic}, "bwd": {}}, record_property, "wild_generic_", keep,
                emu={"fwd": {"plain": cv.sc_fwd(d.in1, d.in2, d.p, torch.float32)}})
    c, y, x, _ = poison[0]
    outside = torch.tensor([[not (0 <= y + ph - 4 < H and 0 <= x + pw - 4 < W) for pw in range(9)] for ph in range(9)])
    assert 0 < int(outside.sum()) < 81
    for nme, t in (("fast", got["fwd"]["plain"]), ("fast_fused", got["fwd"]["fused"]), ("generic", generic)):
        record_property("wild_%s_touched" % nme, _counts(t[~keep_f]))
        record_property("wild_%s_nan_tap_with_partner_outside" % nme, _counts(t[0, :, :, y, x][outside]))
        record_property("wild_%s_nan_tap_with_partner_inside" % nme, _counts(t[0, :, :, y, x][~outside]))
    for form in ("plain", "fused"):
        record_property("wild_%s_gin2_touched" % form, _counts(got["bwd"][form][1][~keep_2]))


# --------------------------------------------------------------------------- FlowNet correlation
def fc_forward(in1, in2, f, gshape, shift=(0, 0, 0)):
    lib = _lib()
    B, C, H, W = in1.shape
    f1, f2, fo = _in(in1, shift[0]), _in(in2, shift[1]), _out(gshape, shift[2])
    return _twice(lambda: lib.pcfa_flownet_corr_fwd(f1.ptr(), f2.ptr(), fo.ptr(), B, C, H, W, *cv.fc_args(f), stream()),
                  [fo], [f1, f2])[0]


def fc_backward(in1, in2, g, f, shift=(0, 0, 0, 0, 0)):
    lib = _lib()
    B, C, H, W = in1.shape
    f1, f2, fg, o1, o2 = _in(in1, shift[0]), _in(in2, shift[1]), _in(g, shift[2]), _out(in1.shape, shift[3]), _out(in1.shape, shift[4])
    return tuple(_twice(lambda: lib.pcfa_flownet_corr_bwd(f1.ptr(), f2.ptr(), fg.ptr(), o1.ptr(), o2.ptr(), B, C, H, W,
                                                          *cv.fc_args(f), stream()), [o1, o2], [f1, f2, fg]))


def fc_run(d, shift=0):
    a, b = getattr(d, "f_in1", d.in1), getattr(d, "f_in2", d.in2)
    got = {"fwd": fc_forward(a, b, d.f, d.gshape, (shift, 0, 0))}
    if d.backward:
        got["bwd"] = fc_backward(d.in1, d.in2, d.g, d.f, (shift, 0, 0, 0, 0))
    return got


@pytest.mark.parametrize("case", cv.FC_FAST, ids=lambda c: c.name)
def test_fcorr_fast(record_property, case):
    """fcorr_fwd_fast_kernel and fcorr_bwd_fast_kernel<+1, -1>; once more with grad_out, grad_in1 and grad_in2 each 1, 2 or 3
    floats off a 16-byte boundary (the fast path asks alignment of in1 and in2 only: the same kernels, the same bits); and
    the forward with `out` shifted, which takes the generic kernel (where C is a power of two, also the backward with in1
    shifted: the generic kernels on the exact operands)."""
    f, fargs = cv.flownet(), cv.fc_args(cv.flownet())
    pl = cv.fcorr_plan(*case.shape, f)
    assert pl.label == "fast"
    record_property("path", "fcorr fast, %d chunks, tail %d, %s" % (pl.chunks, pl.tail, pl.divide))
    d = cv.fc_data(case.shape, fargs, "random")
    got = fc_run(d)
    r = cv.fc_check(d, got, record_property)
    record_property("worst_elem_ratio", "%.3g" % r[0])
    record_property("worst_stat_ratio", "%.3g" % r[1])
    for k in range(3):
        shift = tuple((1 + (k + j) % 3) if j == k else 0 for j in range(3))
        again = fc_backward(d.in1, d.in2, d.g, f, (0, 0) + shift)
        cv.fc_check(d, {"fwd": got["fwd"], "bwd": again}, record_property, "shift%d%d%d_" % shift)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(again, got["bwd"])), "a shifted gradient changed the result"
    assert cv.fcorr_plan(*case.shape, f, aligned=False).label == "generic"
    shifted = fc_forward(d.in1, d.in2, f, d.gshape, (0, 0, 1))
    cv.fc_check(d, {"fwd": shifted}, record_property, "out_shifted_generic_")
    if pl.pow2:
        e = cv.fc_data(case.shape, fargs, "integer")
        cv.fc_check(e, fc_run(e), record_property)
        exact_generic = fc_forward(e.in1, e.in2, f, e.gshape, (0, 0, 1))
        cv.fc_check(e, {"fwd": exact_generic}, record_property, "out_shifted_generic_")
        # in1 one float off: the generic backward kernels on the same exact operands
        generic_bwd = fc_backward(e.in1, e.in2, e.g, f, (1, 0, 0, 0, 0))
        cv.fc_check(e, {"fwd": exact_generic, "bwd": generic_bwd}, record_property, "in1_shifted_generic_")
        for k, pos in enumerate(cv.fc_positions(case.shape, pl.dsize)):
            o = cv.fc_onehot(case.shape, fargs, pos)
            cv.fc_check(o, fc_run(o), record_property, "pos%d_" % k)


@pytest.mark.parametrize("case", cv.FC_GENERIC, ids=lambda c: c.name)
def test_fcorr_generic(record_property, case):
    """fcorr_fwd_generic_kernel and fcorr_bwd_generic_kernel<1, 2> (stride1 = 2: the forward alone)."""
    pl = cv.fcorr_plan(*case.shape, case.f, aligned=case.shift == 0)
    assert pl.label == "generic"
    record_property("path", "fcorr generic: " + case.route)
    oc, oh, ow = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    assert _lib().pcfa_flownet_corr_out_size(case.shape[2], case.shape[3], *cv.fc_args(case.f), ctypes.byref(oc), ctypes.byref(oh),
                                             ctypes.byref(ow)) == 0
    assert (oc.value, oh.value, ow.value) == (pl.dsize ** 2, pl.oH, pl.oW)
    d = cv.fc_data(case.shape, cv.fc_args(case.f), "random")
    assert d.backward == case.backward
    r = cv.fc_check(d, fc_run(d, case.shift), record_property)
    record_property("worst_elem_ratio", "%.3g" % r[0])
    record_property("worst_stat_ratio", "%.3g" % r[1])


def test_fcorr_statuses():
    lib = _lib()
    s = stream()
    shape = cv.FC_SHAPE
    B, C, H, W = shape
    f = cv.flownet(4, 1, 4, 2, 2)
    pl = cv.fcorr_plan(*shape, f)
    gshape = (B, pl.dsize ** 2, pl.oH, pl.oW)
    a, b, g = cv.operands(shape, gshape, "random", salt=9)
    fa, fb, fg, fo, o1, o2 = _in(a), _in(b), _in(g), _out(gshape), _out(shape), _out(shape)
    every = [fa, fb, fg, fo, o1, o2]
    p = [q.ptr() for q in every]

    def refused(status, want):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(q) for q in every), "a refused call touched a buffer"

    refused(lib.pcfa_flownet_corr_bwd(p[0], p[1], p[2], p[4], p[5], B, C, H, W, *cv.fc_args(f), s), PCFA_ERR_UNSUPPORTED)   # stride1 = 2
    for bad in ((0, 2, 4, 1, 2), (0, 1, 20, 1, 2), (-1, 1, 4, 1, 2), (4, 1, 4, 0, 2), (4, 1, 4, 1, 0)):   # even k; empty output; ..
        assert cv.fcorr_plan(*shape, cv.flownet(*bad)) is None
        refused(lib.pcfa_flownet_corr_fwd(p[0], p[1], p[3], B, C, H, W, *bad, s), PCFA_ERR_INVALID_ARG)
        refused(lib.pcfa_flownet_corr_bwd(p[0], p[1], p[2], p[4], p[5], B, C, H, W, *bad, s), PCFA_ERR_INVALID_ARG)
    ok = (4, 1, 4, 1, 2)
    for k in (0, 1, 3):
        q = [p[0], p[1], p[3]]
        q[(0, 1, 3).index(k)] = None
        refused(lib.pcfa_flownet_corr_fwd(*q, B, C, H, W, *ok, s), PCFA_ERR_INVALID_ARG)
    for k in range(5):
        q = [p[0], p[1], p[2], p[4], p[5]]
        q[k] = None
        refused(lib.pcfa_flownet_corr_bwd(*q, B, C, H, W, *ok, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_flownet_corr_fwd(p[0], p[1], p[3], 0, C, H, W, *ok, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_flownet_corr_bwd(p[0], p[1], p[2], p[4], p[5], B, 0, H, W, *ok, s), PCFA_ERR_INVALID_ARG)


# --------------------------------------------------------------------------- ChannelNorm
@pytest.mark.parametrize("shape,huge", cv.CN_RUNS, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_channelnorm(record_property, shape, huge):
    lib = _lib()
    s = stream()
    B, C, H, W = shape
    x, dy = cv.cn_inputs(shape, huge)
    norm = cv.cn_ref_fwd(x)[0].float()
    fx, fo = _in(x), _out((B, 1, H, W))
    got_norm = _twice(lambda: lib.pcfa_channelnorm_fwd(fx.ptr(), fo.ptr(), B, C, H * W, 2, s), [fo], [fx])[0]
    fn, fd, fg = _in(norm), _in(dy), _out(shape)
    got_gin = _twice(lambda: lib.pcfa_channelnorm_bwd(fx.ptr(), fn.ptr(), fd.ptr(), fg.ptr(), B, C, H * W, 2, s), [fg], [fx, fn, fd])[0]
    r = cv.cn_check(shape, huge, got_norm, got_gin, record_property)
    record_property("worst_elem_ratio", "%.3g" % r[0])
    every = [fx, fo, fn, fd, fg]
    for q in (fo, fg):                      # written above: what a refused call must leave is their present state
        q.bits0 = q.buf.view(torch.int32).clone()
    calls = [(lib.pcfa_channelnorm_fwd(fx.ptr(), fo.ptr(), B, C, H * W, 1, s), PCFA_ERR_UNSUPPORTED),
             (lib.pcfa_channelnorm_bwd(fx.ptr(), fn.ptr(), fd.ptr(), fg.ptr(), B, C, H * W, 3, s), PCFA_ERR_UNSUPPORTED),
             (lib.pcfa_channelnorm_fwd(None, fo.ptr(), B, C, H * W, 2, s), PCFA_ERR_INVALID_ARG),
             (lib.pcfa_channelnorm_fwd(fx.ptr(), fo.ptr(), B, 0, H * W, 2, s), PCFA_ERR_INVALID_ARG),
             (lib.pcfa_channelnorm_bwd(fx.ptr(), fn.ptr(), fd.ptr(), None, B, C, H * W, 2, s), PCFA_ERR_INVALID_ARG),
             (lib.pcfa_channelnorm_bwd(fx.ptr(), fn.ptr(), fd.ptr(), fg.ptr(), B, C, 0, 2, s), PCFA_ERR_INVALID_ARG)]
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == [c[1] for c in calls]
    assert all(unchanged(q) for q in every), "a refused call touched a buffer"
