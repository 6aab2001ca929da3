"""The upsamplers through the C-ABI on fenced buffers (tests/fenced.py), against float64: pcfa_convex_upsample_fwd / _bwd,
pcfa_upsample_bilinear_fwd / _bwd, pcfa_upsample_nearest4_fwd / _bwd (csrc/upsample_ops.hip).  References, emulations,
inputs, case tables and gates are those of tests/upsample.py (every bound is derived in its docstring, which also names the
cases that reach each kernel); tests/test_upsample_host_cpu.py shows on the CPU that the cases hold their classes and that the
fp32 emulations pass every gate.

Inputs sit between NaN; outputs and the convex backward's workspace (exactly pcfa_convex_upsample_workspace_floats() long)
are pre-filled with a sentinel NaN.  Each call checks (_twice of tests/test_warp_f64_gpu.py): the status; every input and
every fence bit-unchanged; no sentinel or non-finite value left in an output; a second call from the same state gives
identical bits (no kernel here uses atomics).  Ratios and worst groups are recorded as junit properties.

The convex wild case (a pixel whose nine logits are all -inf, all +inf or all NaN): fences, inputs and statuses as everywhere;
the gates on everything such a pixel does not feed -- not its own 64 outputs, its grad_mask column and the 3 x 3 grad_flow
neighbourhood, whose contents are recorded.
"""
import pytest
import torch

from pcfa_amd import _hip
from tests import upsample as up
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, SENTINEL, Fenced, stream
from tests.gates import dense_stride, unchanged
from tests.test_warp_f64_gpu import _bits, _twice, _ws

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


def _lib():
    return _hip.load()


def _in(t, shift=0):
    return Fenced(t.shape, dense_stride(t.shape), NAN_BITS, shift).write(t)


def _out(shape, shift=0):
    return Fenced(tuple(shape), dense_stride(tuple(shape)), SENTINEL, shift)


def _holds(v):
    return "%d: %d nan, %d inf, %d zero, %d other" % (v.numel(), int(v.isnan().sum()), int(v.isinf().sum()), int((v == 0).sum()),
                                                      int((torch.isfinite(v) & (v != 0)).sum()))


# --------------------------------------------------------------------------- convex
def run_convex(c, fwd=True, bwd=True, shift=0):
    """(out, grad_flow, grad_mask) of one case; shift: floats of misalignment of flow, mask, grad_flow, grad_mask and the
    workspace (out and grad_out must be 16-B aligned)."""
    lib = _lib()
    N, H, W = c.shape
    ff, fm = _in(c.flow, shift), _in(c.mask, shift)
    dec = (lambda m: None) if c.poisoned is None else (lambda m: ~m)
    out = gf = gm = None
    if fwd:
        fo = _out((N, 2, 8 * H, 8 * W))
        out = _twice(lambda: lib.pcfa_convex_upsample_fwd(ff.ptr(), fm.ptr(), fo.ptr(), N, H, W, stream()), [fo], [ff, fm],
                     decided=[dec(getattr(c.poisoned, "out", None))])[0]
    if bwd:
        fg, fgf, fgm = _in(c.gout), _out((N, 2, H, W), shift), _out((N, 576, H, W), shift)
        nws = int(lib.pcfa_convex_upsample_workspace_floats(N, H, W))
        assert nws == 18 * N * H * W
        ws = _ws(4 * nws, shift)
        gf, gm = _twice(lambda: lib.pcfa_convex_upsample_bwd(ff.ptr(), fm.ptr(), fg.ptr(), fgf.ptr(), fgm.ptr(), ws.ptr(), N, H, W,
                                                             stream()), [fgf, fgm], [ff, fm, fg], ws,
                        decided=[dec(getattr(c.poisoned, "gf", None)), dec(getattr(c.poisoned, "gm", None))])
    return out, gf, gm


@pytest.mark.parametrize("shape", up.CONVEX_SHAPES, ids=str)
def test_convex_upsample(record_property, shape):
    """pcfa_convex_upsample_fwd and _bwd: grad_out random, zero and one-hot."""
    for variant in up.CONVEX_GOUTS:
        c = up.convex_case(shape, variant)
        out, gf, gm = run_convex(c, fwd=variant == "random")
        up.convex_check(c, out, gf, gm, record_property, variant + "_")
        if variant == "zero":
            assert bool((gf == 0).all()) and bool((gm == 0).all()), "zero grad_out must give exact zeros"


def test_convex_upsample_unaligned_operands(record_property):
    """flow, mask, grad_flow, grad_mask and the workspace 4 bytes off a 16-byte boundary: the same bits."""
    c = up.convex_case((2, 3, 65))
    a, b = run_convex(c), run_convex(c, shift=1)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    up.convex_check(c, *b, record_property, "shift_")


def test_convex_upsample_wild(record_property):
    c = up.convex_case(up.WILD_SHAPE, "random", True)
    out, gf, gm = run_convex(c)
    up.convex_check(c, out, gf, gm, record_property, "wild_")
    for name, t, m in (("out", out, c.poisoned.out), ("grad_flow", gf, c.poisoned.gf), ("grad_mask", gm, c.poisoned.gm)):
        record_property("wild_poisoned_" + name, _holds(t[m.expand_as(t)]))


def test_convex_upsample_statuses():
    lib = _lib()
    c = up.convex_case((2, 1, 5))
    N, H, W = c.shape
    ff, fm, fg = _in(c.flow), _in(c.mask), _in(c.gout)
    fg1 = _in(c.gout, 1)
    fo, fo1, fgf, fgm = _out((N, 2, 8 * H, 8 * W)), _out((N, 2, 8 * H, 8 * W), 1), _out((N, 2, H, W)), _out((N, 576, H, W))
    ws = _ws(4 * 18 * N * H * W)
    every = [ff, fm, fg, fg1, fo, fo1, fgf, fgm, ws]
    s = stream()
    p = lambda f: f.ptr()   # noqa: E731

    def refused(status, want=PCFA_ERR_INVALID_ARG):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    fwd = lambda a=p(ff), b=p(fm), o=p(fo), N_=N, H_=H, W_=W: lib.pcfa_convex_upsample_fwd(a, b, o, N_, H_, W_, s)   # noqa: E731
    bwd = lambda a=p(ff), b=p(fm), g=p(fg), x=p(fgf), y=p(fgm), w=p(ws), N_=N, H_=H, W_=W: \
        lib.pcfa_convex_upsample_bwd(a, b, g, x, y, w, N_, H_, W_, s)   # noqa: E731
    for k in "abo":
        refused(fwd(**{k: None}))
    for k in "abgxyw":
        refused(bwd(**{k: None}))
    refused(fwd(o=p(fo1)))
    refused(bwd(g=p(fg1)))
    for kw in (dict(N_=0), dict(H_=0), dict(W_=0), dict(N_=65536), dict(H_=65536), dict(N_=-1)):
        refused(fwd(**kw))
        refused(bwd(**kw))
    assert int(lib.pcfa_convex_upsample_workspace_floats(0, H, W)) == -1
    assert int(lib.pcfa_convex_upsample_workspace_floats(3, 5, 7)) == 18 * 3 * 5 * 7


# --------------------------------------------------------------------------- bilinear
def run_bilinear_fwd(shape, f, mul):
    lib = _lib()
    P, H, W = shape
    x, _ = up.bilinear_inputs(shape, f)
    fx, fo = _in(x), _out((P, H * f, W * f))
    return _twice(lambda: lib.pcfa_upsample_bilinear_fwd(fx.ptr(), fo.ptr(), P, H, W, f, mul, stream()), [fo], [fx])[0]


def run_bilinear_bwd(shape, f, mul, variant):
    lib = _lib()
    P, H, W = shape
    fg, fo = _in(up.bilinear_gout(shape, f, variant)), _out((P, H, W))
    return _twice(lambda: lib.pcfa_upsample_bilinear_bwd(fg.ptr(), fo.ptr(), P, H, W, f, mul, stream()), [fo], [fg])[0]


@pytest.mark.parametrize("shape", up.BILINEAR_SHAPES, ids=str)
@pytest.mark.parametrize("f", up.FACTORS)
def test_upsample_bilinear(record_property, shape, f):
    """pcfa_upsample_bilinear_fwd and _bwd at mul 20, 1, -0.5; grad_out random, zero and one-hot at the corners and inside (mul
    20); the adjoint identity on the kernel's own outputs."""
    for mul in up.MULS:
        tag = "mul%g_" % mul
        y = run_bilinear_fwd(shape, f, mul)
        rf = up.bilinear_check_fwd(shape, f, mul, y, record_property, tag)
        for variant in (up.BILINEAR_GOUTS if mul == up.MULS[0] else ("random",)):
            gx = run_bilinear_bwd(shape, f, mul, variant)
            rb = up.bilinear_check_bwd(shape, f, mul, variant, gx, record_property, tag)
            if variant == "random":
                a = up.adjoint_ratio(shape, f, mul, y, gx, rf[2], rb[2])
                record_property(tag + "adjoint_ratio", "%.3g" % a)
                assert a <= 1, ("adjoint identity", a)


def test_upsample_bilinear_statuses():
    lib = _lib()
    shape, f = (2, 7, 5), 2
    P, H, W = shape
    x, g = up.bilinear_inputs(shape, f)
    fx, fg, fo, fgx = _in(x), _in(g), _out(g.shape), _out(x.shape)
    s = stream()
    p = lambda t: t.ptr()   # noqa: E731

    def refused(status, want):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(t) for t in (fx, fg, fo, fgx)), "a refused call touched a buffer"

    for fn, a, b in ((lib.pcfa_upsample_bilinear_fwd, fx, fo), (lib.pcfa_upsample_bilinear_bwd, fg, fgx)):
        refused(fn(None, p(b), P, H, W, f, 20.0, s), PCFA_ERR_INVALID_ARG)
        refused(fn(p(a), None, P, H, W, f, 20.0, s), PCFA_ERR_INVALID_ARG)
        refused(fn(p(a), p(b), 0, H, W, f, 20.0, s), PCFA_ERR_INVALID_ARG)
        refused(fn(p(a), p(b), P, 0, W, f, 20.0, s), PCFA_ERR_INVALID_ARG)
        refused(fn(p(a), p(b), P, H, 0, f, 20.0, s), PCFA_ERR_INVALID_ARG)
        refused(fn(p(a), p(b), P, H, W, 0, 20.0, s), PCFA_ERR_INVALID_ARG)
        refused(fn(p(a), p(b), P, H, W, -2, 20.0, s), PCFA_ERR_INVALID_ARG)
        refused(fn(p(a), p(b), 65536, H, W, f, 20.0, s), PCFA_ERR_UNSUPPORTED)
    refused(lib.pcfa_upsample_bilinear_fwd(p(fx), p(fo), P, 16384, W, 4, 20.0, s), PCFA_ERR_UNSUPPORTED)    # H f = 65536
    refused(lib.pcfa_upsample_bilinear_bwd(p(fg), p(fgx), P, 65536, W, 1, 20.0, s), PCFA_ERR_UNSUPPORTED)


# --------------------------------------------------------------------------- nearest-4
@pytest.mark.parametrize("shape", up.NEAREST_SHAPES, ids=str)
@pytest.mark.parametrize("div", [0, 1])
def test_upsample_nearest4(shape, div):
    """Bit-equal to nn.Upsample(scale_factor=4, mode='nearest')(x op 20) and to the float64 sum of the 16 gradients op 20."""
    lib = _lib()
    P, H, W = shape
    x, gy, y, gx = up.nearest4_case(shape, div)
    fx, fo = _in(x), _out(y.shape)
    got = _twice(lambda: lib.pcfa_upsample_nearest4_fwd(fx.ptr(), fo.ptr(), P, H, W, up.NEAREST_S, div, stream()), [fo], [fx])[0]
    assert torch.equal(_bits(got), _bits(y))
    fg, fgx = _in(gy), _out(x.shape)
    got = _twice(lambda: lib.pcfa_upsample_nearest4_bwd(fg.ptr(), fgx.ptr(), P, H, W, up.NEAREST_S, div, stream()), [fgx], [fg])[0]
    assert torch.equal(_bits(got), _bits(gx))
    for t in (fo, fgx):                 # the refusals below must leave the results as they are
        t.bits0 = t.buf.view(torch.int32).clone()
    s = stream()
    for status in (lib.pcfa_upsample_nearest4_fwd(fx.ptr(), fo.ptr(), P, H, W, 0.0, 1, s),
                   lib.pcfa_upsample_nearest4_bwd(fg.ptr(), fgx.ptr(), P, H, W, 0.0, 1, s),
                   lib.pcfa_upsample_nearest4_fwd(None, fo.ptr(), P, H, W, 20.0, div, s),
                   lib.pcfa_upsample_nearest4_bwd(fg.ptr(), fgx.ptr(), P, 0, W, 20.0, div, s)):
        assert status == PCFA_ERR_INVALID_ARG
    assert lib.pcfa_upsample_nearest4_fwd(fx.ptr(), fo.ptr(), 65536, H, W, 20.0, div, s) == PCFA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(unchanged(t) for t in (fx, fg, fo, fgx)), "a refused call touched a buffer"
