"""The correlation pyramid's build and backward through the C-ABI on fenced buffers (tests/fenced.py), against float64
computed from the same fp32 inputs, on every path of the host's dispatch: pcfa_corr_f2ext_fwd, pcfa_corr_pyramid_fwd
(csrc/corr_pyramid.hip, the pooled epilogue of csrc/gemm_tile.hpp), pcfa_corr_pyramid_fwd_bf16x3 (csrc/gemm_bf16x3.hip),
pcfa_corr_pyramid_bwd and pcfa_corr_pyramid_bwd_windows.  The references, the dispatch and store-map mirrors, the gates
and the shape tables are those of tests/pyramid.py; tests/test_pyramid_host_cpu.py shows on the CPU that a plain fp32
implementation passes every gate on every table case and that the mutants do not.

Inputs sit between NaN; outputs and the workspace sit between a sentinel NaN and are pre-filled with it, inside as well.
Each call checks (_twice): the status; every input and every fence bit-unchanged; a second call from the same initial
state gives identical bits.  A store past a slab reaches at most 2 W floats, far inside the fence of 16384.

Forward: the products are fed the CPU's f2ext (pyramid.f2ext_kernel32, which pcfa_corr_f2ext_fwd must equal bit for bit).
Level texels meet both gates per level; EVERY other float of every slab -- pads in x, pad rows in y, the zero tile -- is
+0.0 bit for bit, so no sentinel is left anywhere inside.  The library offers no probe of the path it took: the mirror
(pyramid.fwd_path) is the statement, recorded per case; on the pool path the positions that lost their sentinel must be
the store map's (pyramid.store_map), which ties that mirror to the kernel.

Backward: the dense call takes a dpyr that is random and non-zero in every slab position (pads and the zero tile must not
reach a gradient); the windowed call one that is non-zero on every position lookup.window_mask marks and exact zero
elsewhere, so a dropped segment edge shows in one element; its reference is the float64 backward of that dpyr.  The dense
fallbacks of the windowed call must give the dense call's bits.

Ratios are recorded as junit properties (--junitxml=FILE -o junit_family=xunit1).  PCFA_PYRAMID_UNPOOL=1 is read once per
process and has its own child-process test (tests/test_gpu_parity.py); it is not covered here.
"""
import ctypes

import pytest
import torch

from pcfa_amd import _hip
from tests import pyramid as pm
from tests.fenced import (NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, PCFA_ERR_WORKSPACE, SENTINEL, TINY, Fenced,
                          gamma, stream)
from tests.gates import dense_stride, unchanged
from tests.test_gemm_bf16x3_gpu import gates as bf16x3_gates
from tests.test_pyramid_bwd_segments_gpu import make_coords

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


def _lib():
    return _hip.load()


def _in(t, shift=0):
    return Fenced(t.shape, dense_stride(t.shape), NAN_BITS, shift).write(t)


def _out(shape):
    return Fenced(tuple(shape), dense_stride(tuple(shape)), SENTINEL)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _twice(call, outs, ins, scratch=()):
    """The per-call checks; returns the outputs of the first call on the CPU.  outs and scratch start from the sentinel
    (inside and fence) on both calls."""
    assert call() == 0
    torch.cuda.synchronize()
    gots = [o.view().clone() for o in outs]
    assert all(unchanged(f) for f in ins), "an input was written"
    assert all(o.fence_intact() for o in list(outs) + list(scratch)), "a store landed outside an output"
    for o in list(outs) + list(scratch):
        o.buf.view(torch.int32).copy_(o.bits0)
    assert call() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(o.view()), _bits(g)) for o, g in zip(outs, gots)), "not repeatable bit for bit"
    assert all(unchanged(f) for f in ins) and all(o.fence_intact() for o in list(outs) + list(scratch))
    return [g.cpu() for g in gots]


# --------------------------------------------------------------------------- pcfa_corr_f2ext_fwd
@pytest.mark.parametrize("c", pm.F2EXT, ids=pm.cid)
def test_f2ext(record_property, c):
    """Bit-equal to the fp32 restatement of the kernel's pooling, level l within gamma(3 l) of float64, every non-texel
    position +0.0."""
    lay, ref = pm.case_layout(c), pm.reference(c)
    fb, fo = _in(ref.f2), _out((c.B * c.D, lay.slab))
    got, = _twice(lambda: _lib().pcfa_corr_f2ext_fwd(fb.ptr(), fo.ptr(), c.B, c.D, c.H, c.W, c.L, stream()), [fo], [fb])
    assert pm.nontexel_faults(got, lay).shape[0] == 0, "a pad column of f2ext is not +0.0"
    assert torch.equal(_bits(got), _bits(ref.ext32)), "f2ext differs from (((p0 + p1) + p[wp]) + p[wp + 1]) / 4"
    want, mag = pm.f2ext(ref.f2, lay), pm.f2ext(ref.f2.abs(), lay)
    for l in range(c.L):
        idx = lay.index[l].reshape(-1)
        err = (got[:, idx].double() - want[:, idx]).abs()
        if l > 0:
            record_property("level%d_ratio" % l, "%.3g" % float((err / (gamma(3 * l) * mag[:, idx] + 3 * l * TINY)).max()))
        assert bool((err <= gamma(3 * l) * mag[:, idx] + 3 * l * TINY).all()), l      # (level 0 is a copy: no error at all)


# --------------------------------------------------------------------------- the forward products
def _x3_gate(D):
    return lambda got, want, P, l: bf16x3_gates(got, want, P, D, 0, extra=3 * l)


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("c", pm.FORWARD, ids=pm.cid)
def test_forward(record_property, c, arith):
    lib = _lib()
    lay, ref = pm.case_layout(c), pm.reference(c)
    Q = c.H * c.W
    a = _in(ref.f1.reshape(c.B, c.D, Q), c.shift)
    ext = _in(ref.ext32.reshape(c.B, c.D, lay.slab))
    pyr = _out((c.B * Q, lay.slab))
    fn, mirror = ((lib.pcfa_corr_pyramid_fwd, pm.fwd_path) if arith == "f32" else
                  (lib.pcfa_corr_pyramid_fwd_bf16x3, pm.fwd_bf16x3_path))
    got, = _twice(lambda: fn(a.ptr(), ext.ptr(), pyr.ptr(), c.B, c.D, c.H, c.W, c.L, stream()), [pyr], [a, ext])
    path = mirror(c.D, c.H, c.W, c.L, c.shift)
    record_property("path", path)
    if path == "pool":
        pos = torch.tensor(sorted({p for p, _ in pm.store_map(lay)}))
        assert int(pos.min()) >= 0 and int(pos.max()) < lay.slab
        want = torch.zeros(lay.slab, dtype=torch.bool)
        want[pos] = True
        written = _bits(got) != SENTINEL
        wrong = torch.nonzero(written != want.view(1, -1))
        assert wrong.shape[0] == 0, ("(row, position) stored though the store map has no writer, or the reverse",
                                     wrong[:8].tolist())
    pm.check_forward(got, c, record_property, gate=None if arith == "f32" else _x3_gate(c.D))


# --------------------------------------------------------------------------- the backward products
def _bwd_buffers(c, dpyr, windows):
    lib = _lib()
    lay, ref = pm.case_layout(c), pm.reference(c)
    Q = c.H * c.W
    size = lib.pcfa_corr_pyramid_bwd_windows_workspace_bytes if windows else lib.pcfa_corr_pyramid_bwd_workspace_bytes
    nbytes = int(size(c.B, c.D, c.H, c.W, c.L))
    assert nbytes > 0
    return dict(fd=_in(dpyr, c.dshift), a=_in(ref.f1.reshape(c.B, c.D, Q), c.shift),
                ext=_in(ref.ext32.reshape(c.B, c.D, lay.slab)), o1=_out((c.B, c.D, Q)), o2=_out((c.B, c.D, Q)),
                ws=_out(((nbytes + 3) // 4,)), nbytes=nbytes)


def run_dense(c, dpyr, windows_workspace=False):
    lib, b = _lib(), _bwd_buffers(c, dpyr, windows_workspace)
    return _twice(lambda: lib.pcfa_corr_pyramid_bwd(b["fd"].ptr(), b["a"].ptr(), b["ext"].ptr(), b["o1"].ptr(), b["o2"].ptr(),
                                                    b["ws"].ptr(), ctypes.c_size_t(b["nbytes"]), c.B, c.D, c.H, c.W, c.L,
                                                    stream()),
                  [b["o1"], b["o2"]], [b["fd"], b["a"], b["ext"]], [b["ws"]])


def run_windows(c, dpyr, coords, n_lists=None):
    """n_lists: how many coordinate lists are passed (default: all; more than there are: the lists repeat)."""
    lib, b = _lib(), _bwd_buffers(c, dpyr, True)
    fcs = [_in(x) for x in coords]
    n = n_lists or len(fcs)
    ptrs = (ctypes.c_void_p * n)(*[fcs[i % len(fcs)].ptr().value for i in range(n)])
    return _twice(lambda: lib.pcfa_corr_pyramid_bwd_windows(b["fd"].ptr(), b["a"].ptr(), b["ext"].ptr(), b["o1"].ptr(),
                                                            b["o2"].ptr(), b["ws"].ptr(), ctypes.c_size_t(b["nbytes"]), ptrs, n,
                                                            pm.R, c.B, c.D, c.H, c.W, c.L, stream()),
                  [b["o1"], b["o2"]], [b["fd"], b["a"], b["ext"]] + fcs, [b["ws"]])


@pytest.mark.parametrize("c", pm.BWD_DENSE, ids=pm.cid)
def test_backward_dense(record_property, c):
    p1, p2 = pm.bwd_paths(c.D, c.H, c.W, c.L, c.shift, 0, c.dshift)
    record_property("path_df1", p1)
    record_property("path_df2", p2)
    dpyr = pm.dense_dpyr(c)
    pm.check_backward(*run_dense(c, dpyr), dpyr, c, record_property)


def _coords(kind, c):
    """(the lists passed to the call, the lists whose lookups receive a gradient)"""
    if kind in pm.LOOKUP_KINDS:
        cs = pm.lookup_coords(kind, c)
        return cs, cs
    cs, skip = make_coords(kind, c.B, c.H, c.W)
    return cs, [x for i, x in enumerate(cs) if i != skip]


@pytest.mark.parametrize("kind", ("drift", "outside", "spread", "nograd") + pm.LOOKUP_KINDS)
@pytest.mark.parametrize("c", pm.WINDOWS, ids=pm.cid)
def test_backward_windows(record_property, c, kind):
    record_property("path", pm.bwd_windows_path(c.D, c.H, c.W, c.L, 3))
    cs, used = _coords(kind, c)
    dpyr = pm.window_dpyr(c, used, pm.R)
    assert kind == "outside" or float(dpyr.abs().max()) > 0
    pm.check_backward(*run_windows(c, dpyr, cs), dpyr, c, record_property)


@pytest.mark.parametrize("case", pm.WINDOW_FALLBACKS, ids=lambda f: "%s-%dlists" % (pm.cid(f[0]), f[1]))
def test_backward_windows_dense_fallback(record_property, case):
    """Q % 4 != 0, five levels, more lists than MAX_COORDS: the dense products, bit for bit."""
    c, n = case
    assert pm.bwd_windows_path(c.D, c.H, c.W, c.L, n) == "dense fallback"
    cs = pm.lookup_coords("sweep", c)[:3]
    dpyr = pm.window_dpyr(c, cs, pm.R)
    w1, w2 = run_windows(c, dpyr, cs, n)
    d1, d2 = run_dense(c, dpyr, windows_workspace=True)
    assert torch.equal(_bits(w1), _bits(d1)) and torch.equal(_bits(w2), _bits(d2)), "not the dense call's bits"
    pm.check_backward(w1, w2, dpyr, c, record_property)


# --------------------------------------------------------------------------- refusals
def test_refusals():
    """Refused calls return the header's status and leave every buffer -- fences and insides -- untouched."""
    lib = _lib()
    c = pm.Case(1, 4, 9, 32, 4)
    B, D, H, W, L = c[:5]
    lay, ref = pm.case_layout(c), pm.reference(c)
    Q = H * W
    b = _bwd_buffers(c, pm.dense_dpyr(c), True)
    f2, pyr, eo = _in(ref.f2), _out((B * Q, lay.slab)), _out((B * D, lay.slab))
    co = _in(make_coords("drift", B, H, W)[0][0])
    every = [b[k] for k in ("fd", "a", "ext", "o1", "o2", "ws")] + [f2, pyr, eo, co]
    a, ext, fd, o1, o2, ws = (b[k].ptr() for k in ("a", "ext", "fd", "o1", "o2", "ws"))
    dense_bytes = int(lib.pcfa_corr_pyramid_bwd_workspace_bytes(B, D, H, W, L))
    win_bytes = b["nbytes"]
    assert pm.bwd_windows_path(D, H, W, L, 1) == "runs" and win_bytes > dense_bytes
    ptrs = (ctypes.c_void_p * 1)(co.ptr().value)
    null = (ctypes.c_void_p * 1)(None)

    def refused(status, want):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    bad_dims = [(0, L), (B, 0), (B, 9)]
    for fn in (lib.pcfa_corr_pyramid_fwd, lib.pcfa_corr_pyramid_fwd_bf16x3):
        for args in ((None, ext, pyr.ptr()), (a, None, pyr.ptr()), (a, ext, None)):
            refused(fn(*args, B, D, H, W, L, stream()), PCFA_ERR_INVALID_ARG)
        for Bx, Lx in bad_dims:
            refused(fn(a, ext, pyr.ptr(), Bx, D, H, W, Lx, stream()), PCFA_ERR_INVALID_ARG)
    for args in ((None, eo.ptr()), (f2.ptr(), None)):
        refused(lib.pcfa_corr_f2ext_fwd(*args, B, D, H, W, L, stream()), PCFA_ERR_INVALID_ARG)
    for Bx, Lx in bad_dims:
        refused(lib.pcfa_corr_f2ext_fwd(f2.ptr(), eo.ptr(), Bx, D, H, W, Lx, stream()), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_corr_f2ext_fwd(f2.ptr(), eo.ptr(), 1, 1, 4, 16, 4, stream()), PCFA_ERR_INVALID_ARG)     # a level of size 0
    refused(lib.pcfa_corr_f2ext_fwd(f2.ptr(), eo.ptr(), 1, 1, 270, 480, 4, stream()), PCFA_ERR_UNSUPPORTED)  # levels > 64 KB of LDS

    def dense(p=(fd, a, ext, o1, o2), w=ws, n=dense_bytes, Bx=B, Lx=L):
        return lib.pcfa_corr_pyramid_bwd(*p, w, ctypes.c_size_t(n), Bx, D, H, W, Lx, stream())

    def windows(p=(fd, a, ext, o1, o2), w=ws, n=win_bytes, cs=ptrs, nc=1, r=pm.R, Bx=B, Lx=L):
        return lib.pcfa_corr_pyramid_bwd_windows(*p, w, ctypes.c_size_t(n), cs, nc, r, Bx, D, H, W, Lx, stream())

    for fn in (dense, windows):
        for i in range(5):
            refused(fn(p=tuple(None if k == i else x for k, x in enumerate((fd, a, ext, o1, o2)))), PCFA_ERR_INVALID_ARG)
        refused(fn(w=None), PCFA_ERR_INVALID_ARG)
        for Bx, Lx in bad_dims:
            refused(fn(Bx=Bx, Lx=Lx), PCFA_ERR_INVALID_ARG)
    refused(dense(n=dense_bytes - 4), PCFA_ERR_WORKSPACE)
    refused(windows(n=win_bytes - 4), PCFA_ERR_WORKSPACE)
    refused(windows(r=-1), PCFA_ERR_INVALID_ARG)
    refused(windows(cs=null), PCFA_ERR_INVALID_ARG)
