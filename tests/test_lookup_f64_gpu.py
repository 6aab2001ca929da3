"""The correlation lookups through the C-ABI on fenced buffers (tests/fenced.py), against float64 computed from the same
fp32 inputs, with windows steered onto every edge, sub-tile offset, pad texel and clamp of every level:
pcfa_corr_lookup_fwd / _bwd (csrc/corr_lookup.hip) and pcfa_lookup_convc1_pack_weights / _fwd / _bwd
(csrc/corr_lookup_conv.hip).  The references, the census of window classes, the coordinate cases, the shape tables and the
gates are those of tests/lookup.py; tests/test_lookup_host_cpu.py shows on the CPU that the cases reach every reachable
class and that a plain fp32 implementation passes every gate (worst statistical ratio there: 0.45 of the bound with the
factor MARGIN = 2, so no further margin is taken).

The pyramid is built on the CPU (random levels through lookup.tile: pad texels and the zero tile are exact zeros), which
isolates the lookups from the GEMM.  Inputs sit between NaN, outputs are pre-filled with a sentinel NaN, dpyr with seeded
non-zero values.  Each call checks (_twice): the status; every input and every fence bit-unchanged; no sentinel or
non-finite value left in an output; a second call from the same initial state gives identical bits.  The backwards must
leave dpyr bit-unchanged outside the lookups' windows (pcfa_corr_pyramid_bwd_windows skips what no window reaches).

Gates: |Y - Y64| <= 2 gamma(n) P + 2 u A + n 2^-126 and rel_l2 <= 2 u sqrt(n) over everything, per level and per census class
of at least 256 elements, with n = 8 (lookup forward: 1 - f, the product of the two factors, the product with the texel,
three sums, + 2 spare), 8 + k (scatter of k accumulated lookups: + one add into dpyr each), 324 + 1 + 8 = 333 (fused forward)
and 256 + 9 = 265 (fused backward).  Ratios and worst classes are recorded as junit properties (--junitxml=FILE -o
junit_family=xunit1).

Non-finite coordinates: make_origin clamps the floor to +-1e8 before the conversion to int (fmaxf / fminf return the other
operand for NaN) and the integer origin is then clamped to [-16, 4 tw] x [-16, th4] by clamp_origin (csrc/corr_window.hpp,
the one statement behind make_piece via Block::init, fwd_pieces and piece_setup via level_setup), so every address
is in range for any float; such a window has no piece inside its level.  The `nonfinite` case asserts that every other query
passes the gates, that the poisoned queries' dpyr slabs are bit-unchanged and that the fences hold; what the poisoned queries'
own forward outputs hold (NaN: 0 x NaN) is recorded, not asserted.
"""
import pytest
import torch

from pcfa_amd import _hip
from tests import lookup as lk
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, SENTINEL, Fenced, stream
from tests.gates import dense_stride, unchanged
from tests.test_winograd_f64_gpu import _mask_tensor

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


def _lib():
    return _hip.load()


def _fenced(t, fill=NAN_BITS):
    return Fenced(t.shape, dense_stride(t.shape), fill).write(t)


def _out(shape):
    return Fenced(shape, dense_stride(shape), SENTINEL)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _twice(call, out, ins, reset, finite=None):
    """The per-call checks; returns the output of the first call on the CPU.  reset(): the output's initial state for
    the second call (forward: -7 everywhere; backward: dpyr0).  finite: the elements that must be finite (default: all)."""
    assert call() == 0
    torch.cuda.synchronize()
    got = out.view().clone()
    assert all(unchanged(f) for f in ins), "an input was written"
    assert out.fence_intact(), "a store landed outside the output"
    ok = torch.isfinite(got).cpu()
    assert bool((ok if finite is None else ok | ~finite.expand_as(ok)).all()), \
        "non-finite output: a sentinel, or a NaN read from a fence"
    reset()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.view()), _bits(got)), "not repeatable bit for bit"
    assert all(unchanged(f) for f in ins) and out.fence_intact()
    return got.cpu()


def _cid(c):
    return "%s-%s" % (lk.sid(c[0]), c[1])


def _coords(shape, name):
    return dict(lk.cases(shape))[name]


def _keep(shape, coords):
    B, H, W, L, r = shape
    return lk.query_keep(lk.sanitize(coords)[1], B, H, W)


def _record_poisoned(record_property, got, shape, coords):
    B, H, W, L, r = shape
    bad = ~_keep(shape, coords).expand_as(got)
    if bool(bad.any()):
        v = got[bad]
        record_property("poisoned_outputs", "%d: %d nan, %d inf, %d zero, %d other" % (
            v.numel(), int(v.isnan().sum()), int(v.isinf().sum()), int((v == 0).sum()),
            int((torch.isfinite(v) & (v != 0)).sum())))


# --------------------------------------------------------------------------- the un-fused lookup
def run_lookup_fwd(shape, coords):
    lib = _lib()
    B, H, W, L, r = shape
    fp, fc = _fenced(lk.pyramid(shape)[1]), _fenced(coords)
    fo = _out((B, L * (2 * r + 1) ** 2, H, W))
    return _twice(lambda: lib.pcfa_corr_lookup_fwd(fp.ptr(), fc.ptr(), fo.ptr(), B, H, W, L, r, stream()), fo, [fp, fc],
                  lambda: fo.view().fill_(-7.0), _keep(shape, coords))


def run_lookup_bwd(shape, coords_list, gos, dpyr0):
    """The backwards of the lookups, accumulated into dpyr0 one call after the other."""
    lib = _lib()
    B, H, W, L, r = shape
    fcs, fgs = [_fenced(c) for c in coords_list], [_fenced(g) for g in gos]
    fd = _fenced(dpyr0, SENTINEL)

    def call():
        for fc, fg in zip(fcs, fgs):
            status = lib.pcfa_corr_lookup_bwd(fd.ptr(), fc.ptr(), fg.ptr(), B, H, W, L, r, stream())
            if status:
                return status
        return 0

    return _twice(call, fd, fcs + fgs, lambda: fd.view().copy_(dpyr0))


@pytest.mark.parametrize("case", lk.case_ids(lk.UNFUSED), ids=_cid)
def test_lookup_fwd(record_property, case):
    """pcfa_corr_lookup_fwd against lookup64, n = 8."""
    shape, name = case
    coords = _coords(shape, name)
    got = run_lookup_fwd(shape, coords)
    _record_poisoned(record_property, got, shape, coords)
    lk.check_lookup_fwd(got, shape, coords, record_property)


@pytest.mark.parametrize("case", lk.case_ids(lk.UNFUSED), ids=_cid)
def test_lookup_bwd(record_property, case):
    """pcfa_corr_lookup_bwd: dpyr bit-unchanged outside the windows, dpyr0 + scatter64 inside, n = 9."""
    shape, name = case
    B, H, W, L, r = shape
    coords = _coords(shape, name)
    go, dpyr0 = lk.gradients(shape, L * (2 * r + 1) ** 2)
    got = run_lookup_bwd(shape, [coords], [go], dpyr0)
    lk.check_lookup_bwd(got, dpyr0, shape, [coords], [go], record_property)


@pytest.mark.parametrize("shape", lk.UNFUSED, ids=lk.sid)
def test_lookup_bwd_accumulated(record_property, shape):
    """All of the shape's k lookups accumulated into one dpyr, n = 8 + k."""
    B, H, W, L, r = shape
    coords = [c for _, c in lk.cases(shape)]
    gos = [lk.gradients(shape, L * (2 * r + 1) ** 2, seed=k)[0] for k in range(len(coords))]
    dpyr0 = lk.gradients(shape, L * (2 * r + 1) ** 2)[1]
    got = run_lookup_bwd(shape, coords, gos, dpyr0)
    record_property("lookups", len(coords))
    lk.check_lookup_bwd(got, dpyr0, shape, coords, gos, record_property)


# --------------------------------------------------------------------------- the fused lookup + convc1
def pack(Wt):
    """pcfa_lookup_convc1_pack_weights into a NaN-fenced buffer of the documented size: (fenced weight, fenced packed)."""
    lib = _lib()
    floats = int(lib.pcfa_lookup_convc1_packed_floats(lk.COUT))
    assert floats == 2 * lk.COUT * lk.KP
    fw, fp = _fenced(Wt), Fenced((floats,), (1,), NAN_BITS)
    assert lib.pcfa_lookup_convc1_pack_weights(fw.ptr(), fp.ptr(), lk.COUT, lk.CIN, stream()) == 0
    torch.cuda.synchronize()
    assert unchanged(fw) and fp.fence_intact(), "packing wrote outside its buffer"
    assert bool(torch.isfinite(fp.view()).all()), "packing left a float unwritten"
    fp.bits0 = fp.buf.view(torch.int32).clone()
    return fw, fp


def run_convc1_fwd(shape, coords, Wt, bias, relu):
    lib = _lib()
    B, H, W, L, r = shape
    fw, fpk = pack(Wt)
    fp, fc, fb = _fenced(lk.pyramid(shape)[1]), _fenced(coords), _fenced(bias)
    fo = _out((B, lk.COUT, H, W))
    return _twice(lambda: lib.pcfa_lookup_convc1_fwd(fp.ptr(), fc.ptr(), fpk.ptr(), fb.ptr(), fo.ptr(), B, H, W, L, r, lk.COUT,
                                                     relu, stream()),
                  fo, [fw, fpk, fp, fc, fb], lambda: fo.view().fill_(-7.0), _keep(shape, coords))


def run_convc1_bwd(shape, coords, Wt, out, go, relu, dpyr0):
    lib = _lib()
    B, H, W, L, r = shape
    fw, fpk = pack(Wt)
    fc, fy, fg = _fenced(coords), _fenced(out), _fenced(go)
    fd = _fenced(dpyr0, SENTINEL)
    return _twice(lambda: lib.pcfa_lookup_convc1_bwd(fd.ptr(), fc.ptr(), fpk.ptr(), fy.ptr(), fg.ptr(), B, H, W, L, r, lk.COUT,
                                                     relu, stream()),
                  fd, [fw, fpk, fc, fy, fg], lambda: fd.view().copy_(dpyr0))


def test_convc1_pack():
    """Every float of the packed buffer is written and finite, the fences hold, the non-zero values are those of W taken
    twice (the forward and the backward operand order) and the rest -- 7 zero rows per level and operand order -- exact
    zeros; refused calls return the header's status and leave every buffer untouched."""
    lib = _lib()
    Wt = lk.nonzero_randn((lk.COUT, lk.CIN), torch.Generator().manual_seed(7))
    fw, fpk = pack(Wt)
    p = fpk.view().cpu()
    assert int((p == 0).sum()) == 2 * lk.COUT * (lk.KP - lk.CIN)
    for half in p.view(2, -1):
        assert torch.equal(half[half != 0].sort().values, Wt.reshape(-1).sort().values)
    assert int(lib.pcfa_lookup_convc1_packed_floats(128)) == -1

    shape = (1, 8, 8, 4, 4)
    B, H, W, L, r = shape
    gen = torch.Generator().manual_seed(8)
    fresh = Fenced((2 * lk.COUT * lk.KP,), (1,), NAN_BITS)
    fp, fc = _fenced(lk.pyramid(shape)[1]), _fenced(lk.identity(B, H, W))
    fb, fo = _fenced(torch.randn(lk.COUT, generator=gen)), _out((B, lk.COUT, H, W))
    fg = _fenced(torch.randn(B, lk.COUT, H, W, generator=gen))
    fy = _fenced(torch.randn(B, lk.COUT, H, W, generator=gen))
    fd = _fenced(lk.gradients(shape, lk.COUT)[1], SENTINEL)
    every = [fw, fpk, fresh, fp, fc, fb, fo, fg, fy, fd]

    def refused(status, want):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    refused(lib.pcfa_lookup_convc1_pack_weights(fw.ptr(), fresh.ptr(), 128, lk.CIN, stream()), PCFA_ERR_UNSUPPORTED)
    refused(lib.pcfa_lookup_convc1_pack_weights(fw.ptr(), fresh.ptr(), lk.COUT, lk.CIN - 1, stream()), PCFA_ERR_UNSUPPORTED)
    for Lx, rx, cout in ((3, 4, lk.COUT), (4, 3, lk.COUT), (4, 4, 128)):
        refused(lib.pcfa_lookup_convc1_fwd(fp.ptr(), fc.ptr(), fpk.ptr(), fb.ptr(), fo.ptr(), B, H, W, Lx, rx, cout, 1, stream()),
                PCFA_ERR_UNSUPPORTED)
        refused(lib.pcfa_lookup_convc1_bwd(fd.ptr(), fc.ptr(), fpk.ptr(), fy.ptr(), fg.ptr(), B, H, W, Lx, rx, cout, 1, stream()),
                PCFA_ERR_UNSUPPORTED)
    refused(lib.pcfa_lookup_convc1_fwd(fp.ptr(), fc.ptr(), fpk.ptr(), None, fo.ptr(), B, H, W, L, r, lk.COUT, 1, stream()),
            PCFA_ERR_INVALID_ARG)


FUSED_CASES = [(c, relu) for c in lk.case_ids(lk.FUSED) for relu in (0, 1)]


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "%s-relu%d" % (_cid(c[0]), c[1]))
def test_convc1_fwd(record_property, case):
    """pcfa_lookup_convc1_fwd against convc1_64(lookup64), n = 333, P and A pushed through |W| (ReLU is 1-Lipschitz)."""
    (shape, name), relu = case
    coords = _coords(shape, name)
    Wt, bias = lk.conv_weights()
    got = run_convc1_fwd(shape, coords, Wt, bias, relu)
    _record_poisoned(record_property, got, shape, coords)
    lk.check_convc1_fwd(got, shape, coords, Wt, bias, relu, record_property)


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "%s-relu%d" % (_cid(c[0]), c[1]))
def test_convc1_bwd(record_property, case):
    """pcfa_lookup_convc1_bwd with a crafted `out` (negatives, +-0, positive subnormals and normals): the ReLU mask is an
    input, no tie can blur the comparison.  dpyr bit-unchanged outside the windows, gated inside, n = 265."""
    (shape, name), relu = case
    B, H, W, L, r = shape
    coords = _coords(shape, name)
    Wt, _ = lk.conv_weights()
    go, dpyr0 = lk.gradients(shape, lk.COUT)
    out = _mask_tensor((B, lk.COUT, H, W), torch.Generator().manual_seed(3))
    got = run_convc1_bwd(shape, coords, Wt, out, go, relu, dpyr0)
    lk.check_convc1_bwd(got, dpyr0, shape, coords, Wt, out, go, relu, record_property)


def selectors():
    """Two 0/1 matrices [256][324] whose rows select all 324 taps once: rows 0..255 -> taps 0..255, rows 0..67 -> taps
    256..323 (the other rows zero)."""
    a, b = torch.zeros(lk.COUT, lk.CIN), torch.zeros(lk.COUT, lk.CIN)
    a[torch.arange(256), torch.arange(256)] = 1.0
    b[torch.arange(68), 256 + torch.arange(68)] = 1.0
    return (a, slice(0, 256), 256), (b, slice(256, 324), 68)


@pytest.mark.parametrize("case", [(s, n) for s in lk.FUSED[:2] for n in ("identity", "sweep0", "sweep2", "fractions")], ids=_cid)
def test_convc1_selects_taps(record_property, case):
    """W a 0/1 selection, bias 0, no ReLU: every product and sum of the 1x1 convolution is exact, so the fused kernels
    return their own taps and take their own tap gradients.

    Forward: the taps are NOT those of pcfa_corr_lookup_fwd bit for bit (measured on MI355X: they differ wherever a
    product with a weight is inexact).  Both kernels write t00 w00 + t01 w01 + t10 w10 + t11 w11 and hipcc contracts the
    first two terms either way round: the fused kernel computes fma(t00, w00, rn(t01 w01)) for every tap, the un-fused
    radius-4 kernel fma(t01, w01, rn(t00 w00)) for its tap columns a = 0..7 and the fused kernel's form for a = 8 (ISA of
    both kernels); the two fmas that follow are the same.  Both are roundings of the same blend, so the fused taps go
    through the lookup's own float64 gate (n = 8, per census class) and the rows that select nothing must be exact zeros;
    the share of taps that differ from the un-fused kernel's is recorded.

    Backward: the tap gradients W^T g are exact and the scatter is written with explicit fmaf in both kernels: the fused
    dpyr equals that of pcfa_corr_lookup_bwd fed the same tap gradients bit for bit (asserted), and passes the float64
    gate."""
    shape, name = case
    B, H, W, L, r = shape
    coords = _coords(shape, name)
    taps = run_lookup_fwd(shape, coords)
    go, dpyr0 = lk.gradients(shape, lk.COUT)
    ones = torch.ones(B, lk.COUT, H, W)
    fused_taps = torch.empty_like(taps)
    for k, (Wsel, chans, rows) in enumerate(selectors()):
        got = run_convc1_fwd(shape, coords, Wsel, torch.zeros(lk.COUT), 0)
        fused_taps[:, chans] = got[:, :rows]
        assert bool((got[:, rows:] == 0).all()), "a row that selects nothing is not zero"
        d_fused = run_convc1_bwd(shape, coords, Wsel, ones, go, 0, dpyr0)
        lk.check_convc1_bwd(d_fused, dpyr0, shape, coords, Wsel, ones, go, 0, record_property, "sel%d_bwd_" % k)
        g_taps = torch.zeros(B, lk.CIN, H, W)
        g_taps[:, chans] = go[:, :rows]
        d_unfused = run_lookup_bwd(shape, [coords], [g_taps], dpyr0)
        assert torch.equal(_bits(d_fused), _bits(d_unfused)), "the fused scatter differs from pcfa_corr_lookup_bwd's"
    record_property("fused_taps_differing_from_unfused", "%.3g" % float((fused_taps != taps).double().mean()))
    lk.check_lookup_fwd(fused_taps, shape, coords, record_property, "sel_fwd_")
