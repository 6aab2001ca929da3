"""pcfa_conv3x3_run_strided (csrc/conv3x3.hip): the direct F(2x2,3x3) launch over images that are channel prefixes of wider
slabs, through the C-ABI on fenced buffers (tests/fenced.py) whose gaps between the images hold sentinels.

The claim is bit identity, not a tolerance: every image equals the same image run alone through pcfa_conv3x3_run on a dense
copy.  Each call also checks the status, that the fences, the gaps and the inputs are unchanged, and that a second call
gives identical bits.  Shapes: the smallest at which the addressing can go wrong -- K not a multiple of 8 with N not a
multiple of 32 and a ragged last tile in both directions, and K a multiple of 8 with exactly one tile.
"""
import functools

import pytest
import torch

from pcfa_amd import _hip
from tests.fenced import DEV, NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, SENTINEL, Fenced, stream
from tests.gates import dense_stride, unchanged

pytestmark = pytest.mark.gpu
SLOPE = 0.1
SHAPES = [(3, 14, 40, 9, 19), (3, 16, 64, 8, 16)]
# name -> (bias, act, mask, mask_channels as a fraction of N, addend)
CASES = {"plain": (False, 0, False, 0, False), "bias_relu": (True, 1, False, 0, False),
         "mask_all": (False, 0, True, 0, False), "mask_prefix_addend": (False, 0, True, 0.5, True),
         "addend": (False, 0, False, 0, True)}


def _lib():
    return _hip.load()


@functools.lru_cache(maxsize=None)
def _problem(B, K, N, H, W):
    """inputs (CPU) and the packed forward weights (device, fenced) of one shape, shared by its cases"""
    gen = torch.Generator().manual_seed(K * 131 + N * 17 + H * W)
    x = torch.randn(B, K, H, W, generator=gen)
    w = torch.randn(N, K, 3, 3, generator=gen) / (9 * K) ** .5
    bias = torch.randn(N, generator=gen)
    mask = torch.randn(B, N, H, W, generator=gen)
    mask = torch.where(torch.rand(B, N, H, W, generator=gen) < 0.2, torch.zeros(()), mask)
    addend = torch.randn(B, N, H, W, generator=gen)
    lib = _lib()
    fw = Fenced(w.shape, dense_stride(w.shape), NAN_BITS).write(w)
    fp = Fenced((int(lib.pcfa_conv3x3_packed_floats(K, N)),), (1,), NAN_BITS)
    assert lib.pcfa_conv3x3_pack_weights(fw.ptr(), fp.ptr(), None, N, K, stream()) == 0
    torch.cuda.synchronize()
    assert fp.fence_intact()
    fp.bits0 = fp.buf.view(torch.int32).clone()
    return x, bias, mask, addend, fp


def _slab(t, channels):
    """t [B, C, H, W] as the leading C channels of a fenced slab with `channels` > C channels per image"""
    B, C, H, W = t.shape
    assert channels > C
    return Fenced((B, C, H, W), (channels * H * W, H * W, W, 1), SENTINEL).write(t)


def _dense(t):
    return Fenced(t.shape, dense_stride(t.shape), NAN_BITS).write(t)


def _strided(x, xs, fp, bias, mask, ms, addend, as_, out, os_, B, K, N, H, W, act, slope, mc):
    return _lib().pcfa_conv3x3_run_strided(x, xs, fp.ptr(), bias, mask, ms, addend, as_, out, os_, B, K, N, H, W, act, slope,
                                           mc, None, 0, stream())


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_%dto%d_%dx%d" % s)
def test_strided_equals_each_image_alone(shape, case):
    B, K, N, H, W = shape
    has_bias, act, has_mask, mc_frac, has_addend = CASES[case]
    x, bias, mask, addend, fp = _problem(*shape)
    plane = H * W
    mc = int(N * mc_frac)
    slope = SLOPE if has_mask else 0.
    # strides strictly larger than dense for all four tensors
    kx, kn = (K + 7) // 8 * 8 + (2 if K % 8 == 0 else 0), (N + 31) // 32 * 32 + (24 if N % 32 == 0 else 0)
    fx = _slab(x, kx)
    fm = _slab(mask, kn) if has_mask else None
    fa = _slab(addend, kn + 3) if has_addend else None
    fb = _dense(bias) if has_bias else None
    fo = Fenced((B, N, H, W), ((kn + 1) * plane, plane, W, 1), SENTINEL)
    ptr = lambda f: None if f is None else f.ptr()  # noqa: E731

    def run():
        rc = _strided(fx.ptr(), kx * plane, fp, ptr(fb), ptr(fm), kn * plane, ptr(fa), (kn + 3) * plane, fo.ptr(),
                      (kn + 1) * plane, B, K, N, H, W, act, slope, mc)
        torch.cuda.synchronize()
        return rc

    assert run() == 0
    assert fo.fence_intact(), "wrote outside the images (fence or gap)"
    for f in (fx, fm, fa, fb, fp):
        assert f is None or unchanged(f), "an input changed"
    got = fo.view().clone()
    assert bool(torch.isfinite(got).all()), "an output element was not written"

    for b in range(B):   # the same image alone, dense, through the existing entry
        dx = _dense(x[b:b + 1])
        dm = _dense(mask[b:b + 1]) if has_mask else None
        da = _dense(addend[b:b + 1]) if has_addend else None
        do = Fenced((1, N, H, W), dense_stride((1, N, H, W)), SENTINEL)
        assert _lib().pcfa_conv3x3_run(dx.ptr(), fp.ptr(), ptr(fb), ptr(dm), ptr(da), do.ptr(), 1, K, N, H, W, act, slope, mc,
                                       None, 0, stream()) == 0
        torch.cuda.synchronize()
        assert do.fence_intact()
        assert torch.equal(got[b:b + 1], do.view()), "image %d differs from its dense single-image run" % b

    fo.view().fill_(-7.)
    fo.bits0 = fo.buf.view(torch.int32).clone()
    assert run() == 0
    assert fo.fence_intact() and torch.equal(fo.view(), got), "the second call gave other bits"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_%dto%d_%dx%d" % s)
def test_refusals(shape):
    B, K, N, H, W = shape
    x, bias, mask, addend, fp = _problem(*shape)
    plane = H * W
    fx, fm, fa = _slab(x, K + 2), _slab(mask, N + 2), _slab(addend, N + 2)
    fo = Fenced((B, N, H, W), ((N + 2) * plane, plane, W, 1), SENTINEL)
    xs, ns = (K + 2) * plane, (N + 2) * plane
    ok = dict(xs=xs, ms=ns, as_=ns, os_=ns)
    for short in ("xs", "ms", "as_", "os_"):   # one stride below channels * H * W
        kw = dict(ok)
        kw[short] = (K if short == "xs" else N) * plane - 1
        rc = _strided(fx.ptr(), kw["xs"], fp, None, fm.ptr(), kw["ms"], fa.ptr(), kw["as_"], fo.ptr(), kw["os_"], B, K, N, H,
                      W, 0, SLOPE, 0)
        assert rc == PCFA_ERR_INVALID_ARG, (short, rc)
    # the strides of absent tensors are ignored
    assert _strided(fx.ptr(), xs, fp, None, None, 0, None, 0, fo.ptr(), ns, B, K, N, H, W, 0, 0., 0) == 0
    torch.cuda.synchronize()
    assert fo.fence_intact() and unchanged(fx) and unchanged(fm) and unchanged(fa)


def test_unsupported_dispatch_is_refused():
    """One small image with 8 channel chunks: pcfa_conv3x3_run's rules slice K over workgroups (workspace > 0)."""
    B, K, N, H, W = 1, 64, 32, 8, 16
    lib = _lib()
    assert lib.pcfa_conv3x3_workspace_bytes(B, K, N, H, W) > 0 and lib.pcfa_conv3x3_algo(B, K, N, H, W) == 23
    x, _, _, _, fp = _problem(B, K, N, H, W)
    fx = _slab(x, K + 8)
    fo = Fenced((B, N, H, W), dense_stride((B, N, H, W)), SENTINEL)
    rc = _strided(fx.ptr(), (K + 8) * H * W, fp, None, None, 0, None, 0, fo.ptr(), N * H * W, B, K, N, H, W, 0, 0., 0)
    torch.cuda.synchronize()
    assert rc == PCFA_ERR_UNSUPPORTED
    assert unchanged(fo), "a refused call wrote"


def test_live_prefix_of_the_packing():
    """N = 32 of a 64-channel packing: the first 32 channels of the N = 64 result bit for bit; the rest of the slab stays."""
    B, K, N, H, W = SHAPES[1]
    x, bias, mask, addend, fp = _problem(B, K, N, H, W)
    plane = H * W
    fx, fm, fb = _slab(x, K + 8), _slab(mask, N + 8), _dense(bias)
    full = Fenced((B, N, H, W), (N * plane, plane, W, 1), SENTINEL)
    assert _strided(fx.ptr(), (K + 8) * plane, fp, fb.ptr(), fm.ptr(), (N + 8) * plane, None, 0, full.ptr(), N * plane, B, K, N,
                    H, W, 0, SLOPE, 0) == 0
    half = Fenced((B, N // 2, H, W), (N * plane, plane, W, 1), SENTINEL)   # the same slab, 32 live channels per image
    assert _strided(fx.ptr(), (K + 8) * plane, fp, fb.ptr(), fm.ptr(), (N + 8) * plane, None, 0, half.ptr(), N * plane, B, K,
                    N // 2, H, W, 0, SLOPE, 0) == 0
    torch.cuda.synchronize()
    assert full.fence_intact() and half.fence_intact(), "channels >= 32 of the slab lost their sentinel"
    assert torch.equal(half.view(), full.view()[:, :N // 2])
    assert unchanged(fx) and unchanged(fm) and unchanged(fp)
