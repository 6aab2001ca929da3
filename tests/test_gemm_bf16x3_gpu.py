"""The split-bf16 GEMM core (csrc/gemm_bf16x3.hip: pcfa_gemm_bf16x3, pcfa_corr_pyramid_fwd_bf16x3) against float64.

Every fp32 operand is split into three round-to-nearest bf16 pieces, a = a0 + a1 + a2 exactly, and the six products
a_i b_j with i + j <= 2 run on v_mfma_f32_32x32x16_bf16 (exact products, fp32 accumulation).  The claim is fp32 accuracy,
so the variant is held to the fp32 core's gates (tests/test_gemm_core_gpu.py), on fenced operands, with every reference
computed in float64 from the same fp32 inputs.  u = 2^-24.

Element bound (holds for ANY summation order, also inside the MFMA's 16-term block, whose internal rounding is not
documented):

    |C - C64| <= 2 gamma(n6) |alpha| (|A||B|) + u |alpha| (|A||B|) + tiny,     n6 = 6 K + splits + 8

n6: six accumulations per k, at most five combines (the `lo` and `hi` accumulators, the ordered split-K reduction),
alpha (two roundings), one spare; the factor 2 as in the fp32 test.  The second term is the truncation: the dropped
a1 b2 + a2 b1 + a2 b2 are at most u |a b| per product (tests/test_mfma_switch_host_cpu.py).  tiny = 6 K 2^-126.

Statistical gate, unchanged from the fp32 core:   rel_l2(C, C64) <= 2 u sqrt(K + splits + 2).
A kernel that lost a cross term of order 2^-8 (i + j = 1) or 2^-16 (i + j = 2) does not pass it:
test_three_products_fail_the_gate shows the gate sees the smaller of the two.

Each case calls twice and asserts equal bits, records its ratios as junit properties, and records the fp32 kernel's
rel-L2 ratio on the same operands next to its own.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from pcfa_amd import _hip, hip_ops
from tests.fenced import (DEV, NAN_BITS, PCFA_ERR_UNSUPPORTED, PCFA_ERR_WORKSPACE, SENTINEL, U, Fenced, gamma)
from tests.fenced import stream as _stream
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))


def n6(K, splits=1, extra=0):
    return 6 * K + splits + 8 + extra


def gates(got, want64, absprod64, K, splits=1, extra=0):
    """(worst element err / bound, rel-L2 / (2 u sqrt(K + splits + 2 + extra))); both must be <= 1."""
    got = got.detach().double().cpu()
    bound = 2 * gamma(n6(K, splits, extra)) * absprod64 + U * absprod64 + 6 * K * 2.0 ** -126
    elem = float(((got - want64).abs() / bound).max())
    rel = rel_l2(got, want64) / (2 * U * math.sqrt(K + splits + 2 + extra))
    return elem, rel


def _fast_rule(lay, M, N, K, lda, ldb, bsA, bsB, shift):
    """The host rule that picks the branch-free FAST loader (the fp32 twin's rule, restated in gemm_bf16x3.hip)."""
    ak, bk = lay
    vec_a = shift % 4 == 0 and lda % 4 == 0 and (M if ak else K) % 4 == 0 and bsA % 4 == 0
    vec_b = ldb % 4 == 0 and (N if bk else K) % 4 == 0 and bsB % 4 == 0
    return vec_a and vec_b and K % 4 == 0 and min(M, N, K) >= 4


def operands(M, N, K, batch=1, bsA0=False, seed=0):
    gen = torch.Generator().manual_seed(seed * 7919 + M * 131 + N * 17 + K)
    return torch.randn(1 if bsA0 else batch, M, K, generator=gen), torch.randn(batch, K, N, generator=gen)


def run_gemm(lay, A, B, splits=1, alpha=1.0, lda_pad=0, ldb_pad=0, ldc_pad=0, bs_pad=0, shift=0, ws_short=0,
             check_fast=None, entry="pcfa_gemm_bf16x3"):
    """One call of `entry` on fenced operands A [batch or 1, M, K], B [batch, K, N] (A with one batch item: bsA = 0);
    returns (C [batch, M, N] float32 CPU, status).  Layout (a_kmajor, b_kmajor): A(m, k) at A[m lda + k] (0) or
    A[k lda + m] (1); B(k, n) at B[n ldb + k] (0) or B[k ldb + n] (1).  Called twice: equal bits."""
    ak, bk = lay
    batch, K, N = B.shape
    M = A.shape[1]
    bsA0 = A.shape[0] == 1 and batch > 1
    lda = (M if ak else K) + lda_pad
    ldb = (N if bk else K) + ldb_pad
    ldc = N + ldc_pad
    bsA = 0 if bsA0 else lda * (K if ak else M) + bs_pad
    bsB = ldb * (K if bk else N) + bs_pad
    bsC = ldc * M + (bs_pad if splits == 1 else 0)
    if check_fast is not None:
        assert _fast_rule(lay, M, N, K, lda, ldb, bsA, bsB, shift) == check_fast
    fa = Fenced((A.shape[0], M, K), (bsA, 1, lda) if ak else (bsA, lda, 1), NAN_BITS, shift).write(A)
    fb = Fenced((batch, K, N), (bsB, ldb, 1) if bk else (bsB, 1, ldb), NAN_BITS).write(B)
    fc = Fenced((batch, M, N), (bsC, ldc, 1), SENTINEL)
    lib = _hip.load()
    wbytes = int(getattr(lib, entry + "_workspace_bytes")(M, N, batch, splits))
    fw = Fenced((max(wbytes // 4, 1),), (1,), NAN_BITS) if splits > 1 else None
    fn = getattr(lib, entry)

    def call():
        return fn(fa.ptr(), fb.ptr(), fc.ptr(), M, N, K, lda, ldb, ldc, ak, bk, batch, bsA, bsB, bsC,
                  ctypes.c_float(alpha), splits, fw.ptr() if fw else None, ctypes.c_size_t(max(wbytes - ws_short, 0)),
                  _stream())

    st = call()
    torch.cuda.synchronize()
    C = fc.view().clone()
    assert fa.fence_intact() and fb.fence_intact(), "an operand was written"
    assert fc.fence_intact(), "a store landed outside C"
    assert fw is None or fw.fence_intact(), "a store landed outside the workspace"
    if st == 0:
        assert call() == 0
        torch.cuda.synchronize()
        assert torch.equal(fc.view().view(torch.int32), C.view(torch.int32)), "not repeatable bit for bit"
    else:
        assert torch.equal(fc.buf.view(torch.int32), fc.bits0), "a refused call touched C"
    return C.cpu(), st


def check_gemm(record_property, lay, M, N, K, batch=1, splits=1, alpha=1.0, bsA0=False, scale=(1.0, 1.0), **kw):
    A, B = operands(M, N, K, batch, bsA0)
    A, B = A * scale[0], B * scale[1]
    C, st = run_gemm(lay, A, B, splits=splits, alpha=alpha, **kw)
    assert st == 0, st
    assert bool(torch.isfinite(C).all()), "non-finite C: a NaN fence value or an unwritten element reached C"
    A64, B64 = A.double(), B.double()
    want = alpha * torch.matmul(A64, B64)
    absprod = abs(alpha) * torch.matmul(A64.abs(), B64.abs())
    elem, rel = gates(C, want, absprod, K, splits)
    C32, st32 = run_gemm(lay, A, B, splits=splits, alpha=alpha, entry="pcfa_gemm_f32", **kw)
    assert st32 == 0
    record_property("elem_ratio", "%.3g" % elem)
    record_property("rel_ratio", "%.3g" % rel)
    record_property("f32_rel_ratio", "%.3g" % (rel_l2(C32.double(), want) / (2 * U * math.sqrt(K + splits + 2))))
    print("bf16x3 elem %.3g rel %.3g | f32 rel %.3g" % (elem, rel, rel_l2(C32.double(), want) /
                                                       (2 * U * math.sqrt(K + splits + 2))))
    assert elem <= 1 and rel <= 1, (elem, rel)
    return C, want


LAYOUTS = [(0, 0), (0, 1), (1, 1)]
SIZES = [(4, 4, 4), (128, 128, 16), (129, 257, 16), (127, 128, 768)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "%d%d" % l)
def test_layouts_and_sizes(record_property, lay, size):
    """The three layouts from one block with one k-step up to several blocks with ragged M / N and 48 k-steps; dense
    operands, so the shapes whose dimensions allow it run the FAST loader and the others the masked one."""
    M, N, K = size
    check_gemm(record_property, lay, M, N, K)


@pytest.mark.parametrize("loader", ["fast", "masked"])
@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "%d%d" % l)
def test_both_loaders(record_property, lay, loader):
    """One aligned shape on both loaders (A's base pointer moved one float off 16-B alignment forces the masked one):
    several k-steps, two blocks along N."""
    check_gemm(record_property, lay, 128, 256, 64, alpha=0.5, shift=0 if loader == "fast" else 1,
               check_fast=loader == "fast")


@pytest.mark.parametrize("K", [1, 15, 17, 33])
@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "%d%d" % l)
def test_k_tails(record_property, lay, K):
    """K off the 16-wide k-step of the MFMA at 32x32: the tail of the last step contributes exact zeros, never the NaN
    behind the operand."""
    check_gemm(record_property, lay, 32, 32, K)


LOADERS = [  # (id, layout, M, N, K, batch, kwargs, fast)
    ("ld+4", (0, 1), 128, 128, 64, 1, dict(lda_pad=4, ldb_pad=4, alpha=-3.0), True),
    ("ld+3", (0, 1), 128, 128, 64, 1, dict(lda_pad=3, ldb_pad=3, alpha=-3.0), False),
    ("ld+4-00", (0, 0), 129, 127, 33, 1, dict(lda_pad=4, ldb_pad=4, alpha=0.3), False),
    ("ld+4-11", (1, 1), 128, 256, 64, 1, dict(lda_pad=4, ldb_pad=8, alpha=0.3), True),
    ("ld+3-11", (1, 1), 128, 256, 64, 1, dict(lda_pad=3, ldb_pad=5), False),
    ("ldc", (0, 1), 129, 127, 33, 1, dict(ldc_pad=5, alpha=1.7), False),
    ("ldc-fast", (1, 1), 128, 128, 16, 1, dict(ldc_pad=4, alpha=-3.0), True),
    ("shift1", (0, 0), 128, 128, 64, 1, dict(shift=1, alpha=1.7), False),
    ("shift2-11", (1, 1), 128, 128, 64, 1, dict(shift=2), False),
    ("batch2-bsA0", (0, 1), 127, 256, 64, 2, dict(bsA0=True, alpha=0.3), True),
    ("batch2-bsA0-masked", (0, 1), 129, 257, 33, 2, dict(bsA0=True, alpha=-3.0), False),
    ("batch2-bs-pad", (0, 0), 127, 129, 64, 2, dict(bs_pad=8, lda_pad=4), True),
]


@pytest.mark.parametrize("case", LOADERS, ids=[c[0] for c in LOADERS])
def test_loaders(record_property, case):
    """Leading dimensions past the row length (% 4 == 0 keeps FAST, odd forces the masked loader), ldc > N, an A base
    pointer off 16-B alignment, batch 2 with bsA = 0 (one A for every batch item, as conv1x1 calls it) and with padded
    batch strides, and alpha that is no power of two.  The padding between rows is NaN: any read of it poisons C."""
    _, lay, M, N, K, batch, kw, fast = case
    check_gemm(record_property, lay, M, N, K, batch=batch, check_fast=fast, **kw)


SPLITS = [  # (layout, M, N, K, batch, splits, alpha)
    ((0, 1), 127, 128, 768, 1, 8, 1.0),      # attn . v's form
    ((1, 1), 128, 128, 768, 2, 8, 0.3),      # attn^T . g's form
    ((0, 0), 128, 128, 48, 2, 8, -3.0),      # kchunk 16: splits 3..7 start past K and write exact zeros
    ((0, 1), 129, 127, 48, 1, 8, 1.0),       # the same on the masked loader
    ((1, 1), 128, 128, 100, 2, 3, 1.0),      # kchunk 48: ragged K tail in the last split
]


@pytest.mark.parametrize("case", SPLITS, ids=lambda c: "%d%d-%dx%dx%d-b%d-s%d" % (c[0] + c[1:6]))
def test_split_k(record_property, case):
    """Split-K into the fenced workspace + the ordered reduction, including more splits than K tiles."""
    lay, M, N, K, batch, splits, alpha = case
    check_gemm(record_property, lay, M, N, K, batch=batch, splits=splits, alpha=alpha)


def test_refusals():
    """A short workspace gives PCFA_ERR_WORKSPACE and the (1, 0) layout PCFA_ERR_UNSUPPORTED, like the fp32 twin; the
    fences and C stay untouched (run_gemm asserts both)."""
    A, B = operands(64, 64, 32)
    assert run_gemm((0, 1), A, B, splits=3, ws_short=4)[1] == PCFA_ERR_WORKSPACE
    assert run_gemm((0, 1), A, B, splits=3, ws_short=4, entry="pcfa_gemm_f32")[1] == PCFA_ERR_WORKSPACE
    assert run_gemm((1, 0), A, B)[1] == PCFA_ERR_UNSUPPORTED
    assert run_gemm((1, 0), A, B, entry="pcfa_gemm_f32")[1] == PCFA_ERR_UNSUPPORTED


@pytest.mark.parametrize("scale", [(2.0 ** 60, 2.0 ** -60), (2.0 ** -60, 2.0 ** 60)], ids=["A-up", "A-down"])
@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "%d%d" % l)
def test_exponent_range(record_property, lay, scale):
    """A scaled by 2^60 and B by 2^-60 (and the reverse): the pieces a1, a2 sit 2^-8 and 2^-16 below, far from either end
    of the exponent range, and the split is scale-invariant -- both gates hold unchanged."""
    check_gemm(record_property, lay, 128, 128, 64, scale=scale)


@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: "%d%d" % l)
def test_non_finite_operand(record_property, lay):
    """One +inf in row 5 of A: that row of C is non-finite (not necessarily +inf: inf - inf in the split makes NaN), every
    other row passes the gates."""
    M, N, K = 32, 32, 16
    A, B = operands(M, N, K)
    A[0, 5, 3] = float("inf")
    C, st = run_gemm(lay, A, B)
    assert st == 0
    assert not bool(torch.isfinite(C[0, 5]).any()), "row 5 holds a finite value"
    keep = [r for r in range(M) if r != 5]
    assert bool(torch.isfinite(C[0, keep]).all())
    A64, B64 = A[:, keep].double(), B.double()
    elem, rel = gates(C[:, keep], torch.matmul(A64, B64), torch.matmul(A64.abs(), B64.abs()), K)
    record_property("elem_ratio", "%.3g" % elem)
    record_property("rel_ratio", "%.3g" % rel)
    assert elem <= 1 and rel <= 1, (elem, rel)


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _split3(a):
    a0 = _bf(a)
    a1 = _bf(a - a0)
    return a0, a1, _bf((a - a0) - a1)


def test_three_products_fail_the_gate(record_property):
    """Discrimination: at (127, 128, 768) a CPU model that keeps only a0 b0 + a0 b1 + a1 b0 (float64 accumulation, i.e.
    NO rounding error of its own) fails the statistical gate, and the model with all six products passes it: the gate
    sees a lost term of order 2^-16."""
    M, N, K = 127, 128, 768
    A, B = operands(M, N, K)
    want = torch.matmul(A.double(), B.double())
    pa, pb = [p.double() for p in _split3(A)], [p.double() for p in _split3(B)]

    def model(order):
        return sum(torch.matmul(pa[i], pb[j]) for i in range(3) for j in range(3) if i + j <= order)

    gate = 2 * U * math.sqrt(K + 1 + 2)
    three, six = rel_l2(model(1), want) / gate, rel_l2(model(2), want) / gate
    record_property("three_products_rel_ratio", "%.3g" % three)
    record_property("six_products_rel_ratio", "%.3g" % six)
    assert three > 1, three
    assert six < 0.05, six


# --------------------------------------------------------------------------- the pyramid forward
def _pyramid64(f1, f2, levels):
    """models/raft/corr.py:13-27 in float64: f1^T f2 / sqrt(D), then 2x2 average pooling per level (an empty level where
    the level below is a single row or column)."""
    B, D, H, W = f1.shape
    vol = torch.matmul(f1.reshape(B, D, H * W).transpose(1, 2), f2.reshape(B, D, H * W)) / math.sqrt(D)
    lvl = vol.reshape(B * H * W, 1, H, W)
    out = [lvl]
    for _ in range(levels - 1):
        h, w = lvl.shape[-2:]
        lvl = F.avg_pool2d(lvl, 2, stride=2) if h >= 2 and w >= 2 else lvl.new_zeros(lvl.shape[0], 1, h // 2, w // 2)
        out.append(lvl)
    return out


def _level_maps(H, W, L):
    """Per level (columns of the slab in row-major texel order, h, w), from pcfa_corr_level_offset's extents and
    pcfa_corr_tiled_index."""
    lib = _hip.load()
    maps = []
    for l in range(L):
        h, w = ctypes.c_int(), ctypes.c_int()
        off = lib.pcfa_corr_level_offset(H, W, L, l, ctypes.byref(h), ctypes.byref(w))
        assert off >= 0
        idx = torch.tensor([lib.pcfa_corr_tiled_index(H, W, L, l, y, x) for y in range(h.value) for x in range(w.value)],
                           dtype=torch.long)
        assert idx.numel() == 0 or int(idx.min()) >= off
        maps.append((idx, h.value, w.value))
    return maps


def _f2ext_host(f2, maps, slab):
    """fmap2 and its successively pooled copies in the slab's column order, pad columns 0 (what pcfa_corr_f2ext_fwd
    writes; built here for layouts with an empty last level, which that entry point refuses)."""
    B, D = f2.shape[:2]
    out = torch.zeros(B, D, slab)
    lvl = f2
    for l, (idx, h, w) in enumerate(maps):
        if l > 0:
            lvl = F.avg_pool2d(lvl, 2, stride=2) if h >= 1 and w >= 1 else lvl.new_zeros(B, D, h, w)
        out[:, :, idx] = lvl.reshape(B, D, h * w)
    return out


PYRAMID = [(1, 5, 7), (2, 5, 7), (1, 17, 21), (2, 17, 21),       # Q % 4 != 0: masked loader, product against the pooled f2ext
           (1, 8, 20),                                           # the same product on the FAST loader
           (1, 16, 16), (1, 12, 32), (2, 16, 32)]                # W % 16 == 0: levels 1-2 pooled in the epilogue


@pytest.mark.parametrize("shape", PYRAMID, ids=lambda s: "B%d-%dx%d" % s)
def test_pyramid_forward_vs_float64(record_property, shape):
    """pcfa_corr_pyramid_fwd_bf16x3 (D = 256, 4 levels) into a fenced pyr against the float64 pyramid: 5x7 (Q % 4 != 0:
    masked loader; its fourth level is empty), 17x21 (odd level sizes), 8x20 (FAST loader) and three W % 16 == 0 shapes
    on the pooled epilogue (one query block; H % 16 != 0; two batch items of four query blocks).  Level l is within the
    element bound with n6 + 3 l and the statistical gate with the fp32 pyramid test's n = D + 3 l + 2: three additions
    per 2x2 average, of the accumulators in the epilogue or of fmap2 in f2ext; the scale 1/16 is exact.  Every texel of
    every level is written.  Tile-padding columns and the closing zero tile are exactly 0 -- except, on the pooled
    epilogue, the pad texels of levels 1 and 2, which this test leaves unexamined when H % 16 != 0 (the shared
    epilogue, gemm_tile.hpp, once left some of those pad rows unwritten; it zeroes them now, and
    tests/test_pyramid_f64_gpu.py asserts +0 in every float outside the level texels).  Two calls give equal bits."""
    B, H, W = shape
    D, L = 256, 4
    lib = _hip.load()
    gen = torch.Generator().manual_seed(B * 1000 + H * W)
    f1 = torch.randn(B, D, H, W, generator=gen)
    f2 = torch.randn(B, D, H, W, generator=gen)
    slab = int(lib.pcfa_corr_slab_floats(H, W, L))
    maps = _level_maps(H, W, L)
    Q = H * W
    a = Fenced((B, D, Q), (D * Q, Q, 1), NAN_BITS).write(f1.reshape(B, D, Q))
    ext = Fenced((B, D, slab), (D * slab, slab, 1), NAN_BITS)
    if all(h >= 1 and w >= 1 for _, h, w in maps):
        b = torch.empty_like(f2, device=DEV).copy_(f2)
        assert lib.pcfa_corr_f2ext_fwd(ctypes.c_void_p(b.data_ptr()), ext.ptr(), B, D, H, W, L, _stream()) == 0
        torch.cuda.synchronize()
        ext.bits0 = ext.buf.view(torch.int32).clone()
    else:
        ext.write(_f2ext_host(f2, maps, slab))
    pyr = Fenced((B * Q, slab), (slab, 1), SENTINEL)

    def call():
        return lib.pcfa_corr_pyramid_fwd_bf16x3(a.ptr(), ext.ptr(), pyr.ptr(), B, D, H, W, L, _stream())

    assert call() == 0
    torch.cuda.synchronize()
    got = pyr.view().clone()
    assert a.fence_intact() and ext.fence_intact() and pyr.fence_intact()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(pyr.view().view(torch.int32), got.view(torch.int32)), "not repeatable bit for bit"
    got = got.cpu()
    pooled = W % 16 == 0 and Q % 4 == 0        # the host rule of the pooled epilogue (D % 4 == 0, L >= 3 hold here)

    want = _pyramid64(f1.double(), f2.double(), L)
    wabs = _pyramid64(f1.double().abs(), f2.double().abs(), L)
    used = torch.zeros(slab, dtype=torch.bool)
    worst_e = worst_r = 0.
    for l, (idx, h, w) in enumerate(maps):
        assert tuple(want[l].shape[-2:]) == (h, w)
        if h * w == 0:
            continue
        used[idx] = True
        assert bool(torch.isfinite(got[:, idx]).all()), "a texel of level %d was never written" % l
        e, r = gates(got[:, idx], want[l].reshape(B * Q, h * w), wabs[l].reshape(B * Q, h * w), D, 0, extra=3 * l)
        worst_e, worst_r = max(worst_e, e), max(worst_r, r)
    if pooled and H % 16 != 0:
        off1, off3 = (int(lib.pcfa_corr_level_offset(H, W, L, l, None, None)) for l in (1, 3))
        used[off1:off3] = True
    assert bool((got[:, ~used] == 0).all()), "a tile-padding column is not exactly 0"
    record_property("elem_ratio", "%.3g" % worst_e)
    record_property("rel_ratio", "%.3g" % worst_r)
    print("pyramid bf16x3 elem %.3g rel %.3g" % (worst_e, worst_r))
    assert worst_e <= 1 and worst_r <= 1, (worst_e, worst_r)


def test_corr_block_takes_the_switch():
    """ops.corr.CorrBlock(..., mfma="bf16x3") builds the same pyramid as mfma="f32" to fp32 accuracy (not bit for bit) and
    refuses an unknown arithmetic."""
    gen = torch.Generator().manual_seed(11)
    f1, f2 = torch.randn(1, 256, 8, 16, generator=gen).to(DEV), torch.randn(1, 256, 8, 16, generator=gen).to(DEV)
    p32 = hip_ops.CorrBlock(f1, f2, num_levels=4, radius=4).corr_pyramid
    px3 = hip_ops.CorrBlock(f1, f2, num_levels=4, radius=4, mfma="bf16x3").corr_pyramid
    for x, y in zip(p32, px3):
        assert rel_l2(y.double().cpu(), x.double().cpu()) <= 4 * U * math.sqrt(256 + 3)
    with pytest.raises(ValueError):
        hip_ops.CorrBlock(f1, f2, num_levels=4, radius=4, mfma="tf32")
