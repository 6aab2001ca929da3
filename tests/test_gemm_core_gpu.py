"""The fp32 MFMA GEMM core of csrc/corr_pyramid.hip (gemm_f32_mfma_body) and its callers, against float64 on the CPU.

One hand-written core carries the correlation pyramid's forward (pooled epilogue) and backward (sparse window, dense
and split-K products), conv1x1 and every GMA attention product through pcfa_gemm_f32.  Every reference here is
float64, computed from the same fp32 inputs the kernel saw.

Gates.  u = 2^-24.  For a product of K terms the classic bound |fl(sum) - sum| <= gamma_n * sum|a_k b_k| with
gamma_n = n u / (1 - n u) holds for ANY summation order, so it cannot flake on cancellation:

    |C - C64|_ij <= c * gamma_n * |alpha| * (|A| |B|)_ij + tiny,    n = K + splits + 2

n counts the roundings one output element sees: K fma steps, splits - 1 additions of the ordered split-K reduction,
and at most two for alpha (the kernel divides by fl(1/alpha): two roundings unless alpha is a power of two), + 1
spare.  c = 2 covers an MFMA that rounds the product and the addition separately (two roundings per term) rather
than fusing them.  tiny = K * 2^-126 covers flushed subnormal products.  Random data sits far inside this worst case,
so a second, statistical gate follows what the kernel actually achieves: rounding errors of a K-term sum walk
randomly, rel-L2 ~ u sqrt(K / 3) for zero-mean data, and

    rel_l2(C, C64) <= 2 * u * sqrt(n).

Dropping one 16-wide K tile, an empty split, a split in the reduction or applying alpha twice is orders of magnitude
outside both.  Each case also repeats its call and asserts identical bits.

Every test records its worst err / bound ratios as junit properties (``--junitxml=FILE -o junit_family=xunit1``) so
that the gates' headroom is visible.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from pcfa_amd import _hip, hip_ops
from tests.fenced import (DEV, FENCE, NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED,  # noqa: F401
                          PCFA_ERR_WORKSPACE, SENTINEL, TINY, U, Fenced, gamma)
from tests.fenced import stream as _stream
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))


def _gate(got, want64, absprod64, n, c=2.0, tiny=0.0):
    """(elementwise err / bound max, rel-L2 / bound); both must be <= 1."""
    got = got.detach().double().cpu()
    bound = c * gamma(n) * absprod64 + tiny
    elem = float(((got - want64).abs() / bound).max())
    rel = rel_l2(got, want64) / (2 * U * math.sqrt(n))
    return elem, rel


# --------------------------------------------------------------------------- 1. pcfa_gemm_f32 through the C-ABI
def _fast_rule(lay, M, N, K, lda, ldb, bsA, bsB, shift):
    """The host rule of pcfa_gemm_f32 that picks the branch-free FAST loader (corr_pyramid.hip, vecA / vecB / fast)."""
    ak, bk = lay
    vec_a = shift % 4 == 0 and lda % 4 == 0 and (M if ak else K) % 4 == 0 and bsA % 4 == 0
    vec_b = ldb % 4 == 0 and (N if bk else K) % 4 == 0 and bsB % 4 == 0
    return vec_a and vec_b and K % 4 == 0 and min(M, N, K) >= 4


def run_gemm(lay, M, N, K, batch=1, splits=1, alpha=1.0, lda_pad=0, ldb_pad=0, ldc_pad=0, bs_pad=0, bsA0=False,
             shift=0, seed=0, ws_short=0, check_fast=None):
    """One pcfa_gemm_f32 call on fenced operands; returns (C [batch, M, N] float32 CPU, want64, absprod64, status).
    Layout (a_kmajor, b_kmajor): A(m, k) at A[m lda + k] (0) or A[k lda + m] (1); B(k, n) at B[n ldb + k] (0) or
    B[k ldb + n] (1).  The pads widen the leading dimensions / batch strides past dense; shift moves A's base pointer
    off 16-B alignment."""
    ak, bk = lay
    gen = torch.Generator().manual_seed(seed * 7919 + M * 131 + N * 17 + K)
    A = torch.randn(1 if bsA0 else batch, M, K, generator=gen)
    B = torch.randn(batch, K, N, generator=gen)
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
    wbytes = int(lib.pcfa_gemm_f32_workspace_bytes(M, N, batch, splits))
    fw = Fenced((max(wbytes // 4, 1),), (1,), NAN_BITS) if splits > 1 else None

    def call():
        return lib.pcfa_gemm_f32(fa.ptr(), fb.ptr(), fc.ptr(), M, N, K, lda, ldb, ldc, ak, bk, batch, bsA, bsB, bsC,
                                 ctypes.c_float(alpha), splits, fw.ptr() if fw else None,
                                 ctypes.c_size_t(max(wbytes - ws_short, 0)), _stream())

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
    A64, B64 = A.double(), B.double()
    want = alpha * torch.matmul(A64, B64)
    absprod = abs(alpha) * torch.matmul(A64.abs(), B64.abs())
    return C.cpu(), want, absprod, st


def check_gemm(record_property, K, splits, *args, **kw):
    C, want, absprod, st = run_gemm(*args, K=K, splits=splits, **kw)
    assert st == 0, st
    assert bool(torch.isfinite(C).all()), "non-finite C: a NaN fence value or an unwritten element reached C"
    elem, rel = _gate(C, want, absprod, K + splits + 2, tiny=K * 2.0 ** -126)
    record_property("elem_ratio", "%.3g" % elem)
    record_property("rel_ratio", "%.3g" % rel)
    assert elem <= 1 and rel <= 1, (elem, rel)


# (layout, M, N, K): shapes where the FAST loader runs with dense aligned operands; each also runs on the masked loader
BOTH_LOADERS = [((0, 1), 4, 4, 4), ((0, 1), 128, 128, 16), ((0, 1), 127, 128, 768), ((0, 0), 129, 257, 16),
                ((0, 0), 257, 127, 768), ((1, 1), 128, 4, 768), ((1, 1), 4, 128, 16), ((1, 1), 128, 128, 1028)]


@pytest.mark.parametrize("loader", ["fast", "masked"])
@pytest.mark.parametrize("case", BOTH_LOADERS, ids=lambda c: "%d%d-%dx%dx%d" % (c[0] + c[1:]))
def test_gemm_both_loaders(record_property, case, loader):
    """Both loaders at one shape: FAST (dense, aligned, K % 4 == 0) and the masked loader, reached by moving A's base
    pointer one float off 16-B alignment.  Each must pass the gates (module docstring, c = 2); they need not agree
    bit for bit."""
    lay, M, N, K = case
    check_gemm(record_property, K, 1, lay, M, N, alpha=0.5 if K == 768 else 1.0,
               shift=0 if loader == "fast" else 1, check_fast=loader == "fast")


MASKED_SHAPES = [((0, 1), 1, 1, 1), ((0, 0), 3, 129, 3), ((1, 1), 129, 3, 17), ((0, 1), 257, 127, 33),
                 ((0, 0), 127, 1, 15), ((1, 1), 1, 257, 1027), ((0, 1), 129, 129, 1027), ((1, 1), 3, 4, 4)]


@pytest.mark.parametrize("case", MASKED_SHAPES, ids=lambda c: "%d%d-%dx%dx%d" % (c[0] + c[1:]))
def test_gemm_masked_edges(record_property, case):
    """Tile-edge and degenerate shapes on the masked loader (M, N or K off the multiples of 4 / 128 / 16): the edge
    loads are zero-filled, never read from the NaN fence."""
    lay, M, N, K = case
    check_gemm(record_property, K, 1, lay, M, N, alpha=-3.0 if K > 16 else 1.0, check_fast=False)


STRIDES = [  # (id, layout, M, N, K, batch, splits, alpha, kwargs, fast)
    ("ld+4", (0, 1), 128, 128, 768, 1, 1, 1.0, dict(lda_pad=4, ldb_pad=4), True),
    ("ld+3", (0, 1), 128, 128, 768, 1, 1, 1.0, dict(lda_pad=3, ldb_pad=3), False),
    ("ld+4-00", (0, 0), 129, 127, 33, 1, 1, 0.5, dict(lda_pad=4, ldb_pad=4), False),
    ("ld+4-11", (1, 1), 128, 256, 64, 1, 1, 1.0, dict(lda_pad=4, ldb_pad=8), True),
    ("ld+3-11", (1, 1), 128, 256, 64, 1, 1, 1.0, dict(lda_pad=3, ldb_pad=5), False),
    ("ldc", (0, 1), 129, 127, 33, 1, 1, 1.0, dict(ldc_pad=5), False),
    ("ldc-fast", (1, 1), 128, 128, 16, 1, 1, -3.0, dict(ldc_pad=4), True),
    ("batch3-bs", (0, 0), 127, 129, 768, 3, 1, 1.0, dict(bs_pad=8, lda_pad=4), True),
    ("batch3-bs-odd", (1, 1), 128, 128, 64, 3, 1, 0.5, dict(bs_pad=7), False),
    ("bsA0", (0, 1), 127, 256, 768, 2, 1, 1.0, dict(bsA0=True), True),
    ("bsA0-split3", (0, 1), 127, 256, 768, 3, 3, 0.5, dict(bsA0=True), True),
    ("bsA0-split3-masked", (0, 1), 129, 257, 33, 2, 3, -3.0, dict(bsA0=True), False),
]


@pytest.mark.parametrize("case", STRIDES, ids=[c[0] for c in STRIDES])
def test_gemm_strides(record_property, case):
    """Leading dimensions past the row length (% 4 == 0 keeps FAST, odd forces the masked loader), ldc > N, batch 3
    with non-dense batch strides, and bsA = 0 (one A for every batch, as conv1x1 calls it) with and without split-K.
    The padding between rows is NaN: any read of it poisons C."""
    _, lay, M, N, K, batch, splits, alpha, kw, fast = case
    check_gemm(record_property, K, splits, lay, M, N, batch=batch, alpha=alpha, check_fast=fast, **kw)


SPLITS = [  # (layout, M, N, K, batch, splits, alpha)
    ((0, 0), 128, 128, 20, 2, 8, -3.0),      # kchunk 16: splits 2..7 start past K (nk <= 0 from split 4 on)
    ((0, 1), 129, 127, 17, 3, 8, 0.5),       # masked loader, six empty splits
    ((0, 0), 4, 4, 33, 2, 8, 1.0),           # kchunk 16: splits 3..7 empty
    ((0, 1), 128, 128, 4, 2, 3, 1.0),        # K < BK: one live split
    ((1, 1), 128, 128, 1027, 2, 3, 1.0),     # ragged K tail in the last split
    ((1, 1), 128, 128, 1028, 2, 3, -3.0),    # kchunk 352: the tail past 3 * 336 lives in the last split
    ((0, 1), 257, 129, 768, 2, 2, 0.5),
    ((0, 0), 127, 257, 768, 3, 8, 1.0),
]


@pytest.mark.parametrize("case", SPLITS, ids=lambda c: "%d%d-%dx%dx%d-b%d-s%d" % (c[0] + c[1:6]))
def test_gemm_split_k(record_property, case):
    """Split-K into the workspace + the ordered reduction, batch > 1, alpha in {1, 0.5, -3}, including splits that
    start past K (their partials must be exact zeros).  n = K + splits + 2 (module docstring)."""
    lay, M, N, K, batch, splits, alpha = case
    check_gemm(record_property, K, splits, lay, M, N, batch=batch, alpha=alpha)


def test_gemm_refusals():
    """Refused calls return their status and leave C (sentinel NaN bits) untouched: alpha = 0, a short or missing
    workspace, split-K with ldc != N or a non-dense batch stride of C, and the (1, 0) layout."""
    lib = _hip.load()
    M, N, K = 64, 64, 32
    a = Fenced((M, K), (K, 1), NAN_BITS).write(torch.randn(M, K))
    b = Fenced((K, N), (N, 1), NAN_BITS).write(torch.randn(K, N))

    def status(lay=(0, 1), alpha=1.0, splits=1, ldc=N, batch=1, bsC=M * N, ws=True, short=0):
        c = Fenced((batch, M, N), (bsC, ldc, 1), SENTINEL)
        nbytes = int(lib.pcfa_gemm_f32_workspace_bytes(M, N, batch, splits))
        w = torch.empty(max(nbytes // 4, 1), device=DEV)
        st = lib.pcfa_gemm_f32(a.ptr(), b.ptr(), c.ptr(), M, N, K, K if lay[0] == 0 else M, N, ldc, lay[0], lay[1],
                               batch, 0, 0, bsC, ctypes.c_float(alpha), splits,
                               ctypes.c_void_p(w.data_ptr()) if ws else None, ctypes.c_size_t(max(nbytes - short, 0)),
                               _stream())
        torch.cuda.synchronize()
        assert torch.equal(c.buf.view(torch.int32), c.bits0), "a refused call touched C"
        return st

    assert status(alpha=0.0) == PCFA_ERR_INVALID_ARG
    assert status(splits=3, short=4) == PCFA_ERR_WORKSPACE
    assert status(splits=3, ws=False) == PCFA_ERR_WORKSPACE
    assert status(splits=3, ldc=N + 4) == PCFA_ERR_UNSUPPORTED
    assert status(splits=2, batch=2, bsC=M * N + 4) == PCFA_ERR_UNSUPPORTED
    assert status(lay=(1, 0)) == PCFA_ERR_UNSUPPORTED


# --------------------------------------------------------------------------- 2. correlation pyramid at real shapes
def _grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([xs, ys], 0).float()[None].repeat(B, 1, 1, 1)


def pyramid64(f1, f2, levels):
    """models/raft/corr.py:13-27 restated in float64: f1^T f2 / sqrt(D), then 2x2 average pooling per level."""
    B, D, H, W = f1.shape
    vol = torch.matmul(f1.reshape(B, D, H * W).transpose(1, 2), f2.reshape(B, D, H * W)) / math.sqrt(D)
    lvl = vol.reshape(B * H * W, 1, H, W)
    out = [lvl]
    for _ in range(levels - 1):
        lvl = F.avg_pool2d(lvl, 2, stride=2)
        out.append(lvl)
    return out


def lookup_loss64(pyr, coords, gos, r=4):
    """sum_i <lookup(pyr, coords_i), g_i> in float64 (models/raft/corr.py:29-50, bilinear_sampler through grid_sample):
    channel l (2r+1)^2 + a (2r+1) + b samples level l at (cx / 2^l + a - r, cy / 2^l + b - r).  All lookups of a level
    go through ONE grid_sample (their windows stacked along the grid's rows): the same sum, one pass over the level."""
    n1 = 2 * r + 1
    offs = torch.arange(-r, r + 1, dtype=torch.float64)
    wx, wy = offs.view(n1, 1).expand(n1, n1), offs.view(1, n1).expand(n1, n1)
    loss = 0.
    for lv, vol in enumerate(pyr):
        h, w = vol.shape[-2:]
        grids, gs = [], []
        for c, g in zip(coords, gos):
            cx = c[:, 0].reshape(-1, 1, 1).double() / 2 ** lv
            cy = c[:, 1].reshape(-1, 1, 1).double() / 2 ** lv
            grids.append(torch.stack([2 * (cx + wx) / (w - 1) - 1, 2 * (cy + wy) / (h - 1) - 1], -1))
            gs.append(g[:, lv * n1 * n1:(lv + 1) * n1 * n1].permute(0, 2, 3, 1).reshape(-1, 1, n1, n1))
        taps = F.grid_sample(vol, torch.cat(grids, 1), align_corners=True)
        loss = loss + (taps * torch.cat(gs, 2).double()).sum()
    return loss


PYRAMID = [(1, 55, 128), (2, 55, 128), (1, 47, 156), (2, 47, 156), (2, 45, 67)]


@pytest.mark.parametrize("shape", PYRAMID, ids=lambda s: "B%d-%dx%d" % s)
def test_corr_pyramid_vs_float64(record_property, shape):
    """CorrBlock (D = 256, 4 levels, radius 4) at Sintel's 55x128 features (pooled-epilogue forward, W % 16 == 0), at
    KITTI's 47x156 (375x1242 padded to 376x1248: W % 16 != 0, the plain forward product against the pooled f2ext) and
    at 45x67 (odd level sizes 22x33 / 11x16 / 5x8, Q % 4 != 0: masked loaders, dense backward).

    Forward: every level against the float64 pyramid with the elementwise gate of the module docstring, |A||B| the
    same pyramid of |f1|, |f2|, n = D + 3 l + 2 at level l: D fma steps, three additions per 2x2 average (of the
    level-0 accumulators in the epilogue, or of fmap2 in f2ext -- both before any product is rounded further), the
    scale 1/16 is exact, + 2 spare.  c = 2 as in the module docstring.

    Backward: f1.grad, f2.grad through 12 RAFT-like lookups against float64 autograd of the pyramid + grid_sample
    restatement, on the sparse window products (default) and the dense ones (bwd_windows=False).  Gate: rel-L2 <=
    2 u sqrt(n), the random-walk form of the module docstring, where n counts the non-zero terms of one sum: a dpyr row
    holds at most 12 lookups x L levels x (2r + 2)^2 bilinear taps (the rest are exact zeros, and adding them is
    exact in either product), + 8 splits + 48 accumulations into one dpyr element (12 lookups x 4 corners) + 3 L for
    the pooling adjoint.  The kernel's fp32 sample position (cx / 2^l + a - r) moves a weight by <= u |x|, with random
    sign: well inside the same budget."""
    B, H, W = shape
    D, L = 256, 4
    gen = torch.Generator().manual_seed(B * 1000 + H * W)
    f1 = torch.randn(B, D, H, W, generator=gen)
    f2 = torch.randn(B, D, H, W, generator=gen)
    base = _grid(B, H, W)
    coords = [base + 0.7 * i * torch.randn(B, 2, 1, 1, generator=gen)
              + (0.3 + 0.2 * i) * torch.randn(B, 2, H, W, generator=gen) for i in range(12)]
    gos = [torch.randn(B, L * 81, H, W, generator=gen) for _ in range(12)]

    def run(windows, want_levels=False):
        a, b = f1.to(DEV).requires_grad_(True), f2.to(DEV).requires_grad_(True)
        blk = hip_ops.CorrBlock(a, b, num_levels=L, radius=4, bwd_windows=windows)
        levels = [p.detach().cpu() for p in blk.corr_pyramid] if want_levels else None
        loss = sum((blk(c.to(DEV)) * g.to(DEV)).sum() for c, g in zip(coords, gos))
        loss.backward()
        return levels, a.grad.cpu(), b.grad.cpu()

    levels, ga, gb = run(True, want_levels=True)
    _, ga2, gb2 = run(True)
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2), "sparse backward not repeatable bit for bit"
    _, da, db = run(False)

    f1d, f2d = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    pyr = pyramid64(f1d, f2d, L)
    with torch.no_grad():
        pabs = pyramid64(f1.double().abs(), f2.double().abs(), L)
    worst_e = worst_r = 0.
    for lv in range(L):
        got, want = levels[lv], pyr[lv].detach()
        assert got.shape == want.shape and bool(torch.isfinite(got).all())
        e, r = _gate(got, want, pabs[lv], D + 3 * lv + 2, tiny=D * 2.0 ** -126)
        worst_e, worst_r = max(worst_e, e), max(worst_r, r)
    del pabs
    record_property("fwd_elem_ratio", "%.3g" % worst_e)
    record_property("fwd_rel_ratio", "%.3g" % worst_r)
    assert worst_e <= 1 and worst_r <= 1, (worst_e, worst_r)

    lookup_loss64(pyr, coords, gos).backward()
    del pyr
    bound = 2 * U * math.sqrt(12 * L * (2 * 4 + 2) ** 2 + 8 + 48 + 3 * L)
    ratios = {name: rel_l2(g, ref.grad) / bound
              for name, g, ref in (("sparse_df1", ga, f1d), ("sparse_df2", gb, f2d), ("dense_df1", da, f1d),
                                   ("dense_df2", db, f2d))}
    for name, v in ratios.items():
        record_property(name + "_ratio", "%.3g" % v)
    assert max(ratios.values()) <= 1, ratios


# --------------------------------------------------------------------------- 3. GMA on gemm="hip" at GMA's size
def test_gma_attention_at_gma_size_vs_float64(record_property):
    """GMA's attention (models/gma/gma.py:34-77,79-115) with every product on pcfa_gemm_f32 (Config.gma_gemm = "hip")
    at its real size: N = 55 x 128 = 7040, one head, d = 128; attention_softmax, 3 x attn_times_value, backward (the
    split-K = 8 products), against float64 torch.

    attn, elementwise: the similarity s = scale q k^T carries E = 2 gamma_{d+2} scale (|q||k|^T) (module docstring);
    the row softmax turns that into attn64 (E_ij + max_j E_ij) (the shared max cancels), the rounding of s - m into
    u |s - m| on each exponent and u max_j |s - m| on their sum, and the sum and normalisation into <= 64 u (32-term
    per-thread chains, 10 tree additions, 2 ulp of expf, reciprocal and product, with spare).
    Outputs and gradients, rel-L2: 2 u sqrt(n) as in the module docstring with n = N + 8 + 2 for the products over N,
    plus the attention's own relative error (its rel-L2 against float64, measured here) which every product carries."""
    h, n, d = 1, 55 * 128, 128
    gen = torch.Generator().manual_seed(7040)
    q, k = torch.randn(1, h, n, d, generator=gen), torch.randn(1, h, n, d, generator=gen)
    vs = [torch.randn(1, h, n, d, generator=gen) for _ in range(3)]
    gos = [torch.randn(1, h, n, d, generator=gen) for _ in range(3)]
    scale = d ** -0.5

    def run():
        qg, kg = q.to(DEV).requires_grad_(True), k.to(DEV).requires_grad_(True)
        vg = [v.to(DEV).requires_grad_(True) for v in vs]
        attn = hip_ops.attention_softmax(qg, kg, scale, gemm="hip")
        share = hip_ops.AttnGradShare("hip")
        outs = [hip_ops.attn_times_value(attn, v, share) for v in vg]
        sum((o * g.to(DEV)).sum() for o, g in zip(outs, gos)).backward()
        return [attn.detach().cpu()] + [o.detach().cpu() for o in outs] + [qg.grad.cpu(), kg.grad.cpu()] + \
            [v.grad.cpu() for v in vg]

    got = run()
    again = run()
    assert all(torch.equal(x, y) for x, y in zip(got, again)), "not repeatable bit for bit"
    del again
    attn = got[0]

    qd, kd = q.double().requires_grad_(True), k.double().requires_grad_(True)
    vd = [v.double().requires_grad_(True) for v in vs]
    s = scale * qd @ kd.transpose(-1, -2)
    attn_d = torch.softmax(s, dim=-1)
    outs_d = [attn_d @ v for v in vd]
    sum((o * g.double()).sum() for o, g in zip(outs_d, gos)).backward()
    with torch.no_grad():
        E = 2 * gamma(d + 2) * scale * (q.double().abs() @ k.double().abs().transpose(-1, -2))
        sm = s - s.max(-1, keepdim=True).values
        bound = attn_d * (E + E.max(-1, keepdim=True).values + U * (sm.abs() + sm.abs().max(-1, keepdim=True).values)
                          + 64 * U) + TINY
        del E, sm
        elem = float(((attn.double() - attn_d).abs() / bound).max())
        del bound
        attn_rel = rel_l2(attn, attn_d)
    record_property("attn_elem_ratio", "%.3g" % elem)
    prod = 2 * U * math.sqrt(n + 8 + 2) + attn_rel
    ratios = {"out%d" % i: rel_l2(got[1 + i], outs_d[i]) / prod for i in range(3)}
    ratios.update({"dv%d" % i: rel_l2(got[6 + i], vd[i].grad) / prod for i in range(3)})
    ratios["dq"] = rel_l2(got[4], qd.grad) / prod
    ratios["dk"] = rel_l2(got[5], kd.grad) / prod
    for name, v in ratios.items():
        record_property(name + "_ratio", "%.3g" % v)
    assert elem <= 1, elem
    assert max(ratios.values()) <= 1, ratios


SOFTMAX = [  # (cols, base pointer shift in floats, spread): register path up to 8192 columns, generic loop past it,
    (8192, 0, 10.0),   # for cols % 4 != 0 and for a misaligned row
    (8196, 0, 10.0),
    (7041, 0, 10.0),
    (7040, 1, 10.0),
    (8192, 0, 80.0),
    (7041, 0, 80.0),
    (7040, 1, 80.0),
]


@pytest.mark.parametrize("case", SOFTMAX, ids=lambda c: "%d-shift%d-spread%d" % c)
def test_softmax_rows_vs_float64(record_property, case):
    """pcfa_softmax_rows_fwd / _bwd (gma_ops.hip) at and around the register-path limit (NT * NV * 4 = 8192
    columns), on a misaligned view, and on rows spread over +-spread (odd rows shifted by +spread / 2 more, so that
    exp overflows in fp32 unless the row maximum is subtracted first).
    Forward, elementwise: y64 u (|x - m| + max_j |x - m| + 64) (the rounding of x - m on each exponent and on the sum;
    per-thread chains <= 33 terms, 10 tree additions, 2 ulp of expf, reciprocal and product, with spare).
    Backward gx = y (gy - sum_j gy_j y_j) on the same fp32 y, gy: |y| (gamma_64 sum_j |gy_j y_j| + 2 u |gy - dot|)."""
    cols, shift, spread = case
    rows = 24
    gen = torch.Generator().manual_seed(cols + shift)
    x = spread * (2 * torch.rand(rows, cols, generator=gen) - 1)
    x[1::2] += spread / 2
    gy = torch.randn(rows, cols, generator=gen)

    def place(t):
        buf = torch.full((t.numel() + shift,), float("nan"), device=DEV)
        buf[shift:].copy_(t.flatten())
        return buf

    lib = _hip.load()
    xb, yb, gb, ob = place(x), place(torch.zeros(rows, cols)), place(gy), place(torch.zeros(rows, cols))

    def p(b):
        return ctypes.c_void_p(b.data_ptr() + 4 * shift)

    assert lib.pcfa_softmax_rows_fwd(p(xb), p(yb), rows, cols, _stream()) == 0
    y = yb[shift:].clone()
    assert lib.pcfa_softmax_rows_fwd(p(xb), p(yb), rows, cols, _stream()) == 0
    assert torch.equal(yb[shift:], y)
    y = y.view(rows, cols).cpu()
    x64 = x.double()
    y64 = torch.softmax(x64, -1)
    xm = (x64 - x64.max(-1, keepdim=True).values).abs()
    e_fwd = float(((y.double() - y64).abs() / (y64 * U * (xm + xm.max(-1, keepdim=True).values + 64) + TINY)).max())
    assert bool(torch.isfinite(y).all()) and float((y.double().sum(-1) - 1).abs().max()) < 1e-5

    # backward on the kernel's own fp32 y
    assert lib.pcfa_softmax_rows_bwd(p(yb), p(gb), p(ob), rows, cols, _stream()) == 0
    gx = ob[shift:].clone()
    assert lib.pcfa_softmax_rows_bwd(p(yb), p(gb), p(ob), rows, cols, _stream()) == 0
    assert torch.equal(ob[shift:], gx)
    gx = gx.view(rows, cols).cpu().double()
    yd, gyd = y.double(), gy.double()
    dot = (gyd * yd).sum(-1, keepdim=True)
    want = yd * (gyd - dot)
    bnd = yd.abs() * (gamma(64) * (gyd * yd).abs().sum(-1, keepdim=True) + 2 * U * (gyd - dot).abs()) + TINY
    e_bwd = float(((gx - want).abs() / bnd).max())
    record_property("fwd_elem_ratio", "%.3g" % e_fwd)
    record_property("bwd_elem_ratio", "%.3g" % e_bwd)
    assert e_fwd <= 1 and e_bwd <= 1, (e_fwd, e_bwd)
