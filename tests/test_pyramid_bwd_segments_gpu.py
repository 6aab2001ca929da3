"""The K-segment tables of the correlation pyramid's windowed backward (csrc/corr_pyramid.hip: corr_window_runs_kernel,
corr_window_run_segments_kernel, and the rows tables they fall back to) and the two products that walk them.

Cover property: the tables are read back from the workspace (ops.corr.window_segment_tables, as the work recorder reads
them) and checked against a numpy brute force over the same coordinates (tools/pyramid_bwd_segments.py: touched()):
every (query, slab column) some lookup's (2r+2)^2 window can touch lies inside a segment of that query's block (table A)
and of that column's block (table B); every list is ascending, non-overlapping, in multiples of 16, inside the slab /
inside Q (table B: inside the record's hull), and no longer than its capacity.  The tables must also equal the numpy
restatement the counting tool uses, segment for segment: table A is the rows scheme (windows clipped in y only) at every
shape, table B the runs scheme (clipped in x as well) inside the rows scheme's hull -- for W % 16 != 0 the rows scheme,
which must be produced unchanged.

Shapes: 9x32 (one run column pair, H % 8 != 0), 13x64 (odd pooled sizes), 24x48, 24x40 (W % 16 != 0: the rows tables),
55x128 with B = 2 (the workload's feature map, once: item 0 drifts, item 1 is the spread that overflows table B).

Products: at D = 64 the gradients of the windowed path against the dense path of the same build, the bound of
test_pyramid_backward_windows_matches_dense (2e-6 relative L2: the skipped terms are exact zeros, only the order of the
split-K partial sums differs); two windowed runs must be bit-identical."""
import ctypes

import numpy as np
import pytest
import torch

from pcfa_amd import _hip, hip_ops
from pcfa_amd.ops import corr as corr_ops
from pcfa_amd.ops.core import _call, _ptr
from tests.util import rel_l2
from tools import pyramid_bwd_segments as seg

pytestmark = pytest.mark.gpu
DEV = "cuda"
L, R = 4, 4
SETS = ["drift", "outside", "nan", "spread", "nograd"]


def _grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([xs, ys], 0).float()[None].repeat(B, 1, 1, 1)


def make_coords(kind, B, H, W, seed=5):
    """-> (list of [B, 2, H, W] coordinate tensors, index of the lookup whose output gets no gradient or None)."""
    gen = torch.Generator().manual_seed(seed)
    base = _grid(B, H, W)
    drift = lambda n: [base + 0.7 * i * torch.randn(B, 2, 1, 1, generator=gen) +   # noqa: E731
                       (0.3 + 0.2 * i) * torch.randn(B, 2, H, W, generator=gen) for i in range(n)]
    if kind == "drift":          # identity plus a slow drift over 12 lookups
        return drift(12), None
    if kind == "outside":        # everything far outside the map: empty ranges
        return [base + 1000.0 + i for i in range(3)], None
    if kind == "nan":            # one NaN in one query: its run reaches everything, its neighbours do not
        cs = drift(3)
        cs[1][0, 1, H // 2, W // 2 + 1] = float("nan")
        if W % 16 == 0:          # (and one in cx: the rows tables look at cy only, the runs table at both)
            cs[2][0, 0, H // 2, 1] = float("nan")
        return cs, None
    if kind == "spread":         # every query row reaches every texel row, narrow in x: the longest lists there can be
        cs = []
        for _ in range(3):
            c = base + 0.5 * torch.randn(B, 2, H, W, generator=gen)
            c[:, 1] = torch.rand(B, H, W, generator=gen) * H
            cs.append(c)
        return cs, None
    if kind == "nograd":         # a lookup whose output receives no gradient
        return drift(5), 2
    raise ValueError(kind)


def read_tables(coords, B, H, W, D=4):
    """Run pcfa_corr_pyramid_bwd_windows on a zero gradient; -> (tables A, B as [b][block] -> [(begin, end)], the
    widening each record took, table B's hulls, pcfa_corr_pyramid_bwd_windows_tables's row)."""
    lib = _hip.load()
    slab = int(lib.pcfa_corr_slab_floats(H, W, L))
    Q = H * W
    cs = [c.to(DEV).contiguous() for c in coords]
    dpyr = torch.zeros(B * Q, slab, device=DEV)
    f1, f2e = torch.zeros(B, D, Q, device=DEV), torch.zeros(B, D, slab, device=DEV)
    df1, df2 = torch.empty_like(f1), torch.empty_like(f1)
    nbytes = lib.pcfa_corr_pyramid_bwd_windows_workspace_bytes(B, D, H, W, L)
    ws = torch.empty((nbytes + 3) // 4, device=DEV, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * len(cs))(*[c.data_ptr() for c in cs])
    _call("pcfa_corr_pyramid_bwd_windows", _ptr(dpyr), _ptr(f1), _ptr(f2e), _ptr(df1), _ptr(df2), _ptr(ws),
          ctypes.c_size_t(nbytes), ptrs, len(cs), R, B, D, H, W, L)
    torch.cuda.synchronize()
    rec, nbA, info = corr_ops.window_segment_tables(ws, B, D, H, W, L)
    nbB = info[2]
    rec = rec.numpy()
    lists = [[(int(r[4 + 2 * i]), int(r[5 + 2 * i])) for i in range(int(r[0]))] for r in rec]
    A = [lists[b * nbA:(b + 1) * nbA] for b in range(B)]
    Bt = [lists[B * nbA + b * nbB:B * nbA + (b + 1) * nbB] for b in range(B)]
    modes = {"A": [int(r[1]) for r in rec[:B * nbA]], "B": [int(r[1]) for r in rec[B * nbA:]]}
    hulls = [[(int(r[2]), int(r[3])) for r in rec[B * nbA + b * nbB:B * nbA + (b + 1) * nbB]] for b in range(B)]
    return A, Bt, modes, hulls, info


def check_cover(coords, B, H, W):
    c = np.stack([x.numpy() for x in coords]).astype(np.float32)      # [n, B, 2, H, W]
    P = seg.Layout(H, W, L)
    A, Bt, modes, hulls, info = read_tables(coords, B, H, W)
    rec_ints, nbA, nbB, run, cap = info[:5]
    assert run == (16 if W % 16 == 0 else 0) and rec_ints == 4 + 2 * cap
    Q = H * W
    T = seg.touched(c, R, P)
    for b in range(B):
        assert len(A[b]) == nbA and len(Bt[b]) == nbB
        for table, limit in ((A[b], P.slab), (Bt[b], Q)):
            for s in table:
                assert len(s) <= cap
                assert all(x % 16 == 0 and y % 16 == 0 and 0 <= x < y <= limit for x, y in s), s
                assert all(s[i][1] <= s[i + 1][0] for i in range(len(s) - 1)), s
        for s, h in zip(Bt[b], hulls[b]):
            assert all(h[0] <= x and y <= h[1] for x, y in s), (s, h)
        for j, s in enumerate(A[b]):
            qs = np.arange(j * 128, min(j * 128 + 128, Q))
            assert not (T[b][qs] & ~seg.seg_mask(s, P.slab)[None]).any(), ("table A", b, j)
        for j, s in enumerate(Bt[b]):
            cols = np.arange(j * 128, min(j * 128 + 128, P.slab))
            assert not (T[b][:, cols] & ~seg.seg_mask(s, Q)[:, None]).any(), ("table B", b, j)
    # the restatement of the counting tool, segment for segment
    rows = seg.rows_table(c, R, P)
    wantA, rowsB = seg.rows_segments(rows, H, W, P)
    want_hulls = [[s[0] if s else (0, 0) for s in t] for t in rowsB]
    if run:
        wantB, want_hulls, want_modes = seg.run_segments(rows, seg.runs_table(c, R, P), H, W, P, cap)
        assert modes["B"] == want_modes
    else:
        wantB = rowsB
    assert A == wantA and Bt == wantB and hulls == want_hulls
    return A, Bt, modes, P


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("shape", [(9, 32), (13, 64), (24, 48), (24, 40)], ids=lambda s: "%dx%d" % s)
def test_segment_tables_cover_every_window(shape, kind):
    H, W = shape
    coords, _ = make_coords(kind, 1, H, W)
    A, Bt, modes, P = check_cover(coords, 1, H, W)
    if kind == "outside":
        assert seg.steps([A[0]]) + seg.steps([Bt[0]]) == 0
    if kind == "nan":       # the NaN query's row reaches every column block (and so does its run)
        q = (H // 2) * W + W // 2 + 1
        assert all(seg.seg_mask(s, H * W)[q] for s in Bt[0][:P.zero // 128])


def test_segment_tables_workload_shape():
    """55x128, B = 2: item 0 drifts like a refinement, item 1 is the spread (55 reaching query rows per block of df2ext,
    more than the capacity: whole query rows, which merge)."""
    B, H, W = 2, 55, 128
    d, _ = make_coords("drift", 1, H, W)
    s, _ = make_coords("spread", 1, H, W)
    coords = [torch.cat([d[i], s[i % len(s)]]) for i in range(len(d))]
    A, Bt, modes, P = check_cover(coords, B, H, W)
    nbB = len(Bt[0])
    assert max(modes["B"][nbB:]) >= 1    # the spread does not fit the lists
    rows = seg.rows_segments(seg.rows_table(np.stack([x.numpy() for x in coords])[:, :1], R, P), H, W, P)
    assert seg.steps([Bt[0]]) < seg.steps([rows[1][0]]) / 1.5     # (the drift: 23384 -> 12845 steps)


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("shape", [(9, 32), (13, 64), (24, 48), (24, 40)], ids=lambda s: "%dx%d" % s)
def test_windowed_products_match_dense(shape, kind):
    H, W = shape
    B, D = 1, 64
    gen = torch.Generator().manual_seed(11)
    f1 = torch.randn(B, D, H, W, generator=gen).to(DEV)
    f2 = torch.randn(B, D, H, W, generator=gen).to(DEV)
    coords, skip = make_coords(kind, B, H, W)
    coords = [c.to(DEV) for c in coords]
    gos = [torch.randn(B, 324, H, W, generator=gen).to(DEV) for _ in coords]

    def run(windows):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        blk = hip_ops.CorrBlock(a, b, bwd_windows=windows)
        loss = 0.
        for i, (c, g) in enumerate(zip(coords, gos)):
            out = blk(c)
            if i != skip:
                loss = loss + (out * g).sum()
        loss.backward()
        return a.grad, b.grad

    (a1, b1), (a0, b0), (a2, b2) = run(True), run(False), run(True)
    for w, d in ((a1, a0), (b1, b0)):
        fin = torch.isfinite(d)                     # (a NaN coordinate may leave NaN gradients: in the same places)
        assert torch.equal(torch.isfinite(w), fin)
        if kind == "outside":
            assert float(d.abs().max()) == 0 and float(w.abs().max()) == 0
        else:
            assert float(d[fin].abs().max()) > 0
            assert rel_l2(w[fin], d[fin]) < 2e-6, rel_l2(w[fin], d[fin])
    # deterministic (NaN != NaN: compare the bits)
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and torch.equal(b1.view(torch.int32), b2.view(torch.int32))
