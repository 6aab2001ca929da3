"""The numpy restatement of the pyramid backward's K-segment tables (tools/pyramid_bwd_segments.py), without a GPU: on
random small cases its segment sets are supersets of the brute-force touched sets, for the rows scheme, the runs scheme
(the library's) and the patch scheme (counted only) at every widening, and the rows scheme's step counts follow the
kernel's formula (tile rows (ylo >> 2) .. (yhi >> 2) of tw * 16 columns each)."""
import numpy as np
import pytest

from tools import pyramid_bwd_segments as seg

R = 4


def _coords(kind, rng, n, B, H, W):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    base = np.stack([xx, yy])[None, None].repeat(n, 0).repeat(B, 1)
    if kind == "drift":
        c = base + rng.normal(0, 1.5, base.shape)
    elif kind == "outside":
        c = base + 1000
    elif kind == "nan_y":
        c = base.copy()
        c[1, 0, 1, rng.integers(H), rng.integers(W)] = np.nan
    elif kind == "nan_x":
        c = base.copy()
        c[1, 0, 0, rng.integers(H), rng.integers(W)] = np.nan
    elif kind == "random":
        c = rng.random(base.shape) * np.array([W, H], np.float32)[None, None, :, None, None]
    else:
        c = base + rng.normal(0, 6, base.shape)
    return c.astype(np.float32)


@pytest.mark.parametrize("kind", ["drift", "outside", "nan_y", "nan_x", "random", "jumpy"])
@pytest.mark.parametrize("shape", [(9, 32), (13, 64), (17, 96)], ids=lambda s: "%dx%d" % s)
def test_restatement_covers_brute_force(shape, kind):
    H, W = shape
    n, B = 3, 2
    c = _coords(kind, np.random.default_rng(H * 131 + len(kind)), n, B, H, W)
    P = seg.Layout(H, W, 4)
    T = seg.touched(c, R, P)
    Q = H * W
    if kind != "nan_x":   # (the rows scheme looks at cy only: the lookup's texel ROWS do not depend on cx)
        rows = seg.rows_table(c, R, P)
        A0, B0 = seg.rows_segments(rows, H, W, P)
        for b in range(B):
            for j, s in enumerate(A0[b]):
                qs = np.arange(j * 128, min(j * 128 + 128, Q))
                assert not (T[b][qs] & ~seg.seg_mask(s, P.slab)[None]).any()
                # the kernel's formula: whole tile rows of the hull of the block's query rows, per level
                want = 0
                for l in range(4):
                    rr = rows[b, l, (j * 128) // W:min((j * 128 + 127) // W, H - 1) + 1]
                    rr = rr[rr[:, 0] <= rr[:, 1]]
                    if len(rr):
                        want += ((int(rr[:, 1].max()) >> 2) + 1 - (int(rr[:, 0].min()) >> 2)) * P.tw[l]
                assert seg.steps([[s]]) == want
            for j, s in enumerate(B0[b]):
                cols = np.arange(j * 128, min(j * 128 + 128, P.slab))
                assert not (T[b][:, cols] & ~seg.seg_mask(s, Q)[:, None]).any()
    runs = seg.runs_table(c, R, P)
    # the runs scheme (the library's table B): inside the rows scheme's hull, still a cover, at every widening
    rows = seg.rows_table(c, R, P)
    for cap in (seg.CAP, 2, 4):
        B2, hulls, modes = seg.run_segments(rows, runs, H, W, P, cap)
        for b in range(B):
            for j, (s, h) in enumerate(zip(B2[b], hulls[b])):
                assert len(s) <= cap and all(h[0] <= x < y <= h[1] and x % 16 == 0 and y % 16 == 0 for x, y in s)
                assert all(s[i][1] < s[i + 1][0] for i in range(len(s) - 1))
                assert sum(seg.split_steps(s, h)) == seg.steps([[s]])     # the splits of the hull miss no step
                if kind != "nan_x":    # (the hull looks at cy only, like the lookup's rows)
                    cols = np.arange(j * 128, min(j * 128 + 128, P.slab))
                    assert not (T[b][:, cols] & ~seg.seg_mask(s, Q)[:, None]).any()
    for PW, PH in ((32, 4), (16, 8)):
        for caps in ((seg.CAP_A, seg.CAP_B), (3, 2), (5, 4)):   # tiny capacities: every widening
            A1, B1, modes = seg.patch_segments(runs, H, W, P, PW, PH, *caps)
            for b in range(B):
                for table, limit, cap in ((A1[b], P.slab, max(caps[0], 4)), (B1[b], Q, caps[1])):
                    for s in table:
                        assert len(s) <= cap
                        assert all(x % 16 == 0 and y % 16 == 0 and 0 <= x < y <= limit for x, y in s)
                        assert all(s[i][1] < s[i + 1][0] for i in range(len(s) - 1))
                for j, s in enumerate(A1[b]):
                    qs = seg.patch_queries(j, H, W, PW, PH)
                    assert not (T[b][qs[qs >= 0]] & ~seg.seg_mask(s, P.slab)[None]).any()
                for j, s in enumerate(B1[b]):
                    cols = np.arange(j * 128, min(j * 128 + 128, P.slab))
                    assert not (T[b][:, cols] & ~seg.seg_mask(s, Q)[:, None]).any()
            if kind == "jumpy" and H >= 13 and caps == (3, 2):   # (narrow windows on several tile rows: both lists overflow)
                assert max(modes["A"]) == 1 and max(modes["B"]) >= 1


def test_patches_partition_the_queries():
    for H, W, PW, PH in ((9, 32, 16, 8), (13, 64, 32, 4), (55, 128, 16, 8)):
        qs = np.concatenate([seg.patch_queries(j, H, W, PW, PH) for j in range((W // PW) * -(-H // PH))])
        assert sorted(qs[qs >= 0]) == list(range(H * W))
