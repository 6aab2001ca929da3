#!/usr/bin/env python3
"""numpy restatement of the K-segment tables of the correlation pyramid's windowed backward (csrc/corr_pyramid.hip) and a
count of the BK = 16 steps the two products execute under them.

  rows scheme   : corr_window_rows_kernel / corr_window_segments_kernel -- one (min cy, max cy) per query row; a block of
                  dfmap1 is 128 consecutive queries, its segments are whole tile rows; a block of df2ext gets the hull of
                  the query rows that reach its tile rows.
  runs scheme   : corr_window_runs_kernel / corr_window_run_segments_kernel (what the library does) -- dfmap1 as in the
                  rows scheme; df2ext keeps the rows scheme's hull (its splits share it) and walks, per reaching query
                  row inside it, one segment of the runs of 16 queries whose windows reach the block in x AND y.
  patch scheme  : counted, not built into the library -- df2ext as in the runs scheme without the hull; a block of dfmap1
                  is a PW x PH patch of queries and gets one segment of tile columns per tile row.  It splits dfmap1's
                  sums differently from the rows scheme, so its results differ in their last bits.

usage: pyramid_bwd_segments.py DUMP.npz     (DUMP from tools/dump_closure_coords.py)
Prints the step counts of both schemes for the patch shapes 32x4 and 16x8 as a markdown table.
"""
import sys

import numpy as np

BN, BK, RUN = 128, 16, 16
CAP = 48                # SEG_CAP of corr_pyramid.hip
CAP_A, CAP_B = 32, 48   # the capacities the patch scheme was counted with


class Layout:
    """PyrLayout / pcfa_make_layout (csrc/common.hpp)."""

    def __init__(self, H, W, L):
        self.L, self.h, self.w, self.tw, self.off = L, [], [], [], []
        off, h, w = 0, H, W
        for _ in range(L):
            self.h.append(h)
            self.w.append(w)
            self.tw.append((w + 3) // 4)
            self.off.append(off)
            off += ((h + 3) // 4) * ((w + 3) // 4) * 16
            h //= 2
            w //= 2
        self.zero = off
        self.slab = off + 16

    def level_end(self, l):
        return self.off[l + 1] if l + 1 < self.L else self.zero

    def index(self, l, y, x):
        return self.off[l] + (((y >> 2) * self.tw[l] + (x >> 2)) << 4) + ((y & 3) << 2) + (x & 3)


def _texels(lo, hi, l, r, n):
    """min / max of a coordinate (float32 arrays) -> the texels [a, c] of level l its windows can touch (one of slack)."""
    inv = np.float32(1.0 / (1 << l))
    flo = np.clip(np.floor(lo.astype(np.float32) * inv), -1.0e8, 1.0e8).astype(np.int64)
    fhi = np.clip(np.floor(hi.astype(np.float32) * inv), -1.0e8, 1.0e8).astype(np.int64)
    return np.maximum(flo - r - 1, 0), np.minimum(fhi + r + 2, n - 1)


def _minmax(c, axis):
    """min / max over `axis`; a NaN anywhere -> (-3e38, 3e38): everything."""
    bad = np.isnan(c).any(axis=axis)
    lo, hi = np.fmin.reduce(c, axis=axis), np.fmax.reduce(c, axis=axis)   # (fmin / fmax skip NaN)
    return np.where(bad, np.float32(-3.0e38), lo), np.where(bad, np.float32(3.0e38), hi)


def _merge(segs):
    out = []
    for b, e in segs:
        if out and out[-1][1] == b:
            out[-1][1] = e
        else:
            out.append([b, e])
    return [tuple(s) for s in out]


# ------------------------------------------------------------------------------------------------ rows scheme
def rows_table(coords, r, P):
    """coords [n, B, 2, H, W] float32 -> rows[B][L][H][2]."""
    n, B, _, H, W = coords.shape
    lo, hi = _minmax(coords[:, :, 1].transpose(1, 2, 0, 3).reshape(B, H, n * W), 2)
    out = np.zeros((B, P.L, H, 2), np.int64)
    for l in range(P.L):
        out[:, l, :, 0], out[:, l, :, 1] = _texels(lo, hi, l, r, P.h[l])
    return out


def rows_segments(rows, H, W, P):
    """-> (segA, segB): per batch item a list over blocks of segment lists [(begin, end), ...]."""
    B, Q = rows.shape[0], H * W
    nbA, nbB = -(-Q // BN), -(-P.slab // BN)
    A, Bt = [], []
    for b in range(B):
        ta = []
        for j in range(nbA):
            qa, qb = (j * BN) // W, min((j * BN + BN - 1) // W, H - 1)
            segs = []
            for l in range(P.L):
                rr = rows[b, l, qa:qb + 1]
                rr = rr[rr[:, 0] <= rr[:, 1]]
                if len(rr):
                    ylo, yhi = int(rr[:, 0].min()), int(rr[:, 1].max())
                    segs.append((P.off[l] + (ylo >> 2) * P.tw[l] * 16, P.off[l] + ((yhi >> 2) + 1) * P.tw[l] * 16))
            ta.append(_merge(segs))
        tb = []
        for j in range(nbB):
            ca, cb = j * BN, min(j * BN + BN, P.slab) - 1
            qlo, qhi = 1 << 30, -1
            for l in range(P.L):
                a, c = max(ca, P.off[l]), min(cb, P.level_end(l) - 1)
                if a > c:
                    continue
                ya, yb = ((a - P.off[l]) // (P.tw[l] * 16)) * 4, ((c - P.off[l]) // (P.tw[l] * 16)) * 4 + 3
                rr = rows[b, l]
                hit = np.nonzero((rr[:, 0] <= rr[:, 1]) & (rr[:, 0] <= yb) & (rr[:, 1] >= ya))[0]
                if len(hit):
                    qlo, qhi = min(qlo, int(hit[0])), max(qhi, int(hit[-1]))
            tb.append([((qlo * W) // BK * BK, min(-(-((qhi + 1) * W) // BK) * BK, -(-Q // BK) * BK))] if qlo <= qhi else [])
        A.append(ta)
        Bt.append(tb)
    return A, Bt


# ---------------------------------------------------------------------------------------------- patch scheme
def runs_table(coords, r, P):
    """coords [n, B, 2, H, W] -> runs[B][L][H][NR][4] = texels (xlo, xhi, ylo, yhi) per run of 16 queries; W % 16 == 0."""
    n, B, _, H, W = coords.shape
    NR = W // RUN
    c = coords.reshape(n, B, 2, H, NR, RUN).transpose(1, 2, 3, 4, 0, 5).reshape(B, 2, H, NR, n * RUN)
    bad = np.isnan(c).any(axis=(1, 4))                       # a NaN in x or y: the run reaches everything
    out = np.zeros((B, P.L, H, NR, 4), np.int64)
    for ch, k in ((0, 0), (1, 2)):
        lo, hi = _minmax(c[:, ch], 3)
        lo, hi = np.where(bad, np.float32(-3.0e38), lo), np.where(bad, np.float32(3.0e38), hi)
        for l in range(P.L):
            out[:, l, :, :, k], out[:, l, :, :, k + 1] = _texels(lo, hi, l, r, P.w[l] if ch == 0 else P.h[l])
    return out


def patch_segments(runs, H, W, P, PW, PH, cap_a=CAP_A, cap_b=CAP_B):
    """-> (segA, segB, modes): block j of segA = patch (j // (W / PW), j % (W / PW)); modes = the widening each record took."""
    assert PW * PH == BN and PW % RUN == 0 and W % PW == 0
    B, NR = runs.shape[0], W // RUN
    npx, npy = W // PW, -(-H // PH)
    nbB = -(-P.slab // BN)
    A, Bt, modes = [], [], {"A": [], "B": []}
    for b in range(B):
        ta = []
        for j in range(npx * npy):
            py, px = divmod(j, npx)
            hull = []
            for l in range(P.L):
                rr = runs[b, l, py * PH:min(py * PH + PH, H), px * (PW // RUN):(px + 1) * (PW // RUN)].reshape(-1, 4)
                rr = rr[(rr[:, 0] <= rr[:, 1]) & (rr[:, 2] <= rr[:, 3])]
                hull.append((int(rr[:, 0].min()), int(rr[:, 1].max()), int(rr[:, 2].min()), int(rr[:, 3].max()))
                            if len(rr) else None)
            for mode in (0, 1):   # 0: clipped in x ; 1: whole tile rows
                segs = []
                for l, hl in enumerate(hull):
                    if hl is None:
                        continue
                    xlo, xhi, ylo, yhi = hl
                    if mode == 1:
                        segs.append((P.off[l] + (ylo >> 2) * P.tw[l] * 16, P.off[l] + ((yhi >> 2) + 1) * P.tw[l] * 16))
                    else:
                        segs += [(P.off[l] + (ty * P.tw[l] + (xlo >> 2)) * 16, P.off[l] + (ty * P.tw[l] + (xhi >> 2) + 1) * 16)
                                 for ty in range(ylo >> 2, (yhi >> 2) + 1)]
                segs = _merge(segs)
                if len(segs) <= cap_a:
                    break
            ta.append(segs)
            modes["A"].append(mode)
        tb = []
        for j in range(nbB):
            ca, cb = j * BN, min(j * BN + BN, P.slab) - 1
            reach = np.zeros((H, NR), bool)
            for l in range(P.L):
                a, c = max(ca, P.off[l]), min(cb, P.level_end(l) - 1)
                if a > c:
                    continue
                ta_, tb_ = (a - P.off[l]) >> 4, (c - P.off[l]) >> 4
                tya, tyb = ta_ // P.tw[l], tb_ // P.tw[l]
                txa, txb = (ta_ % P.tw[l], tb_ % P.tw[l]) if tya == tyb else (0, P.tw[l] - 1)
                rr = runs[b, l]
                reach |= ((rr[..., 0] <= rr[..., 1]) & (rr[..., 2] <= rr[..., 3]) & (rr[..., 0] <= txb * 4 + 3) &
                          (rr[..., 1] >= txa * 4) & (rr[..., 2] <= tyb * 4 + 3) & (rr[..., 3] >= tya * 4))
            qys = np.nonzero(reach.any(1))[0]
            for mode in (0, 1, 2):   # 0: the runs' hull per query row ; 1: whole query rows ; 2: one hull
                if mode == 2:
                    segs = [(int(qys[0]) * W, (int(qys[-1]) + 1) * W)] if len(qys) else []
                    break
                segs = []
                for qy in qys:
                    rx = np.nonzero(reach[qy])[0]
                    lo, hi = (int(rx[0]), int(rx[-1])) if mode == 0 else (0, NR - 1)
                    segs.append((int(qy) * W + RUN * lo, int(qy) * W + RUN * (hi + 1)))
                segs = _merge(segs)
                if len(segs) <= cap_b:
                    break
            tb.append(segs)
            modes["B"].append(mode)
        A.append(ta)
        Bt.append(tb)
    return A, Bt, modes


def run_segments(rows, runs, H, W, P, cap=CAP):
    """The runs scheme's table B -> (segB, hulls [b][block] -> (begin, end), modes)."""
    B, NR, Q = runs.shape[0], W // RUN, H * W
    _, hullB = rows_segments(rows, H, W, P)
    Bt, hulls, modes = [], [], []
    for b in range(B):
        tb, th = [], []
        for j in range(-(-P.slab // BN)):
            ca, cb = j * BN, min(j * BN + BN, P.slab) - 1
            hull = hullB[b][j][0] if hullB[b][j] else (0, 0)
            in_hull = np.zeros(H, bool)
            reach = np.zeros((H, NR), bool)
            for l in range(P.L):
                a, c = max(ca, P.off[l]), min(cb, P.level_end(l) - 1)
                if a > c:
                    continue
                ta_, tb_ = (a - P.off[l]) >> 4, (c - P.off[l]) >> 4
                tya, tyb = ta_ // P.tw[l], tb_ // P.tw[l]
                txa, txb = (ta_ % P.tw[l], tb_ % P.tw[l]) if tya == tyb else (0, P.tw[l] - 1)
                rw, rr = rows[b, l], runs[b, l]
                in_hull |= (rw[:, 0] <= rw[:, 1]) & (rw[:, 0] <= tyb * 4 + 3) & (rw[:, 1] >= tya * 4)
                reach |= ((rr[..., 0] <= rr[..., 1]) & (rr[..., 2] <= rr[..., 3]) & (rr[..., 0] <= txb * 4 + 3) &
                          (rr[..., 1] >= txa * 4) & (rr[..., 2] <= tyb * 4 + 3) & (rr[..., 3] >= tya * 4))
            reach &= in_hull[:, None]
            qys = np.nonzero(reach.any(1))[0]
            for mode in (0, 1, 2):   # 0: the runs' hull per query row ; 1: whole query rows ; 2: one hull
                if mode == 2:
                    segs = [(int(qys[0]) * W, (int(qys[-1]) + 1) * W)] if len(qys) else []
                    break
                segs = []
                for qy in qys:
                    rx = np.nonzero(reach[qy])[0]
                    lo, hi = (int(rx[0]), int(rx[-1])) if mode == 0 else (0, NR - 1)
                    segs.append((int(qy) * W + RUN * lo, int(qy) * W + RUN * (hi + 1)))
                segs = _merge(segs)
                if len(segs) <= cap:
                    break
            tb.append(segs)
            th.append(hull)
            modes.append(mode)
        Bt.append(tb)
        hulls.append(th)
    return Bt, hulls, modes


def split_steps(segs, hull, splits=8):
    """BK steps each split of a df2ext block walks: the splits share the hull, each walks the segments inside its share."""
    total = (hull[1] - hull[0]) // BK
    out = []
    for s in range(splits):
        k0, k1 = hull[0] + total * s // splits * BK, hull[0] + total * (s + 1) // splits * BK
        out.append(sum(max(0, min(e, k1) - max(b, k0)) // BK for b, e in segs))
    return out


def patch_queries(j, H, W, PW, PH):
    """Query indices of patch block j, -1 for patch rows at or beyond H (column n of the block -> query)."""
    py, px = divmod(j, W // PW)
    n = np.arange(BN)
    y, x = py * PH + n // PW, px * PW + n % PW
    return np.where(y < H, y * W + x, -1)


# ------------------------------------------------------------------------------------------------------------- counting
def steps(table):
    return sum((e - b) // BK for item in table for blk in item for b, e in blk)


def touched(coords, r, P):
    """Brute force: touched[b][q, slab column] = some lookup's (2r+2)^2 window of query q can add into that column."""
    n, B, _, H, W = coords.shape
    out = np.zeros((B, H * W, P.slab), bool)
    q = np.arange(H * W)
    for b in range(B):
        for i in range(n):
            cx, cy = coords[i, b, 0].reshape(-1).astype(np.float64), coords[i, b, 1].reshape(-1).astype(np.float64)
            nan = np.isnan(cx) | np.isnan(cy)
            out[b, nan, :P.zero] = True          # a NaN coordinate promises nothing: everything
            for l in range(P.L):
                fx = np.clip(np.floor(np.where(nan, 0, cx) / (1 << l)), -1e8, 1e8).astype(np.int64)
                fy = np.clip(np.floor(np.where(nan, 0, cy) / (1 << l)), -1e8, 1e8).astype(np.int64)
                for dy in range(-r, r + 2):
                    for dx in range(-r, r + 2):
                        x, y = fx + dx, fy + dy
                        ok = (x >= 0) & (x < P.w[l]) & (y >= 0) & (y < P.h[l]) & ~nan
                        out[b, q[ok], P.off[l] + (((y[ok] >> 2) * P.tw[l] + (x[ok] >> 2)) << 4) + ((y[ok] & 3) << 2) + (x[ok] & 3)] = True
    return out


def seg_mask(segs, n):
    m = np.zeros(n, bool)
    for b, e in segs:
        m[b:min(e, n)] = True
    return m


def main():
    d = np.load(sys.argv[1])
    coords, r, L = d["coords"].astype(np.float32), int(d["radius"]), int(d["levels"])
    n, B, _, H, W = coords.shape
    P = Layout(H, W, L)
    D = int(d["D"]) if "D" in d else 256
    rows = rows_table(coords, r, P)
    A0, B0 = rows_segments(rows, H, W, P)
    sa0, sb0 = steps(A0), steps(B0)
    print("%d lookups, B = %d, feature map %dx%d, %d levels, radius %d, slab %d" % (n, B, H, W, L, r, P.slab))
    counted = {"rows": (sa0, sb0)}
    dense = -(-H * W // BN) * (P.slab // BK) + -(-P.slab // BN) * (-(-H * W // BK))
    print()
    print("| scheme | dfmap1 steps | df2ext steps | sum | against rows | longest list A / B | widened A / B |")
    print("|---|---|---|---|---|---|---|")
    print("| dense | | | %d | | | |" % dense)
    print("| rows (clipped in y only) | %d | %d | %d | 1.00 | %d / %d | |" % (sa0, sb0, sa0 + sb0, max(len(s) for t in A0 for s in t),
                                                                  max(len(s) for t in B0 for s in t)))
    runs = runs_table(coords, r, P)
    B2, hulls, modes2 = run_segments(rows, runs, H, W, P)
    counted["runs"] = (sa0, steps(B2))
    print("| runs (library): dfmap1 as rows | %d | %d | %d | %.2fx fewer | %d / %d | - / %d |" % (
        sa0, steps(B2), sa0 + steps(B2), (sa0 + sb0) / float(sa0 + steps(B2)), max(len(s) for t in A0 for s in t),
        max(len(s) for t in B2 for s in t), sum(m > 0 for m in modes2)))
    for PW, PH in ((32, 4), (16, 8)):
        if W % PW:
            continue
        A1, B1, modes = patch_segments(runs, H, W, P, PW, PH, 1 << 20, 1 << 20)
        sa, sb = steps(A1), steps(B1)
        _, _, capped = patch_segments(runs, H, W, P, PW, PH)
        counted["patch %dx%d" % (PW, PH)] = (steps(patch_segments(runs, H, W, P, PW, PH)[0]), steps(patch_segments(runs, H, W, P, PW, PH)[1]))
        print("| patch %dx%d | %d | %d | %d | %.2fx fewer | %d / %d | %d / %d |" % (
            PW, PH, sa, sb, sa + sb, (sa0 + sb0) / float(sa + sb), max(len(s) for t in A1 for s in t),
            max(len(s) for t in B1 for s in t), sum(m > 0 for m in capped["A"]), sum(m > 0 for m in capped["B"])))
    if "issued_dfmap1" in d:   # what the kernels of the dumping build walked (its work recorder)
        k = tuple(int(round(float(d[n]) / (2.0 * D * BN * BK))) for n in ("issued_dfmap1", "issued_df2ext"))
        same = [name for name, v in counted.items() if v == k]
        print()
        print("steps of the dumping build's own tables (work recorder): dfmap1 %d, df2ext %d = %s"
              % (k[0], k[1], ", ".join(same) if same else "NONE of the schemes above"))
    print()
    print("per level of df2ext's blocks (by the level of the block's first column), rows -> patch 32x4:")
    if W % 32 == 0:
        _, B1, _ = patch_segments(runs, H, W, P, 32, 4, 1 << 20, 1 << 20)
        for l in range(L):
            js = [j for j in range(len(B0[0])) if P.off[l] <= j * BN < P.level_end(l)]
            print("  level %d: %d -> %d" % (l, steps([[t[j] for j in js] for t in B0]), steps([[t[j] for j in js] for t in B1])))


if __name__ == "__main__":
    main()
