"""The correlation lookups (csrc/corr_lookup.hip, csrc/corr_lookup_conv.hip) for the float64 tests: a Python mirror of
the pyramid layout (common.hpp: pcfa_make_layout, pcfa_tiled_index), the lookup, its transpose and the fused 1x1
convolution written once from the header's statement (include/pcfa_hip.h: channel l (2r+1)^2 + a (2r+1) + b samples
level l at (cx / 2^l + a - r, cy / 2^l + b - r), bilinear, zeros outside), a census of where every window sits
against its level's edges, tiles, pad texels and the kernels' clamps, coordinate builders that steer windows there, and
the shape tables and gates of tests/test_lookup_f64_gpu.py and tests/test_lookup_host_cpu.py.  No GPU, no ctypes.

Every reference takes a dtype: float64 is the reference proper, float32 the "plain fp32" implementation the CPU module
pushes through the same gates (a gate a plain fp32 implementation misses would be no gate).

Gates (u = 2^-24, gamma and TINY of tests/fenced.py):
  elementwise  |Y - Y64| <= 2 gamma(n) P + 2 u A + n TINY, P the blend of |texel| with the float64 weights, A the unweighted
               sum of the corner magnitudes: fx = xl - floor(xl) and 1 - fx are rounded absolutely (u / 2 each, so a weight
               is off by up to 2 u absolutely); with cx = -2^-30 fp32 has fx = 1 and drops a term float64 keeps.
  statistical  rel_l2 <= MARGIN u sqrt(n), over everything, per level and per census class of at least 256 elements.
n per entry (the longest chain of roundings one term goes through, + 2 spare as elsewhere):
  N_FWD     = 8   1 - f, the product of the two factors, the product with the texel, three sums
  n_bwd(k)  = 8 + k   the same chain, + one add into dpyr per accumulated lookup
  N_CONV_FWD = 324 + 1 + N_FWD   the 324-term dot product and the bias on top of the blend
  N_CONV_BWD = 256 + n_bwd(1)    the 256-term dot product under the scatter
"""
import functools
import math
import types

import torch

from tests.fenced import TINY, U, gamma

MAX_LEVELS = 8          # PCFA_MAX_LEVELS
N_FWD = 8
N_CONV_FWD = 324 + 1 + N_FWD
COUT, CIN = 256, 324
KL, KP = 88, 352        # padded tap rows per level / in all (corr_lookup_conv.hip)
MARGIN = 2.0            # rel_l2 <= MARGIN u sqrt(n): the factor 2 of tests/test_gemm_core_gpu.py; the plain fp32 CPU
#                         implementation stays below it on every table case (tests/test_lookup_host_cpu.py prints its ratios)


def n_bwd(k=1):
    return N_FWD + k


N_CONV_BWD = COUT + n_bwd(1)


# --------------------------------------------------------------------------- layout
@functools.lru_cache(maxsize=None)
def layout(H, W, L):
    """pcfa_make_layout: h, w, tw, th (tiles per row / column), off per level, zero (the all-zero tile), slab; plus
    index[l]: the [h_l][w_l] slab positions of level l (pcfa_tiled_index)."""
    assert 1 <= L <= MAX_LEVELS and H >= 1 and W >= 1
    lay = types.SimpleNamespace(H=H, W=W, L=L, h=[], w=[], tw=[], th=[], off=[], index=[])
    off, h, w = 0, H, W
    for _ in range(L):
        lay.h.append(h)
        lay.w.append(w)
        lay.tw.append((w + 3) // 4)
        lay.th.append((h + 3) // 4)
        lay.off.append(off)
        off += ((h + 3) // 4) * ((w + 3) // 4) * 16
        h //= 2
        w //= 2
    lay.zero = off
    lay.slab = off + 16
    for l in range(L):
        y = torch.arange(max(lay.h[l], 0)).view(-1, 1)
        x = torch.arange(max(lay.w[l], 0)).view(1, -1)
        lay.index.append(lay.off[l] + (((y >> 2) * lay.tw[l] + (x >> 2)) << 4) + ((y & 3) << 2) + (x & 3))
    return lay


def tile(levels, lay):
    """[N][slab] from the levels [N][h_l][w_l]: pad texels and the zero tile hold exact zeros."""
    N = levels[0].shape[0]
    out = torch.zeros(N, lay.slab, dtype=levels[0].dtype)
    for l, lv in enumerate(levels):
        assert lv.shape == (N, lay.h[l], lay.w[l])
        out[:, lay.index[l].reshape(-1)] = lv.reshape(N, -1)
    return out


def untile(mat, lay):
    return [mat[:, lay.index[l].reshape(-1)].reshape(-1, lay.h[l], lay.w[l]) for l in range(lay.L)]


def level_of_slab(lay):
    """[slab] level of every slab position (pad texels included), -1 for the zero tile."""
    lv = torch.full((lay.slab,), -1, dtype=torch.long)
    for l in range(lay.L):
        lv[lay.off[l]:(lay.off[l + 1] if l + 1 < lay.L else lay.zero)] = l
    return lv


# --------------------------------------------------------------------------- the lookup and its transpose
BIG = 1.0e30   # stands in for a non-finite coordinate in the references: every window far outside, no contribution


def sanitize(coords):
    """(coords with the queries that hold a non-finite coordinate moved far outside, bad [B Q])"""
    bad = ~torch.isfinite(coords).all(dim=1, keepdim=True)
    return torch.where(bad, torch.full((), BIG), coords), bad.reshape(-1)


def origins(coords, l, r, dtype=torch.float64):
    """x0, y0 (integer window origins, [B Q]) and the shared fractions of level l: coords / 2^l is exact, the floor
    is clamped to +-1e8 before the conversion (as make_origin in the kernels)."""
    c = coords.to(dtype)
    inv = 1.0 / (1 << l)
    xl, yl = c[:, 0].reshape(-1) * inv, c[:, 1].reshape(-1) * inv
    flx, fly = xl.floor(), yl.floor()
    return (flx.clamp(-1e8, 1e8).long() - r, fly.clamp(-1e8, 1e8).long() - r, xl - flx, yl - fly)


def _window(x0, y0, h, w, win):
    off = torch.arange(win)
    X = (x0.view(-1, 1, 1) + off.view(1, 1, win)).expand(-1, win, win)
    Y = (y0.view(-1, 1, 1) + off.view(1, win, 1)).expand(-1, win, win)
    ok = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
    return X, Y, ok


def _weights(fx, fy):
    fx, fy = fx.view(-1, 1, 1), fy.view(-1, 1, 1)
    return (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy


def lookup(levels, coords, r, dtype=torch.float64, bound=True):
    """pcfa_corr_lookup_fwd in `dtype` from the fp32 coordinates: (out [B][L (2r+1)^2][H][W], P, A)."""
    B, _, H, W = coords.shape
    N, n1, win = B * H * W, 2 * r + 1, 2 * r + 2
    outs = [[], [], []]
    for l, lv in enumerate(levels):
        lv = lv.to(dtype)
        h, w = lv.shape[-2:]
        x0, y0, fx, fy = origins(coords, l, r, dtype)
        X, Y, ok = _window(x0, y0, h, w, win)
        idx = torch.where(ok, Y.clamp(0, h - 1) * w + X.clamp(0, w - 1), torch.full((), h * w, dtype=torch.long))
        flat = torch.cat([lv.reshape(N, h * w), torch.zeros(N, 1, dtype=dtype)], 1)
        C = flat.gather(1, idx.reshape(N, -1)).reshape(N, win, win)                       # [q][y][x]
        ws = _weights(fx, fy)
        for k, (t, wk) in enumerate(((C, ws), (C.abs(), ws), (C.abs(), (1, 1, 1, 1)))[:3 if bound else 1]):
            v = wk[0] * t[:, :-1, :-1] + wk[1] * t[:, :-1, 1:] + wk[2] * t[:, 1:, :-1] + wk[3] * t[:, 1:, 1:]   # [q][b][a]
            outs[k].append(v.permute(0, 2, 1).reshape(N, n1 * n1))                        # channel a (2r+1) + b
    res = [torch.cat(o, 1).reshape(B, H * W, -1).permute(0, 2, 1).reshape(B, -1, H, W).contiguous() for o in outs if o]
    return tuple(res) if bound else res[0]


def lookup64(levels64, coords, r):
    return lookup(levels64, coords, r, torch.float64)


def scatter(coords, go, r, lay, dtype=torch.float64, go_abs=None, bound=True):
    """The exact transpose of `lookup` into a [B Q][slab] matrix in `dtype`: (D, P, A); P and A from |go| (or go_abs)."""
    B, _, H, W = coords.shape
    N, n1, win = B * H * W, 2 * r + 1, 2 * r + 2
    srcs = [go.to(dtype)] + ([(go if go_abs is None else go_abs).to(dtype).abs()] * 2 if bound else [])
    outs = [torch.zeros(N, lay.slab, dtype=dtype) for _ in srcs]
    rows = torch.arange(N).view(-1, 1, 1).expand(-1, win, win)
    for l in range(lay.L):
        h, w = lay.h[l], lay.w[l]
        x0, y0, fx, fy = origins(coords, l, r, dtype)
        X, Y, ok = _window(x0, y0, h, w, win)
        ws = _weights(fx, fy)
        pos = lay.index[l][Y[ok], X[ok]]
        for k, (src, out) in enumerate(zip(srcs, outs)):
            G = src.reshape(B, lay.L, n1, n1, H * W)[:, l].permute(0, 3, 2, 1).reshape(N, n1, n1)   # [q][b][a]
            wk = ws if k < 2 else (1, 1, 1, 1)
            d = torch.zeros(N, win, win, dtype=dtype)
            d[:, :-1, :-1] += wk[0] * G      # the kernels' order per texel: w00, w01, w10, w11
            d[:, :-1, 1:] += wk[1] * G
            d[:, 1:, :-1] += wk[2] * G
            d[:, 1:, 1:] += wk[3] * G
            out[rows[ok], pos] = d[ok]
    return tuple(outs) if bound else outs[0]


def scatter64(coords, go, r, lay, go_abs=None):
    return scatter(coords, go, r, lay, torch.float64, go_abs)


def window_mask(coords_list, r, lay):
    """[B Q][slab] bool: texels inside some (2r+2)^2 window of some lookup and inside their level."""
    B, _, H, W = coords_list[0].shape
    N, win = B * H * W, 2 * r + 2
    m = torch.zeros(N, lay.slab, dtype=torch.bool)
    rows = torch.arange(N).view(-1, 1, 1).expand(-1, win, win)
    for coords in coords_list:
        for l in range(lay.L):
            x0, y0, _, _ = origins(coords, l, r)
            X, Y, ok = _window(x0, y0, lay.h[l], lay.w[l], win)
            m[rows[ok], lay.index[l][Y[ok], X[ok]]] = True
    return m


def convc1(taps, W, bias, relu, dtype=torch.float64):
    """relu(W . taps + bias) per pixel: taps [B][324][H][W], W [256][324]; one matmul."""
    B, C, H, Wd = taps.shape
    y = torch.matmul(W.to(dtype), taps.to(dtype).reshape(B, C, H * Wd)) + bias.to(dtype).view(1, -1, 1)
    return (torch.relu(y) if relu else y).reshape(B, -1, H, Wd)


def convc1_64(taps64, W, bias, relu):
    return convc1(taps64, W, bias, relu)


def convc1_t(g, out, W, relu, dtype=torch.float64):
    """W^T (g [out > 0]): the tap gradients [B][324][H][W]; the mask comes from the `out` that is passed in."""
    B, C, H, Wd = g.shape
    gm = g.to(dtype)
    if relu:
        gm = torch.where(out > 0, gm, torch.zeros((), dtype=dtype))
    return torch.matmul(W.to(dtype).t(), gm.reshape(B, C, H * Wd)).reshape(B, -1, H, Wd)


# --------------------------------------------------------------------------- census
BASES = ("clamp_lo", "clamp_hi", "outside", "lo_cut", "hi_cut", "both_cut", "inside")


def axis_codes(o, n, r):
    """Class code of every integer origin `o` along one axis of a level of extent n (padded to n4 = 4 ceil(n / 4)):
    base * 8 + pad * 4 + (o & 3) for the overlapping classes, base * 8 otherwise."""
    win, n4 = 2 * r + 2, (n + 3) // 4 * 4
    over = (o + win > 0) & (o < n)
    lo, hi = o < 0, o + win > n
    base = torch.where(lo & hi, 5, torch.where(lo, 3, torch.where(hi, 4, 6)))
    base = torch.where(over, base, torch.full_like(o, 2))
    base = torch.where(o < -16, torch.zeros_like(o), base)
    base = torch.where(o > n4, torch.ones_like(o), base)
    pad = over & hi & (n % 4 != 0)
    return base * 8 + torch.where(over, pad.long() * 4 + (o & 3), torch.zeros_like(o))


def code_name(c):
    base, pad, ox = c >> 3, (c >> 2) & 1, c & 3
    return BASES[base] + ("+pad" if pad else "") + ("/o%d" % ox if base >= 3 else "")


def _cut(codes):
    return ((codes >> 3) >= 3) & ((codes >> 3) <= 5)


def window_classes(H, W, L, r, coords):
    """Per level: (x codes [B Q], y codes [B Q], corner [B Q]: x cut and y cut at once) of finite coordinates."""
    lay = layout(H, W, L)
    res = []
    for l in range(L):
        x0, y0, _, _ = origins(coords, l, r)
        cx, cy = axis_codes(x0, lay.w[l], r), axis_codes(y0, lay.h[l], r)
        res.append((cx, cy, _cut(cx) & _cut(cy)))
    return res


def census(H, W, L, r, coords_list):
    """Per level {"x": names, "y": names, "corner": bool} over all the windows of coords_list."""
    out = [{"x": set(), "y": set(), "corner": False} for _ in range(L)]
    for coords in coords_list:
        coords, _ = sanitize(coords)
        for l, (cx, cy, corner) in enumerate(window_classes(H, W, L, r, coords)):
            out[l]["x"] |= {code_name(c) for c in cx.unique().tolist()}
            out[l]["y"] |= {code_name(c) for c in cy.unique().tolist()}
            out[l]["corner"] |= bool(corner.any())
    return out


def origin_range(n4):
    return torch.arange(-24, n4 + 9)


def reachable(H, W, L, r):
    """What brute force over every integer origin in [-24, 4 tw + 8] (resp. th4) can produce, per level."""
    lay = layout(H, W, L)
    out = []
    for l in range(L):
        cx = axis_codes(origin_range(4 * lay.tw[l]), lay.w[l], r)
        cy = axis_codes(origin_range(4 * lay.th[l]), lay.h[l], r)
        out.append({"x": {code_name(c) for c in cx.tolist()}, "y": {code_name(c) for c in cy.tolist()},
                    "corner": bool(_cut(cx).any() and _cut(cy).any())})
    return out


# --------------------------------------------------------------------------- coordinates
def identity(B, H, W):
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([x, y]).unsqueeze(0).repeat(B, 1, 1, 1)


def sweep(B, H, W, L, r, l, seed=0):
    """Origins of level l walking the whole range [-24, 4 tw + 8] x [-24, th4 + 8]: x by one per query, y by a stride
    coprime to its range, plus fractional parts below 0.99."""
    lay = layout(H, W, L)
    gen = torch.Generator().manual_seed(1000 * seed + 17 * l + H * W)
    xs, ys = origin_range(4 * lay.tw[l]), origin_range(4 * lay.th[l])
    i = torch.arange(B * H * W)
    stride = next(s for s in (7, 11, 13, 5, 3, 1) if math.gcd(s, len(ys)) == 1)
    x0, y0 = xs[i % len(xs)], ys[(i * stride + i // len(xs)) % len(ys)]
    fr = torch.rand(2, B * H * W, generator=gen) * 0.99
    c = torch.stack([(x0 + r).float() + fr[0], (y0 + r).float() + fr[1]]) * float(1 << l)    # [2][B Q]
    return c.reshape(2, B, H, W).permute(1, 0, 2, 3).contiguous()


FRACTIONS = (0.0, 0.5, 2.0 ** -20, 1 - 2.0 ** -20, -2.0 ** -30)


def fractions(B, H, W):
    """Integer origins plus every pair of {0, 0.5, 2^-20, 1 - 2^-20, -2^-30}; the last only survives next to the
    integer 0 and rounds fx to exactly 1.0f (2^-20 and 1 - 2^-20: next to integers below 4)."""
    c = identity(B, H, W).reshape(B, 2, -1)
    i = torch.arange(H * W)
    pick = torch.stack([i % 5, (i // 5) % 5])                                 # [2][Q]
    fr = torch.tensor(FRACTIONS, dtype=torch.float64)[pick]
    base = c.double()
    base = torch.where(pick >= 2, base % 4, base)
    base = torch.where(pick == 4, torch.zeros((), dtype=torch.float64), base)
    return (base + fr).float().reshape(B, 2, H, W)


FAR = (1.0e4, -1.0e4, 3.0e38, -3.0e38)


def far(B, H, W):
    """+-1e4 and +-3e38 on either axis, the other axis far as well or on the identity grid."""
    c = identity(B, H, W).reshape(B, 2, -1)
    i = torch.arange(H * W)
    pick = torch.stack([i % 5, (i // 5) % 5])
    vals = torch.tensor((0.0,) + FAR, dtype=torch.float32)[pick]
    return torch.where(pick == 0, c, vals).reshape(B, 2, H, W)


def poisoned_queries(H, W):
    Q = H * W
    return (1, Q // 2, Q - 1)


def nonfinite(B, H, W):
    """far's grid with NaN (x), +inf (y) and -inf (both) in three queries per image."""
    c = far(B, H, W).reshape(B, 2, -1).clone()
    a, b, d = poisoned_queries(H, W)
    c[:, 0, a] = float("nan")
    c[:, 1, b] = float("inf")
    c[:, :, d] = float("-inf")
    return c.reshape(B, 2, H, W)


# --------------------------------------------------------------------------- shape tables: (B, H, W, L, r)
UNFUSED = [
    (2, 13, 22, 4, 4),    # 13x22, 6x11, 3x5, 1x2: every level padded in both axes; Q = 286: Q % 32 = 30, Q % 4 = 2
    (1, 16, 32, 4, 4),    # whole tiles; Q % 32 = 0
    (1, 8, 8, 4, 4),      # 1x1 top level
    (1, 33, 35, 5, 2),    # five levels, radius 2
    (1, 32, 40, 6, 3),    # six levels down to 2x2 and 1x1, radius 3
    (2, 9, 7, 1, 1),      # one level, radius 1
    (1, 18, 27, 3, 2),    # three levels, radius 2
]
FUSED = [
    (2, 13, 22, 4, 4),    # Q % 4 != 0: every tile takes the backward's per-float path
    (1, 12, 25, 4, 4),    # Q = 300: full tiles and one ragged tile
    (1, 16, 32, 4, 4),    # all tiles full
    (1, 8, 8, 4, 4),      # the smallest shape
]


def sid(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def cases(shape):
    """The shape's named lookups: identity, one sweep per level, fractions, far, nonfinite."""
    B, H, W, L, r = shape
    out = [("identity", identity(B, H, W))]
    out += [("sweep%d" % l, sweep(B, H, W, L, r, l)) for l in range(L)]
    out += [("fractions", fractions(B, H, W)), ("far", far(B, H, W)), ("nonfinite", nonfinite(B, H, W))]
    return tuple(out)


def case_names(shape):
    L = shape[3]
    return ["identity"] + ["sweep%d" % l for l in range(L)] + ["fractions", "far", "nonfinite"]


def case_ids(table):
    return [(s, name) for s in table for name in case_names(s)]


@functools.lru_cache(maxsize=None)
def pyramid(shape, seed=0):
    """Random levels [B Q][h_l][w_l] (fp32) and their tiled slabs."""
    B, H, W, L, r = shape
    lay = layout(H, W, L)
    gen = torch.Generator().manual_seed(seed * 7919 + H * 131 + W * 17 + L + r)
    levels = [torch.randn(B * H * W, lay.h[l], lay.w[l], generator=gen) for l in range(L)]
    return levels, tile(levels, lay)


def nonzero_randn(shape, gen):
    t = torch.randn(*shape, generator=gen)
    return torch.where(t == 0, torch.ones(()), t)


@functools.lru_cache(maxsize=None)
def gradients(shape, channels, seed=0):
    """grad_out [B][channels][H][W] and dpyr0 [B Q][slab] (no zero of either sign)."""
    B, H, W, L, r = shape
    gen = torch.Generator().manual_seed(seed * 7919 + H * 37 + W * 11 + channels)
    return torch.randn(B, channels, H, W, generator=gen), nonzero_randn((B * H * W, layout(H, W, L).slab), gen)


@functools.lru_cache(maxsize=None)
def conv_weights(seed=0):
    gen = torch.Generator().manual_seed(seed + 4242)
    return torch.randn(COUT, CIN, generator=gen) / 18.0, 0.1 * torch.randn(COUT, generator=gen)


# --------------------------------------------------------------------------- gates
def _ratio(num, den):
    return float((num / den).max()) if num.numel() else 0.0


def class_groups(shape, coords_list):
    """name -> [B Q][L] bool: the (query, level) windows of each census class (per axis, and the corner class), over the
    lookups given (a window is in a class if any of the lookups puts it there)."""
    B, H, W, L, r = shape
    groups = {}
    for coords in coords_list:
        coords, _ = sanitize(coords)
        for l, (cx, cy, corner) in enumerate(window_classes(H, W, L, r, coords)):
            for axis, codes in (("x", cx), ("y", cy)):
                for c in codes.unique().tolist():
                    g = groups.setdefault("l%d/%s/%s" % (l, axis, code_name(c)), torch.zeros(B * H * W, L, dtype=torch.bool))
                    g[:, l] |= codes == c
            g = groups.setdefault("l%d/corner" % l, torch.zeros(B * H * W, L, dtype=torch.bool))
            g[:, l] |= corner
    return groups


def blend_gates(got, want, P, A, n, per_window, groups, record, prefix="", keep=None):
    """Both gates; records and returns (elementwise ratio, statistical ratio, its worst class).  want, P, A: float64, of
    got's shape; per_window(t) sums t into [B Q][K] (K = L: per (query, level) window; K = 1: per query, every level's
    classes then group the queries); groups: class_groups; keep: bool, broadcastable to got -- the elements that take
    part (default: all)."""
    err = got.double() - want
    ratio = err.abs() / (2 * gamma(n) * P + 2 * U * A + n * TINY)
    ones = torch.ones_like(want)
    if keep is not None:
        keep = keep.expand_as(want)
        zero = torch.zeros((), dtype=torch.float64)
        ratio, err, want, ones = (torch.where(keep, t, zero) for t in (ratio, err, want, ones))
    e2, w2, cnt = per_window(err * err), per_window(want * want), per_window(ones)
    K = e2.shape[1]
    sel = {"all": torch.ones_like(e2, dtype=torch.bool)}
    for l in range(K if K > 1 else 0):
        sel["level%d" % l] = torch.zeros_like(e2, dtype=torch.bool)
        sel["level%d" % l][:, l] = True
    for name, g in groups.items():
        sel[name] = g if K > 1 else g.any(dim=1, keepdim=True)
    stat, worst, lim = 0.0, "", MARGIN * U * math.sqrt(n)
    for name, m in sel.items():
        if float(cnt[m].sum()) < 256 or float(w2[m].sum()) == 0.0:
            continue
        s = math.sqrt(float(e2[m].sum()) / float(w2[m].sum())) / lim
        if not s <= stat:
            stat, worst = s, name
    elem = float(ratio.max())
    record(prefix + "elem_ratio", "%.3g" % elem)
    record(prefix + "stat_ratio", "%.3g" % stat)
    record(prefix + "stat_worst_class", worst)
    assert elem <= 1, ("elementwise", elem)
    assert stat <= 1, ("statistical", stat, worst)
    return elem, stat, worst


def per_level_channels(B, H, W, L):
    """per_window of a lookup output [B][L n][H][W]: [B Q][L]"""
    return lambda t: t.reshape(B, L, -1, H * W).sum(2).permute(0, 2, 1).reshape(B * H * W, L)


def per_query(t):
    """per_window of a fused output [B][256][H][W]: [B Q][1]"""
    return t.sum(1).reshape(-1, 1)


def per_level_slab(lay):
    """per_window of a slab matrix [B Q][slab]: [B Q][L]"""
    lv = level_of_slab(lay) + 1
    return lambda t: torch.zeros(t.shape[0], lay.L + 1, dtype=t.dtype).index_add_(1, lv, t)[:, 1:]


# --------------------------------------------------------------------------- the checks of one call's result
def query_keep(bad, B, H, W):
    return (~bad).reshape(B, 1, H, W)


def check_lookup_fwd(got, shape, coords, record, prefix=""):
    """pcfa_corr_lookup_fwd's result [B][L (2r+1)^2][H][W] of the shape's pyramid against lookup64."""
    B, H, W, L, r = shape
    clean, bad = sanitize(coords)
    want, P, A = lookup64([lv.double() for lv in pyramid(shape)[0]], clean, r)
    return blend_gates(got, want, P, A, N_FWD, per_level_channels(B, H, W, L), class_groups(shape, [clean]), record, prefix,
                       query_keep(bad, B, H, W))


def outside_unchanged(got, dpyr0, mask):
    """dpyr is bit-equal to dpyr0 outside the windows (pad texels and the zero tile included)"""
    return torch.equal(got.view(torch.int32)[~mask], dpyr0.view(torch.int32)[~mask])


def check_lookup_bwd(got, dpyr0, shape, coords_list, gos, record, prefix=""):
    """dpyr [B Q][slab] after the lookups' backwards accumulated into dpyr0: bit-unchanged outside the windows, gated
    against dpyr0 + sum of scatter64 inside (n = n_bwd(lookups))."""
    B, H, W, L, r = shape
    lay = layout(H, W, L)
    clean = [sanitize(c)[0] for c in coords_list]
    mask = window_mask(clean, r, lay)
    assert outside_unchanged(got, dpyr0, mask), "dpyr changed outside the windows"
    want, P, A = dpyr0.double(), dpyr0.double().abs(), torch.zeros(dpyr0.shape, dtype=torch.float64)
    for c, go in zip(clean, gos):
        d, p, a = scatter64(c, go, r, lay)
        want, P, A = want + d, P + p, A + a
    return blend_gates(got, want, P, A, n_bwd(len(clean)), per_level_slab(lay), class_groups(shape, clean), record, prefix,
                       mask)


def check_convc1_fwd(got, shape, coords, Wt, bias, relu, record, prefix=""):
    """pcfa_lookup_convc1_fwd's result [B][256][H][W] against convc1_64(lookup64); P and A pushed through |W|."""
    B, H, W, L, r = shape
    clean, bad = sanitize(coords)
    taps, P, A = lookup64([lv.double() for lv in pyramid(shape)[0]], clean, r)
    want = convc1_64(taps, Wt, bias, relu)
    Pc = convc1(P, Wt.abs(), bias.abs(), 0)
    Ac = convc1(A, Wt.abs(), torch.zeros_like(bias), 0)
    return blend_gates(got, want, Pc, Ac, N_CONV_FWD, per_query, class_groups(shape, [clean]), record, prefix,
                       query_keep(bad, B, H, W))


def check_convc1_bwd(got, dpyr0, shape, coords, Wt, out, go, relu, record, prefix=""):
    """dpyr after pcfa_lookup_convc1_bwd: bit-unchanged outside the windows, gated against
    dpyr0 + scatter64(W^T (go [out > 0])) inside."""
    B, H, W, L, r = shape
    lay = layout(H, W, L)
    clean, _ = sanitize(coords)
    mask = window_mask([clean], r, lay)
    assert outside_unchanged(got, dpyr0, mask), "dpyr changed outside the windows"
    dt = convc1_t(go, out, Wt, relu)
    dt_abs = convc1_t(go.abs(), out, Wt.abs(), relu)
    d, p, a = scatter64(clean, dt, r, lay, go_abs=dt_abs)
    return blend_gates(got, dpyr0.double() + d, dpyr0.double().abs() + p, a, N_CONV_BWD, per_level_slab(lay),
                       class_groups(shape, [clean]), record, prefix, mask)


# --------------------------------------------------------------------------- plain fp32 on the CPU
def fp32_lookup_fwd(shape, coords):
    return lookup(pyramid(shape)[0], sanitize(coords)[0], shape[4], torch.float32, bound=False)


def fp32_lookup_bwd(dpyr0, shape, coords_list, gos):
    B, H, W, L, r = shape
    d = dpyr0.clone()
    for c, go in zip(coords_list, gos):
        d = d + scatter(sanitize(c)[0], go, r, layout(H, W, L), torch.float32, bound=False)
    return d


def fp32_convc1_fwd(shape, coords, Wt, bias, relu):
    return convc1(fp32_lookup_fwd(shape, coords), Wt, bias, relu, torch.float32)


def fp32_convc1_bwd(dpyr0, shape, coords, Wt, out, go, relu):
    B, H, W, L, r = shape
    dt = convc1_t(go, out, Wt, relu, torch.float32)
    return dpyr0 + scatter(sanitize(coords)[0], dt, r, layout(H, W, L), torch.float32, bound=False)
