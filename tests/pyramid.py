"""The all-pairs correlation pyramid (csrc/corr_pyramid.hip, the pooled epilogue of csrc/gemm_tile.hpp, the twin entry
point of csrc/gemm_bf16x3.hip) for the float64 tests: references written from the header's statement for fp32 inputs, a
mirror of the host's dispatch rules and of the pooled epilogue's store map, the gates and the shape tables of
tests/test_pyramid_f64_gpu.py and tests/test_pyramid_host_cpu.py.  The layout, tile / untile and the coordinate builders
are those of tests/lookup.py.  No GPU, no ctypes.

Statement (include/pcfa_hip.h, csrc/common.hpp): pyr[b Q + q][idx(l, y, x)] = avg_pool^l(fmap1[b, :, q] . fmap2[b] /
sqrt(D))[y][x], 2x2 average pooling with the odd last row / column dropped, every other float of a slab +0;
f2ext[b D + d] = the same chain on the plane fmap2[b, d]; the backward is the adjoint: dfmap1 = dpyr . f2ext^T / sqrt(D),
dfmap2 = the adjoint of the pooling chain applied to fmap1 . dpyr / sqrt(D), both reading the level texels of dpyr only.

Every reference takes a dtype: float64 is the reference proper, float32 the "plain fp32" implementation the CPU module
pushes through the same gates.

Gates (u = 2^-24, gamma and TINY of tests/fenced.py; the forms of tests/test_gemm_core_gpu.py):
  elementwise  |Y - Y64| <= 2 gamma(n) (|A||B|) + n TINY, |A||B| the same operation on the magnitudes of its inputs
  statistical  rel_l2 <= 2 u sqrt(n), over everything and (forward) per level
n per quantity (the longest chain of roundings behind one element):
  forward, level l   D + 3 l + 2        D fma steps, three additions per 2x2 average, + 2 (the division, one spare);
                                        over all levels at once: the n of the last level (every level is within its own)
  dfmap1             T + 8 + 2          T = the slab's level texels (the terms of one sum), the 8 split-K partials
  dfmap2             Q + 8 + 2 L + 2    Q terms, 8 partials, one add and one division per pooling level
"""
import collections
import functools
import math
import types

import torch
import torch.nn.functional as F

from tests import lookup as lk
from tests.fenced import TINY, U, gamma

BWD_SPLITS = 8
MAX_COORDS = 32
RUN = 16
RUNS_MAX_H = 1024
BM = BN = 128

# B, D, H, W, L; shift / dshift: floats by which fmap1 / dpyr are moved off their 16-byte alignment
Case = collections.namedtuple("Case", "B D H W L shift dshift", defaults=(0, 0))


def cid(c):
    return "B%d-D%d-%dx%d-L%d" % c[:5] + ("-shift%d" % c.shift if c.shift else "") + ("-dshift%d" % c.dshift if c.dshift else "")


def case_layout(c):
    return lk.layout(c.H, c.W, c.L)


# --------------------------------------------------------------------------- references
def chain(x, L):
    """[N][h][w] -> the L levels of the 2x2 average-pooling chain (an empty level below a single row or column)."""
    out = [x]
    for _ in range(L - 1):
        h, w = x.shape[-2:]
        x = F.avg_pool2d(x.unsqueeze(1), 2, stride=2).squeeze(1) if h >= 2 and w >= 2 else x.new_zeros(x.shape[0], h // 2, w // 2)
        out.append(x)
    return out


def texel_mask(lay):
    """[slab] bool: the level texels (everything else is a pad texel or the zero tile)."""
    m = torch.zeros(lay.slab, dtype=torch.bool)
    for l in range(lay.L):
        m[lay.index[l].reshape(-1)] = True
    return m


def f2ext(f2, lay, dtype=torch.float64):
    """[B D][slab]: lookup.tile of every plane of fmap2 and its pooled copies."""
    B, D, H, W = f2.shape
    return lk.tile(chain(f2.reshape(B * D, H, W).to(dtype), lay.L), lay)


def f2ext_kernel32(f2, lay):
    """f2ext_fwd_kernel's own arithmetic in fp32, level from level: (((p0 + p1) + p[wp]) + p[wp + 1]) / 4.  Additions and a
    division by 4 of fp32 values, each rounded once: the kernel must give these bits."""
    B, D, H, W = f2.shape
    x = f2.reshape(B * D, H, W).float()
    levels = [x]
    for l in range(1, lay.L):
        h, w = lay.h[l], lay.w[l]
        p = levels[-1]
        x = (((p[:, 0:2 * h:2, 0:2 * w:2] + p[:, 0:2 * h:2, 1:2 * w:2]) + p[:, 1:2 * h:2, 0:2 * w:2])
             + p[:, 1:2 * h:2, 1:2 * w:2]) / 4.0
        levels.append(x.reshape(B * D, h, w))
    return lk.tile(levels, lay)


def pyramid(f1, f2, lay, dtype=torch.float64, pool=chain):
    """[B Q][slab]: f1^T f2 / sqrt(D), the pooling chain per query, tiled."""
    B, D, H, W = f1.shape
    Q = H * W
    vol = torch.matmul(f1.reshape(B, D, Q).to(dtype).transpose(1, 2), f2.reshape(B, D, Q).to(dtype)) / math.sqrt(D)
    return lk.tile(pool(vol.reshape(B * Q, H, W), lay.L), lay)


def bwd(dpyr, f1, ext, lay, dtype=torch.float64, mask=True):
    """(dfmap1 [B][D][Q], dfmap2 [B][D][Q]) from dpyr [B Q][slab], fmap1 [B][D][H][W] and f2ext [B D][slab]; the level
    texels of dpyr only (mask=False: a mutant's switch, lets the products read every column)."""
    B, D, H, W = f1.shape
    Q = H * W
    g = dpyr.to(dtype)
    if mask:
        g = torch.where(texel_mask(lay), g, torch.zeros((), dtype=dtype))
    g = g.reshape(B, Q, lay.slab)
    df1 = torch.matmul(ext.to(dtype).reshape(B, D, lay.slab), g.transpose(1, 2)) / math.sqrt(D)
    t = torch.matmul(f1.reshape(B, D, Q).to(dtype), g) / math.sqrt(D)
    t = t.reshape(B * D, lay.slab)
    gl = [t[:, lay.index[l].reshape(-1)].reshape(B * D, lay.h[l], lay.w[l]) for l in range(lay.L)]   # (untile; empty levels)
    x = torch.zeros(B * D, H, W, dtype=dtype, requires_grad=True)
    loss = sum((a * b).sum() for a, b in zip(chain(x, lay.L), gl))
    loss.backward()
    return df1, x.grad.reshape(B, D, Q)


# --------------------------------------------------------------------------- the host's dispatch rules
def _fast(Q, D, shift1, shift_ext):
    return Q % 4 == 0 and shift1 % 4 == 0 and shift_ext % 4 == 0 and D % 4 == 0 and Q >= 4


def fwd_path(D, H, W, L, shift1=0, shift_ext=0):
    """pcfa_corr_pyramid_fwd (corr_pyramid.hip): "pool" (levels 1-2 pooled in the epilogue), "vector" (the branch-free
    loader on the product against all of f2ext) or "masked" (the predicated loader).  PCFA_PYRAMID_POOL=0 (a developer's
    A/B switch) is not mirrored."""
    if _fast(H * W, D, shift1, shift_ext):
        return "pool" if L >= 3 and W % 16 == 0 else "vector"
    return "masked"


def fwd_bf16x3_path(D, H, W, L, shift1=0, shift_ext=0):
    """pcfa_corr_pyramid_fwd_bf16x3 (gemm_bf16x3.hip): the same three paths by the same rule, restated there."""
    if _fast(H * W, D, shift1, shift_ext):
        return "pool" if L >= 3 and W % 16 == 0 else "vector"
    return "masked"


def bwd_paths(D, H, W, L, shift1=0, shift_ext=0, shift_d=0):
    """pcfa_corr_pyramid_bwd: (dfmap1's product, df2ext's product), each "vector" or "masked".  dfmap1 runs along the slab
    (a multiple of 16 floats) and asks for aligned f2ext and dpyr only; df2ext runs along the queries."""
    Q = H * W
    p1 = "vector" if shift_ext % 4 == 0 and shift_d % 4 == 0 else "masked"
    p2 = "vector" if Q % 4 == 0 and shift1 % 4 == 0 and shift_d % 4 == 0 and Q >= 4 else "masked"
    return p1, p2


def bwd_windows_path(D, H, W, L, n_coords, shift1=0, shift_ext=0, shift_d=0):
    """pcfa_corr_pyramid_bwd_windows: "runs" (df2ext's lists clipped in x as well), "rows" (both tables from the rows
    table) or "dense fallback" (the products of pcfa_corr_pyramid_bwd)."""
    Q = H * W
    fast = Q % 4 == 0 and shift1 % 4 == 0 and shift_ext % 4 == 0 and shift_d % 4 == 0 and Q >= 4
    if n_coords < 1 or n_coords > MAX_COORDS or not fast or H > 65535 or L > 4:
        return "dense fallback"
    return "runs" if W % RUN == 0 and H <= RUNS_MAX_H and L <= 4 else "rows"


# --------------------------------------------------------------------------- the pooled epilogue's store map
def store_map(lay, guarded=True):
    """[(slab position, writer)] of every store one query row receives on the pool path: gemm_tile_epilogue<POOL>'s
    index arithmetic (gemm_tile.hpp) and the tail blocks [off_tail, slab), restated.  Kept in step with the kernel BY
    HAND; tests/test_pyramid_f64_gpu.py ties it to the kernel (the positions that lose their sentinel are this map's).
    Writers: "gemm0" the level-0 columns, "tail" levels >= 3 and the zero tile, ("pool1" | "pool2" | "pad1" | "pad2",
    ty, tx) the level-0 tile whose thread pools into, or zeroes a pad row of, level 1 / 2.
    guarded=False: the map before the stores were confined to their level's own tile rows (every level-0 tile stored into
    levels 1 and 2 unconditionally and nothing wrote the pad rows no tile pools into) -- the mutant of the store-map test."""
    assert lay.L >= 3 and lay.W % 16 == 0
    tw0, th0 = lay.tw[0], lay.th[0]
    tiles0 = th0 * tw0
    off_tail = lay.off[3] if lay.L > 3 else lay.zero
    stores = [(p, "gemm0") for p in range(tiles0 * 16)] + [(p, "tail") for p in range(off_tail, lay.slab)]
    r1, r2 = (lay.h[1] + 3) // 4, (lay.h[2] + 3) // 4
    for T0 in range(tiles0):
        ty, tx = divmod(T0, tw0)
        last = guarded and ty == th0 - 1          # only the last level-0 tile row is guarded: the others lie inside
        in1, in2 = not last or (ty >> 1) < r1, not last or (ty >> 2) < r2
        d1 = lay.off[1] + ((ty >> 1) * lay.tw[1] + (tx >> 1)) * 16 + 2 * (ty & 1) * 4 + 2 * (tx & 1)
        d2 = lay.off[2] + ((ty >> 2) * lay.tw[2] + (tx >> 2)) * 16 + (ty & 3) * 4 + (tx & 3)
        if in1:
            stores += [(d1 + 4 * Y + X, ("pool1", ty, tx)) for Y in range(2) for X in range(2)]
        if in2:
            stores.append((d2, ("pool2", ty, tx)))
        if last and in1 and not ty & 1:
            stores += [(d1 + 4 * Y + X, ("pad1", ty, tx)) for Y in (2, 3) for X in range(2)]
        if last and in2:
            stores += [(d2 + 4 * (y - (ty & 3)), ("pad2", ty, tx)) for y in range((ty & 3) + 1, 4)]
    return stores


def store_map_faults(lay, guarded=True):
    """(positions outside [0, slab), positions with more than one writer, positions with none) of store_map."""
    pos = torch.tensor([p for p, _ in store_map(lay, guarded)])
    outside = sorted(set(pos[(pos < 0) | (pos >= lay.slab)].tolist()))
    cnt = torch.bincount(pos[(pos >= 0) & (pos < lay.slab)], minlength=lay.slab)
    return outside, torch.nonzero(cnt > 1).reshape(-1).tolist(), torch.nonzero(cnt == 0).reshape(-1).tolist()


# --------------------------------------------------------------------------- gates
def n_fwd(D, l):
    return D + 3 * l + 2


def n_df1(lay):
    return int(texel_mask(lay).sum()) + BWD_SPLITS + 2


def n_df2(Q, L):
    return Q + BWD_SPLITS + 2 * L + 2


def elem_ratio(got, want, P, n):
    return float(((got.double() - want).abs() / (2 * gamma(n) * P + n * TINY)).max()) if want.numel() else 0.0


def stat_ratio(got, want, n):
    num, den = float((got.double() - want).norm()), float(want.norm())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den / (2 * U * math.sqrt(n))


def fp32_gate(D):
    """The forward's gate of one level for the fp32 arithmetic: (got, want, P, l) -> (elementwise, statistical) ratio."""
    return lambda got, want, P, l: (elem_ratio(got, want, P, n_fwd(D, l)), stat_ratio(got, want, n_fwd(D, l)))


def nontexel_faults(got, lay):
    """The (row, slab position) of every float outside the level texels whose bits are not +0.0."""
    bits = got.contiguous().view(torch.int32)
    bad = (bits != 0) & ~texel_mask(lay)
    return torch.nonzero(bad)


def check_forward(got, c, record, prefix="", gate=None, stat_n=None):
    """A pyramid [B Q][slab] (fp32, on the CPU) of the case's inputs: every float outside the level texels is +0.0 bit for
    bit, every texel finite and inside both gates per level, the statistical gate over all levels at once.  gate: the
    level gate (default fp32_gate(D)); stat_n: the n of the all-levels statistical gate (default n_fwd(D, L - 1))."""
    lay = case_layout(c)
    ref = reference(c)
    gate = gate or fp32_gate(c.D)
    faults = nontexel_faults(got, lay)
    record(prefix + "nontexel_not_zero", int(faults.shape[0]))
    worst_e = worst_s = 0.0
    tex = texel_mask(lay)
    for l in range(c.L):
        idx = lay.index[l].reshape(-1)
        if idx.numel() == 0:
            continue
        g = got[:, idx]
        assert bool(torch.isfinite(g).all()), "level %d holds a non-finite texel (a sentinel: never written)" % l
        e, s = gate(g, ref.pyr[:, idx], ref.pyr_abs[:, idx], l)
        record(prefix + "level%d_elem_ratio" % l, "%.3g" % e)
        record(prefix + "level%d_stat_ratio" % l, "%.3g" % s)
        worst_e, worst_s = max(worst_e, e), max(worst_s, s)
    s_all = stat_ratio(got[:, tex], ref.pyr[:, tex], stat_n or n_fwd(c.D, c.L - 1))
    worst_s = max(worst_s, s_all)
    record(prefix + "elem_ratio", "%.3g" % worst_e)
    record(prefix + "stat_ratio", "%.3g" % worst_s)
    print("%s%s forward: elementwise %.3g statistical %.3g, %d non-texel floats not +0" % (prefix, cid(c), worst_e, worst_s,
                                                                                        faults.shape[0]))
    assert faults.shape[0] == 0, ("floats outside the level texels are not +0.0: (row, position)", faults[:8].tolist())
    assert worst_e <= 1, ("elementwise", worst_e)
    assert worst_s <= 1, ("statistical", worst_s)
    return worst_e, worst_s


def check_backward(got1, got2, dpyr, c, record, prefix=""):
    """dfmap1, dfmap2 [B][D][Q] (fp32, on the CPU) against bwd in float64 of the same dpyr, both gates on both."""
    lay = case_layout(c)
    ref = reference(c)
    want1, want2 = bwd(dpyr, ref.f1, ref.ext32, lay)
    P1, P2 = bwd(dpyr.abs(), ref.f1.abs(), ref.ext32.abs(), lay)
    out = []
    for name, got, want, P, n in (("df1", got1, want1, P1, n_df1(lay)), ("df2", got2, want2, P2, n_df2(c.H * c.W, c.L))):
        got = got.reshape(want.shape)
        assert bool(torch.isfinite(got).all()), name + " holds a non-finite value"
        e, s = elem_ratio(got, want, P, n), stat_ratio(got, want, n)
        record(prefix + name + "_elem_ratio", "%.3g" % e)
        record(prefix + name + "_stat_ratio", "%.3g" % s)
        out += [e, s]
    print("%s%s backward: df1 elementwise %.3g statistical %.3g, df2 elementwise %.3g statistical %.3g" % (
        (prefix, cid(c)) + tuple(out)))
    assert max(out[0], out[2]) <= 1, ("elementwise (df1, df2)", out[0], out[2])
    assert max(out[1], out[3]) <= 1, ("statistical (df1, df2)", out[1], out[3])
    return out


# --------------------------------------------------------------------------- inputs and references per case
@functools.lru_cache(maxsize=3)
def reference(c):
    """The case's seeded inputs and float64 forward: f1, f2 [B][D][H][W] (fp32), ext32 = f2ext_kernel32 (what the products
    are fed), pyr and pyr_abs [B Q][slab] (float64).  Computed once per case and shared; do not write into it."""
    gen = torch.Generator().manual_seed(c.B * 100003 + c.D * 1009 + c.H * 131 + c.W * 17 + c.L)
    f1 = torch.randn(c.B, c.D, c.H, c.W, generator=gen)
    f2 = torch.randn(c.B, c.D, c.H, c.W, generator=gen)
    lay = case_layout(c)
    return types.SimpleNamespace(f1=f1, f2=f2, ext32=f2ext_kernel32(f2, lay), pyr=pyramid(f1, f2, lay),
                                 pyr_abs=pyramid(f1.abs(), f2.abs(), lay))


def dense_dpyr(c, seed=0):
    """Random, finite and non-zero in every slab position, pad texels and the zero tile included."""
    gen = torch.Generator().manual_seed(seed * 7919 + c.H * 37 + c.W * 11 + c.D)
    return lk.nonzero_randn((c.B * c.H * c.W, case_layout(c).slab), gen)


def window_dpyr(c, coords_list, r, seed=0):
    """Random and non-zero on every position lookup.window_mask marks for the lookups given, exact zero elsewhere."""
    mask = lk.window_mask(list(coords_list), r, case_layout(c)) if coords_list else None
    d = dense_dpyr(c, seed + 1)
    return torch.where(mask, d, torch.zeros(())) if mask is not None else torch.zeros_like(d)


# --------------------------------------------------------------------------- shape tables
POOL = [                        # pool path: every class of H mod 16, both stray-store kinds, both past-the-slab shapes
    Case(1, 4, 8, 16, 4),       # H % 16 = 8: pad rows of level 2 no tile pools into; one query block
    Case(2, 20, 9, 32, 4),      # H % 8 = 1: the tile row below levels 1 and 2 (level 2, level 3 row 0, the zero tile)
    Case(1, 64, 9, 64, 4),      # the same, past the slab: positions 1008..1015
    Case(2, 4, 9, 64, 3),       # ... at L = 3 (the tail is the zero tile alone)
    Case(1, 20, 10, 32, 4),     # H % 16 = 10: pad rows of level 1 (and 2) unwritten
    Case(1, 64, 12, 16, 4),
    Case(1, 4, 13, 64, 4),      # H % 16 = 13: nothing stray, nothing unwritten; Q = 832: seven row blocks
    Case(2, 20, 16, 32, 4),     # whole tiles on every level
    Case(3, 4, 17, 16, 4),      # H % 16 = 1: below levels 1 and 2; three batch items
    Case(1, 20, 18, 32, 4),     # H % 16 = 2: below level 2 only, level 1 pad rows unwritten
    Case(1, 64, 19, 48, 4),     # H % 16 = 3
    Case(1, 4, 20, 16, 4),
    Case(1, 20, 21, 16, 4),
    Case(1, 64, 24, 48, 4),
    Case(2, 4, 25, 32, 4),      # H % 8 = 1, H % 16 = 9
    Case(1, 20, 33, 64, 4),     # past the slab: positions 2992..2995; Q = 2112
    Case(1, 4, 36, 64, 5),      # five levels: the tail holds levels 3 and 4
]
VECTOR = [
    Case(1, 4, 6, 10, 4),       # W % 16 != 0; the fourth level is empty (6x10, 3x5, 1x2, 0x1)
    Case(2, 20, 13, 20, 4),
    Case(1, 64, 12, 24, 4),
    Case(1, 20, 8, 16, 2),      # W % 16 == 0 but L < 3: pool refused
    Case(2, 4, 16, 16, 1),
    Case(1, 64, 8, 8, 4),       # level 3 is 1x1
]
MASKED = [
    Case(2, 4, 5, 7, 4),        # Q % 4 != 0; the fourth level is empty
    Case(1, 20, 9, 13, 4),
    Case(1, 64, 23, 37, 4),
    Case(1, 6, 8, 16, 4),       # D % 4 != 0
    Case(1, 20, 9, 32, 4, 1),   # fmap1 one float off its alignment
]
FORWARD = POOL + VECTOR + MASKED
F2EXT = [Case(2, 6, 13, 22, 4), Case(1, 4, 9, 32, 4), Case(1, 20, 36, 64, 5), Case(3, 4, 8, 8, 4), Case(1, 4, 16, 16, 1)]
BWD_DENSE = [                   # (dfmap1's product, df2ext's product): vector / masked each
    Case(2, 20, 9, 32, 4), Case(1, 64, 13, 64, 4), Case(1, 4, 6, 10, 4), Case(1, 20, 8, 16, 2), Case(1, 4, 36, 64, 5),
    Case(2, 4, 5, 7, 4), Case(1, 64, 23, 37, 4),      # Q % 4 != 0: df2ext masked
    Case(1, 20, 9, 32, 4, 1),                         # fmap1 shifted: df2ext masked
    Case(1, 6, 8, 16, 4, 0, 1),                       # dpyr shifted: both masked
    Case(1, 20, 9, 13, 4, 0, 2),
]
R = 4                           # the lookups' radius of the windowed backward
WINDOWS = [Case(1, 20, 9, 32, 4), Case(2, 64, 16, 32, 4),         # runs tables
           Case(1, 64, 24, 40, 4), Case(2, 20, 6, 10, 4)]         # rows tables
WINDOW_FALLBACKS = [(Case(1, 20, 23, 37, 4), 3), (Case(1, 4, 16, 32, 5), 3), (Case(1, 20, 9, 32, 4), 33)]   # (case, lists)
LOOKUP_KINDS = ("sweep", "fractions", "far")


def lookup_coords(kind, c):
    """The coordinate lists of tests/lookup.py for a windows case: one sweep per level, the fractions, the far grid."""
    if kind == "sweep":
        return [lk.sweep(c.B, c.H, c.W, c.L, R, l) for l in range(c.L)]
    return [{"fractions": lk.fractions, "far": lk.far}[kind](c.B, c.H, c.W)]
