"""The mirror, the float64 references, the census and the gates of tests/lookup.py on the CPU (no GPU).

The layout mirror against the library's host-only entry points; lookup64 against the oracle's grid_sample form in
float64; scatter64 as the adjoint of lookup64; the coverage condition -- every census class brute force can reach is hit
by the shape's handful of lookups; and the same lookup, scatter and 1x1 convolution in plain fp32 torch through every gate
on every table case: the gates are ones a plain fp32 implementation stays within, so a kernel that misses them is wrong
and not merely differently rounded.  The worst ratios are printed (pytest -s) and recorded as junit properties.
"""
import os

import pytest
import torch

from tests import lookup as lk
from tests.test_winograd_f64_gpu import _mask_tensor

torch.set_num_threads(min(16, torch.get_num_threads()))
SHAPES = sorted(set(lk.UNFUSED + lk.FUSED))


def _lib():
    from pcfa_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip.load()


# --------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("shape", SHAPES, ids=lk.sid)
def test_layout_matches_the_library(shape):
    """pcfa_corr_slab_floats, pcfa_corr_level_offset and pcfa_corr_tiled_index (every texel) against layout()."""
    import ctypes
    lib = _lib()
    B, H, W, L, r = shape
    lay = lk.layout(H, W, L)
    assert int(lib.pcfa_corr_slab_floats(H, W, L)) == lay.slab == lay.zero + 16
    seen = torch.zeros(lay.slab, dtype=torch.long)
    for l in range(L):
        h, w = ctypes.c_int(), ctypes.c_int()
        assert int(lib.pcfa_corr_level_offset(H, W, L, l, ctypes.byref(h), ctypes.byref(w))) == lay.off[l]
        assert (h.value, w.value) == (lay.h[l], lay.w[l]) and lay.tw[l] == -(-lay.w[l] // 4)
        for y in range(lay.h[l]):
            for x in range(lay.w[l]):
                assert int(lib.pcfa_corr_tiled_index(H, W, L, l, y, x)) == int(lay.index[l][y, x])
        seen[lay.index[l].reshape(-1)] += 1
        assert int(lib.pcfa_corr_tiled_index(H, W, L, l, lay.h[l], 0)) == -1
    assert int(seen.max()) == 1 and int(seen[lay.zero:].sum()) == 0       # injective, and nothing in the zero tile
    assert int(lib.pcfa_corr_slab_floats(H, W, 0)) == -1 and int(lib.pcfa_corr_slab_floats(H, W, lk.MAX_LEVELS + 1)) == -1


@pytest.mark.parametrize("shape", SHAPES, ids=lk.sid)
def test_tile_untile(shape):
    B, H, W, L, r = shape
    lay = lk.layout(H, W, L)
    levels, tiled = lk.pyramid(shape)
    assert all(torch.equal(a, b) for a, b in zip(levels, lk.untile(tiled, lay)))
    texels = torch.zeros(lay.slab, dtype=torch.bool)
    for l in range(L):
        texels[lay.index[l].reshape(-1)] = True
    assert bool((tiled[:, ~texels] == 0).all()) and int(texels.sum()) == sum(h * w for h, w in zip(lay.h, lay.w))
    assert bool((lk.level_of_slab(lay)[texels] >= 0).all()) and bool((lk.level_of_slab(lay)[lay.zero:] == -1).all())


def test_lookup64_equals_the_oracle(oracle_ops):
    """oracle.ops.corr_lookup (grid_sample, zeros padding) in float64 on coordinates that straddle every edge (its
    normalised coordinates divide by extent - 1: no level of extent 1 here)."""
    shape = (1, 16, 32, 4, 4)
    B, H, W, L, r = shape
    levels = [lv.double() for lv in lk.pyramid(shape)[0]]
    gen = torch.Generator().manual_seed(5)
    coords = lk.identity(B, H, W) + 6 * torch.randn(B, 2, H, W, generator=gen)
    want = oracle_ops.corr_lookup([lv.unsqueeze(1) for lv in levels], coords.double(), r)
    got, P, A = lk.lookup64(levels, coords, r)
    assert got.shape == want.shape == (B, L * 81, H, W)
    assert float((got - want).abs().max()) <= 1e-12
    assert bool((P >= got.abs() * (1 - 1e-12)).all()) and bool((A >= P * (1 - 1e-12)).all())


@pytest.mark.parametrize("shape", SHAPES, ids=lk.sid)
def test_scatter64_is_the_adjoint_of_lookup64(shape):
    """<lookup64(p), g> == <p, scatter64(g)> to 1e-12 (relative to the sum of the magnitudes), on every finite case; and
    scatter64 touches window_mask only."""
    B, H, W, L, r = shape
    lay = lk.layout(H, W, L)
    levels = [lv.double() for lv in lk.pyramid(shape)[0]]
    p = lk.tile(levels, lay)
    g = lk.gradients(shape, L * (2 * r + 1) ** 2)[0].double()
    for name, coords in lk.cases(shape):
        coords, _ = lk.sanitize(coords)
        out, P, _ = lk.lookup64(levels, coords, r)
        d, _, a = lk.scatter64(coords, g, r, lay)
        lhs, rhs = float((out * g).sum()), float((p * d).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(float((P * g.abs()).sum()), 1.0), (name, lhs, rhs)
        mask = lk.window_mask([coords], r, lay)
        assert bool((d[~mask] == 0).all()) and bool((a[~mask] == 0).all()), name
        assert not bool(mask[:, lay.zero:].any())


# --------------------------------------------------------------------------- the coverage condition
def test_census_classes():
    """The classes by hand on 13x22 (level 0: w = 22, tw = 6; level 3: 1x2), r = 4: window of 10 texels."""
    o = torch.tensor([-17, -16, -10, -9, -1, 0, 12, 13, 21, 22, 24, 25])
    names = [lk.code_name(c) for c in lk.axis_codes(o, 22, 4).tolist()]
    assert names == ["clamp_lo", "outside", "outside", "lo_cut/o3", "lo_cut/o3", "inside/o0", "inside/o0", "hi_cut+pad/o1",
                     "hi_cut+pad/o1", "outside", "outside", "clamp_hi"]
    names = {lk.code_name(c) for c in lk.axis_codes(torch.arange(-24, 13), 2, 4).tolist()}
    assert names == {"clamp_lo", "clamp_hi", "outside", "lo_cut/o3", "lo_cut/o0", "hi_cut+pad/o0", "hi_cut+pad/o1"} | \
        {"both_cut+pad/o%d" % k for k in range(4)}
    assert {lk.code_name(c) for c in lk.axis_codes(torch.arange(-24, 41), 32, 4).tolist()} >= {"hi_cut/o3", "inside/o2"}


@pytest.mark.parametrize("shape", SHAPES, ids=lk.sid)
def test_cases_reach_every_reachable_class(shape):
    """The census over the shape's lookups equals reachable() at every level: a condition, not a measurement."""
    B, H, W, L, r = shape
    cases = lk.cases(shape)
    assert [n for n, _ in cases] == lk.case_names(shape) and len(cases) <= L + 4
    got, want = lk.census(H, W, L, r, [c for _, c in cases]), lk.reachable(H, W, L, r)
    for l in range(L):
        for key in ("x", "y"):
            assert got[l][key] == want[l][key], (l, key, sorted(want[l][key] - got[l][key]), sorted(got[l][key] - want[l][key]))
        assert got[l]["corner"] == want[l]["corner"], l


def test_special_coordinates():
    """fractions holds the value that rounds fx to exactly 1.0f; nonfinite poisons three queries per image."""
    c = lk.fractions(1, 13, 22)
    assert bool((c == -2.0 ** -30).any()) and bool((c == 0.5).any()) and bool((c == 2.0 ** -20).any())
    x0, _, fx, _ = lk.origins(c, 0, 4, torch.float32)
    assert bool(((fx == 1.0) & (x0 == -5)).any())
    bad = lk.sanitize(lk.nonfinite(2, 13, 22))[1]
    assert int(bad.sum()) == 6 and not bool(lk.sanitize(lk.far(2, 13, 22))[1].any())
    assert float(lk.far(1, 13, 22).abs().max()) == float(torch.tensor(3.0e38))


# --------------------------------------------------------------------------- plain fp32 inside every gate
WORST = {}


def _note(record_property, entry, res):
    elem, stat, worst = res
    w = WORST.setdefault(entry, [0.0, 0.0, ""])
    if stat > w[1]:
        w[1], w[2] = stat, worst
    w[0] = max(w[0], elem)
    print("%s: plain fp32 elementwise %.3g, statistical %.3g (%s); worst so far %.3g / %.3g (%s)" % ((entry, elem, stat, worst) + tuple(w)))


@pytest.mark.parametrize("case", lk.case_ids(lk.UNFUSED), ids=lambda c: "%s-%s" % (lk.sid(c[0]), c[1]))
def test_fp32_lookup_passes_the_gates(record_property, case):
    shape, name = case
    B, H, W, L, r = shape
    coords = dict(lk.cases(shape))[name]
    _note(record_property, "lookup_fwd", lk.check_lookup_fwd(lk.fp32_lookup_fwd(shape, coords), shape, coords, record_property))
    go, dpyr0 = lk.gradients(shape, L * (2 * r + 1) ** 2)
    got = lk.fp32_lookup_bwd(dpyr0, shape, [coords], [go])
    _note(record_property, "lookup_bwd", lk.check_lookup_bwd(got, dpyr0, shape, [coords], [go], record_property, "bwd_"))


@pytest.mark.parametrize("shape", lk.UNFUSED, ids=lk.sid)
def test_fp32_accumulated_scatter_passes_the_gates(record_property, shape):
    B, H, W, L, r = shape
    coords = [c for _, c in lk.cases(shape)]
    gos = [lk.gradients(shape, L * (2 * r + 1) ** 2, seed=k)[0] for k in range(len(coords))]
    dpyr0 = lk.gradients(shape, L * (2 * r + 1) ** 2)[1]
    got = lk.fp32_lookup_bwd(dpyr0, shape, coords, gos)
    _note(record_property, "lookup_bwd_acc", lk.check_lookup_bwd(got, dpyr0, shape, coords, gos, record_property))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", lk.case_ids(lk.FUSED), ids=lambda c: "%s-%s" % (lk.sid(c[0]), c[1]))
def test_fp32_convc1_passes_the_gates(record_property, case, relu):
    shape, name = case
    B, H, W, L, r = shape
    coords = dict(lk.cases(shape))[name]
    Wt, bias = lk.conv_weights()
    got = lk.fp32_convc1_fwd(shape, coords, Wt, bias, relu)
    _note(record_property, "convc1_fwd", lk.check_convc1_fwd(got, shape, coords, Wt, bias, relu, record_property))
    go, dpyr0 = lk.gradients(shape, lk.COUT)
    out = _mask_tensor((B, lk.COUT, H, W), torch.Generator().manual_seed(3))
    got = lk.fp32_convc1_bwd(dpyr0, shape, coords, Wt, out, go, relu)
    _note(record_property, "convc1_bwd",
          lk.check_convc1_bwd(got, dpyr0, shape, coords, Wt, out, go, relu, record_property, "bwd_"))


def test_gates_catch_a_wrong_kernel():
    """The per-class step's point: one window column misplaced by a texel in the right-edge-cut, ox = 3 class only, an
    error the global rel-L2 of the whole output would average away, fails the gates."""
    shape = (1, 16, 32, 4, 4)
    coords = dict(lk.cases(shape))["sweep0"]
    got = lk.fp32_lookup_fwd(shape, coords).clone()
    cx = lk.window_classes(16, 32, 4, 4, coords)[0][0]
    hit = (cx == lk.axis_codes(torch.tensor([27]), 32, 4)[0]).reshape(1, 1, 16, 32)
    assert int(hit.sum()) >= 4
    got[:, :81] = torch.where(hit, got[:, :81].roll(1, dims=1), got[:, :81])
    with pytest.raises(AssertionError):
        lk.check_lookup_fwd(got, shape, coords, lambda *_: None)
    # the +-2 u A term alone is no loophole: an error of 1e-6 of a texel fails too
    got = lk.fp32_lookup_fwd(shape, coords) * (1 + 1e-6)
    with pytest.raises(AssertionError):
        lk.check_lookup_fwd(got, shape, coords, lambda *_: None)
