"""The references, mirrors and gates of tests/pyramid.py on the CPU (no GPU).

The same pyramid build and backward in plain fp32 torch go through every gate on every table case: the gates are ones a
plain fp32 implementation stays within, so a kernel that misses them is wrong and not merely differently rounded (its
ratios are printed, pytest -s, and recorded as junit properties).  The dispatch mirror names every path at least twice
over the tables.  Mutants -- a zero over one level-3 texel, a 16-wide K segment dropped from either backward product, a
pooling that keeps the odd last row, a pad float left at the sentinel, dfmap2 from a dpyr whose pad columns are read --
each fail a gate or an assertion.  The pooled epilogue's store map gives every slab position exactly one writer and no
store outside [0, slab) on every pool-path layout of H in 8..80, W in {16, 32, 48, 64}, L in {3, 4, 5}; the map without
the guards (what the epilogue did before) fails there, at exactly the heights its arithmetic predicts.
"""
import collections

import pytest
import torch
import torch.nn.functional as F

from tests import lookup as lk
from tests import pyramid as pm
from tests.fenced import SENTINEL

torch.set_num_threads(min(16, torch.get_num_threads()))


def _fp32_forward(c):
    ref = pm.reference(c)
    return pm.pyramid(ref.f1, ref.f2, pm.case_layout(c), torch.float32)


def _fp32_backward(c, dpyr):
    ref = pm.reference(c)
    return pm.bwd(dpyr, ref.f1, ref.ext32, pm.case_layout(c), torch.float32)


# --------------------------------------------------------------------------- plain fp32 through the gates
@pytest.mark.parametrize("c", pm.FORWARD, ids=pm.cid)
def test_plain_fp32_forward_passes_the_gates(record_property, c):
    pm.check_forward(_fp32_forward(c), c, record_property, "fp32_")


@pytest.mark.parametrize("c", pm.F2EXT, ids=pm.cid)
def test_f2ext_restatement_is_within_gamma_of_float64(c):
    """f2ext_kernel32 against the float64 chain: level l within gamma(3 l) (level 0 is a copy), pads exact zeros."""
    lay = pm.case_layout(c)
    f2 = pm.reference(c).f2
    got, want, mag = pm.f2ext_kernel32(f2, lay), pm.f2ext(f2, lay), pm.f2ext(f2.abs(), lay)
    assert pm.nontexel_faults(got, lay).shape[0] == 0
    for l in range(c.L):
        idx = lay.index[l].reshape(-1)
        assert bool(((got[:, idx].double() - want[:, idx]).abs() <= pm.gamma(3 * l) * mag[:, idx] + 3 * l * pm.TINY).all()), l


@pytest.mark.parametrize("c", pm.BWD_DENSE, ids=pm.cid)
def test_plain_fp32_dense_backward_passes_the_gates(record_property, c):
    dpyr = pm.dense_dpyr(c)
    pm.check_backward(*_fp32_backward(c, dpyr), dpyr, c, record_property, "fp32_")


@pytest.mark.parametrize("kind", pm.LOOKUP_KINDS)
@pytest.mark.parametrize("c", pm.WINDOWS + [f[0] for f in pm.WINDOW_FALLBACKS[:2]], ids=pm.cid)
def test_plain_fp32_windowed_backward_passes_the_gates(record_property, c, kind):
    dpyr = pm.window_dpyr(c, pm.lookup_coords(kind, c), pm.R)
    tex = pm.texel_mask(pm.case_layout(c))
    assert bool((dpyr[:, ~tex] == 0).all()) and float(dpyr.abs().max()) > 0
    pm.check_backward(*_fp32_backward(c, dpyr), dpyr, c, record_property, "fp32_")


def test_bwd_is_the_adjoint_of_the_pyramid():
    """<pyramid(f1, f2), g> differentiated by autograd in float64 equals bwd(g, f1, f2ext) to 1e-12."""
    c = pm.Case(2, 6, 13, 22, 4)
    lay, ref = pm.case_layout(c), pm.reference(c)
    a, b = ref.f1.double().requires_grad_(True), ref.f2.double().requires_grad_(True)
    g = pm.dense_dpyr(c).double()
    (pm.pyramid(a, b, lay) * g).sum().backward()
    df1, df2 = pm.bwd(g, ref.f1, pm.f2ext(ref.f2, lay), lay)
    for got, want in ((df1, a.grad), (df2, b.grad)):
        want = want.reshape(got.shape)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# --------------------------------------------------------------------------- the dispatch mirror
def test_dispatch_mirror_names_every_path_twice():
    fwd = collections.Counter(pm.fwd_path(c.D, c.H, c.W, c.L, c.shift) for c in pm.FORWARD)
    x3 = collections.Counter(pm.fwd_bf16x3_path(c.D, c.H, c.W, c.L, c.shift) for c in pm.FORWARD)
    assert all(pm.fwd_path(c.D, c.H, c.W, c.L, c.shift) == want
               for table, want in ((pm.POOL, "pool"), (pm.VECTOR, "vector"), (pm.MASKED, "masked")) for c in table)
    dense = [pm.bwd_paths(c.D, c.H, c.W, c.L, c.shift, 0, c.dshift) for c in pm.BWD_DENSE]
    p1, p2 = collections.Counter(p[0] for p in dense), collections.Counter(p[1] for p in dense)
    win = collections.Counter([pm.bwd_windows_path(c.D, c.H, c.W, c.L, 3) for c in pm.WINDOWS] +
                              [pm.bwd_windows_path(c.D, c.H, c.W, c.L, n) for c, n in pm.WINDOW_FALLBACKS])
    print(dict(fwd), dict(x3), dict(p1), dict(p2), dict(win))
    for counts, names in ((fwd, ("pool", "vector", "masked")), (x3, ("pool", "vector", "masked")),
                          (p1, ("vector", "masked")), (p2, ("vector", "masked")),
                          (win, ("runs", "rows", "dense fallback"))):
        assert all(counts[n] >= 2 for n in names), (counts, names)
    assert all(pm.bwd_windows_path(c.D, c.H, c.W, c.L, n) == "dense fallback" for c, n in pm.WINDOW_FALLBACKS)


# --------------------------------------------------------------------------- mutants
MUTANT = pm.Case(2, 20, 13, 20, 4)       # 13x20, 6x10, 3x5, 1x2: every level padded, level 1 has a pad row above row 12


def test_mutant_zero_over_a_level3_texel():
    c = pm.Case(1, 20, 24, 48, 4)
    lay = pm.case_layout(c)
    got = _fp32_forward(c)
    idx = lay.index[3].reshape(-1)
    q, k = divmod(int(got[:, idx].abs().argmax()), idx.numel())
    got[q, idx[k]] = 0.0
    with pytest.raises(AssertionError, match="elementwise"):
        pm.check_forward(got, c, lambda *a: None)


@pytest.mark.parametrize("product", ["df1", "df2"])
def test_mutant_dropped_k_segment(product):
    c = MUTANT
    lay, ref = pm.case_layout(c), pm.reference(c)
    dpyr = pm.dense_dpyr(c)
    cut = dpyr.clone()
    if product == "df1":
        cut[:, lay.off[1]:lay.off[1] + 16] = 0.0           # one 16-wide segment of the slab
        got = (pm.bwd(cut, ref.f1, ref.ext32, lay, torch.float32)[0], _fp32_backward(c, dpyr)[1])
    else:
        cut[c.H * c.W + 32:c.H * c.W + 48] = 0.0            # sixteen queries of the second image
        got = (_fp32_backward(c, dpyr)[0], pm.bwd(cut, ref.f1, ref.ext32, lay, torch.float32)[1])
    with pytest.raises(AssertionError, match="elementwise"):
        pm.check_backward(*got, dpyr, c, lambda *a: None)


def test_mutant_pooling_keeps_the_odd_last_row():
    """avg_pool2d with ceil_mode: a level of ceil(h / 2) rows.  The tiling refuses its shape; cut back to the layout's
    rows it still differs in nothing -- so the mutant that matters averages the odd row INTO the last pooled row."""
    c = MUTANT
    lay, ref = pm.case_layout(c), pm.reference(c)

    def ceil_chain(x, L):
        out = [x]
        for _ in range(L - 1):
            x = F.avg_pool2d(x.unsqueeze(1), 2, stride=2, ceil_mode=True).squeeze(1)
            out.append(x)
        return out

    with pytest.raises(AssertionError):
        pm.pyramid(ref.f1, ref.f2, lay, torch.float32, pool=ceil_chain)

    def folded_chain(x, L):                      # the odd last row is added into the last window
        out = [x]
        for l in range(1, L):
            h = x.shape[1]
            y = pm.chain(x, 2)[1].clone()
            if h % 2 and h > 1:
                y[:, -1] = (y[:, -1] * 4 + x[:, -1, 0:2 * y.shape[2]:2] + x[:, -1, 1:2 * y.shape[2]:2]) / 6
            x = y
            out.append(x)
        return out

    with pytest.raises(AssertionError, match="elementwise"):
        pm.check_forward(pm.pyramid(ref.f1, ref.f2, lay, torch.float32, pool=folded_chain), c, lambda *a: None)


def test_mutant_pad_float_left_at_the_sentinel():
    c = MUTANT
    lay = pm.case_layout(c)
    pads = torch.nonzero(~pm.texel_mask(lay)).reshape(-1)
    for p in (int(pads[0]), int(pads[len(pads) // 2]), lay.slab - 1):
        got = _fp32_forward(c)
        got.view(torch.int32)[c.H * c.W + 3, p] = SENTINEL
        with pytest.raises(AssertionError, match="outside the level texels"):
            pm.check_forward(got, c, lambda *a: None)
    got = _fp32_forward(c)
    got[0, int(pads[0])] = -0.0                  # a negative zero is not +0.0 either
    with pytest.raises(AssertionError, match="outside the level texels"):
        pm.check_forward(got, c, lambda *a: None)


def test_mutant_df2_reads_pad_columns():
    """The adjoint of the pooling taken over the padded tiles: level 1's pad row 6 lands on row 12 of dfmap2."""
    c = MUTANT
    lay, ref = pm.case_layout(c), pm.reference(c)
    dpyr = pm.dense_dpyr(c)
    df1, df2 = _fp32_backward(c, dpyr)
    t = torch.matmul(ref.f1.reshape(c.B, c.D, -1), dpyr.reshape(c.B, -1, lay.slab)) / c.D ** 0.5    # df2ext, pads and all
    mut = df2.clone().reshape(c.B, c.D, c.H, c.W)
    y1 = lay.h[1]                                 # the first pad row of level 1
    assert y1 % 4 != 0 and 2 * y1 < c.H
    for x in range(lay.w[1]):
        p = lay.off[1] + ((y1 >> 2) * lay.tw[1] + (x >> 2)) * 16 + (y1 & 3) * 4 + (x & 3)
        mut[:, :, 2 * y1, 2 * x:2 * x + 2] += t[:, :, p].reshape(c.B, c.D, 1) / 4
    with pytest.raises(AssertionError, match="elementwise"):
        pm.check_backward(df1, mut.reshape(c.B, c.D, -1), dpyr, c, lambda *a: None)
    pm.check_backward(df1, df2, dpyr, c, lambda *a: None)


# --------------------------------------------------------------------------- the store map
POOL_LAYOUTS = [(H, W, L) for L in (3, 4, 5) for W in (16, 32, 48, 64) for H in range(8, 81)
                if pm.fwd_path(4, H, W, L) == "pool"]
# H % 8 == 1: the last level-0 tile row lies below level 1's tile rows; H % 16 in {1, 2, 3}: below level 2's
STRAY_HEIGHTS = [9, 17, 18, 19, 25, 33, 34, 35, 41, 49, 50, 51, 57, 65, 66, 67, 73]


def test_store_map_one_writer_per_slab_position():
    assert len(POOL_LAYOUTS) == 3 * 4 * 73
    for H, W, L in POOL_LAYOUTS:
        outside, twice, never = pm.store_map_faults(lk.layout(H, W, L))
        assert not outside and not twice and not never, ((H, W, L), outside[:4], twice[:4], never[:4])


def test_store_map_without_the_guards_fails():
    """The unguarded map (every level-0 tile stores into levels 1 and 2): stores land on other writers' positions or past
    the slab at exactly STRAY_HEIGHTS, and pad rows stay unwritten at every H % 16 outside {13, 14, 15, 0, 1}."""
    stray = [H for H in range(8, 81) if any(pm.store_map_faults(lk.layout(H, 64, 4), guarded=False)[:2])]
    assert stray == STRAY_HEIGHTS, stray
    past = ((9, 64, 4, 1008, list(range(1008, 1016))),       # level-0 texels (0..1, 0..3) of the next query's row
            (9, 64, 3, 976, list(range(976, 984)) + list(range(992, 1000)) + list(range(1008, 1016))),
            (33, 64, 4, 2992, list(range(2992, 2996))))
    for H, W, L, slab, want in past:
        lay = lk.layout(H, W, L)
        assert lay.slab == slab and pm.store_map_faults(lay, guarded=False)[0] == want
    lay = lk.layout(9, 32, 4)
    twice = set(pm.store_map_faults(lay, guarded=False)[1])
    assert set(lay.index[2].reshape(-1).tolist()) <= twice and set(lay.index[3][0].tolist()) <= twice \
        and set(range(lay.zero, lay.slab)) & twice
    clean = sorted({H % 16 for H in range(8, 81) if not pm.store_map_faults(lk.layout(H, 32, 4), guarded=False)[2]})
    assert clean == [0, 1, 13, 14, 15], clean
    bad = [s for s in POOL_LAYOUTS if any(pm.store_map_faults(lk.layout(*s), guarded=False))]
    assert len(bad) > len(POOL_LAYOUTS) // 2
