"""Config.ondemand_lookup, the tile geometry of the tiled on-demand lookup and the classification rule, without a GPU.

predict_routes restates the rule of include/pcfa_hip.h (pcfa_corr_ondemand_fwd_tiled) in NumPy with the exported
geometry; tests/test_corr_ondemand_tiled_gpu.py compares pcfa_corr_ondemand_tile_routes against it.  The inputs of that
suite are checked here to reach the routes they are meant to reach, so that no GPU test exercises one route only.
"""
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pcfa_amd import _hip
from pcfa_amd import config as pcfa_config
from tests.test_corr_ondemand_gpu import KINDS, coords_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 4


@functools.lru_cache(maxsize=None)
def geometry():
    import ctypes
    lib = _hip.load()
    tw, th, mp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _hip.check(lib.pcfa_corr_ondemand_tile_geometry(ctypes.byref(tw), ctypes.byref(th), ctypes.byref(mp)), "geometry")
    return tw.value, th.value, mp.value


def tile_boxes(coords, levels=L, r=4):
    """[B][tiles][levels] of (bw * bh, ok) from coords [B][2][H][W] (float32 tensor), tiles in raster order."""
    tw, th, _ = geometry()
    c = coords.numpy().astype(np.float32)
    B, _, H, W = c.shape
    win = 2 * r + 2
    out = []
    for b in range(B):
        per_image = []
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                per_level = []
                for lv in range(levels):
                    inv = np.float32(1.0 / (1 << lv))
                    fl = np.floor(c[b, :, y0:y0 + th, x0:x0 + tw] * inv)            # float32, as make_origin
                    with np.errstate(invalid="ignore"):
                        ok = bool((np.abs(fl) < np.float32(1.0e8)).all())            # NaN fails
                    o = np.clip(np.nan_to_num(fl, nan=-1.0e8), -1.0e8, 1.0e8).astype(np.int64) - r
                    bw = int(o[0].max() - o[0].min()) + win
                    bh = int(o[1].max() - o[1].min()) + win
                    per_level.append((bw * bh, ok))
                per_image.append(per_level)
        out.append(per_image)
    return out


def predict_routes(coords, levels=L, r=4):
    """(counts[levels][2] = pairs on the (matrix, per-query) route, matrix[B][tiles][levels] bool)."""
    mp = geometry()[2]
    boxes = tile_boxes(coords, levels, r)
    matrix = np.array([[[ok and p <= mp for (p, ok) in t] for t in img] for img in boxes], dtype=bool)
    counts = np.stack([matrix.sum((0, 1)), (~matrix).sum((0, 1))], 1)
    return counts, matrix


def _grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([xs, ys], 0).float()[None].repeat(B, 1, 1, 1)


def tiled_coords(kind, B, H, W, gen):
    """coords_case plus the two kinds of the tiled suite.
    mixed: left part smooth, right part uniform, the seam inside a tile column: one launch holds both routes and tiles
    that straddle them.  edge: a smooth zoom about the map centre, so that the windows hang off all four map sides (some
    lie outside altogether) while neighbouring queries stay 1.2 texels apart."""
    if kind == "mixed":
        a, b = coords_case("smooth", B, H, W, gen), coords_case("uniform", B, H, W, gen)
        left = (torch.arange(W) < W // 2 + 3).view(1, 1, 1, W)
        return torch.where(left, a, b)
    if kind == "edge":
        centre = torch.tensor([(W - 1) / 2., (H - 1) / 2.]).view(1, 2, 1, 1)
        return centre + 1.2 * (_grid(B, H, W) - centre) + 0.2 * torch.randn(B, 2, H, W, generator=gen)
    return coords_case(kind, B, H, W, gen)


def case_inputs(B, D, H, W, kind):
    """(f1, f2, coords) of the tiled suite: test_forward_vs_float64's seeding."""
    kinds = KINDS + ["mixed", "edge"]
    gen = torch.Generator().manual_seed(B * 7919 + H * W + kinds.index(kind))
    f1, f2 = torch.randn(B, D, H, W, generator=gen), torch.randn(B, D, H, W, generator=gen)
    return f1, f2, tiled_coords(kind, B, H, W, gen)


def test_config_ondemand_lookup_values():
    assert pcfa_config.Config().ondemand_lookup == "per_query"
    assert pcfa_config.Config(ondemand_lookup="tiled").ondemand_lookup == "tiled"
    assert dataclasses.replace(pcfa_config.Config(), corr="on_demand", ondemand_lookup="tiled").ondemand_lookup == "tiled"
    with pytest.raises(ValueError, match="Config.ondemand_lookup"):
        pcfa_config.Config(ondemand_lookup="matrix")


def test_env_sets_default_in_fresh_interpreter():
    env = dict(os.environ, PCFA_ONDEMAND_LOOKUP="tiled")
    p = subprocess.run([sys.executable, "-c", "from pcfa_amd import config; print(config.DEFAULT.ondemand_lookup)"],
                       capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == "tiled"


def test_tile_geometry_within_stated_range():
    tw, th, mp = geometry()
    assert (tw, th) in ((8, 8), (8, 4))
    lo, hi = ((420, 576) if tw * th == 64 else (384, 512))
    assert lo <= mp <= hi, mp
    lib = _hip.load()
    assert lib.pcfa_corr_ondemand_tile_geometry(None, None, None) != 0


def test_tiled_entry_points_share_the_per_query_signatures():
    for name in ("fwd", "bwd"):
        assert _hip.SIGNATURES["pcfa_corr_ondemand_%s_tiled" % name] == _hip.SIGNATURES["pcfa_corr_ondemand_" + name]


def test_workspace_still_linear_with_the_tile_table():
    lib = _hip.load()
    b1 = lib.pcfa_corr_ondemand_workspace_bytes(1, 256, 55, 128, 4)
    # features, pyramid, int64 accumulator and both gradient sums dominate; the table is 16 B per (tile, level)
    rows = sum((55 >> l) * (128 >> l) for l in range(4))
    assert b1 - (2 * 55 * 128 + 4 * rows) * 256 * 4 < 64 * 1024


@pytest.mark.parametrize("shape", [(1, 55, 128), (2, 17, 23)], ids=lambda s: "B%d-%dx%d" % s)
def test_smooth_and_edge_inputs_are_all_matrix(shape):
    B, H, W = shape
    mp = geometry()[2]
    for kind in ("smooth", "edge"):
        c = case_inputs(B, 256, H, W, kind)[2]
        counts, _ = predict_routes(c)
        assert (counts[:, 1] == 0).all(), (kind, counts)
        largest = max(p for img in tile_boxes(c) for t in img for (p, _) in t)
        assert largest <= min(mp, 420 if kind == "smooth" else mp), (kind, largest)
    c = case_inputs(B, 256, H, W, "edge")[2]
    x0, y0 = c[:, 0].floor() - 4, c[:, 1].floor() - 4
    assert x0.min() < 0 and y0.min() < 0 and x0.max() + 10 > W and y0.max() + 10 > H   # windows off all four sides


def test_uniform_integer_mixed_inputs_reach_the_per_query_route():
    B, H, W = 1, 55, 128
    counts, _ = predict_routes(case_inputs(B, 256, H, W, "uniform")[2])
    assert (counts[:, 0] == 0).all(), counts
    counts, _ = predict_routes(case_inputs(B, 256, H, W, "integer")[2])
    assert 3 * counts[0, 1] >= 2 * counts[0].sum(), counts
    assert (counts[1:, 1] == 0).all(), counts
    counts, matrix = predict_routes(case_inputs(B, 256, H, W, "mixed")[2])
    assert (counts > 0).all(), counts      # both routes at every level of one launch
    tw = geometry()[0]
    seam = (W // 2 + 3) // tw               # the tile column that holds smooth and uniform queries
    ntx = -(-W // tw)
    assert matrix[0].reshape(-1, ntx, L)[:, :seam].all() and not matrix[0].reshape(-1, ntx, L)[:, seam].any()


def test_nonfinite_or_guarded_coordinate_sends_the_tile_per_query():
    c = case_inputs(1, 256, 17, 23, "smooth")[2].clone()
    c[0, 0, 3, 4] = float("nan")
    c[0, 1, 10, 12] = 3.0e9
    _, matrix = predict_routes(c)
    ntx = -(-23 // geometry()[0])
    th = geometry()[1]
    bad = {(3 // th) * ntx + 0, (10 // th) * ntx + 1}
    for t in range(matrix.shape[1]):
        assert (not matrix[0, t].any()) if t in bad else matrix[0, t].all(), t
