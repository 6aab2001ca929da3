"""The float64 Winograd evaluator, its error bound and the dispatch mirror of tests/winograd.py, on the CPU (no GPU).

The signed transforms must reproduce the direct convolution in float64; the fp32 emulation of each algorithm (the
kernels' order of summation) must stay inside the rigorous bound; the Python mirror of the host dispatch rules must agree
with the library's host-only entry points.
"""
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import winograd as wg
from tests.fenced import TINY, gamma

torch.set_num_threads(min(16, torch.get_num_threads()))

RAGGED = [(1, 3, 2, 1, 1), (2, 5, 3, 7, 9), (1, 16, 4, 13, 22), (2, 9, 33, 10, 6), (1, 3, 5, 2, 3)]


@pytest.mark.parametrize("algo", ["f23", "f43"])
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "%dx%dx%dx%dx%d" % s)
def test_winograd_conv3x3_f64_equals_conv2d(algo, shape):
    B, K, N, H, W = shape
    gen = torch.Generator().manual_seed(K * 100 + H * W)
    x = torch.randn(B, K, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(N, K, 3, 3, generator=gen, dtype=torch.float64)
    want = F.conv2d(x, w, padding=1)
    got = wg.winograd_conv3x3(x, w, algo)
    assert got.shape == want.shape
    assert wg.rel_l2_64(got, want) < 1e-12
    # the data gradient form (flipped, channel-transposed weights) against conv_transpose2d
    g = torch.randn(B, N, H, W, generator=gen, dtype=torch.float64)
    got = wg.winograd_conv3x3(g, w.transpose(0, 1).flip(-1, -2), algo)
    assert wg.rel_l2_64(got, F.conv_transpose2d(g, w, padding=1)) < 1e-12


@pytest.mark.parametrize("vertical", [0, 1])
@pytest.mark.parametrize("shape", [(1, 3, 2, 1, 1), (2, 8, 5, 3, 9), (1, 16, 32, 6, 10)], ids=lambda s: "%dx%dx%dx%dx%d" % s)
def test_winograd_f25_f64_equals_conv(shape, vertical):
    B, C, N, H, W = shape
    gen = torch.Generator().manual_seed(C + H * W + vertical)
    x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(N, C, 5, generator=gen, dtype=torch.float64)
    w4 = w.view(N, C, 5, 1) if vertical else w.view(N, C, 1, 5)
    want = F.conv2d(x, w4, padding=(2, 0) if vertical else (0, 2))
    got = wg.winograd_sepconv5(x, w, vertical)
    assert got.shape == want.shape
    assert wg.rel_l2_64(got, want) < 1e-12


EMUL = [("f23", (1, 64, 32, 9, 14), [], 1), ("f23", (1, 64, 32, 9, 14), [("interleave", 2)], 2),
        ("f23", (1, 37, 8, 6, 6), [("slices", 3)], 3), ("f43", (1, 64, 32, 10, 12), [("interleave", 2)], 1),
        ("f43", (1, 256, 16, 9, 8), [("ksplit", 4), ("interleave", 2)], 4)]


@pytest.mark.parametrize("case", EMUL, ids=lambda c: "%s-%s-%d" % (c[0], "x".join(map(str, c[1])), c[3]))
def test_fp32_emulation_inside_bound(case):
    """The fp32 emulation at random data: inside the rigorous bound (tests/winograd.py) by a wide margin, and its rel-L2
    in the range the kernels achieve (F(2x2,3x3) ~3e-7, F(4x4,3x3) ~2e-6)."""
    algo, (B, K, N, H, W), splits, nsplit = case
    gen = torch.Generator().manual_seed(K + N)
    x = torch.randn(B, K, H, W, generator=gen)
    w = torch.randn(N, K, 3, 3, generator=gen) / (9 * K) ** .5
    want = F.conv2d(x.double(), w.double(), padding=1)
    emu = wg.winograd_conv3x3(x, w, algo, dtype=torch.float32, partials=wg.chunk_partials(K, splits))
    P = wg.winograd_conv3x3(x.double(), w.double(), algo, absval=True)
    n = K + nsplit + (12 if algo == "f23" else 16) + 2
    ratio = float(((emu.double() - want).abs() / (2 * gamma(n) * P + n * TINY)).max())
    assert ratio < 0.05, ratio
    rel = wg.rel_l2_64(emu, want)
    assert 1e-8 < rel < (1e-6 if algo == "f23" else 6e-6), rel


def test_chunk_partials():
    assert wg.chunk_partials(20, []) == [list(range(20))]
    assert wg.chunk_partials(20, [("interleave", 2)]) == [list(range(8)) + list(range(16, 20)), list(range(8, 16))]
    assert [len(p) for p in wg.chunk_partials(96, [("slices", 6)])] == [16] * 6
    assert [len(p) for p in wg.chunk_partials(40, [("ksplit", 2), ("interleave", 2)])] == [8, 8, 16, 8]   # chunks [0, 1] [2, 3, 4]


def _lib():
    from pcfa_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip.load()


GRID_B, GRID_K, GRID_N = [1, 2, 3], [1, 3, 8, 21, 64, 96, 176, 192, 384, 565], [1, 32, 64, 128, 196]
GRID_HW = [(1, 1), (3, 2), (6, 20), (12, 40), (24, 80), (48, 64), (50, 64), (55, 128), (64, 256), (96, 320), (30, 68)]


def test_conv3x3_mirror_matches_host():
    """pcfa_conv3x3_algo and pcfa_conv3x3_workspace_bytes (the workspace reveals ksl and ksplit) against the mirror
    over a grid of shapes, under this process's environment."""
    lib = _lib()
    bad = []
    for B, K, N, (H, W) in itertools.product(GRID_B, GRID_K, GRID_N, GRID_HW):
        algo = 43 if wg.use_f43(B, K, N, H, W) else 23
        ws = wg.conv3x3_workspace_bytes(B, K, N, H, W)
        got = (lib.pcfa_conv3x3_algo(B, K, N, H, W), int(lib.pcfa_conv3x3_workspace_bytes(B, K, N, H, W)))
        if got != (algo, ws):
            bad.append(((B, K, N, H, W), got, (algo, ws)))
    assert not bad, bad[:10]


def test_sepconv5_mirror_matches_host():
    lib = _lib()
    prev = lib.pcfa_sepconv5_algo(-1)
    bad = []
    try:
        for enabled in (1, 0):
            lib.pcfa_sepconv5_algo(enabled)
            for B, Ca, Cb, Cout, H, W, v in itertools.product([1, 2], [8, 32, 64, 128], [0, 24, 64, 128],
                                                              [32, 64, 96, 128, 256], [1, 9, 55], [64, 128, 136], [0, 1]):
                want = wg.sepconv5_uses_winograd(B, Ca, Cb, Cout, H, W, v, enabled=bool(enabled))
                if bool(lib.pcfa_sepconv5_uses_winograd(B, Ca, Cb, Cout, H, W, v)) != want:
                    bad.append((enabled, B, Ca, Cb, Cout, H, W, v))
    finally:
        lib.pcfa_sepconv5_algo(prev)
    assert not bad, bad[:10]
