"""The tiled execution of the on-demand correlation lookup (Config.ondemand_lookup = "tiled", csrc/corr_ondemand_tiled.hpp)
against float64 on the CPU, against the per-query kernels, and inside the RAFT / GMA closures.

Gates are those of tests/test_corr_ondemand_gpu.py: the forward's order-free bound |out - out64| <= 2 gamma_n *
lookup(|f1|, |f2|), rel-L2 <= 2 u sqrt(n), n = D + 3 L + 8; the backward's distance to float64 autograd within 2x that of
the all-pairs CorrBlock on the same case.  Every case also compares pcfa_corr_ondemand_tile_routes with the NumPy
restatement of the classification rule (tests/test_corr_ondemand_tiled_host_cpu.py, which checks that the inputs reach
both routes).
"""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from oracle import ops as oracle
from pcfa_amd import _hip, hip_ops
from pcfa_amd import config as pcfa_config
from tests import closure_util
from tests.fenced import NAN_BITS, U, gamma
from tests.test_corr_ondemand_gpu import AP, DEV, coords_case, window_lookup64
from tests.test_corr_ondemand_tiled_host_cpu import case_inputs, geometry, predict_routes, tiled_coords
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

L = 4
TILED = dataclasses.replace(pcfa_config.DEFAULT, corr="on_demand", ondemand_lookup="tiled")


def run_abi(f1, f2, coords, entry, levels=L, r=4):
    """prepare + one forward entry point through the C-ABI, the output NaN-fenced on both sides (run_fwd_abi's pattern);
    returns (out, fences intact, counts[levels][2] of the lookup's classification)."""
    lib = _hip.load()
    B, D, H, W = f1.shape
    ws = torch.empty(int(lib.pcfa_corr_ondemand_workspace_bytes(B, D, H, W, levels)), device=DEV, dtype=torch.uint8)
    n = B * levels * (2 * r + 1) ** 2 * H * W
    fence = 4096
    buf = torch.full((n + 2 * fence,), float("nan"), device=DEV)
    out = buf[fence:fence + n]
    a, b, c = f1.to(DEV).contiguous(), f2.to(DEV).contiguous(), coords.to(DEV).contiguous()
    counts = torch.full((levels, 2), -1, device=DEV, dtype=torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()  # noqa: E731
    _hip.check(lib.pcfa_corr_ondemand_prepare(P(a), P(b), P(ws), B, D, H, W, levels, s), "prepare")
    _hip.check(getattr(lib, entry)(P(ws), P(c), P(out), B, D, H, W, levels, r, s), entry)
    if entry.endswith("_tiled"):
        _hip.check(lib.pcfa_corr_ondemand_tile_routes(P(ws), B, D, H, W, levels, P(counts), s), "tile_routes")
    torch.cuda.synchronize()
    bits = buf.view(torch.int32)
    fences_ok = bool((bits[:fence] == NAN_BITS).all()) and bool((bits[fence + n:] == NAN_BITS).all())
    return out.view(B, levels * (2 * r + 1) ** 2, H, W).cpu().clone(), fences_ok, counts.cpu().numpy()


@functools.lru_cache(maxsize=None)
def forward_case(B, D, H, W, kind, r=4):
    """inputs and the float64 lookups of (values, absolute values), computed once per case"""
    f1, f2, c = case_inputs(B, D, H, W, kind)
    if r == 4:
        want, absref = window_lookup64(f1, f2, c), window_lookup64(f1.abs(), f2.abs(), c)
    else:   # window_lookup64 is written for r = 4: the oracle's volume at the small shape
        want = oracle.corr_lookup(oracle.corr_pyramid(f1.double(), f2.double(), L), c.double(), r)
        absref = oracle.corr_lookup(oracle.corr_pyramid(f1.abs().double(), f2.abs().double(), L), c.double(), r)
    return f1, f2, c, want, absref


def check_forward(B, D, H, W, kind, r=4):
    f1, f2, c, want, absref = forward_case(B, D, H, W, kind, r)
    got, fences_ok, routes = run_abi(f1, f2, c, "pcfa_corr_ondemand_fwd_tiled", r=r)
    again, _, _ = run_abi(f1, f2, c, "pcfa_corr_ondemand_fwd_tiled", r=r)
    assert fences_ok, "a store left the output"
    assert bool(torch.isfinite(got).all()), "an output element was not written"
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "repeated call differs"
    assert np.array_equal(routes, predict_routes(c, r=r)[0]), (routes, predict_routes(c, r=r)[0])
    n = D + 3 * L + 8
    elem = float(((got.double() - want).abs() / (2 * gamma(n) * absref + 2.0 ** -126)).max())
    rel = rel_l2(got.double(), want) / (2 * U * math.sqrt(n))
    print("elem_ratio %.3g rel_ratio %.3g routes %s" % (elem, rel, routes.tolist()))
    assert elem <= 1 and rel <= 1, (elem, rel)


SHAPES = [(1, 8, 8), (1, 17, 23), (2, 17, 23), (1, 55, 128)]
FWD_KINDS = ["smooth", "integer", "uniform", "split", "mixed", "edge"]


@pytest.mark.parametrize("kind", FWD_KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-%dx%d" % s)
def test_forward_vs_float64(shape, kind):
    check_forward(shape[0], 256, shape[1], shape[2], kind)


@pytest.mark.parametrize("D,r", [(36, 4), (512, 4), (256, 1), (256, 3)])
@pytest.mark.parametrize("kind", ["smooth", "mixed"])
def test_forward_other_depths_and_radii(D, r, kind):
    check_forward(1, D, 17, 23, kind, r)


def test_routes_of_the_suite_inputs():
    """The device classification on the inputs whose predicted routes the host suite asserts: all-matrix, all-per-query,
    and both in one launch."""
    for shape, kind in (((1, 55, 128), "smooth"), ((2, 17, 23), "smooth"), ((1, 55, 128), "uniform"),
                        ((1, 55, 128), "integer"), ((1, 55, 128), "split"), ((1, 55, 128), "mixed")):
        f1, f2, c = case_inputs(shape[0], 256, shape[1], shape[2], kind)
        _, _, routes = run_abi(f1, f2, c, "pcfa_corr_ondemand_fwd_tiled")
        want = predict_routes(c)[0]
        assert np.array_equal(routes, want), (shape, kind, routes, want)
        tw, th, _ = geometry()
        assert int(routes.sum()) == L * shape[0] * -(-shape[1] // th) * -(-shape[2] // tw)


def test_nonfinite_coordinate_tile_is_bit_equal_to_per_query():
    B, D, H, W = 1, 256, 17, 23
    f1, f2, c = case_inputs(B, D, H, W, "smooth")
    c = c.clone()
    c[0, 0, 3, 4] = float("nan")
    c[0, 1, 10, 12] = 3.0e9
    counts, matrix = predict_routes(c)
    tiled, ok_t, routes = run_abi(f1, f2, c, "pcfa_corr_ondemand_fwd_tiled")
    per_query, ok_q, _ = run_abi(f1, f2, c, "pcfa_corr_ondemand_fwd")
    assert ok_t and ok_q
    assert np.array_equal(routes, counts) and (counts[:, 1] == 2).all(), (routes, counts)
    tw, th, _ = geometry()
    ntx = -(-W // tw)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tile = (ys // th) * ntx + xs // tw
    on_per_query = torch.from_numpy(~matrix[0].all(1))[tile]                # [H][W]
    assert int(on_per_query.sum()) == 2 * tw * th
    a, b = tiled.view(torch.int32)[0][:, on_per_query], per_query.view(torch.int32)[0][:, on_per_query]
    assert torch.equal(a, b), "per-query route of the tiled lookup differs from pcfa_corr_ondemand_fwd"
    assert bool(torch.isfinite(tiled[0][:, ~on_per_query]).all())   # the other tiles: matrix route, every element written


# --------------------------------------------------------------------------- backward
def _grads(cls, f1, f2, coords, gos, r=4, **kw):
    a, b = f1.to(DEV).requires_grad_(True), f2.to(DEV).requires_grad_(True)
    blk = cls(a, b, num_levels=L, radius=r, **kw)
    loss = sum((blk(c.to(DEV)) * g.to(DEV)).sum() for c, g in zip(coords, gos))
    loss.backward()
    return a.grad.cpu(), b.grad.cpu()


@functools.lru_cache(maxsize=None)
def backward_case(B, D, H, W, kinds, r=4):
    """inputs, float64 autograd of the oracle and the all-pairs CorrBlock's distance to it, computed once per case"""
    gen = torch.Generator().manual_seed(B * 31 + H * W + D + r)
    f1, f2 = torch.randn(B, D, H, W, generator=gen), torch.randn(B, D, H, W, generator=gen)
    coords = [tiled_coords(k, B, H, W, gen) for k in kinds]
    n1 = 2 * r + 1
    gos = [torch.randn(B, L * n1 * n1, H, W, generator=gen) for _ in coords]
    f1d, f2d = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    pyr = oracle.corr_pyramid(f1d, f2d, L)
    sum((oracle.corr_lookup(pyr, c.double(), r) * g.double()).sum() for c, g in zip(coords, gos)).backward()
    ap1, ap2 = _grads(hip_ops.CorrBlock, f1, f2, coords, gos, r)
    return f1, f2, coords, gos, f1d.grad, f2d.grad, rel_l2(ap1.double(), f1d.grad), rel_l2(ap2.double(), f2d.grad)


def check_backward(B, D, H, W, kinds, r=4):
    f1, f2, coords, gos, g1, g2, ap_df1, ap_df2 = backward_case(B, D, H, W, kinds, r)
    t1, t2 = _grads(hip_ops.OnDemandCorrBlock, f1, f2, coords, gos, r, lookup="tiled")
    t1b, t2b = _grads(hip_ops.OnDemandCorrBlock, f1, f2, coords, gos, r, lookup="tiled")
    assert torch.equal(t1, t1b) and torch.equal(t2, t2b), "tiled backward not repeatable bit for bit"
    e = {"tiled_df1": rel_l2(t1.double(), g1), "tiled_df2": rel_l2(t2.double(), g2), "ap_df1": ap_df1, "ap_df2": ap_df2}
    print({k: "%.3g" % v for k, v in e.items()})
    assert e["tiled_df1"] <= 2 * e["ap_df1"], e
    assert e["tiled_df2"] <= 2 * e["ap_df2"], e


@pytest.mark.parametrize("shape", [(1, 55, 128), (2, 17, 23), (1, 17, 23)], ids=lambda s: "B%d-%dx%d" % s)
def test_backward_three_lookups_vs_float64(shape):
    """Three lookups sharing one build (accumulate = 0, 1, 1) against ONE summed float64 gradient."""
    check_backward(shape[0], 256, shape[1], shape[2], ("smooth", "uniform", "split"))


@pytest.mark.parametrize("kind", ["smooth", "mixed"])
def test_backward_single_kind_vs_float64(kind):
    check_backward(2, 256, 17, 23, (kind,))


@pytest.mark.parametrize("D,r", [(36, 4), (512, 4), (256, 1), (256, 3)])
def test_backward_other_depths_and_radii(D, r):
    check_backward(1, D, 17, 23, ("smooth", "mixed"), r)


def test_backward_nan_grad_is_never_finite_garbage():
    B, D, H, W = 1, 256, 17, 23
    gen = torch.Generator().manual_seed(5)
    f1 = torch.randn(B, D, H, W, generator=gen).to(DEV).requires_grad_(True)
    f2 = torch.randn(B, D, H, W, generator=gen).to(DEV).requires_grad_(True)
    blk = hip_ops.OnDemandCorrBlock(f1, f2, num_levels=L, radius=4, lookup="tiled")
    c = coords_case("smooth", B, H, W, gen).to(DEV)
    out = blk(c)
    go = torch.randn(out.shape, generator=gen).to(DEV)
    go[0, 40, 8, 11] = float("nan")
    (out * go).sum().backward()
    assert not bool(torch.isfinite(f2.grad).any())
    assert not bool(torch.isfinite(f1.grad).all())


def test_lookup_keyword_is_validated():
    f = torch.randn(1, 256, 16, 16, device=DEV)
    with pytest.raises(ValueError, match="lookup"):
        hip_ops.OnDemandCorrBlock(f, f.clone(), lookup="matrix")


# --------------------------------------------------------------------------- closures
@pytest.mark.parametrize("net", ["RAFT", "GMA"])
def test_closure_tiled_vs_all_pairs(net):
    """test_closure_on_demand_vs_all_pairs at 128x160 with the tiled lookups, at its tolerances."""
    tgt = "neg_flow" if net == "GMA" else "zero"
    a = closure_util.run_closure(net, 128, 160, "change_of_variables", False, tgt, "aee", 21, torch.device(DEV),
                                 config=TILED)
    b = closure_util.run_closure(net, 128, 160, "change_of_variables", False, tgt, "aee", 21, torch.device(DEV), config=AP)
    scale = float(b["flow"].abs().max())
    assert float((a["flow"] - b["flow"]).abs().max()) <= 1e-3 * scale
    assert abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"]), (a["loss"], b["loss"])
    for x, y in zip(a["grads"], b["grads"]):
        assert rel_l2(x, y) < 1e-2, rel_l2(x, y)


def test_tiled_closure_runs_the_tile_kernels():
    import bench
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device(DEV)
    model = bench.load_model("RAFT", dev, True, TILED)
    st = bench.AttackStepper("RAFT", 128, 160, dev, 3, use_graph=False, model=model)
    st.optimizer.zero_grad()
    st.closure_body()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.optimizer.zero_grad()
        st.closure_body()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    for k in ("od_classify_kernel", "od_fwd_tile_kernel", "od_bwd_tile_kernel"):
        assert any(k in n for n in names), k


def test_raft_tiled_graph_replays_and_pairs_in_flight_bit_identical_to_solo():
    """test_raft_pairs_in_flight_bit_identical_to_solo's pattern: the closure captured in a hipGraph and replayed twice, solo
    twice over (equal bits) and as two pairs in flight (equal to solo)."""
    import bench
    from pcfa_amd import attack_PCFA
    dev = torch.device(DEV)
    own = bench.load_model("RAFT", dev, True, TILED)
    flight = attack_PCFA.PairsInFlight(
        lambda k: bench.AttackStepper("RAFT", 128, 160, dev, 51 + k, use_graph=True, model=own), 2, dev)
    last = flight.run(2)
    for k in (0, 1):
        runs = []
        for _ in range(2):
            own._pcfa_pair_graphs.clear()
            solo = bench.AttackStepper("RAFT", 128, 160, dev, 51 + k, use_graph=True, model=own)
            solo.step()
            runs.append((tuple(solo.step()), solo.delta1.clone()))
            del solo
        assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]), "two captured runs differ"
        assert runs[0][0] == tuple(last[k]), k
        assert torch.equal(flight.attacks[k].delta1, runs[0][1])
    own._pcfa_pair_graphs.clear()
