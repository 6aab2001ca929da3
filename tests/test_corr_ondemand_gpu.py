"""OnDemandCorrBlock (Config.corr = "on_demand", csrc/corr_ondemand.hip) against float64 on the CPU, against the all-pairs
CorrBlock, and inside the RAFT / GMA closures.

Float64 references.  The small cases use oracle.ops.corr_pyramid + corr_lookup in float64.  The window reference below
(window_lookup64) computes the same lookup without the O(Q^2) volume: the dot products of each query with the pooled fmap2
at the (2r+2)^2 integer positions of its window, blended bilinearly.  It agrees with the oracle to float64 rounding
(test_window_reference_matches_oracle) and carries the 136x240 cases, whose volume would not fit in host memory.

Forward gate (tests/test_gemm_core_gpu.py's style, u = 2^-24):
    |out - out64| <= 2 gamma_n * lookup(|f1|, |f2|) + tiny,   n = D + 3 L + 8
(D fma steps, three additions per 2x2 average per level, the 1/sqrt(D) scale, four blend products and three sums), and
rel_l2(out, out64) <= 2 u sqrt(n).
"""
import dataclasses
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as oracle
from pcfa_amd import _hip, hip_ops
from pcfa_amd import config as pcfa_config
from tests import closure_util
from tests.fenced import NAN_BITS, U, gamma
from tests.util import load_golden, max_abs, rel_l2, t

pytestmark = pytest.mark.gpu

DEV = "cuda"
OD = dataclasses.replace(pcfa_config.DEFAULT, corr="on_demand")
AP = dataclasses.replace(pcfa_config.DEFAULT, corr="all_pairs")
R, L = 4, 4
N1 = 2 * R + 1


def _grid(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([xs, ys], 0).float()[None].repeat(B, 1, 1, 1)


def window_lookup64(f1, f2, coords, levels=L, r=R, chunk=1024):
    """out[B][L (2r+1)^2][H][W] in float64 from the pooled fmap2 pyramid (no all-pairs volume)."""
    f1, f2, coords = f1.double(), f2.double(), coords.double()
    B, D, H, W = f1.shape
    Q, win = H * W, 2 * r + 2
    f1q = f1.reshape(B, D, Q).transpose(1, 2)                       # [B][Q][D]
    out = torch.zeros(B, levels, N1 * N1, Q, dtype=torch.float64)
    lvl = f2
    off = torch.arange(win)
    for lv in range(levels):
        if lv:
            lvl = F.avg_pool2d(lvl, 2, stride=2)
        h, w = lvl.shape[-2:]
        rows = torch.cat([lvl.reshape(B, D, h * w).transpose(1, 2), torch.zeros(B, 1, D, dtype=torch.float64)], 1)
        cx, cy = coords[:, 0].reshape(B, Q) / 2 ** lv, coords[:, 1].reshape(B, Q) / 2 ** lv
        fx, fy = cx - cx.floor(), cy - cy.floor()
        X = cx.floor().long()[..., None, None] - r + off.view(1, 1, 1, win)   # [B][Q][1][win]  (x index i)
        Y = cy.floor().long()[..., None, None] - r + off.view(1, 1, win, 1)   # [B][Q][win][1]  (y index j)
        ok = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        idx = torch.where(ok, Y.clamp(0, h - 1) * w + X.clamp(0, w - 1), torch.full_like(ok, h * w, dtype=torch.long))
        for b in range(B):
            for q0 in range(0, Q, chunk):
                sl = slice(q0, min(Q, q0 + chunk))
                g = rows[b][idx[b, sl].reshape(-1)].reshape(-1, win, win, D)   # [q][j][i][D]
                C = torch.einsum("qjid,qd->qji", g, f1q[b, sl]) / math.sqrt(D)
                ax = fx[b, sl].view(-1, 1, 1)
                ay = fy[b, sl].view(-1, 1, 1)
                # tap (a, bb): x = a, y = bb; blend of (a, bb), (a+1, bb), (a, bb+1), (a+1, bb+1)
                c00, c01 = C[:, :-1, :-1], C[:, :-1, 1:]
                c10, c11 = C[:, 1:, :-1], C[:, 1:, 1:]
                v = ((1 - ax) * (1 - ay) * c00 + ax * (1 - ay) * c01 + (1 - ax) * ay * c10 + ax * ay * c11)  # [q][bb][a]
                out[b, lv, :, sl] = v.permute(2, 1, 0).reshape(N1 * N1, -1)       # channel a (2r+1) + bb
    return out.reshape(B, levels * N1 * N1, H, W)


def coords_case(kind, B, H, W, gen):
    base = _grid(B, H, W)
    if kind == "smooth":
        return base + 1.5 * torch.randn(B, 2, 1, 1, generator=gen) + 0.7 * torch.randn(B, 2, H, W, generator=gen)
    if kind == "integer":
        return base + torch.randint(-6, 7, (B, 2, H, W), generator=gen).float()
    if kind == "uniform":
        lo = torch.tensor([-20., -20.]).view(1, 2, 1, 1)
        span = torch.tensor([W + 40., H + 40.]).view(1, 2, 1, 1)
        return lo + span * torch.rand(B, 2, H, W, generator=gen)
    if kind == "split":   # neighbouring queries alternate between two far-apart targets
        c = base.clone()
        c[:, :, :, 0::2] += torch.tensor([0.3 * W, 0.25 * H]).view(1, 2, 1, 1)
        c[:, :, :, 1::2] -= torch.tensor([0.3 * W, 0.2 * H]).view(1, 2, 1, 1)
        return c + 0.3 * torch.randn(B, 2, H, W, generator=gen)
    raise ValueError(kind)


def run_fwd_abi(f1, f2, coords, levels=L, r=R):
    """prepare + fwd through the C-ABI, the output NaN-fenced on both sides; returns (out, fences intact)."""
    lib = _hip.load()
    B, D, H, W = f1.shape
    ws = torch.empty(int(lib.pcfa_corr_ondemand_workspace_bytes(B, D, H, W, levels)), device=DEV, dtype=torch.uint8)
    n = B * levels * (2 * r + 1) ** 2 * H * W
    fence = 4096
    buf = torch.full((n + 2 * fence,), float("nan"), device=DEV)
    out = buf[fence:fence + n]
    a, b, c = f1.to(DEV).contiguous(), f2.to(DEV).contiguous(), coords.to(DEV).contiguous()
    s = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()  # noqa: E731
    _hip.check(lib.pcfa_corr_ondemand_prepare(P(a), P(b), P(ws), B, D, H, W, levels, s), "prepare")
    _hip.check(lib.pcfa_corr_ondemand_fwd(P(ws), P(c), P(out), B, D, H, W, levels, r, s), "fwd")
    torch.cuda.synchronize()
    bits = buf.view(torch.int32)
    fences_ok = bool((bits[:fence] == NAN_BITS).all()) and bool((bits[fence + n:] == NAN_BITS).all())
    return out.view(B, levels * (2 * r + 1) ** 2, H, W).cpu().clone(), fences_ok


def test_window_reference_matches_oracle():
    gen = torch.Generator().manual_seed(7)
    B, D, H, W = 2, 32, 17, 23
    f1, f2 = torch.randn(B, D, H, W, generator=gen).double(), torch.randn(B, D, H, W, generator=gen).double()
    c = coords_case("uniform", B, H, W, gen).double()
    ref = oracle.corr_lookup(oracle.corr_pyramid(f1, f2, L), c, R)
    got = window_lookup64(f1, f2, c)
    assert float((ref - got).abs().max()) <= 1e-12 * float(ref.abs().max())


SHAPES = [(1, 55, 128), (2, 55, 128), (1, 17, 23), (2, 17, 23), (1, 136, 240), (2, 136, 240)]
KINDS = ["smooth", "integer", "uniform", "split"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-%dx%d" % s)
def test_forward_vs_float64(record_property, shape, kind):
    B, H, W = shape
    D = 256
    gen = torch.Generator().manual_seed(B * 7919 + H * W + KINDS.index(kind))
    f1, f2 = torch.randn(B, D, H, W, generator=gen), torch.randn(B, D, H, W, generator=gen)
    c = coords_case(kind, B, H, W, gen)
    got, fences_ok = run_fwd_abi(f1, f2, c)
    again, _ = run_fwd_abi(f1, f2, c)
    assert fences_ok, "a store left the output"
    assert bool(torch.isfinite(got).all()), "an output element was not written"
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "repeated call differs"
    want = window_lookup64(f1, f2, c)
    absref = window_lookup64(f1.abs(), f2.abs(), c)
    n = D + 3 * L + 8
    elem = float(((got.double() - want).abs() / (2 * gamma(n) * absref + 2.0 ** -126)).max())
    rel = rel_l2(got.double(), want) / (2 * U * math.sqrt(n))
    record_property("elem_ratio", "%.3g" % elem)
    record_property("rel_ratio", "%.3g" % rel)
    assert elem <= 1 and rel <= 1, (elem, rel)


@pytest.mark.parametrize("kind", KINDS)
def test_forward_matches_all_pairs_lookup(kind):
    """Same features and coordinates through CorrBlock (pcfa_corr_lookup_fwd on the pyramid): same channel order,
    agreement to fp32 rounding."""
    B, D, H, W = 2, 256, 55, 128
    gen = torch.Generator().manual_seed(11 + KINDS.index(kind))
    f1, f2 = torch.randn(B, D, H, W, generator=gen).to(DEV), torch.randn(B, D, H, W, generator=gen).to(DEV)
    c = coords_case(kind, B, H, W, gen).to(DEV)
    with torch.no_grad():
        a = hip_ops.CorrBlock(f1, f2, num_levels=L, radius=R)(c).cpu()
        b = hip_ops.OnDemandCorrBlock(f1, f2, num_levels=L, radius=R)(c).cpu()
    absref = window_lookup64(f1.cpu().abs(), f2.cpu().abs(), c.cpu())
    assert a.shape == b.shape
    assert float(((a.double() - b.double()).abs() / (4 * gamma(D + 3 * L + 8) * absref + 2.0 ** -126)).max()) <= 1


@pytest.mark.parametrize("tag", ["a", "b"])
def test_ondemand_block_vs_reference_golden(tag):
    """tests/test_gpu_parity.py::test_corr_block_vs_reference_golden's lookups and gradients, at its tolerances."""
    g = load_golden("corr_block_" + tag)
    f1, f2 = t(g["fmap1"], DEV).requires_grad_(True), t(g["fmap2"], DEV).requires_grad_(True)
    blk = hip_ops.OnDemandCorrBlock(f1, f2, num_levels=4, radius=4)
    outs = [blk(t(g[k], DEV)) for k in ("coords0", "coords1", "coords2")]
    omax = float(np.abs(g["out1"]).max())
    for i, o in enumerate(outs):
        assert o.shape == g["out%d" % i].shape
        assert max_abs(o, t(g["out%d" % i])) <= 3e-5 * omax, i
    go = t(g["grad_out"], DEV)
    ((outs[1] * go).sum() + (outs[2] * go.flip(1)).sum()).backward()
    assert rel_l2(f1.grad, t(g["dfmap1"])) < 2e-5
    assert rel_l2(f2.grad, t(g["dfmap2"])) < 2e-5


def _three_lookup_grads(cls, f1, f2, coords, gos):
    a, b = f1.to(DEV).requires_grad_(True), f2.to(DEV).requires_grad_(True)
    blk = cls(a, b, num_levels=L, radius=R)
    loss = sum((blk(c.to(DEV)) * g.to(DEV)).sum() for c, g in zip(coords, gos))
    loss.backward()
    return a.grad.cpu(), b.grad.cpu()


@pytest.mark.parametrize("shape", [(1, 55, 128), (2, 17, 23)], ids=lambda s: "B%d-%dx%d" % s)
def test_backward_three_lookups_vs_float64(record_property, shape):
    """dfmap1 / dfmap2 of three lookups with different coordinates sharing one build, against float64 autograd of
    oracle.corr_pyramid + corr_lookup; the distance must stay within 2x that of the all-pairs CorrBlock on the same case.
    Repeated runs give identical bits."""
    B, H, W = shape
    D = 256
    gen = torch.Generator().manual_seed(B * 31 + H * W)
    f1, f2 = torch.randn(B, D, H, W, generator=gen), torch.randn(B, D, H, W, generator=gen)
    coords = [coords_case(k, B, H, W, gen) for k in ("smooth", "uniform", "split")]
    gos = [torch.randn(B, L * N1 * N1, H, W, generator=gen) for _ in coords]
    od1, od2 = _three_lookup_grads(hip_ops.OnDemandCorrBlock, f1, f2, coords, gos)
    od1b, od2b = _three_lookup_grads(hip_ops.OnDemandCorrBlock, f1, f2, coords, gos)
    assert torch.equal(od1, od1b) and torch.equal(od2, od2b), "on-demand backward not repeatable bit for bit"
    ap1, ap2 = _three_lookup_grads(hip_ops.CorrBlock, f1, f2, coords, gos)
    f1d, f2d = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    pyr = oracle.corr_pyramid(f1d, f2d, L)
    sum((oracle.corr_lookup(pyr, c.double(), R) * g.double()).sum() for c, g in zip(coords, gos)).backward()
    e = {"od_df1": rel_l2(od1.double(), f1d.grad), "od_df2": rel_l2(od2.double(), f2d.grad),
         "ap_df1": rel_l2(ap1.double(), f1d.grad), "ap_df2": rel_l2(ap2.double(), f2d.grad)}
    for k, v in e.items():
        record_property(k, "%.3g" % v)
    assert e["od_df1"] <= 2 * e["ap_df1"], e
    assert e["od_df2"] <= 2 * e["ap_df2"], e


def test_backward_nan_grad_is_never_finite_garbage():
    B, D, H, W = 1, 256, 17, 23
    gen = torch.Generator().manual_seed(5)
    f1 = torch.randn(B, D, H, W, generator=gen).to(DEV).requires_grad_(True)
    f2 = torch.randn(B, D, H, W, generator=gen).to(DEV).requires_grad_(True)
    blk = hip_ops.OnDemandCorrBlock(f1, f2, num_levels=L, radius=R)
    c = coords_case("smooth", B, H, W, gen).to(DEV)
    out = blk(c)
    go = torch.randn(out.shape, generator=gen).to(DEV)
    go[0, 40, 8, 11] = float("nan")
    (out * go).sum().backward()
    assert not bool(torch.isfinite(f2.grad).any())
    assert not bool(torch.isfinite(f1.grad).all())


def test_refuses_coords_requiring_grad():
    f = torch.randn(1, 256, 16, 16, device=DEV)
    blk = hip_ops.OnDemandCorrBlock(f, f.clone())
    with pytest.raises(RuntimeError, match="requires_grad"):
        blk(_grid(1, 16, 16).to(DEV).requires_grad_(True))
    assert blk.lookup_conv_relu(_grid(1, 16, 16).to(DEV), None, None) is None


# --------------------------------------------------------------------------- closures
@pytest.mark.parametrize("net", ["RAFT", "GMA"])
@pytest.mark.parametrize("h,w", [(128, 160), (436, 1024)])
def test_closure_on_demand_vs_all_pairs(net, h, w):
    """The same weights and inputs under both switches, at test_flownet2_hip_closure_vs_library_build's tolerances."""
    tgt = "neg_flow" if net == "GMA" else "zero"
    a = closure_util.run_closure(net, h, w, "change_of_variables", False, tgt, "aee", 21, torch.device(DEV), config=OD)
    b = closure_util.run_closure(net, h, w, "change_of_variables", False, tgt, "aee", 21, torch.device(DEV), config=AP)
    scale = float(b["flow"].abs().max())
    assert float((a["flow"] - b["flow"]).abs().max()) <= 1e-3 * scale
    assert abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"]), (a["loss"], b["loss"])
    for x, y in zip(a["grads"], b["grads"]):
        assert rel_l2(x, y) < 1e-2, rel_l2(x, y)


def test_closure_raft_on_demand_vs_reference_golden():
    g = load_golden("closure_raft")
    leaves = [t(g["leaf0"]), t(g["leaf1"])]
    r = closure_util.run_closure("RAFT", 128, 160, "change_of_variables", False, "zero", "aee", 1, torch.device(DEV),
                                 images=(t(g["image1"].astype(np.float32)), t(g["image2"].astype(np.float32))),
                                 leaves=leaves, config=OD)
    scale = float(np.abs(g["flow"]).max())
    assert max_abs(r["flow"], t(g["flow"])) <= 1e-3 * scale
    assert float((r["flow"].cpu() - t(g["flow"])).pow(2).sum(1).sqrt().mean()) <= 1e-3
    assert abs(r["loss"] - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    for i, gr in enumerate(r["grads"]):
        assert rel_l2(gr, t(g["grad%d" % i])) < 1e-2


def test_universal_attack_on_demand_vs_golden(monkeypatch):
    from pcfa_amd import attack_PCFA
    monkeypatch.setattr(pcfa_config, "DEFAULT", OD)
    g = load_golden("universal_raft")
    args, loader = closure_util.universal_case(g)
    res = attack_PCFA.attack_l2_universal(args, data_loader=loader, has_gt=False)
    closure_util.check_universal_against_golden(res, g, rel_l2)


def _peak_closure_bytes(config, h, w):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    r = closure_util.run_closure("RAFT", h, w, "change_of_variables", False, "zero", "aee", 3, torch.device(DEV),
                                 config=config)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    return peak, r


def test_memory_at_1088x1920():
    od, _ = _peak_closure_bytes(OD, 1088, 1920)
    ap, _ = _peak_closure_bytes(AP, 1088, 1920)
    print("peak bytes: on_demand %.2f GB, all_pairs %.2f GB" % (od / 1e9, ap / 1e9))
    assert ap - od >= 10e9, (od, ap)


LIBRARY_KERNELS = ("Cijk_", "miopen", "igemm_", "Im2d2Col", "Col2Im", "naive_conv", "batched_transpose")


def test_on_demand_closure_without_library_kernel():
    import bench
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device(DEV)
    config = dataclasses.replace(OD, conv1x1="hip")
    model = bench.load_model("RAFT", dev, True, config)
    st = bench.AttackStepper("RAFT", 128, 160, dev, 3, use_graph=False, model=model)
    st.optimizer.zero_grad()
    st.closure_body()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.optimizer.zero_grad()
        st.closure_body()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    lib = [n for n in names if any(n.startswith(p) or p.lower() in n.lower() for p in LIBRARY_KERNELS)]
    assert not lib, sorted(set(lib))[:8]
    assert any("od_fwd_kernel" in n for n in names) and any("od_bwd_kernel" in n for n in names)
    assert not any("corr_pyramid" in n or "corr_lookup" in n for n in names)


def test_raft_pairs_in_flight_bit_identical_to_solo():
    import bench
    from pcfa_amd import attack_PCFA
    dev = torch.device(DEV)
    own = bench.load_model("RAFT", dev, True, OD)
    flight = attack_PCFA.PairsInFlight(
        lambda k: bench.AttackStepper("RAFT", 128, 160, dev, 51 + k, use_graph=True, model=own), 2, dev)
    last = flight.run(2)
    for k in (0, 1):
        own._pcfa_pair_graphs.clear()
        solo = bench.AttackStepper("RAFT", 128, 160, dev, 51 + k, use_graph=True, model=own)
        solo.step()
        assert tuple(solo.step()) == tuple(last[k]), k
        assert torch.equal(flight.attacks[k].delta1, solo.delta1)
        del solo
    own._pcfa_pair_graphs.clear()


def test_raft_on_demand_fresh_processes_are_bit_identical():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PCFA_CORR="on_demand")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "process_repro.py"), "--net", "RAFT", "--size",
                        "436x1024", "--box", "change_of_variables", "--steps", "4", "--procs", "2", "--seeds", "0"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode in (0, 1), p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["identical"], rec["first_difference"]
    assert all(pr["graphed"] for run in rec["per_process"] for pr in run)


@pytest.mark.skipif(os.environ.get("PCFA_LONG_TESTS") != "1", reason="2160x3840 closure: set PCFA_LONG_TESTS=1")
def test_on_demand_closure_at_2160x3840():
    peak, r = _peak_closure_bytes(OD, 2160, 3840)
    print("2160x3840 on_demand peak %.2f GB" % (peak / 1e9))
    assert bool(torch.isfinite(r["flow"]).all())
    assert all(bool(torch.isfinite(g).all()) for g in r["grads"])
