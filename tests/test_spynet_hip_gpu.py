"""Config.spynet_ops = "hip": SpyNet's 7x7 convolutions and warp on the package's own kernels (ops.conv7x7, ops.spynet_warp).

conv7x7 is checked against float64 on the CPU with the gates of tests/test_gemm_core_gpu.py: the worst-case bound
|C - C64| <= 2 gamma_n (|W| |X|) + tiny, n = K + 2, and the statistical rel_l2 <= 2 u sqrt(n); outputs sit inside NaN
fences (an element the kernel never wrote stays NaN), and every call is repeated for identical bits.  The warp is checked
against ATen's GPU grid_sample (forward) and a float64 CPU grid_sample + clamp autograd (gradients)."""
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

from pcfa_amd import config as pcfa_config
from pcfa_amd import hip_ops
from tests import closure_util
from tests import warp as warp_ref
from tests.util import load_golden, rel_l2, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
TINY = 2.0 ** -126
FENCE = 4096
HIP = dataclasses.replace(pcfa_config.DEFAULT, spynet_ops="hip")
LIB = dataclasses.replace(pcfa_config.DEFAULT, spynet_ops="lib")

torch.set_num_threads(min(16, torch.get_num_threads()))


def gamma(n):
    return n * U / (1 - n * U)


def fenced_empty(shape):
    """A tensor of `shape` inside a buffer of NaN: (view, buffer, offset)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * FENCE,), float("nan"), device=DEV)
    return buf[FENCE:FENCE + n].view(shape), buf


def run_conv7x7(x, w, b, relu, addend, mask):
    """pcfa_conv7x7 into a NaN-fenced output; returns (out, fence intact)."""
    B, cin, H, W = x.shape
    cout = w.shape[0]
    fwd = hip_ops.conv7x7_pack(w)
    out, buf = fenced_empty((B, cout, H, W))
    hip_ops._call("pcfa_conv7x7", hip_ops._ptr(x), hip_ops._ptr(mask), hip_ops._ptr(fwd), hip_ops._ptr(b),
                  hip_ops._ptr(addend), hip_ops._ptr(out), B, cin, cout, H, W, int(relu))
    torch.cuda.synchronize()
    fence_ok = bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + out.numel():]).all())
    return out.clone(), fence_ok


# (Cin, Cout) of Basic's five layers (SpyNet.py:56-84); the data gradient is (Cout, Cin)
LAYERS = [(8, 32), (32, 64), (64, 32), (32, 16), (16, 2)]
SIZES = [(4, 6), (14, 32), (56, 128), (30, 47)]
CASES = ([(l, d, hw, bs) for l in range(5) for d in (False, True) for hw in SIZES for bs in (1, 2)] +
         [(l, d, (448, 1024), 1) for l in (1, 2) for d in (False, True)])


@pytest.mark.parametrize("layer,dgrad,hw,batch", CASES)
def test_conv7x7_against_float64(layer, dgrad, hw, batch):
    """Forward (bias, ReLU on layers 1-4, the `+ up` addend on layer 5) and data gradient (ReLU mask of layers 1-4 applied
    to the loaded gradient, rotated / channel-transposed weight) of every Basic layer."""
    cin, cout = LAYERS[layer]
    H, W = hw
    g = torch.Generator().manual_seed(1000 * layer + 10 * int(dgrad) + batch + H)
    w = torch.randn(cout, cin, 7, 7, generator=g) / math.sqrt(cin * 49)
    relu = layer < 4
    if not dgrad:
        x = torch.randn(batch, cin, H, W, generator=g)
        b = torch.randn(cout, generator=g)
        add = torch.randn(batch, cout, H, W, generator=g) if layer == 4 else None
        mask = None
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=3)
        absref = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=3)
        if relu:
            ref = ref.clamp_min(0)
        if add is not None:
            ref = ref + add.double()
            absref = absref + add.double().abs()
        wk, bk, n_in = w, b, cin
    else:
        gy = torch.randn(batch, cout, H, W, generator=g)
        mask = torch.randn(batch, cout, H, W, generator=g).clamp_min(0) if relu else None   # a ReLU output: ~half zero
        gm = gy if mask is None else torch.where(mask > 0, gy, torch.zeros_like(gy))
        ref = F.conv_transpose2d(gm.double(), w.double(), padding=3)
        absref = F.conv_transpose2d(gm.double().abs(), w.double().abs(), padding=3)
        x, wk, bk, add, n_in = gy, hip_ops.conv7x7_dgrad_weight(w), None, None, cout
    dev = lambda v: None if v is None else v.contiguous().to(DEV)   # noqa: E731
    args = (dev(x), dev(wk), dev(bk), relu and not dgrad, dev(add), dev(mask))
    out, fence_ok = run_conv7x7(*args)
    assert fence_ok, "pcfa_conv7x7 wrote outside its output"
    assert bool(torch.isfinite(out).all()), "unwritten (NaN) output elements"
    n = n_in * 49 + 2
    err = (out.cpu().double() - ref).abs()
    bound = 2 * gamma(n) * absref + n * TINY
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    if float(ref.norm()) > 0:
        assert float((out.cpu().double() - ref).norm() / ref.norm()) <= 2 * U * math.sqrt(n)
    again, _ = run_conv7x7(*args)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "second call differs"


def test_conv7x7_op_refuses_trainable_weights():
    x = torch.randn(1, 8, 14, 32, device=DEV)
    w = torch.randn(32, 8, 7, 7, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="frozen"):
        hip_ops.conv7x7(x, w, None, relu=True)


def test_conv7x7_op_autograd_matches_library():
    """The autograd op (forward + ReLU-masked data gradient; the addend's identity gradient) against F.conv2d on the GPU."""
    g = torch.Generator().manual_seed(7)
    w1 = (torch.randn(32, 8, 7, 7, generator=g) / 20).to(DEV)
    b1 = torch.randn(32, generator=g).to(DEV)
    w2 = (torch.randn(2, 32, 7, 7, generator=g) / 40).to(DEV)
    x = torch.randn(2, 8, 28, 64, generator=g).to(DEV).requires_grad_()
    up = torch.randn(2, 2, 28, 64, generator=g).to(DEV).requires_grad_()
    gy = torch.randn(2, 2, 28, 64, generator=g).to(DEV)
    y = hip_ops.conv7x7(hip_ops.conv7x7(x, w1, b1, relu=True), w2, None, addend=up)
    gx, gu = torch.autograd.grad(y, (x, up), gy)
    x2, up2 = x.detach().double().requires_grad_(), up.detach().double().requires_grad_()
    y2 = F.conv2d(F.relu(F.conv2d(x2, w1.double(), b1.double(), padding=3)), w2.double(), padding=3) + up2
    gx2, gu2 = torch.autograd.grad(y2, (x2, up2), gy.double())
    assert rel_l2(y.double(), y2) < 1e-6 and rel_l2(gx.double(), gx2) < 1e-6
    assert torch.equal(gu, gy)


# --------------------------------------------------------------------------- warp
def _spy_warp_ref(feat, flow):
    """nets/spynet.backward_warp in the caller's dtype / device (the reference's arithmetic)."""
    from pcfa_amd.nets.spynet import backward_warp
    return backward_warp(feat, flow)


@pytest.mark.parametrize("B,C,H,W,amp", [(1, 3, 14, 32, 3.0), (2, 3, 56, 128, 40.0), (1, 3, 30, 47, 10.0),
                                          (1, 3, 448, 1024, 60.0)])
def test_spynet_warp_against_grid_sample(B, C, H, W, amp):
    """Forward within 4 ulp of max|x| of ATen's GPU grid_sample; the forward and both gradients per element against
    float64 computed from the mirrored fp32 sample positions (tests/warp.py: no pixel can fall into another cell, every
    pixel and texel is decided); both gradients against float64 CPU grid_sample + clamp autograd (flows large enough to
    push the grid past +-1: the clamp mask is exercised) -- a coarse statement, float64 positions fall into other cells;
    repeated calls identical."""
    g = torch.Generator().manual_seed(H * W + B)
    x = torch.randn(B, C, H, W, generator=g)
    flo = torch.randn(B, 2, H, W, generator=g) * amp
    gout = torch.randn(B, C, H, W, generator=g)
    xd, fd = x.to(DEV), flo.to(DEV)
    out = hip_ops.spynet_warp(xd, fd)
    ref = _spy_warp_ref(xd, fd)
    ulp = float(torch.finfo(torch.float32).eps) * float(x.abs().max())
    assert float((out - ref).abs().max()) <= 4 * ulp
    hor = torch.linspace(-1.0, 1.0, W).view(1, 1, 1, W)
    grid_x = hor.double() + flo[:, :1].double() / ((W - 1.0) / 2.0)
    assert bool(((grid_x < -1) | (grid_x > 1)).any()), "the clamp is not exercised"
    x64, f64 = x.double().requires_grad_(), flo.double().requires_grad_()
    gx64, gf64 = torch.autograd.grad(_spy_warp_ref(x64, f64), (x64, f64), gout.double())
    xa, fa = xd.clone().requires_grad_(), fd.clone().requires_grad_()
    gx_aten, gf_aten = torch.autograd.grad(_spy_warp_ref(xa, fa), (xa, fa), gout.to(DEV))   # fp32, atomic scatter
    xr, fr = xd.clone().requires_grad_(), fd.clone().requires_grad_()
    res = []
    for _ in range(2):
        gx, gf = torch.autograd.grad(hip_ops.spynet_warp(xr, fr), (xr, fr), gout.to(DEV))
        res.append((gx.clone(), gf.clone()))
    # per element, from the op's own linspace vectors: 2 gamma(7) P; 2 gamma(5) sum |w g| + k unit / 2; 2 gamma(n + 2) P
    hor, ver = torch.linspace(-1.0, 1.0, W, device=DEV).cpu(), torch.linspace(-1.0, 1.0, H, device=DEV).cpu()
    for got, (want, bound) in zip((out, res[0][0], res[0][1]), warp_ref.spynet_reference(x, flo, hor, ver, gout)):
        assert bool(((got.cpu().double() - want).abs() <= bound).all())
    # the fp32 sample position carries ~u max(H, W) pixels of rounding (ATen's GPU kernel too): 3e-5 of d x at W = 1024
    tol = max(1e-5, 2 * U * max(H, W))
    assert rel_l2(res[0][0].cpu().double(), gx64) < tol
    # d flow: where the fp32 and float64 positions fall on different sides of a texel edge, the tap differences switch
    # (0.4 % rel-L2 at W = 1024, amp 60); ATen's kernel below is the sharp gate, float64 the coarse one
    assert rel_l2(res[0][1].cpu().double(), gf64) < (1e-4 if max(H, W) <= 128 else 1e-2)
    assert rel_l2(res[0][0], gx_aten) < 1e-5 and rel_l2(res[0][1], gf_aten) < 1e-5   # same coordinates as ATen's kernel
    assert float(gf64.abs().sum()) > 0 and bool((gf64 == 0).any())   # the clamp mask zeroes some pixels' flow gradient
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    again = hip_ops.spynet_warp(xd, fd)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))


# --------------------------------------------------------------------------- closure
def test_spynet_hip_closure_vs_reference_golden():
    """tests/test_gpu_parity.py::test_closure_on_gpu_vs_reference_golden's SpyNet case with spynet_ops = "hip", at its tolerances."""
    gold = load_golden("closure_spynet")
    net, h, w, box, joint, tgt, loss, seed = ("SpyNet", 100, 150, "change_of_variables", False, "zero", "mse", 4)
    leaves = [t(gold["leaf0"]), t(gold["leaf1"])]
    r = closure_util.run_closure(net, h, w, box, joint, tgt, loss, seed, torch.device(DEV),
                                 images=(t(gold["image1"].astype(np.float32)), t(gold["image2"].astype(np.float32))),
                                 leaves=leaves, config=HIP)
    scale = float(np.abs(gold["flow"]).max())
    assert float((r["flow"].cpu() - t(gold["flow"])).abs().max()) <= 1e-3 * scale
    assert float((r["flow"].cpu() - t(gold["flow"])).pow(2).sum(1).sqrt().mean()) <= 1e-3
    assert abs(r["loss"] - float(gold["loss"])) <= 1e-4 * abs(float(gold["loss"]))
    for i, gr in enumerate(r["grads"]):
        assert rel_l2(gr, t(gold["grad%d" % i])) < 1e-2


def test_spynet_hip_closure_vs_library_build():
    """The same weights and inputs through the "lib" and "hip" builds: loss rel <= 1e-5, gradient rel-L2 <= 1e-4."""
    a = closure_util.run_closure("SpyNet", 128, 192, "change_of_variables", False, "zero", "aee", 21, torch.device(DEV),
                                 config=HIP)
    b = closure_util.run_closure("SpyNet", 128, 192, "change_of_variables", False, "zero", "aee", 21, torch.device(DEV),
                                 config=LIB)
    assert abs(a["loss"] - b["loss"]) <= 1e-5 * abs(b["loss"]), (a["loss"], b["loss"])
    for x, y in zip(a["grads"], b["grads"]):
        assert rel_l2(x, y) <= 1e-4, rel_l2(x, y)


def test_spynet_hip_closure_without_library_kernel():
    """torch.profiler over one closure: the "hip" build launches no Tensile / MIOpen kernel and no atomic grid_sample or
    up-sampling backward; the "lib" build does."""
    import bench
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device(DEV)
    found = []
    for config in (HIP, LIB):
        model = bench.load_model("SpyNet", dev, True, config)
        st = bench.AttackStepper("SpyNet", 128, 192, dev, 3, use_graph=False, model=model)
        st.optimizer.zero_grad()
        st.closure_body()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            st.optimizer.zero_grad()
            st.closure_body()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
        found.append([n for n in names if n.startswith("Cijk_") or "miopen" in n.lower() or "grid_sampler_2d_backward" in n
                      or "upsample_bilinear2d_backward" in n])
    own, lib = found
    assert not own, own[:5]
    assert any("grid_sampler_2d_backward" in n for n in lib) and any("upsample_bilinear2d_backward" in n for n in lib)
    assert any(n.startswith("Cijk_") or "miopen" in n.lower() for n in lib)


# --------------------------------------------------------------------------- pairs in flight
def test_spynet_pairs_in_flight_bit_identical_to_solo():
    import bench
    from pcfa_amd import attack_PCFA
    dev = torch.device(DEV)
    lib = bench.load_model("SpyNet", dev, True, LIB)
    with pytest.raises(ValueError, match="spynet_ops='hip'"):
        attack_PCFA.PairsInFlight(lambda k: bench.AttackStepper("SpyNet", 128, 192, dev, 51 + k, use_graph=True, model=lib),
                                  2, dev)
    del lib
    own = bench.load_model("SpyNet", dev, True, HIP)
    flight = attack_PCFA.PairsInFlight(
        lambda k: bench.AttackStepper("SpyNet", 128, 192, dev, 51 + k, use_graph=True, model=own), 2, dev)
    last = flight.run(2)
    for k in (0, 1):
        own._pcfa_pair_graphs.clear()
        solo = bench.AttackStepper("SpyNet", 128, 192, dev, 51 + k, use_graph=True, model=own)
        solo.step()
        assert tuple(solo.step()) == tuple(last[k]), k
        assert torch.equal(flight.attacks[k].delta1, solo.delta1)
        del solo
    own._pcfa_pair_graphs.clear()


def test_spynet_attack_l2_pairs_in_flight_equals_sequential(tmp_path, monkeypatch):
    """attack_l2 --net SpyNet --pairs_in_flight 2 (three pairs: one full group, one ragged) equals --pairs_in_flight 1."""
    import glob
    from argparse import Namespace
    from pcfa_amd import attack_PCFA
    monkeypatch.setattr(pcfa_config, "DEFAULT", HIP)   # the models attack_l2 builds take the DEFAULT config
    outs = []
    for nflight in (1, 2):
        folder = str(tmp_path / ("flight%d" % nflight))
        a = Namespace(net="SpyNet", weights="random:1234", dataset="Synthetic", dataset_stage="evaluation", small_run=False,
                      synthetic_size="64x96", synthetic_pairs=3, dstype="final", output_folder=folder, small_save=False,
                      save_frequency=1, no_save=False, unregistered_artifacts=True, joint_perturbation=False, steps=2,
                      universal_perturbation=False, boxconstraint="change_of_variables", batch_size=2, delta_bound=0.005,
                      mu=-1, epochs=1, target="zero", custom_target_path="", loss="aee", pairs_in_flight=nflight)
        res = attack_PCFA.attack_l2(a)
        files = sorted(glob.glob(os.path.join(folder, "**", "*.npy"), recursive=True))
        outs.append((res, {os.path.basename(f): np.load(f) for f in files}))
    (r1, f1), (r2, f2) = outs
    assert r1["pairs"] == r2["pairs"] == 3
    for k in r1:
        assert r1[k] == r2[k] or (np.isnan(r1[k]) and np.isnan(r2[k])), (k, r1[k], r2[k])
    assert f1 and sorted(f1) == sorted(f2)
    for name in f1:
        assert np.array_equal(f1[name], f2[name]), name


# --------------------------------------------------------------------------- fresh processes
def test_spynet_hip_fresh_processes_are_bit_identical():
    """Two fresh processes of the captured-graph SpyNet attack at 436x1024 with PCFA_SPYNET_OPS=hip agree bit for bit
    (tools/process_repro.py: every operator output and gradient of a recorded closure, every loss and metric)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PCFA_SPYNET_OPS="hip")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "process_repro.py"), "--net", "SpyNet", "--size",
                        "436x1024", "--box", "change_of_variables", "--steps", "4", "--procs", "2", "--seeds", "0"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode in (0, 1), p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["identical"], rec["first_difference"]
    assert all(pr["graphed"] for run in rec["per_process"] for pr in run)
