"""Config.flownet2_ops = "hip": FlowNet2 on the package's own kernels (ops.conv_s2_leaky, ops.deconv4s2_leaky,
ops.resample2d_det, ops.upsample_nearest4, ops.conv3x3 at every size).

pcfa_conv_gather is checked against float64 on the CPU with the gates of tests/test_spynet_hip_gpu.py: the worst-case
bound |C - C64| <= 2 gamma_n (|W| |X|) + tiny with n the kernel's own chain length (input channels padded to 4 times the
taps of one window, + 2), and the statistical rel_l2 <= 2 u sqrt(n); operands sit inside NaN fences (tests/fenced.py), and
every call is repeated for identical bits."""
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
from tests.fenced import NAN_BITS, SENTINEL, TINY, U, Fenced, gamma
from tests.util import load_golden, rel_l2, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP = dataclasses.replace(pcfa_config.DEFAULT, flownet2_ops="hip")
LIB = dataclasses.replace(pcfa_config.DEFAULT, flownet2_ops="lib")
SLOPE = 0.1

torch.set_num_threads(min(16, torch.get_num_threads()))

# (Cin, Cout, k, pyramid level of the input) of every stride-2 layer (FlowNetC/S conv1..conv6, FlowNetSD / Fusion conv1..)
S2_LAYERS = [(3, 64, 7, 0), (12, 64, 7, 0), (64, 128, 5, 1), (128, 256, 5, 2), (64, 64, 3, 0), (128, 128, 3, 1),
             (128, 256, 3, 2), (256, 512, 3, 3), (512, 512, 3, 4), (512, 1024, 3, 5)]
# (Cin, Cout, pyramid level of the input) of every deconv (deconv5..2 of FlowNetC/S/SD, deconv1 / deconv0 of Fusion)
DECONV_LAYERS = [(1024, 512, 6), (1026, 256, 5), (770, 128, 4), (386, 64, 3), (128, 32, 2), (162, 16, 1)]
IMAGES = [(448, 1024), (128, 192), "ragged"]


def level_size(img, level):
    if img == "ragged":
        return (13, 27)
    return (img[0] >> level, img[1] >> level)


def cases(layers):
    out = []
    for i in range(len(layers)):
        for dgrad in (False, True):
            for img in IMAGES:
                for batch in ((1,) if img == (448, 1024) else (1, 2)):
                    out.append((i, dgrad, img, batch))
    return out


def fenced_in(x):
    return Fenced(x.shape, x.stride(), NAN_BITS).write(x)


def run_gather(x, mask, packed, bias, cout, OH, OW, stride, taps, npar, offs, act):
    """pcfa_conv_gather with NaN-fenced operands and a sentinel-fenced output: (out, fences intact)."""
    B, cin, H, W = x.shape
    fx = fenced_in(x)
    fm = fenced_in(mask) if mask is not None else None
    out = Fenced((B, cout, OH, OW), (cout * OH * OW, OH * OW, OW, 1), SENTINEL)
    hip_ops._call("pcfa_conv_gather", fx.ptr(), None if fm is None else fm.ptr(), SLOPE, hip_ops._ptr(packed),
                  hip_ops._ptr(bias), out.ptr(), B, cin, H, W, cout, OH, OW, stride, taps, npar, offs[0], offs[1], act,
                  SLOPE)
    torch.cuda.synchronize()
    ok = out.fence_intact() and fx.fence_intact() and (fm is None or fm.fence_intact())
    return out.view().clone(), ok


def leaky_mask(shape, g):
    """A LeakyReLU output: about half of it negative (scaled by the slope)."""
    v = torch.randn(shape, generator=g)
    return torch.where(v > 0, v, v * SLOPE)


def check_against_float64(out, ref, absref, n, args_again):
    assert bool(torch.isfinite(out).all()), "unwritten (NaN) output elements or a read outside an operand"
    err = (out.cpu().double() - ref).abs()
    bound = 2 * gamma(n) * absref + n * TINY
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    if float(ref.norm()) > 0:
        assert float((out.cpu().double() - ref).norm() / ref.norm()) <= 2 * U * math.sqrt(n)
    again, _ = run_gather(*args_again)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "second call differs"


def lrelu64(v):
    return torch.where(v > 0, v, v * SLOPE)


@pytest.mark.parametrize("layer,dgrad,img,batch", cases(S2_LAYERS))
def test_conv_gather_stride2_against_float64(layer, dgrad, img, batch):
    """Stride-2 k x k layers: forward (gather mode, bias + LeakyReLU) and data gradient (parity mode, LeakyReLU backward
    applied to the loaded gradient) against float64."""
    cin, cout, k, level = S2_LAYERS[layer]
    H, W = level_size(img, level)
    pad = k // 2
    OH, OW = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
    g = torch.Generator().manual_seed(1000 * layer + 10 * int(dgrad) + batch + H)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    dev = lambda v: None if v is None else v.contiguous().to(DEV)   # noqa: E731
    if not dgrad:
        x = torch.randn(batch, cin, H, W, generator=g)
        b = torch.randn(cout, generator=g)
        ref = lrelu64(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=pad))
        absref = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=pad)
        packed = hip_ops.gather_pack(w).to(DEV)
        args = (dev(x), None, packed, dev(b), cout, OH, OW, 2, k, 1, (-pad, 0), 2)
        n = -(-cin // 4) * 4 * k * k + 2
    else:
        gy = torch.randn(batch, cout, OH, OW, generator=g)
        mask = leaky_mask((batch, cout, OH, OW), g)
        gm = torch.where(mask > 0, gy, gy * SLOPE).double()
        op = (H - (2 * OH - 2 * pad + k - 2), W - (2 * OW - 2 * pad + k - 2))   # conv_transpose2d back to H x W
        ref = F.conv_transpose2d(gm, w.double(), stride=2, padding=pad, output_padding=op)
        absref = F.conv_transpose2d(gm.abs(), w.double().abs(), stride=2, padding=pad, output_padding=op)
        t_ = (k + 1) // 2
        packed = hip_ops.gather_pack(hip_ops.parity_weights(w, pad)).to(DEV)
        args = (dev(gy), dev(mask), packed, None, cin, H, W, 1, t_, 4, hip_ops.parity_offsets(k, pad), 0)
        n = -(-cout // 4) * 4 * t_ * t_ + 2
    assert tuple(ref.shape[2:]) == tuple(args[5:7])
    out, ok = run_gather(*args)
    assert ok, "pcfa_conv_gather wrote outside its output"
    check_against_float64(out, ref, absref, n, args)


@pytest.mark.parametrize("layer,dgrad,img,batch", cases(DECONV_LAYERS))
def test_conv_gather_deconv_against_float64(layer, dgrad, img, batch):
    """ConvTranspose2d(Cin, Cout, 4, 2, 1): forward (parity mode, bias + LeakyReLU) and data gradient (gather mode, stride
    2, the weight as it is, LeakyReLU backward applied to the loaded gradient) against float64."""
    cin, cout, level = DECONV_LAYERS[layer]
    H, W = level_size(img, level)
    g = torch.Generator().manual_seed(2000 * layer + 10 * int(dgrad) + batch + H)
    w = torch.randn(cin, cout, 4, 4, generator=g) / math.sqrt(cin * 4)
    dev = lambda v: None if v is None else v.contiguous().to(DEV)   # noqa: E731
    if not dgrad:
        x = torch.randn(batch, cin, H, W, generator=g)
        b = torch.randn(cout, generator=g)
        ref = lrelu64(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1))
        absref = F.conv_transpose2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=1)
        packed = hip_ops.gather_pack(hip_ops.parity_weights(w, 1)).to(DEV)
        args = (dev(x), None, packed, dev(b), cout, 2 * H, 2 * W, 1, 2, 4, hip_ops.parity_offsets(4, 1), 2)
        n = -(-cin // 4) * 4 * 4 + 2
    else:
        gy = torch.randn(batch, cout, 2 * H, 2 * W, generator=g)
        mask = leaky_mask((batch, cout, 2 * H, 2 * W), g)
        gm = torch.where(mask > 0, gy, gy * SLOPE).double()
        ref = F.conv2d(gm, w.double(), stride=2, padding=1)
        absref = F.conv2d(gm.abs(), w.double().abs(), stride=2, padding=1)
        packed = hip_ops.gather_pack(w).to(DEV)
        args = (dev(gy), dev(mask), packed, None, cin, H, W, 2, 4, 1, (-1, 0), 0)
        n = -(-cout // 4) * 4 * 16 + 2
    out, ok = run_gather(*args)
    assert ok, "pcfa_conv_gather wrote outside its output"
    check_against_float64(out, ref, absref, n, args)


@pytest.mark.parametrize("H,W", [(2, 3), (1, 2), (4, 6)])
@pytest.mark.parametrize("cin,cout", [(1024, 1024), (512, 512), (1026, 512)])
def test_conv3x3_small_maps_against_float64(H, W, cin, cout):
    """ops.conv3x3 (bias + LeakyReLU, both directions) on the smallest maps the "hip" build gives it (conv6_1 at 128x192
    is 2x3; 1x2 below that) -- the r01 pixel gate is a speed heuristic, not a correctness limit."""
    g = torch.Generator().manual_seed(H * 100 + W + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g)
    x = torch.randn(2, cin, H, W, generator=g)
    gy = torch.randn(2, cout, H, W, generator=g)
    xd = x.to(DEV).requires_grad_()
    y = hip_ops.conv3x3(xd, w.to(DEV), b.to(DEV), False, SLOPE)
    (gx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    x64 = x.double().requires_grad_()
    y64 = F.leaky_relu(F.conv2d(x64, w.double(), b.double(), padding=1), SLOPE)
    (gx64,) = torch.autograd.grad(y64, x64, gy.double())
    assert rel_l2(y.cpu().double(), y64) < 1e-5 and rel_l2(gx.cpu().double(), gx64) < 1e-5


@pytest.mark.parametrize("k,H,W", [(7, 448, 1024), (5, 224, 512), (3, 4, 6), (3, 56, 128), (7, 13, 27)])
def test_conv_s2_leaky_op_autograd(k, H, W):
    """The op's dispatch (pcfa_conv_s2 where it applies, pcfa_conv_gather elsewhere) forward and data gradient against
    float64 autograd."""
    cin = {7: 12, 5: 64, 3: 64}[k]
    cout = {7: 64, 5: 128, 3: 128}[k]
    g = torch.Generator().manual_seed(k * H + W)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g)
    x = torch.randn(1, cin, H, W, generator=g)
    xd = x.to(DEV).requires_grad_()
    y = hip_ops.conv_s2_leaky(xd, w.to(DEV), b.to(DEV), SLOPE)
    gy = torch.randn(y.shape, generator=g)
    (gx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    y64 = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=k // 2), SLOPE)
    # the LeakyReLU factor from the fp32 output, as the op applies it (where the pre-activation is within rounding of 0,
    # float64 may pick the other factor)
    gm = torch.where(y.detach().cpu() > 0, gy, gy * SLOPE).double()
    x64 = x.double().requires_grad_()
    (gx64,) = torch.autograd.grad(F.conv2d(x64, w.double(), stride=2, padding=k // 2), x64, gm)
    assert rel_l2(y.cpu().double(), y64) < 1e-5 and rel_l2(gx.cpu().double(), gx64) < 1e-5


# --------------------------------------------------------------------------- Resample2d, nearest x4
@pytest.mark.parametrize("B,H,W,amp", [(1, 128, 192, 3.0), (2, 436, 1024, 20.0), (1, 13, 27, 40.0)])
def test_resample2d_det_against_float64(B, H, W, amp):
    """grad_in1 and grad_flow per element against the float64 restatement of tests/warp.py (grad_in1: the rounding of an
    addend's products and of the finish, plus half a fixed-point unit per addend that lands on the texel; grad_flow: the
    eight-term chains), grad_flow and the forward equal to the atomic library path's (same arithmetic), identical bits on
    repeated calls and across graph replays."""
    C = 3
    g = torch.Generator().manual_seed(H + W + B)
    x = torch.randn(B, C, H, W, generator=g)
    flow = torch.randn(B, 2, H, W, generator=g) * amp
    gout = torch.randn(B, C, H, W, generator=g)
    xd, fd, gd = x.to(DEV), flow.to(DEV), gout.to(DEV)
    res = []
    for _ in range(2):
        xr, fr = xd.clone().requires_grad_(), fd.clone().requires_grad_()
        out = hip_ops.resample2d_det(xr, fr)
        g1, g2 = torch.autograd.grad(out, (xr, fr), gd)
        res.append((out, g1, g2))
    xa, fa = xd.clone().requires_grad_(), fd.clone().requires_grad_()
    out_a = hip_ops.resample2d(xa, fa)
    g1a, g2a = torch.autograd.grad(out_a, (xa, fa), gd)
    assert torch.equal(res[0][0], out_a) and torch.equal(res[0][2], g2a)
    assert rel_l2(res[0][1], g1a) < 1e-6
    # per texel: 2 gamma(5) sum |w g| + k unit / 2, k the texel's own addend count; grad_flow: 2 gamma(4 C + 4) P + u A
    (ref1, bound1), (ref2, bound2) = warp_ref.resample2d_reference(x, flow, gout)
    assert bool(((res[0][1].cpu().double() - ref1).abs() <= bound1).all())
    assert bool(((res[0][2].cpu().double() - ref2).abs() <= bound2).all())
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # graph replays: the same bits as the eager call
    xs, fs, gs = xd.clone(), fd.clone(), gd.clone()
    outs = [torch.empty_like(xd), torch.empty_like(fd)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        xr, fr = xs.clone().requires_grad_(), fs.clone().requires_grad_()
        torch.autograd.grad(hip_ops.resample2d_det(xr, fr), (xr, fr), gs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xr, fr = xs.requires_grad_(), fs.requires_grad_()
        a, b = torch.autograd.grad(hip_ops.resample2d_det(xr, fr), (xr, fr), gs)
        outs[0].copy_(a)
        outs[1].copy_(b)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int32), res[0][1].view(torch.int32))
        assert torch.equal(outs[1].view(torch.int32), res[0][2].view(torch.int32))


@pytest.mark.parametrize("div", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 112, 256), (2, 32, 48), (1, 3, 5)])
def test_upsample_nearest4_exact(B, H, W, div):
    """Forward equal to nn.Upsample(scale_factor=4, mode='nearest')(x op 20); backward equal to the float64 sum of the 16
    gradients, rounded to fp32, op 20."""
    g = torch.Generator().manual_seed(H * W + int(div))
    x = torch.randn(B, 2, H, W, generator=g) * 7
    gy = torch.randn(B, 2, 4 * H, 4 * W, generator=g)
    xd = x.to(DEV).requires_grad_()
    y = hip_ops.upsample_nearest4(xd, 20.0, div=div)
    (gx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    up = torch.nn.Upsample(scale_factor=4, mode="nearest")
    assert torch.equal(y.cpu(), up(x / 20.0 if div else x * 20.0))
    s64 = gy.double().view(B, 2, H, 4, W, 4).sum((3, 5)).float()
    assert torch.equal(gx.cpu(), s64 / 20.0 if div else s64 * 20.0)
    (gx2,) = torch.autograd.grad(hip_ops.upsample_nearest4(xd, 20.0, div=div), xd, gy.to(DEV))
    assert torch.equal(gx.view(torch.int32), gx2.view(torch.int32))


# --------------------------------------------------------------------------- closure
def test_flownet2_hip_closure_vs_reference_golden():
    """tests/test_gpu_parity.py::test_closure_on_gpu_vs_reference_golden's FlowNet2 case with flownet2_ops = "hip", at its
    tolerances."""
    gold = load_golden("closure_flownet2")
    net, h, w, box, joint, tgt, loss, seed = ("FlowNet2", 128, 192, "change_of_variables", False, "zero", "aee", 5)
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


@pytest.mark.parametrize("h,w", [(128, 192), (436, 1024)])
def test_flownet2_hip_closure_vs_library_build(h, w):
    """The same weights and inputs through the "lib" and "hip" builds, at the golden test's tolerances."""
    a = closure_util.run_closure("FlowNet2", h, w, "change_of_variables", False, "zero", "aee", 21, torch.device(DEV),
                                 config=HIP)
    b = closure_util.run_closure("FlowNet2", h, w, "change_of_variables", False, "zero", "aee", 21, torch.device(DEV),
                                 config=LIB)
    scale = float(b["flow"].abs().max())
    assert float((a["flow"] - b["flow"]).abs().max()) <= 1e-3 * scale
    assert abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"]), (a["loss"], b["loss"])
    for x, y in zip(a["grads"], b["grads"]):
        assert rel_l2(x, y) < 1e-2, rel_l2(x, y)


LIBRARY_KERNELS = ("Cijk_", "miopen", "igemm_", "Im2d2Col", "Col2Im", "naive_conv", "batched_transpose")


def _library_kernel(n):
    return (any(n.startswith(p) or p.lower() in n.lower() for p in LIBRARY_KERNELS)
            or ("upsample_" in n and "backward" in n) or "resample2d_bwd_kernel" in n)


def test_flownet2_hip_closure_without_library_kernel():
    """torch.profiler over one closure: the "hip" build launches no Tensile / MIOpen kernel, no ATen up-sampling backward
    and not the atomic Resample2d backward; the "lib" build does."""
    import bench
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device(DEV)
    found = []
    for config in (HIP, LIB):
        model = bench.load_model("FlowNet2", dev, True, config)
        st = bench.AttackStepper("FlowNet2", 128, 192, dev, 3, use_graph=False, model=model)
        st.optimizer.zero_grad()
        st.closure_body()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            st.optimizer.zero_grad()
            st.closure_body()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
        found.append([n for n in names if _library_kernel(n)])
        del st, model
    own, lib = found
    assert not own, sorted(set(own))[:8]
    assert any("resample2d_bwd_kernel" in n for n in lib)
    assert any(n.startswith("Cijk_") or "miopen" in n.lower() or "igemm" in n or "naive_conv" in n for n in lib)


def test_flownet2_hip_rejects_trainable_weights():
    from pcfa_amd.nets.flownet2 import FlowNetS
    net = pcfa_config.attach(FlowNetS().to(DEV), HIP)
    with pytest.raises(ValueError, match="frozen"):
        net(torch.randn(1, 12, 64, 128, device=DEV))


# --------------------------------------------------------------------------- pairs in flight
def test_flownet2_pairs_in_flight_bit_identical_to_solo():
    import bench
    from pcfa_amd import attack_PCFA
    dev = torch.device(DEV)
    lib = bench.load_model("FlowNet2", dev, True, LIB)
    with pytest.raises(ValueError, match="flownet2_ops='hip'"):
        attack_PCFA.PairsInFlight(
            lambda k: bench.AttackStepper("FlowNet2", 128, 192, dev, 51 + k, use_graph=True, model=lib), 2, dev)
    del lib
    own = bench.load_model("FlowNet2", dev, True, HIP)
    flight = attack_PCFA.PairsInFlight(
        lambda k: bench.AttackStepper("FlowNet2", 128, 192, dev, 51 + k, use_graph=True, model=own), 2, dev)
    last = flight.run(2)
    for k in (0, 1):
        own._pcfa_pair_graphs.clear()
        solo = bench.AttackStepper("FlowNet2", 128, 192, dev, 51 + k, use_graph=True, model=own)
        solo.step()
        assert tuple(solo.step()) == tuple(last[k]), k
        assert torch.equal(flight.attacks[k].delta1, solo.delta1)
        del solo
    own._pcfa_pair_graphs.clear()


def test_flownet2_attack_l2_pairs_in_flight_equals_sequential(tmp_path, monkeypatch):
    """attack_l2 --net FlowNet2 --pairs_in_flight 2 (three 64x128 pairs: one full group, one ragged) equals
    --pairs_in_flight 1."""
    import glob
    from argparse import Namespace
    from pcfa_amd import attack_PCFA
    monkeypatch.setattr(pcfa_config, "DEFAULT", HIP)   # the models attack_l2 builds take the DEFAULT config
    outs = []
    for nflight in (1, 2):
        folder = str(tmp_path / ("flight%d" % nflight))
        a = Namespace(net="FlowNet2", weights="random:1234", dataset="Synthetic", dataset_stage="evaluation",
                      small_run=False, synthetic_size="64x128", synthetic_pairs=3, dstype="final", output_folder=folder,
                      small_save=False, save_frequency=1, no_save=False, unregistered_artifacts=True,
                      joint_perturbation=False, steps=2, universal_perturbation=False, boxconstraint="change_of_variables",
                      batch_size=2, delta_bound=0.005, mu=-1, epochs=1, target="zero", custom_target_path="", loss="aee",
                      pairs_in_flight=nflight)
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
def test_flownet2_hip_fresh_processes_are_bit_identical():
    """Two fresh processes of the captured-graph FlowNet2 attack at 436x1024 with PCFA_FLOWNET2_OPS=hip agree bit for bit
    (tools/process_repro.py: every operator output and gradient of a recorded closure, every loss and metric)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PCFA_FLOWNET2_OPS="hip")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "process_repro.py"), "--net", "FlowNet2", "--size",
                        "436x1024", "--box", "change_of_variables", "--steps", "4", "--procs", "2", "--seeds", "0"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode in (0, 1), p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["identical"], rec["first_difference"]
    assert all(pr["graphed"] for run in rec["per_process"] for pr in run)
