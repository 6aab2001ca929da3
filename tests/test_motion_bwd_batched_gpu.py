"""Config.motion_bwd = "batched" (ops.motion_steps: the motion encoder's two 3x3 data gradients once per backward pass, over
all refinement iterations) against "per_iteration" on a RAFT closure at 64x96 (features 8x12): the loss, both perturbation
gradients and the flow must be bit-identical, eagerly and through a captured graph replayed twice; a two-image input takes
the per-iteration path under either setting.

At 8x12 features the per-iteration launches run with K sliced over workgroups (pcfa_conv3x3_run's rule for small single
images), which one launch over all iterations cannot reproduce bit for bit: there the deferred backward keeps the per-image
launches (no pcfa_conv3x3_run_strided call).  The case at 448x640 (features 56x80: the direct kernel at batch 1, as at the
benchmark's 55x128) is the smallest at which the two batched launches themselves run inside a closure."""
import dataclasses
import functools

import pytest
import torch

from pcfa_amd import attack_PCFA, config
from pcfa_amd.helper_functions import losses, ownutilities
from pcfa_amd.ops import core
from tests import closure_util

pytestmark = pytest.mark.gpu
SMALL, DIRECT, EPS = (64, 96), (448, 640), 1e-7
CFG = {m: dataclasses.replace(config.DEFAULT, motion_bwd=m) for m in ("batched", "per_iteration")}


def _inputs(batch, size=SMALL):
    im = [closure_util.test_images(3 + b, *size) for b in range(batch)]
    a = torch.cat([p[0] for p in im]).float().cuda() / 255.
    b = torch.cat([p[1] for p in im]).float().cuda() / 255.
    g = torch.Generator().manual_seed(11)
    n1 = torch.atanh(2. * (1. - EPS) * a - (1 - EPS)).cpu() + 0.02 * torch.randn(a.shape, generator=g)
    n2 = torch.atanh(2. * (1. - EPS) * b - (1 - EPS)).cpu() + 0.02 * torch.randn(a.shape, generator=g)
    return a, b, n1.cuda(), n2.cuda()


def _closure(model, a, b, n1, n2, iters):
    """(loss, flow) of one PCFA closure (change of variables, zero target, AEE) with `iters` refinement iterations"""
    flow = ownutilities.compute_flow(model, "scaled_input_model", n1, n2, test_mode=True, iters=iters)
    d1, d2 = attack_PCFA.extract_deltas(n1, n2, a, b, "change_of_variables", eps_box=EPS)
    loss = losses.loss_delta_constraint(flow, torch.zeros_like(flow), d1, d2, n1.device, delta_bound=0.005,
                                        mu=2500. / 0.005, f_type="aee")
    return loss, flow


def _counted(fn):
    """fn() with the pcfa_conv3x3_run_strided calls counted"""
    seen = []

    def spy(name, args, invoke):
        if name == "pcfa_conv3x3_run_strided":
            seen.append(args[10])   # B
        return invoke(name, *args)
    core.set_call_spy(spy)
    try:
        return fn(), seen
    finally:
        core.set_call_spy(None)


def _eager(mode, iters, batch, size=SMALL):
    model = closure_util.load_model("RAFT", True, torch.device("cuda", 0), EPS, CFG[mode])
    a, b, n1, n2 = _inputs(batch, size)
    n1.requires_grad_(True)
    n2.requires_grad_(True)

    def run():
        loss, flow = _closure(model, a, b, n1, n2, iters)
        g1, g2 = torch.autograd.grad(loss, (n1, n2))
        return loss.detach().clone(), flow.detach().clone(), g1.clone(), g2.clone()
    out, seen = _counted(run)
    torch.cuda.synchronize()
    return out, seen


@functools.lru_cache(maxsize=None)
def _reference(iters, batch, size=SMALL):
    """the per-iteration graph, eagerly: computed once per (iters, batch, size) and left unchanged"""
    out, seen = _eager("per_iteration", iters, batch, size)
    assert seen == [], "per_iteration launched the strided entry"
    return out


def _same(got, want):
    for name, g, w in zip(("loss", "flow", "grad1", "grad2"), got, want):
        assert bool(torch.isfinite(g).all()), name
        assert torch.equal(g, w), "%s differs (max |d| %.3g)" % (name, float((g - w).abs().max()))
    assert float(want[2].abs().max()) > 0 and float(want[3].abs().max()) > 0


@pytest.mark.parametrize("size,iters", [(SMALL, 3), (SMALL, 12), (DIRECT, 3)], ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
def test_batched_equals_per_iteration_eagerly(size, iters):
    got, seen = _eager("batched", iters, 1, size)
    # the two batched data gradients where one image alone runs the direct kernel; per-image launches otherwise
    assert seen == ([iters, iters] if size == DIRECT else []), seen
    _same(got, _reference(iters, 1, size))


@pytest.mark.parametrize("size,iters", [(SMALL, 3), (SMALL, 12), (DIRECT, 3)], ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else None)
def test_batched_equals_per_iteration_in_a_captured_graph(size, iters):
    want = _reference(iters, 1, size)
    model = closure_util.load_model("RAFT", True, torch.device("cuda", 0), EPS, CFG["batched"])
    a, b, n1, n2 = _inputs(1, size)
    n1.requires_grad_(True)
    n2.requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm-up of the same shapes (workspaces, weight packs)
        loss, flow = _closure(model, a, b, n1, n2, iters)
        torch.autograd.grad(loss, (n1, n2))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    outs = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, flow = _closure(model, a, b, n1, n2, iters)
        g1, g2 = torch.autograd.grad(loss, (n1, n2))
        outs = (loss.detach(), flow.detach(), g1, g2)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _same(outs, want)
        for t in outs:
            t.fill_(float("nan"))


def test_two_images_take_the_per_iteration_path_unchanged():
    got, seen = _eager("batched", 3, 2)
    assert seen == [], "a two-image input must not take the batched path"
    _same(got, _reference(3, 2))
