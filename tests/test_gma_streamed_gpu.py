"""GMA attention without the [N, N] matrix (Config.gma_attention = "streamed"; csrc/gma_attn_stream.hip) against float64.

Kernels through the C-ABI.  Every operand and output sits between NaN fences (tests/fenced.py); the float64 reference
is computed from the same fp32 inputs the kernel saw.  Each entry point is given exact inputs: fwd / dv / dqk receive
lse32 = fp32(lse64) and delta32 = fp32(delta64) and the reference is the kernel's own statement P = exp(s - lse32).
The kernels own blocks of 64 rows and stream blocks of 64, so N = 35, 135 (2 * 64 + 7) and 273 (4 * 64 + 17) all end in
a tail block; 256 and 7040 are exact multiples.

The tolerance is derived, not tuned.  u = 2^-24, gamma_n = n u / (1 - n u) (Higham 3.1), d = 128, N' = N + 64 (the
zero rows of the tail block still pass through the accumulators).  SLACK = 1.01 absorbs products of two error terms.
  logit   s^ = fl(scale * fl(sum_c q_c k_c)): d fma steps and the scaling,
            |s^ - s| <= es := gamma_{d+1} * scale * sum_c |q_c| |k_c|
  lse     the maximum m^ of the rounded logits is exact and lse is invariant under the shift.  The argument fl(s^ - m^)
          is off by a_ij <= es_ij + u (|s_ij| + |m_i|); expf and logf are the HIP math library's device functions,
          documented within 1 ulp (<= 2u relative); the N positive terms are added with at most N roundings:
            |lse^ - lse| <= SLACK (max_j a_ij + 2u + gamma_N) + 2u |lse - m| + u |lse|
  P       the argument fl(s^ - lse) is off by b_ij <= SLACK (es_ij + elog_i + u (|s_ij| + |lse_i|)), elog = 0 where lse
          is an exact input:  eP := |P^ - P| <= P (expm1(b_ij) + 2u SLACK) + 2^-126 (a flushed subnormal)
  out, dv N' accumulation steps of sum_j P_ij v_j:  |out^ - out| <= sum_j (eP_ij + gamma_N' (P_ij + eP_ij)) |v_j|, and
          the same with P^T and |g| for dv
  delta   two fma steps per lane, six shuffle additions and one accumulation per iteration:
            |delta^ - delta| <= gamma_{9+n} sum_i sum_c |g_ic| |out_ic|
  dq, dk  T = [g_1|..|g_n] [v_1|..|v_n]^T: et := gamma_{n d} (|G| |V|^T);  x = T - delta: ex := et + edelta + SLACK u |x|;
          dS = P x:  eds := eP (|x| + ex) + P ex + SLACK u |dS|;  then N' accumulation steps and the final scaling:
            |dq^ - dq| <= SLACK scale sum_j (eds_ij + gamma_N' (|dS_ij| + eds_ij)) |k_j| + u |dq|,  dk with dS^T and |q|
All right-hand sides are evaluated in float64.  The autograd-node test feeds the kernels' own lse and delta into the
later passes, so there elog is the lse bound and edelta = sum_i sum_c (|g| b_out + gamma_{9+n} |g| (|out| + b_out)).
Every case records its worst err / bound ratio as a junit property.

Not gates, recorded as properties for DESIGN 7: the rel-L2 error against float64 of the materialised path
(attention_softmax + attn_times_value with gemm="hip") and of the streamed path on the same inputs.
"""
import ctypes
import dataclasses
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pcfa_amd import _hip, hip_ops
from pcfa_amd import config as pcfa_config
from tests import closure_util
from tests.fenced import DEV, NAN_BITS, PCFA_ERR_UNSUPPORTED, SENTINEL, TINY, U, Fenced, gamma
from tests.fenced import stream as _stream
from tests.util import load_golden, max_abs, rel_l2, t

pytestmark = pytest.mark.gpu

D = 128
SCALE = float(np.float32(D ** -0.5))     # the fp32 value the kernels receive
SLACK = 1.01
KINDS = ("normal", "peaked", "one_hot", "constant")
SHAPES = [(1, 1), (1, 35), (2, 135), (1, 256), (3, 273)]
OD = dataclasses.replace(pcfa_config.DEFAULT, corr="on_demand")
MAT = dataclasses.replace(OD, gma_attention="materialised")
MAT_LIB = dataclasses.replace(MAT, gma_gemm="lib")
MAT_HIP = dataclasses.replace(MAT, gma_gemm="hip")
STR = dataclasses.replace(OD, gma_attention="streamed")


def make_inputs(kind, BH, N, n, seed=0):
    """(q, k, [v_1..v_n], [g_1..g_n]) as fp32 CPU tensors [BH, N, 128]."""
    gen = torch.Generator().manual_seed(1000 * seed + 131 * N + 17 * BH + n + 7 * KINDS.index(kind))
    q = torch.randn(BH, N, D, generator=gen)
    k = torch.randn(BH, N, D, generator=gen)
    if kind == "peaked":          # logits with a standard deviation of ~144: a naive exp overflows
        q, k = 12 * q, 12 * k
    elif kind == "one_hot":       # query i points at key perm(i): that logit is ~22, the others ~N(0, 2^2)
        perm = torch.randperm(N, generator=gen)
        q = 2 * k[:, perm]
    elif kind == "constant":      # all keys equal: P = 1 / N
        k = k[:, :1].expand(BH, N, D).contiguous()
    vs = [torch.randn(BH, N, D, generator=gen) for _ in range(n)]
    gs = [torch.randn(BH, N, D, generator=gen) for _ in range(n)]
    return q.contiguous(), k, vs, gs


def analyse(q, k, vs, gs, dev, chained):
    """float64 values and the module docstring's bounds, on `dev`.  chained = False: lse and delta are exact inputs (their
    fp32 roundings, returned as lse_in / delta_in); True: the true softmax, with the kernels' own lse / delta errors."""
    n, N = len(vs), q.shape[-2]
    Np = N + 64
    q64, k64 = q.double().to(dev), k.double().to(dev)
    v64, g64 = [v.double().to(dev) for v in vs], [g.double().to(dev) for g in gs]
    s = SCALE * (q64 @ k64.mT)
    es = gamma(D + 1) * SCALE * (q64.abs() @ k64.abs().mT)
    m = s.amax(-1, keepdim=True)
    lse = torch.logsumexp(s, -1, keepdim=True)
    a = es + U * (s.abs() + m.abs())
    b_lse = SLACK * (a.amax(-1, keepdim=True) + 2 * U + gamma(N)) + 2 * U * (lse - m).abs() + U * lse.abs()
    del a
    lse_in = lse if chained else lse.float().double()
    elog = b_lse if chained else 0.0
    P = torch.exp(s - lse_in)
    b_arg = SLACK * (es + elog + U * (s.abs() + lse_in.abs()))
    eP = P * (torch.expm1(b_arg) + 2 * U * SLACK) + TINY
    del b_arg, es
    wP = eP + gamma(Np) * (P + eP)
    R = {"s": s, "lse": lse.squeeze(-1), "b_lse": b_lse.squeeze(-1), "lse_in": lse_in.squeeze(-1)}
    R["out"] = [P @ v for v in v64]
    R["b_out"] = [wP @ v.abs() for v in v64]
    R["dv"] = [P.mT @ g for g in g64]
    R["b_dv"] = [wP.mT @ g.abs() for g in g64]
    del wP
    delta = sum((g * o).sum(-1, keepdim=True) for g, o in zip(g64, R["out"]))
    gabs_out = sum((g.abs() * o.abs()).sum(-1, keepdim=True) for g, o in zip(g64, R["out"]))
    R["b_delta"] = (gamma(9 + n) * gabs_out).squeeze(-1)
    if chained:
        delta_in = delta
        edelta = sum((g.abs() * (b + gamma(9 + n) * (o.abs() + b))).sum(-1, keepdim=True)
                     for g, o, b in zip(g64, R["out"], R["b_out"]))
    else:
        delta_in, edelta = delta.float().double(), 0.0
    R["delta"], R["delta_in"] = delta.squeeze(-1), delta_in.squeeze(-1)
    G, V = torch.cat(g64, -1), torch.cat(v64, -1)
    x = G @ V.mT - delta_in
    ex = gamma(n * D) * (G.abs() @ V.abs().mT) + edelta + SLACK * U * x.abs()
    dS = P * x
    eds = eP * (x.abs() + ex) + P * ex + SLACK * U * dS.abs()
    del x, ex, eP, P
    wds = eds + gamma(Np) * (dS.abs() + eds)
    del eds
    R["dq"] = SCALE * (dS @ k64)
    R["b_dq"] = SLACK * SCALE * (wds @ k64.abs()) + U * R["dq"].abs()
    R["dk"] = SCALE * (dS.mT @ q64)
    R["b_dk"] = SLACK * SCALE * (wds.mT @ q64.abs()) + U * R["dk"].abs()
    return R


def rounded_reference_ratios(R):
    """err / bound of the fp32-rounded reference itself, per quantity: must be <= 1 or the bound is wrong."""
    out = {}
    for name, bname in (("lse", "b_lse"), ("out", "b_out"), ("dv", "b_dv"), ("dq", "b_dq"), ("dk", "b_dk")):
        vals, bs = (R[name], R[bname]) if isinstance(R[name], list) else ([R[name]], [R[bname]])
        out[name] = max(float(((v.float().double() - v).abs() / b).max()) for v, b in zip(vals, bs))
    return out


def _fen(x):
    x = x.contiguous()
    return Fenced(tuple(x.shape), tuple(x.stride()), NAN_BITS).write(x.float())


def _fout(*shape):
    stride, acc = [], 1
    for s in reversed(shape):
        stride.insert(0, acc)
        acc *= s
    return Fenced(shape, tuple(stride), SENTINEL)


def _twice(call, outs):
    """Run an entry point, then again: status 0 and equal bits; returns the outputs' fp32 values."""
    assert call() == 0
    torch.cuda.synchronize()
    first = [o.view().clone() for o in outs]
    assert call() == 0
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(o.view().view(torch.int32), f.view(torch.int32)), "not repeatable bit for bit"
    return first


def _ratio(got, want, bound):
    got = got.double()
    assert bool(torch.isfinite(got).all()), "an output element was never written or is not finite"
    return float(((got - want).abs() / bound).max())


def run_kernels(q, k, vs, gs, R, parts=("lse", "fwd", "dv", "delta", "dqk")):
    """The entry points through the C-ABI on fenced operands against analyse(chained=False); returns err / bound ratios."""
    lib = _hip.load()
    BH, N, _ = q.shape
    n = len(vs)
    sc = ctypes.c_float(SCALE)
    fq, fk = _fen(q), _fen(k)
    flse, fdelta = _fen(R["lse_in"]), _fen(R["delta_in"])
    fences, ratios = [fq, fk, flse, fdelta], {}
    if "lse" in parts:
        o = _fout(BH, N)
        [lse] = _twice(lambda: lib.pcfa_attn_stream_lse(fq.ptr(), fk.ptr(), o.ptr(), BH, N, D, sc, _stream()), [o])
        ratios["lse"] = _ratio(lse, R["lse"], R["b_lse"])
        fences.append(o)
    for i in range(n):
        fv, fg = _fen(vs[i]), _fen(gs[i])
        fences += [fv, fg]
        if "fwd" in parts:
            o = _fout(BH, N, D)
            [out] = _twice(lambda: lib.pcfa_attn_stream_fwd(fq.ptr(), fk.ptr(), fv.ptr(), flse.ptr(), o.ptr(), BH, N, D,
                                                            sc, _stream()), [o])
            ratios["out"] = max(ratios.get("out", 0.0), _ratio(out, R["out"][i], R["b_out"][i]))
            fences.append(o)
        if "dv" in parts:
            o = _fout(BH, N, D)
            [dv] = _twice(lambda: lib.pcfa_attn_stream_dv(fq.ptr(), fk.ptr(), fg.ptr(), flse.ptr(), o.ptr(), BH, N, D, sc,
                                                          _stream()), [o])
            ratios["dv"] = max(ratios.get("dv", 0.0), _ratio(dv, R["dv"][i], R["b_dv"][i]))
            fences.append(o)
    if "delta" in parts:
        o = _fout(BH, N)
        fgs, fos = [_fen(g) for g in gs], [_fen(x.float()) for x in R["out"]]

        def delta_calls():
            for i in range(n):
                st = lib.pcfa_attn_stream_delta(fgs[i].ptr(), fos[i].ptr(), o.ptr(), BH * N, D, int(i > 0), _stream())
                if st:
                    return st
            return 0
        [dl] = _twice(delta_calls, [o])
        want = sum((g.double().to(DEV) * x.float().double()).sum(-1) for g, x in zip(gs, R["out"]))
        ratios["delta"] = _ratio(dl, want, R["b_delta"] + TINY)
        fences += fgs + fos + [o]
    if "dqk" in parts:
        fG, fV = _fen(torch.cat(gs, -1)), _fen(torch.cat(vs, -1))
        odq, odk = _fout(BH, N, D), _fout(BH, N, D)
        dq, dk = _twice(lambda: lib.pcfa_attn_stream_dqk(fq.ptr(), fk.ptr(), flse.ptr(), fG.ptr(), fV.ptr(), fdelta.ptr(),
                                                         odq.ptr(), odk.ptr(), BH, N, D, n, sc, _stream()), [odq, odk])
        ratios["dq"] = _ratio(dq, R["dq"], R["b_dq"])
        ratios["dk"] = _ratio(dk, R["dk"], R["b_dk"])
        fences += [fG, fV, odq, odk]
    assert all(f.fence_intact() for f in fences), "a store landed outside an operand or output"
    return ratios


def _check(record_property, ratios):
    for name, r in ratios.items():
        record_property("err_over_bound_" + name, round(r, 4))
    print("err / bound:", {k: round(v, 4) for k, v in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), ratios


# --------------------------------------------------------------------------- kernels through the C-ABI
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "BH%d-N%d" % s)
def test_kernels_vs_float64(record_property, shape, kind, n):
    q, k, vs, gs = make_inputs(kind, shape[0], shape[1], n)
    R = analyse(q, k, vs, gs, DEV, chained=False)
    if kind == "peaked" and shape[1] >= 35:
        assert float(R["s"].abs().max()) > 100
    if kind == "constant":
        assert max_abs(torch.exp(R["s"] - R["lse"].unsqueeze(-1)), torch.full_like(R["s"], 1.0 / shape[1])) < 1e-9
    assert all(r <= 1.0 for r in rounded_reference_ratios(R).values())
    _check(record_property, run_kernels(q, k, vs, gs, R))


def test_product_size_forward(record_property):
    q, k, vs, gs = make_inputs("normal", 1, 7040, 1)
    R = analyse(q, k, vs, gs, DEV, chained=False)
    _check(record_property, run_kernels(q, k, vs, gs, R, parts=("lse", "fwd")))


def test_product_size_backward(record_property):
    q, k, vs, gs = make_inputs("normal", 1, 7040, 1)
    R = analyse(q, k, vs, gs, DEV, chained=False)
    _check(record_property, run_kernels(q, k, vs, gs, R, parts=("dv", "delta", "dqk")))


def test_two_calls_give_equal_bits():
    """run_kernels repeats every entry point and compares bits; here on the case with three heads and a tail block."""
    q, k, vs, gs = make_inputs("one_hot", 3, 273, 3, seed=1)
    run_kernels(q, k, vs, gs, analyse(q, k, vs, gs, DEV, chained=False))


def test_other_head_dimensions_are_refused():
    lib = _hip.load()
    x = torch.zeros(1, 8, 64, device=DEV)
    lse = torch.zeros(1, 8, device=DEV)
    st = lib.pcfa_attn_stream_lse(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr()),
                                  ctypes.c_void_p(lse.data_ptr()), 1, 8, 64, ctypes.c_float(SCALE), _stream())
    assert st == PCFA_ERR_UNSUPPORTED


# --------------------------------------------------------------------------- the autograd node
def _streamed_three_iterations(q, k, vs, gs):
    qd, kd = q.to(DEV).requires_grad_(True), k.to(DEV).requires_grad_(True)
    vd = [v.to(DEV).requires_grad_(True) for v in vs]
    h = hip_ops.streamed_attention(qd, kd, SCALE)
    outs = [hip_ops.streamed_attn_times_value(h, v) for v in vd]
    return qd, kd, vd, h, outs, sum((o * g.to(DEV)).sum() for o, g in zip(outs, gs))


@pytest.mark.parametrize("N", [135, 273])
def test_autograd_node_three_iterations_vs_float64_autograd(record_property, N):
    q, k, vs, gs = make_inputs("normal", 2, N, 3, seed=2)
    R = analyse(q, k, vs, gs, DEV, chained=True)
    # float64 autograd of the plain expression (and the closed forms the bounds are built around agree with it)
    q64, k64 = q.double().to(DEV).requires_grad_(True), k.double().to(DEV).requires_grad_(True)
    v64 = [v.double().to(DEV).requires_grad_(True) for v in vs]
    attn = torch.softmax(SCALE * (q64 @ k64.mT), -1)
    o64 = [attn @ v for v in v64]
    sum((o * g.double().to(DEV)).sum() for o, g in zip(o64, gs)).backward()
    assert rel_l2(R["dq"], q64.grad) < 1e-12 and rel_l2(R["dk"], k64.grad) < 1e-12
    qd, kd, vd, h, outs, loss = _streamed_three_iterations(q, k, vs, gs)
    assert h.pending == 3
    loss.backward(retain_graph=True)
    assert h.pending == 0 and h.gs == [] and h.delta is None
    ratios = {"out": max(_ratio(o.detach(), w.detach(), b) for o, w, b in zip(outs, o64, R["b_out"])),
              "dv": max(_ratio(v.grad, w.grad, b) for v, w, b in zip(vd, v64, R["b_dv"])),
              "dq": _ratio(qd.grad, q64.grad, R["b_dq"]), "dk": _ratio(kd.grad, k64.grad, R["b_dk"]),
              "lse": _ratio(h.lse(), R["lse"], R["b_lse"])}
    _check(record_property, ratios)
    with pytest.raises(RuntimeError, match="retain_graph is not supported"):
        loss.backward()


def test_no_grad_call_saves_nothing():
    q, k, vs, _ = make_inputs("normal", 1, 135, 1, seed=3)
    qd, kd = q.to(DEV).requires_grad_(True), k.to(DEV).requires_grad_(True)
    with torch.no_grad():
        h = hip_ops.streamed_attention(qd, kd, SCALE)
        out = hip_ops.streamed_attn_times_value(h, vs[0].to(DEV))
    assert out.grad_fn is None and not out.requires_grad and h.pending == 0 and h.gs == [] and h.vs == []
    h2 = hip_ops.streamed_attention(qd, kd, SCALE)
    out2 = hip_ops.streamed_attn_times_value(h2, vs[0].to(DEV))
    assert out2.grad_fn is not None and torch.equal(out, out2)


@pytest.mark.parametrize("N", [273, 7040])
def test_rel_l2_of_both_paths_vs_float64(record_property, N):
    """Not a gate: the figures of DESIGN 7.  One iteration, the same inputs through both paths."""
    q, k, vs, gs = make_inputs("normal", 1, N, 1, seed=4)
    R = analyse(q, k, vs, gs, DEV, chained=True)
    g = gs[0].to(DEV)
    qd, kd, vd, _, outs, loss = _streamed_three_iterations(q, k, vs, gs)
    loss.backward()
    qm, km, vm = (x.to(DEV).requires_grad_(True) for x in (q, k, vs[0]))
    attn = hip_ops.attention_softmax(qm, km, SCALE, gemm="hip")
    om = hip_ops.attn_times_value(attn, vm, hip_ops.AttnGradShare("hip"))
    (om * g).sum().backward()
    for name, want, a, b in (("out", R["out"][0], outs[0], om), ("dv", R["dv"][0], vd[0].grad, vm.grad),
                             ("dq", R["dq"], qd.grad, qm.grad), ("dk", R["dk"], kd.grad, km.grad)):
        record_property("rel_l2_streamed_" + name, rel_l2(a, want))
        record_property("rel_l2_materialised_" + name, rel_l2(b, want))
        print("N=%d %s rel-L2 vs float64: streamed %.3e, materialised/hip %.3e" % (N, name, rel_l2(a, want),
                                                                                   rel_l2(b, want)))
        assert rel_l2(a, want) < 1e-4      # sanity only; the gates are the elementwise bounds above


# --------------------------------------------------------------------------- closures
def _gma_closure(config, h, w, seed=21, **kw):
    return closure_util.run_closure("GMA", h, w, "change_of_variables", False, "neg_flow", "aee", seed, torch.device(DEV),
                                    config=config, **kw)


@pytest.mark.parametrize("h,w", [(128, 160), (436, 1024)])
def test_closure_streamed_vs_materialised(h, w):
    """The same weights and inputs under both switches, at test_closure_on_demand_vs_all_pairs's tolerances."""
    a, b = _gma_closure(STR, h, w), _gma_closure(MAT, h, w)
    scale = float(b["flow"].abs().max())
    assert float((a["flow"] - b["flow"]).abs().max()) <= 1e-3 * scale
    assert abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"]), (a["loss"], b["loss"])
    for x, y in zip(a["grads"], b["grads"]):
        assert rel_l2(x, y) < 1e-2, rel_l2(x, y)


def test_closure_streamed_vs_reference_golden():
    g = load_golden("closure_gma")
    leaves = [t(g["leaf0"]), t(g["leaf1"])]
    r = _gma_closure(STR, 128, 160, seed=2, leaves=leaves,
                     images=(t(g["image1"].astype(np.float32)), t(g["image2"].astype(np.float32))))
    scale = float(np.abs(g["flow"]).max())
    assert max_abs(r["flow"], t(g["flow"])) <= 1e-3 * scale
    assert float((r["flow"].cpu() - t(g["flow"])).pow(2).sum(1).sqrt().mean()) <= 1e-3
    assert abs(r["loss"] - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
    for i, gr in enumerate(r["grads"]):
        assert rel_l2(gr, t(g["grad%d" % i])) < 1e-2


def _closure_kernel_names(config, h=128, w=160):
    import bench
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device(DEV)
    model = bench.load_model("GMA", dev, True, config)
    st = bench.AttackStepper("GMA", h, w, dev, 3, use_graph=False, model=model)
    st.optimizer.zero_grad()
    st.closure_body()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.optimizer.zero_grad()
        st.closure_body()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


def test_streamed_closure_runs_the_streamed_kernels():
    """Which kernels ran.  The materialised/lib closure sends, per closure, the similarity product, one attn v and one
    attn^T g per iteration, the shared gradient product and the two dq / dk products to rocBLAS (Cijk_ kernels): with
    n = 6 iterations 1 + 2 n + 1 + 2 = 16.  The streamed closure sends none of them, so every [N, N] product is gone;
    what it keeps are the 1x1 layers that both builds run on the library."""
    n_iter = 6
    streamed, lib = _closure_kernel_names(STR), _closure_kernel_names(MAT_LIB)
    assert any("attn_stream_kernel" in x for x in streamed) and any("attn_stream_delta" in x for x in streamed)
    assert not any("softmax_rows" in x for x in streamed)
    assert any("softmax_rows" in x for x in lib) and not any("attn_stream" in x for x in lib)
    cs, cl = sum(x.startswith("Cijk_") for x in streamed), sum(x.startswith("Cijk_") for x in lib)
    print("Cijk_ launches per closure: streamed %d, materialised/lib %d" % (cs, cl))
    assert cl - cs >= 2 * n_iter + 4, (cs, cl)


def _peak_closure_bytes(config, h, w):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    r = _gma_closure(config, h, w, seed=3)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(), r


def test_memory_at_1088x1920():
    N = (1088 // 8) * (1920 // 8)
    assert N == 32640
    st, _ = _peak_closure_bytes(STR, 1088, 1920)
    mt, _ = _peak_closure_bytes(MAT, 1088, 1920)
    print("peak bytes at 1088x1920: streamed %.2f GB, materialised %.2f GB" % (st / 1e9, mt / 1e9))
    assert mt - st >= 4 * N * N, (st, mt)


def test_gma_pairs_in_flight_bit_identical_to_solo():
    """Streamed GMA goes in flight whatever gma_gemm says (here the default "lib")."""
    import bench
    from pcfa_amd import attack_PCFA
    dev = torch.device(DEV)
    assert STR.gma_gemm == "lib"
    own = bench.load_model("GMA", dev, True, STR)
    flight = attack_PCFA.PairsInFlight(
        lambda k: bench.AttackStepper("GMA", 128, 160, dev, 51 + k, use_graph=True, model=own), 2, dev)
    last = flight.run(2)
    for k in (0, 1):
        own._pcfa_pair_graphs.clear()
        solo = bench.AttackStepper("GMA", 128, 160, dev, 51 + k, use_graph=True, model=own)
        solo.step()
        assert tuple(solo.step()) == tuple(last[k]), k
        assert torch.equal(flight.attacks[k].delta1, solo.delta1)
        del solo
    own._pcfa_pair_graphs.clear()


def test_gma_streamed_fresh_processes_are_bit_identical():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PCFA_GMA_ATTENTION="streamed")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "process_repro.py"), "--net", "GMA", "--size",
                        "128x160", "--steps", "2", "--procs", "2"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode in (0, 1), p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["identical"], rec["first_difference"]


@pytest.mark.skipif(os.environ.get("PCFA_LONG_TESTS") != "1", reason="2160x3840 closure: set PCFA_LONG_TESTS=1")
def test_streamed_closure_at_2160x3840():
    peak, r = _peak_closure_bytes(STR, 2160, 3840)
    print("2160x3840 on_demand + streamed GMA peak %.2f GB" % (peak / 1e9))
    assert bool(torch.isfinite(r["flow"]).all())
    assert all(bool(torch.isfinite(g).all()) for g in r["grads"])
