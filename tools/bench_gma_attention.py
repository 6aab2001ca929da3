"""Config.gma_attention = "materialised" against "streamed": per-kernel device times of the four pcfa_attn_stream_* entry
points (pcfa_timing_arm, through ops.profiling.DispatchTimer) and the eager GMA closure's device time and peak memory.

    python tools/bench_gma_attention.py [--sizes 436x1024,1088x1920] [--reps 5] [--out DIR]

Per size: the streamed attention of one GMA closure replayed on random q, k, v_i, g_i at the closure's map size (one
handle, 6 iterations, their backwards), with the achieved fraction of the fp32 matrix peak per kernel (N^2 * 128
products counted: lse 2, fwd 2, dv 2, dq and dk n + 2 each); then eager closures of a seeded GMA attack pair for the
builds materialised/lib, materialised/hip and streamed, all with corr = "on_demand", ALTERNATED within one session
(rep by rep) and timed with device events after one warm-up closure each, with torch.cuda.max_memory_allocated per
build.  One JSON line per (size, build) and one per size for the kernels; --out also writes them to DIR/bench.jsonl.
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3   # fp32 matrix peak of one MI355X
ITERS = 6
PLAN = {"pcfa_attn_stream_lse": [("lse", 0)], "pcfa_attn_stream_fwd": [("fwd", 0)], "pcfa_attn_stream_dv": [("dv", 0)],
        "pcfa_attn_stream_delta": [("delta", 0)], "pcfa_attn_stream_dqk": [("dq", 0), ("dk", 1)]}
UNITS = {"lse": 2, "fwd": 2, "dv": 2, "dq": ITERS + 2, "dk": ITERS + 2}   # N^2 * 128 products per launch
BUILDS = {"materialised/lib": dict(gma_attention="materialised", gma_gemm="lib"),
          "materialised/hip": dict(gma_attention="materialised", gma_gemm="hip"),
          "streamed": dict(gma_attention="streamed")}


def attention_kernels(N, dev):
    from pcfa_amd import hip_ops
    from pcfa_amd.ops import core, profiling
    gen = torch.Generator().manual_seed(0)
    q = torch.randn(1, 1, N, 128, generator=gen).to(dev)
    k = torch.randn(1, 1, N, 128, generator=gen).to(dev)
    vs = [torch.randn(1, 1, N, 128, generator=gen).to(dev) for _ in range(ITERS)]
    gs = [torch.randn(1, 1, N, 128, generator=gen).to(dev) for _ in range(ITERS)]

    def once():
        a, b = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
        h = hip_ops.streamed_attention(a, b, 128 ** -0.5)
        loss = sum((hip_ops.streamed_attn_times_value(h, v.clone().requires_grad_(True)) * g).sum()
                   for v, g in zip(vs, gs))
        loss.backward()

    once()
    timer = profiling.DispatchTimer(PLAN)
    core.set_dispatch_timer(timer)
    try:
        for _ in range(3):
            once()
    finally:
        core.set_dispatch_timer(None)
    us = {name: round(v[0], 2) for name, v in timer.summary().items()}
    frac = {name: round(UNITS[name] * 2.0 * N * N * 128 / (us[name] * 1e-6) / (PEAK_TFLOPS * 1e12), 3)
            for name in UNITS if name in us}
    return us, frac


def closures(h, w, dev, reps):
    import bench
    from pcfa_amd import config as pcfa_config
    steppers = {}
    for name, kw in BUILDS.items():
        config = dataclasses.replace(pcfa_config.DEFAULT, corr="on_demand", **kw)
        model = bench.load_model("GMA", dev, True, config)
        st = bench.AttackStepper("GMA", h, w, dev, 0, use_graph=False, model=model)
        st.optimizer.zero_grad()
        st.closure_body()          # warm-up
        torch.cuda.synchronize()
        steppers[name] = st
    ms = {name: [] for name in BUILDS}
    peak = {name: 0 for name in BUILDS}
    for _ in range(reps):          # the builds alternate rep by rep
        for name, st in steppers.items():
            st.optimizer.zero_grad()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.closure_body()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
            # what this closure added on top of what the session holds (three models and their static buffers)
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - base)
    return {name: {"closure_ms_median": round(sorted(v)[len(v) // 2], 2), "closure_ms_min": round(min(v), 2),
                   "closure_peak_above_resident_gb": round(peak[name] / 1e9, 3)} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="436x1024,1088x1920")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    lines = []
    for size in [s for s in a.sizes.split(",") if s]:
        h, w = (int(v) for v in size.split("x"))
        N = ((h + 7) // 8) * ((w + 7) // 8)
        us, frac = attention_kernels(N, dev)
        lines.append({"size": size, "N": N, "iterations": ITERS, "kernel_us": us, "fraction_of_fp32_matrix_peak": frac})
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
        res = closures(h, w, dev, a.reps)
        base = res["materialised/lib"]["closure_ms_median"]
        for name, rec in res.items():
            rec = dict({"size": size, "build": name, "corr": "on_demand"}, **rec)
            rec["closure_ratio_to_materialised_lib"] = round(rec["closure_ms_median"] / base, 3)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench.jsonl"), "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
