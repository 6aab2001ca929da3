"""Config.corr = "all_pairs" against "on_demand": per-kernel device times of the correlation (pcfa_timing_arm, through
ops.profiling.DispatchTimer) and one RAFT closure's device time and peak memory.

    python tools/bench_corr_ondemand.py [--sizes 436x1024,1088x1920] [--od-only 2160x3840] [--out DIR]

Per size and switch: the correlation of one RAFT closure replayed on random features at the closure's map size (one
build, 12 lookups, their backwards, the finish), then eager closures of a seeded RAFT attack pair (timed with device
events after one warm-up closure) with torch.cuda.max_memory_allocated.  One JSON line per (size, switch); --out also
writes them to DIR/bench.jsonl.
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLANS = {
    "all_pairs": {"pcfa_corr_f2ext_fwd": [("f2ext_fwd", 0)], "pcfa_corr_pyramid_fwd": [("pyramid_fwd", 0)],
                  "pcfa_corr_lookup_fwd": [("lookup_fwd", 0)], "pcfa_corr_lookup_bwd": [("lookup_bwd", 0)]},
    "on_demand": {"pcfa_corr_ondemand_prepare": [("od_to_rows_f1", 0), ("od_to_rows_f2", 1), ("od_pool_l1", 2)],
                  "pcfa_corr_ondemand_fwd": [("od_fwd", 0)],
                  "pcfa_corr_ondemand_bwd": [("od_absmax_grad", 0), ("od_shift", 1), ("od_bwd", 2), ("od_convert", 3)],
                  "pcfa_corr_ondemand_finish": [("od_finish_df1", 0), ("od_finish_df2", 1)]},
}


def corr_kernels(corr, H, W, dev, iters=12):
    from pcfa_amd import hip_ops
    from pcfa_amd.ops import core, profiling
    gen = torch.Generator().manual_seed(0)
    f1 = torch.randn(1, 256, H, W, generator=gen).to(dev)
    f2 = torch.randn(1, 256, H, W, generator=gen).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = torch.stack([xs, ys], 0).float()[None]
    coords = [(base + 2.0 * torch.randn(1, 2, 1, 1, generator=gen) + 0.5 * torch.randn(1, 2, H, W, generator=gen)).to(dev)
              for _ in range(iters)]
    gos = [torch.randn(1, 324, H, W, generator=gen).to(dev) for _ in range(iters)]
    cls = hip_ops.OnDemandCorrBlock if corr == "on_demand" else hip_ops.CorrBlock

    def once():
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        blk = cls(a, b, num_levels=4, radius=4)
        loss = sum((blk(c) * g).sum() for c, g in zip(coords, gos))
        loss.backward()

    once()
    timer = profiling.DispatchTimer(PLANS[corr])
    core.set_dispatch_timer(timer)
    try:
        for _ in range(3):
            once()
    finally:
        core.set_dispatch_timer(None)
    return {k: round(v[0], 2) for k, v in timer.summary().items()}


def closure(corr, h, w, dev, reps):
    import bench
    from pcfa_amd import config as pcfa_config
    config = dataclasses.replace(pcfa_config.DEFAULT, corr=corr)
    model = bench.load_model("RAFT", dev, True, config)
    st = bench.AttackStepper("RAFT", h, w, dev, 0, use_graph=False, model=model)
    st.optimizer.zero_grad()
    st.closure_body()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.optimizer.zero_grad()
        e0.record()
        st.closure_body()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    peak = torch.cuda.max_memory_allocated()
    del st, model
    return {"closure_ms_median": round(sorted(ms)[len(ms) // 2], 2), "closure_ms_min": round(min(ms), 2),
            "peak_gb": round(peak / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="436x1024,1088x1920")
    ap.add_argument("--od-only", default="2160x3840")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    runs = [(s, c) for s in a.sizes.split(",") if s for c in ("all_pairs", "on_demand")]
    runs += [(s, "on_demand") for s in a.od_only.split(",") if s]
    lines = []
    for size, corr in runs:
        h, w = (int(v) for v in size.split("x"))
        H, W = (h + 7) // 8, (w + 7) // 8   # the padded input's feature map
        rec = {"size": size, "corr": corr, "features": "%dx%d" % (H, W)}
        rec["kernel_us"] = corr_kernels(corr, H, W, dev)
        torch.cuda.empty_cache()
        rec.update(closure(corr, h, w, dev, max(2, a.reps if h * w < 4e6 else 2)))
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench.jsonl"), "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
