"""Config.corr = "all_pairs" against "on_demand" (Config.ondemand_lookup = "per_query" and "tiled"): per-kernel device
times of the correlation (pcfa_timing_arm, through ops.profiling.DispatchTimer) and one RAFT closure's device time and
peak memory.

    python tools/bench_corr_ondemand.py [--sizes 436x1024,1088x1920] [--od-only 2160x3840] [--out DIR]

Per size and leg (all_pairs, on_demand, on_demand_tiled): the correlation of one RAFT closure replayed on random features
at the closure's map size (one build, 12 lookups, their backwards, the finish), then eager closures of a seeded RAFT
attack pair (device events, after one warm-up closure per leg) with torch.cuda.max_memory_allocated.  The legs of a size
are ALTERNATED rep by rep in one process, so drift hits them alike; median and min-max are reported.  The tiled leg also
reports the route shares per level (pcfa_corr_ondemand_tile_routes after every lookup): of the replayed random-feature
lookups and of RAFT's own coordinates over the iterations of the real closure.  One JSON line per (size, leg); --out
also writes them to DIR/bench.jsonl.
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
PLANS["on_demand_tiled"] = dict(PLANS["on_demand"])
del PLANS["on_demand_tiled"]["pcfa_corr_ondemand_fwd"], PLANS["on_demand_tiled"]["pcfa_corr_ondemand_bwd"]
PLANS["on_demand_tiled"].update({
    "pcfa_corr_ondemand_fwd_tiled": [("od_classify_fwd", 0), ("od_fwd_tile", 1), ("od_fwd", 2)],
    "pcfa_corr_ondemand_bwd_tiled": [("od_absmax_grad", 0), ("od_shift", 1), ("od_classify_bwd", 2), ("od_bwd_tile", 3),
                                     ("od_bwd", 4), ("od_convert", 5)]})
LEGS = {"all_pairs": ("all_pairs", "per_query"), "on_demand": ("on_demand", "per_query"),
        "on_demand_tiled": ("on_demand", "tiled")}


class RouteRecorder:
    """Counts the (tile, level) pairs per level and route of every tiled lookup made while it is installed."""

    def __init__(self):
        self.counts = []

    def __enter__(self):
        from pcfa_amd import _hip
        from pcfa_amd.ops import corr
        self._cls, self._orig = corr.OnDemandCorrBlock, corr.OnDemandCorrBlock.__call__
        lib, rec = _hip.load(), self

        def call(blk, coords):
            out = rec._orig(blk, coords)
            st = blk._state
            if st.suffix == "_tiled":
                c = torch.zeros(st.L, 2, device=coords.device, dtype=torch.int32)
                _hip.check(lib.pcfa_corr_ondemand_tile_routes(st.ws.data_ptr(), st.B, st.D, st.H, st.W, st.L, c.data_ptr(),
                                                              torch.cuda.current_stream().cuda_stream), "tile_routes")
                rec.counts.append(c)
            return out

        self._cls.__call__ = call
        return self

    def __exit__(self, *exc):
        self._cls.__call__ = self._orig

    def shares(self):
        """per level: share of the pairs on the matrix route, over all recorded lookups"""
        if not self.counts:
            return None
        tot = torch.stack(self.counts).sum(0).cpu().double()
        return [round(float(m / max(1.0, m + q)), 4) for m, q in tot]


def corr_kernels(leg, H, W, dev, iters=12):
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
    corr, lookup = LEGS[leg]
    cls = hip_ops.OnDemandCorrBlock if corr == "on_demand" else hip_ops.CorrBlock
    kw = {"lookup": lookup} if corr == "on_demand" else {}

    def once():
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        blk = cls(a, b, num_levels=4, radius=4, **kw)
        loss = sum((blk(c) * g).sum() for c, g in zip(coords, gos))
        loss.backward()

    with RouteRecorder() as routes:
        once()
    timer = profiling.DispatchTimer(PLANS[leg])
    core.set_dispatch_timer(timer)
    try:
        for _ in range(3):
            once()
    finally:
        core.set_dispatch_timer(None)
    return {k: round(v[0], 2) for k, v in timer.summary().items()}, routes.shares()


def closures(legs, h, w, dev, reps):
    """{leg: closure times, peak memory, route shares}: one stepper per leg, the legs alternated rep by rep."""
    import bench
    from pcfa_amd import config as pcfa_config
    steppers, res = {}, {}
    for leg in legs:
        corr, lookup = LEGS[leg]
        config = dataclasses.replace(pcfa_config.DEFAULT, corr=corr, ondemand_lookup=lookup)
        model = bench.load_model("RAFT", dev, True, config)
        st = bench.AttackStepper("RAFT", h, w, dev, 0, use_graph=False, model=model)
        st.optimizer.zero_grad()
        with RouteRecorder() as routes:          # the warm-up closure: RAFT's own coordinates, all iterations
            st.closure_body()
        torch.cuda.synchronize()
        steppers[leg] = st
        res[leg] = {"ms": [], "peak": 0, "closure_route_matrix_share": routes.shares()}
    for _ in range(reps):
        for leg, st in steppers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.optimizer.zero_grad()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0.record()
            st.closure_body()
            e1.record()
            torch.cuda.synchronize()
            res[leg]["ms"].append(e0.elapsed_time(e1))
            # the other legs' models and leaves are resident: report this closure's own growth over them
            res[leg]["peak"] = max(res[leg]["peak"], torch.cuda.max_memory_allocated() - base)
    out = {}
    for leg, r in res.items():
        ms = sorted(r["ms"])
        out[leg] = {"closure_ms_median": round(ms[len(ms) // 2], 2), "closure_ms_min": round(ms[0], 2),
                    "closure_ms_max": round(ms[-1], 2), "closure_peak_growth_gb": round(r["peak"] / 1e9, 3)}
        if r["closure_route_matrix_share"] is not None:
            out[leg]["closure_route_matrix_share"] = r["closure_route_matrix_share"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="436x1024,1088x1920")
    ap.add_argument("--od-only", default="2160x3840")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    runs = [(s, ("all_pairs", "on_demand", "on_demand_tiled")) for s in a.sizes.split(",") if s]
    runs += [(s, ("on_demand", "on_demand_tiled")) for s in a.od_only.split(",") if s]
    lines = []
    for size, legs in runs:
        h, w = (int(v) for v in size.split("x"))
        H, W = (h + 7) // 8, (w + 7) // 8   # the padded input's feature map
        recs = {}
        for leg in legs:
            corr, lookup = LEGS[leg]
            recs[leg] = {"size": size, "corr": corr, "ondemand_lookup": lookup, "features": "%dx%d" % (H, W)}
            recs[leg]["kernel_us"], shares = corr_kernels(leg, H, W, dev)
            if shares is not None:
                recs[leg]["replay_route_matrix_share"] = shares
            torch.cuda.empty_cache()
        for leg, r in closures(legs, h, w, dev, max(2, a.reps if h * w < 4e6 else 2)).items():
            recs[leg].update(r)
        torch.cuda.empty_cache()
        for leg in legs:
            print(json.dumps(recs[leg]), flush=True)
            lines.append(recs[leg])
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench.jsonl"), "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
