#!/usr/bin/env python3
"""The GEMM core at the shapes of the path, three ways on the same operands: pcfa_gemm_f32 (fp32 MFMA), pcfa_gemm_bf16x3
(split-bf16 MFMA, Config.mfma = "bf16x3") and torch.matmul (rocBLAS).  Device time from the HIP activity tracer, the three
columns alternated rep by rep; rel-L2 of each result against float64 (computed on the device from the same fp32
operands, on a slice of the output rows where the full product would be slow).

    python tools/bench_gemm.py [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcfa_amd import hip_ops  # noqa: E402

U = 2.0 ** -24


def dev_times(fns, reps):
    """Median device microseconds per call of each fn; the fns alternate rep by rep, one profiler pass per call."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            out[i].append(sum(ev.time_range.elapsed_us() for ev in prof.events() if ev.device_type == DeviceType.CUDA))
    return [(sorted(v)[len(v) // 2], min(v), max(v)) for v in out]


def rel_l2_vs_float64(c, at, bt, rows=512):
    """rel-L2 of c against the float64 product, in units of u, over `rows` evenly spaced output rows."""
    idx = torch.linspace(0, at.shape[0] - 1, min(rows, at.shape[0]), device=c.device).long()
    want = at[idx].double() @ bt.double()
    return float((c[idx].double() - want).norm() / want.norm()) / U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    Q = 7040
    cases = [("pyramid fwd  fmap1^T f2ext", (256, Q), (256, 9616), 1, 1, 1),
             ("sim  q k^T", (Q, 128), (Q, 128), 0, 0, 1),
             ("attn v", (Q, Q), (Q, 128), 0, 1, 8),
             ("attn^T g", (Q, Q), (Q, 128), 1, 1, 8),
             ("d_attn [g|..] [v|..]^T", (Q, 768), (Q, 768), 0, 0, 1)]
    lines = []
    print("%-28s %5s %5s %5s  %-25s %-25s %-25s  rel-L2 / u (f32, bf16x3, rocBLAS)" %
          ("product", "M", "N", "K", "pcfa_gemm_f32", "pcfa_gemm_bf16x3", "rocBLAS"))
    for name, sa, sb, akm, bkn, splits in cases:
        a = torch.randn(*sa, generator=g).to(dev)
        b = torch.randn(*sb, generator=g).to(dev)
        M = sa[1] if akm else sa[0]
        K = sa[0] if akm else sa[1]
        N = sb[1] if bkn else sb[0]
        at = a.t() if akm else a
        bt = b if bkn else b.t()
        fns = [lambda: hip_ops.gemm_f32(a, b, akm, bkn, splits=splits),
               lambda: hip_ops.gemm_f32(a, b, akm, bkn, splits=splits, mfma="bf16x3"),
               lambda: torch.matmul(at, bt)]
        t = dev_times(fns, args.reps)
        err = [rel_l2_vs_float64(fn(), at, bt) for fn in fns]
        fl = 2.0 * M * N * K
        rec = {"product": name, "M": M, "N": N, "K": K, "splits": splits}
        for col, (med, lo, hi), e in zip(("f32", "bf16x3", "lib"), t, err):
            rec[col] = {"us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                        "tflops": round(fl / med / 1e6, 1), "rel_l2_over_u": round(e, 2)}
        lines.append(rec)
        print("%-28s %5d %5d %5d  " % (name, M, N, K) +
              " ".join("%7.1f us (%5.1f TFLOP/s) " % (rec[c]["us_median"], rec[c]["tflops"]) for c in ("f32", "bf16x3", "lib")) +
              "  %.2f  %.2f  %.2f" % tuple(err), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
