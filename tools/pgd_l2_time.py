#!/usr/bin/env python
"""Device time of the three launches of pcfa_pgd_l2_step (`--step_norm l2`) next to pcfa_fgsm_step, in ONE session with the
calibration copy: 3 x 440 x 1024 floats per array (RAFT's padded 436x1024 image), dispatch-packet timestamps
(ops.profiling.DispatchTimer), 30 steps per row after 3 untimed ones.

    warm         steps back to back: the eight arrays (43 MB) stay in the caches
    cold         a float4 copy of 512 MiB before every step, as a network forward and backward lie between two steps of
                 the attack
    projecting   bound 0.003 under epsilon 0.002: the third launch rewrites x and d
    inside       bound 1: s = 1, the third launch returns at once

Prints one JSON object: microseconds per launch, the bytes each launch moves, GB/s.

    python tools/pgd_l2_time.py > profiles/pgd_l2/launch_times.json
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PLAN = {"pcfa_pgd_l2_step": [("gsq", 0), ("step", 1), ("project", 2)], "pcfa_fgsm_step": [("fgsm_step", 0)]}
COPY_FLOATS = 128 * 1024 * 1024      # the calibration copy of bench.py: 512 MiB


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="440x1024", help="HxW of the (padded) image; three channels")
    ap.add_argument("--reps", type=int, default=30)
    opt = ap.parse_args(argv)

    import torch
    from pcfa_amd import _hip, hip_ops, ops
    from pcfa_amd.ops.profiling import DispatchTimer

    dev = torch.device("cuda")
    lib = _hip.load()
    h, w = (int(v) for v in opt.size.lower().split("x"))
    n = 3 * h * w
    gen = torch.Generator(device="cuda").manual_seed(1)
    img = [torch.rand(n, device=dev, generator=gen) for _ in range(2)]
    grad = [torch.randn(n, device=dev, generator=gen) * 1e-3 for _ in range(2)]
    x = [(i + 0.001 * torch.randn(n, device=dev, generator=gen)).clamp_(0, 1) for i in img]
    d = [torch.empty(n, device=dev) for _ in range(2)]
    src, dst = torch.rand(COPY_FLOATS, device=dev), torch.empty(COPY_FLOATS, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy_big():
        _hip.check(lib.pcfa_calib_copy(src.data_ptr(), dst.data_ptr(), COPY_FLOATS, stream), "pcfa_calib_copy")

    def bracket(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    out = {"n_floats_per_array": n, "array_MB": 4 * n / 1e6}
    out["calib_copy_512MiB_GBs"] = 2 * 4 * COPY_FLOATS / bracket(copy_big, 3) / 1e9

    def run(label, fn, cold):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        timer = DispatchTimer(PLAN)
        for _ in range(opt.reps):
            if cold:
                copy_big()
            ops.core.set_dispatch_timer(timer)
            fn()
            ops.core.set_dispatch_timer(None)
        out[label] = {k: round(v[0], 2) for k, v in timer.summary().items()}

    def l2(bound):
        return lambda: hip_ops.pgd_l2_step(x[0], x[1], grad[0], grad[1], img[0], img[1], d[0], d[1], 0.002, bound, False)

    def sign():
        hip_ops.fgsm_step(x[0], x[1], grad[0], grad[1], img[0], img[1], d[0], d[1], 0.00025, False)

    for cold in (False, True):
        tag = "cold" if cold else "warm"
        run("l2_projecting_%s_us" % tag, l2(0.003), cold)
        out["l2_projecting_%s_s" % tag] = hip_ops.pgd_l2_workspace(dev)[3].item()
        run("l2_inside_%s_us" % tag, l2(1.0), cold)
        out["l2_inside_%s_s" % tag] = hip_ops.pgd_l2_workspace(dev)[3].item()
        run("sign_%s_us" % tag, sign, cold)

    nbytes = {"gsq": 2 * 4 * n, "step": 10 * 4 * n, "project": 8 * 4 * n, "fgsm_step": 10 * 4 * n}
    out["bytes"] = nbytes
    for key in ("l2_projecting_warm_us", "l2_projecting_cold_us", "sign_warm_us", "sign_cold_us"):
        out[key.replace("_us", "_GBs")] = {k: round(nbytes[k] / (v * 1e-6) / 1e9, 1) for k, v in out[key].items()}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
