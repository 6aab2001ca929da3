#!/usr/bin/env python3
"""Per-launch medians of pcfa_corr_pyramid_bwd_windows's kernels at the coordinates of a real closure.
usage: bench_pyramid_bwd.py DUMP.npz [reps]     (DUMP from tools/dump_closure_coords.py; PCFA_HIP_LIB picks the build)
The calls run back to back, so dpyr is as warm in the caches as it can be: compare builds, not against the closure."""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from pcfa_amd import _hip
    from pcfa_amd.ops.core import _call, _ptr
    d = np.load(sys.argv[1])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    coords, r, L, D = d["coords"].astype(np.float32), int(d["radius"]), int(d["levels"]), int(d["D"])
    n, B, _, H, W = coords.shape
    dev = torch.device("cuda", 0)
    lib = _hip.load()
    slab, Q = int(lib.pcfa_corr_slab_floats(H, W, L)), H * W
    cs = [torch.from_numpy(c).to(dev).contiguous() for c in coords]
    gen = torch.Generator(device=dev).manual_seed(0)
    dpyr = torch.randn(B * Q, slab, device=dev, generator=gen)
    f1, f2e = torch.randn(B, D, Q, device=dev, generator=gen), torch.randn(B, D, slab, device=dev, generator=gen)
    df1, df2 = torch.empty_like(f1), torch.empty_like(f1)
    nbytes = lib.pcfa_corr_pyramid_bwd_windows_workspace_bytes(B, D, H, W, L)
    ws = torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * n)(*[c.data_ptr() for c in cs])

    def call():
        _call("pcfa_corr_pyramid_bwd_windows", _ptr(dpyr), _ptr(f1), _ptr(f2e), _ptr(df1), _ptr(df2), _ptr(ws),
              ctypes.c_size_t(nbytes), ptrs, n, r, B, D, H, W, L)

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
    acc = {}
    for ev in prof.events():
        if ev.device_type == DeviceType.CUDA:
            acc.setdefault(ev.name.replace("(anonymous namespace)::", "").split("(")[0][-60:], []).append(ev.time_range.elapsed_us())
    tot = 0.0
    for k, v in acc.items():
        per = len(v) // reps
        med = statistics.median(v)
        tot += med * per
        print("%-62s x%d  median %7.1f us  min %7.1f  max %7.1f" % (k, per, med, min(v), max(v)))
    print("sum of medians per call: %.1f us (%d calls)" % (tot, reps))


if __name__ == "__main__":
    main()
