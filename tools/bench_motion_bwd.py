#!/usr/bin/env python3
"""The motion encoder's two 3x3 data gradients (conv: 126 -> 256, convc2: 192 -> 256, at 55x128) per iteration and batched
over 12 iterations: per-launch device durations (HIP activity tracer) of >= 200 launches after >= 50 warm-up launches,
min / median / mean.

  dense     pcfa_conv3x3_run at B = 1 and B = 12, dense, without and with the deferred-ReLU mask (and the 64-tile variant
            at B = 12): expected closure gain = 12 x sum over the two layers of (t_B1 - t_B12 / 12)
  strided   the two launches of ops.corr._MotionFlush as the closure issues them: pcfa_conv3x3_run_strided over the slabs,
            192 live channels of d cf.  PCFA_XCD_MAP_MIN=256 / PCFA_CONV3X3_MT=2 in the environment select the placement.
usage: bench_motion_bwd.py dense|strided [label]"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcfa_amd.ops import conv as C  # noqa: E402
from pcfa_amd.ops.core import _call, _ptr  # noqa: E402

DEV = torch.device("cuda", 0)
H, W, ITERS = 55, 128, 12


def durations(fn, iters=200, warm=50):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    names, d = set(), []
    for ev in prof.events():
        if ev.device_type == DeviceType.CUDA:
            names.add(ev.name[:70])
            d.append(ev.time_range.elapsed_us())
    return d, sorted(names)


def _bwd_packed(K, N):
    w = torch.randn(K, N, 3, 3, device=DEV) / (9 * K) ** .5    # the layer's forward weight [Cout = K][Cin = N]
    return C._conv3x3_packed(w)[1]


def dense():
    med = {}
    for K, N in ((126, 256), (192, 256)):
        bwd = _bwd_packed(K, N)
        for B in (1, ITERS):
            for masked in (0, 1):
                for mt in (1, 2) if B > 1 else (1,):
                    x = torch.randn(B, K, H, W, device=DEV)
                    m = torch.randn(B, N, H, W, device=DEV) if masked else None
                    out = torch.empty(B, N, H, W, device=DEV)
                    if mt == 2:
                        os.environ["PCFA_CONV3X3_MT"] = "2"
                    else:
                        os.environ.pop("PCFA_CONV3X3_MT", None)
                    d, names = durations(lambda: C._conv3x3_run(DEV, _ptr(x), bwd, None, _ptr(m), None, _ptr(out), B, K, N, H, W))
                    med[(K, B, masked, mt)] = statistics.median(d)
                    print("K %3d -> N %3d B %2d mask %d MT %d : min %7.1f median %7.1f mean %7.1f us over %d launches "
                          "(per image: median %6.1f)  %s" % (K, N, B, masked, mt, min(d), statistics.median(d),
                                                             statistics.mean(d), len(d), statistics.median(d) / B, names),
                          flush=True)
    os.environ.pop("PCFA_CONV3X3_MT", None)
    for masked in (0, 1):
        for mt in (1, 2):
            gain = ITERS * sum(med[(K, 1, masked, 1)] - med[(K, ITERS, masked, mt)] / ITERS for K in (126, 192))
            print("expected closure gain (mask %d, B = %d with MT %d): %.1f us" % (masked, ITERS, mt, gain))


def strided(label):
    B, plane = ITERS, H * W
    bwd_c, bwd_c2 = _bwd_packed(126, 256), _bwd_packed(192, 256)
    d_rest = torch.randn(B, 128, H, W, device=DEV)
    cf, cor1 = torch.randn(B, 256, H, W, device=DEV), torch.randn(B, 256, H, W, device=DEV)
    d_cf, d_cor1 = torch.empty(B, 192, H, W, device=DEV), torch.empty(B, 256, H, W, device=DEV)
    z = ctypes.c_size_t(0)

    def conv():
        _call("pcfa_conv3x3_run_strided", _ptr(d_rest), 128 * plane, _ptr(bwd_c), None, _ptr(cf), 256 * plane, None, 0,
              _ptr(d_cf), 192 * plane, B, 126, 192, H, W, 0, 0., 0, None, z)

    def convc2():
        _call("pcfa_conv3x3_run_strided", _ptr(d_cf), 192 * plane, _ptr(bwd_c2), None, _ptr(cor1), 256 * plane, None, 0,
              _ptr(d_cor1), 256 * plane, B, 192, 256, H, W, 0, 0., 0, None, z)

    tot = 0.0
    for name, fn in (("conv   126 -> 192 live (of 256)", conv), ("convc2 192 -> 256", convc2)):
        d, names = durations(fn)
        tot += statistics.median(d)
        print("[%s] %s B %d: min %7.1f median %7.1f mean %7.1f us over %d launches  %s"
              % (label, name, B, min(d), statistics.median(d), statistics.mean(d), len(d), names), flush=True)
    print("[%s] sum of medians %.1f us per closure" % (label, tot))


if __name__ == "__main__":
    torch.manual_seed(0)
    if len(sys.argv) > 1 and sys.argv[1] == "strided":
        strided(sys.argv[2] if len(sys.argv) > 2 else "default")
    else:
        dense()
