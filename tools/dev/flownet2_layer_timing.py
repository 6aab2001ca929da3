#!/usr/bin/env python3
"""Device time of FlowNet2's 5x5 stride-2 layers and deconvolutions at 448x1024 on the flownet2_ops = "hip" kernels
(ops.conv_s2_leaky, ops.deconv4s2_leaky), forward and data gradient, as GFLOP/s and share of the fp32 matrix peak
(157.3 TFLOP/s).  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel view; the numbers printed here are
hipEvent times of REPS back-to-back launches."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from pcfa_amd import hip_ops  # noqa: E402

PEAK = 157.3e12
REPS = int(os.environ.get("REPS", "20"))
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
# (name, kind, Cin, Cout, k, input H, input W)
LAYERS = [("conv2 5x5 64->128", "s2", 64, 128, 5, 224, 512), ("conv3 5x5 128->256", "s2", 128, 256, 5, 112, 256),
          ("conv1 7x7 12->64", "s2", 12, 64, 7, 448, 1024),
          ("deconv5 1024->512", "dc", 1024, 512, 4, 7, 16), ("deconv4 1026->256", "dc", 1026, 256, 4, 14, 32),
          ("deconv3 770->128", "dc", 770, 128, 4, 28, 64), ("deconv2 386->64", "dc", 386, 64, 4, 56, 128),
          ("deconv1 128->32", "dc", 128, 32, 4, 112, 256), ("deconv0 162->16", "dc", 162, 16, 4, 224, 512)]


def timed(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e-3


print("%-22s %9s %9s %8s %9s %8s %6s" % ("layer", "GFLOP", "fwd_us", "fwd_pk", "dgrad_us", "dgrad_pk", ""))
for name, kind, cin, cout, k, H, W in LAYERS:
    x = torch.randn(1, cin, H, W, generator=g).to(dev).requires_grad_()
    b = torch.randn(cout, generator=g).to(dev)
    if kind == "s2":
        w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev)
        op = lambda: hip_ops.conv_s2_leaky(x, w, b, 0.1)   # noqa: E731
        oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        flop = 2.0 * cin * cout * k * k * oh * ow
    else:
        w = (torch.randn(cin, cout, 4, 4, generator=g) / (cin * 4) ** 0.5).to(dev)
        op = lambda: hip_ops.deconv4s2_leaky(x, w, b, 0.1)   # noqa: E731
        flop = 2.0 * cin * cout * 16 * H * W   # 4 taps per output pixel, 2H x 2W outputs
    y = op()
    gy = torch.randn(y.shape, device=dev)
    tf = timed(lambda: op())
    tb = timed(lambda: y.grad_fn.apply(gy))
    print("%-22s %9.2f %9.1f %7.1f%% %9.1f %7.1f%%" % (name, flop / 1e9, tf * 1e6, 100 * flop / tf / PEAK, tb * 1e6,
                                                      100 * flop / tb / PEAK))
