#!/usr/bin/env python3
"""Dump the lookup coordinates of ONE RAFT closure (the tensors the pyramid's windowed backward is given) and the matrix
work its two sparse products report, for tools/pyramid_bwd_segments.py.  usage: dump_closure_coords.py OUT.npz [HxW]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    from pcfa_amd.ops import core, hip
    out = sys.argv[1]
    h, w = (int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "436x1024").split("x"))
    made = []
    make = hip.motion_steps

    def recording(*a, **k):
        steps = make(*a, **k)
        made.append(steps)
        return steps

    hip.motion_steps = recording
    st = bench.AttackStepper("RAFT", h, w, torch.device("cuda", 0), seed=0)
    st.optimizer.zero_grad()
    st._closure_body()          # warm-up: caches, packed weights
    del made[:]
    work = {}
    core.set_work_recorder(work)
    st.optimizer.zero_grad()
    st._closure_body()
    torch.cuda.synchronize()
    core.set_work_recorder(None)
    hip.motion_steps = make
    ms = made[-1]._ms
    corr = ms.corr
    coords = torch.stack([c for c in ms.coords]).cpu().numpy()      # [lookups, B, 2, H, W]
    np.savez_compressed(out, coords=coords, radius=corr.r, levels=corr.L, D=corr.D,
                        issued_dfmap1=work["corr_pyramid_gemm_dfmap1"][1], issued_df2ext=work["corr_pyramid_gemm_df2ext"][1])
    print("%s: %d lookups of %s, dfmap1 %.3f / df2ext %.3f GFLOP issued" % (
        out, coords.shape[0], tuple(coords.shape[1:]), work["corr_pyramid_gemm_dfmap1"][1] * 1e-9,
        work["corr_pyramid_gemm_df2ext"][1] * 1e-9))


if __name__ == "__main__":
    main()
