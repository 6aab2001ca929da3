"""Writes tests/golden/flow_colour.npz: a handful of small flows and what the reference's colorplot_light makes of them.

    python tests/golden/make_artefact_golden.py /path/to/reference

Needs a checkout of the reference (its flow_library goes on sys.path; nothing of it is copied): run where one exists, and
commit the .npz.  The file holds data only: float32 flows [H,W,2], the forced scales, and the reference's uint8 pictures,
auto-scaled and at the forced scale, computed in float64 (the flows are widened before the call).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import artefacts  # noqa: E402


def flows():
    normal = artefacts.normal_flow(3, 8, 12, seed=7)
    grid = artefacts.integer_grid()
    holes = artefacts.with_nans(artefacts.normal_flow(1, 6, 5, seed=8), seed=8)
    out = [normal[0], normal[1], normal[2], grid[0], grid[1], holes[0], np.zeros((2, 3, 4), np.float32),
           artefacts.bin_centres()[0]]
    return [np.ascontiguousarray(np.transpose(f, (1, 2, 0))) for f in out]     # [H,W,2] as colorplot_light takes it


def main(reference):
    sys.path.insert(0, os.path.join(reference, "flow_library"))
    from flow_plot import colorplot_light
    data = {}
    for i, f in enumerate(flows()):
        wide = f.astype(np.float64)
        with np.errstate(invalid="ignore"):
            length = np.sqrt(np.square(wide[..., 0]) + np.square(wide[..., 1]))
        forced = float(np.nanmax(length)) / 2 if np.nanmax(length) > 0 else 1.0
        data["flow_%d" % i] = f
        data["forced_scale_%d" % i] = np.float64(forced)
        data["rgb_auto_%d" % i] = colorplot_light(wide.copy(), auto_scale=True)
        data["rgb_forced_%d" % i] = colorplot_light(wide.copy(), auto_scale=False, max_scale=forced)
    path = os.path.join(HERE, "flow_colour.npz")
    np.savez_compressed(path, **data)
    print("%s: %d flows, %d bytes" % (path, len(flows()), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
