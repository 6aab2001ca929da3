"""What reading the datasets from disk costs: the parts of one sample, and pair-steps/s of the per-pair PCFA driver fed from
files against `--dataset Synthetic`.

    python tools/bench_dataset_load.py [--rounds 3] [--parent DIR] [--out FILE.jsonl] [--keep DIR]

Files.  Written first, from SyntheticPairs (the same seeds the synthetic leg attacks), with the test-side encoder
(tests/png_cases.py): a Sintel-layout tree of `--pairs` scenes of two 436x1024 frames each (8-bit RGB, .flo ground truth)
and a KITTI-layout tree of four 375x1242 pairs (8-bit RGB frames, 16-bit flow PNGs).  Row y of every PNG uses filter type
1 + y % 4 -- Sub, Up, Average, Paeth in turn, so both recurrences are in every file.  The wavefront kernel's time does not
depend on the types; inflate time depends on how well the filtered bytes compress.

Per sample (`sample` leg, one process; warm-up, then `--repeats` runs; median, min, max): file read + inflate on the host,
the upload of the scanlines, the un-filter and the unpack kernel by device events, the one synchronise; and the whole
__getitem__ of both loaders (MpiSintel / KITTI against SyntheticPairs plus its copy to the device).

Per run (`files` / `synthetic` legs, a fresh process each, alternated round after round; `parent`: the synthetic leg in a
built checkout of the parent commit): attack_l2, PWC-Net, 20 steps, 8 pairs, 436x1024, no saving;
(pairs - 1) * steps / (time from the end of the first pair to the end of the last), which holds the loader's time for every
pair but the first.  Prints one JSON line per row and a summary with each leg's spread.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KITTI_PAIRS = 4


def _plan(h):
    return [1 + y % 4 for y in range(h)]


def write_files(root, pairs, size):
    """The two trees under root/sintel and root/kitti."""
    sys.path.insert(0, REPO)
    import numpy as np
    from pcfa_amd.helper_functions import datasets
    from tests import png_cases as P
    h, w = (int(v) for v in size.lower().split("x"))

    def u8(t):
        return np.ascontiguousarray(t.round().clamp(0, 255).byte().permute(1, 2, 0).numpy())
    for i in range(pairs):
        image1, image2, flow = datasets.synthetic_pair(i, h, w)
        scene = os.path.join(root, "sintel", "training", "final", "scene_%02d" % i)
        P.write(os.path.join(scene, "frame_0001.png"), u8(image1), "rgb8", _plan(h))
        P.write(os.path.join(scene, "frame_0002.png"), u8(image2), "rgb8", _plan(h))
        P.write_flo(os.path.join(root, "sintel", "training", "flow", "scene_%02d" % i, "frame_0001.flo"),
                    flow.permute(1, 2, 0).numpy())
    kh, kw = datasets.KITTI_SIZE
    for i in range(KITTI_PAIRS):
        image1, image2, flow = datasets.synthetic_pair(100 + i, kh, kw)
        base = os.path.join(root, "kitti", "training")
        P.write(os.path.join(base, "image_2", "%06d_10.png" % i), u8(image1), "rgb8", _plan(kh))
        P.write(os.path.join(base, "image_2", "%06d_11.png" % i), u8(image2), "rgb8", _plan(kh))
        samples = np.empty((kh, kw, 3), np.uint16)
        # the constant synthetic flow would deflate to nothing: the frame's own texture, up to 4 px, rides on it
        uv = flow + (image1[:2] - 127.5) / 32
        samples[..., :2] = (uv.permute(1, 2, 0).numpy() * 64 + 32768).round().astype(np.uint16)
        samples[..., 2] = 1
        P.write(os.path.join(base, "flow_occ", "%06d_10.png" % i), samples, "rgb16", _plan(kh))


def _stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def sample_leg(a):
    """The parts of one file, and one __getitem__ of each loader; times in milliseconds."""
    sys.path.insert(0, os.getcwd())
    import glob
    import torch
    from pcfa_amd import hip_ops
    from pcfa_amd.helper_functions import datasets, png
    dev = torch.device("cuda")
    h, w = (int(v) for v in a.size.lower().split("x"))
    files = {"sintel_frame": (sorted(glob.glob(os.path.join(a.files, "sintel", "training", "final", "*", "*.png"))), "rgb8",
                              None),
             "kitti_frame": (sorted(glob.glob(os.path.join(a.files, "kitti", "training", "image_2", "*.png"))), "rgb8",
                             datasets.KITTI_SIZE),
             "kitti_flow": (sorted(glob.glob(os.path.join(a.files, "kitti", "training", "flow_occ", "*.png"))),
                            "kitti_flow16", datasets.KITTI_SIZE)}
    for name, (paths, kind, pad_to) in files.items():
        parts = {k: [] for k in ("read_inflate", "upload", "unfilter_kernel", "unpack_kernel", "synchronise")}
        size = filtered_bytes = 0
        for run in range(a.warmup + a.repeats):
            path = paths[run % len(paths)]
            t0 = time.perf_counter()
            with open(path, "rb") as f:
                data = f.read()
            pw, ph, depth, ctype, scan = png.decode_header_and_scanlines(data)
            t1 = time.perf_counter()
            host = torch.frombuffer(bytearray(scan), dtype=torch.uint8)
            filtered = host.to(dev)
            torch.cuda.current_stream().synchronize()
            t2 = time.perf_counter()
            bpp = png.FORMATS[(ctype, depth)][0]
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            hp, wp = pad_to or (ph, pw)
            e[0].record()
            raw = hip_ops.png_unfilter(filtered, ph, pw * bpp, bpp)
            e[1].record()
            e[2].record()
            hip_ops.samples_to_planar(raw, ph, pw, kind, hp, wp)
            e[3].record()
            t3 = time.perf_counter()
            torch.cuda.current_stream().synchronize()
            t4 = time.perf_counter()
            if run >= a.warmup:
                parts["read_inflate"].append(1e3 * (t1 - t0))
                parts["upload"].append(1e3 * (t2 - t1))
                parts["unfilter_kernel"].append(e[0].elapsed_time(e[1]))
                parts["unpack_kernel"].append(e[2].elapsed_time(e[3]))
                parts["synchronise"].append(1e3 * (t4 - t3))
            size, filtered_bytes = len(data), len(scan)
        print("SAMPLE " + json.dumps({"file": name, "file_bytes": size, "inflated_bytes": filtered_bytes, "runs": a.repeats,
                                      "ms": {k: _stats(v) for k, v in parts.items()}}), flush=True)
    loaders = {"MpiSintel": datasets.MpiSintel("training", os.path.join(a.files, "sintel"), "final", True, dev),
               "KITTI": datasets.KITTI("training", os.path.join(a.files, "kitti"), True, dev),
               "SyntheticPairs": datasets.SyntheticPairs(a.pairs, h, w)}
    # Sintel's ground truth is no PNG: the .flo file's read, transpose, valid mask and the two uploads, all on the host
    sintel, times = loaders["MpiSintel"], []
    for run in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        sintel.read_flow(sintel.flow_list[run % len(sintel)])
        torch.cuda.synchronize()
        if run >= a.warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    print("SAMPLE " + json.dumps({"file": "sintel_flo", "file_bytes": os.path.getsize(sintel.flow_list[0]), "runs": a.repeats,
                                  "ms": {"read_transpose_valid_upload": _stats(times)}}), flush=True)
    for name, ds in loaders.items():
        times = []
        for run in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            sample = ds[run % len(ds)]
            if name == "SyntheticPairs":
                sample = [t.to(dev) for t in sample]   # (what the drivers' .to(device) does with a host sample)
            torch.cuda.synchronize()
            if run >= a.warmup:
                times.append(1e3 * (time.perf_counter() - t0))
        print("SAMPLE " + json.dumps({"loader": name, "runs": a.repeats, "ms_per_pair": _stats(times)}), flush=True)


def run_leg(a):
    sys.path.insert(0, os.getcwd())
    import torch
    from pcfa_amd import attack_PCFA
    from pcfa_amd.helper_functions import parsing_file
    argv = ["--net", a.net, "--weights", "random:1234", "--steps", str(a.steps), "--no_save"]
    if a.leg == "files":
        argv += ["--dataset", "Sintel", "--dataset_stage", "training", "--dstype", "final", "--dataset_root",
                 os.path.join(a.files, "sintel")]
    else:
        argv += ["--dataset", "Synthetic", "--synthetic_pairs", str(a.pairs), "--synthetic_size", a.size]
    args = parsing_file.create_parser(stage="training", attack_type="pcfa").parse_args(argv)
    ends = []
    inner = attack_PCFA.pcfa_attack

    def timed(*p, **kw):
        res = inner(*p, **kw)
        torch.cuda.synchronize()
        ends.append(time.perf_counter())
        return res
    attack_PCFA.pcfa_attack = timed
    res = attack_PCFA.attack_l2(args)
    n = len(ends)
    row = {"leg": a.leg, "net": a.net, "size": a.size, "steps": a.steps, "pairs": n,
           "pair_steps_per_s": (n - 1) * a.steps / (ends[-1] - ends[0]), "s_per_pair": (ends[-1] - ends[0]) / (n - 1),
           "aee_min": res["aee_avg_predadv-tgt_min"]}
    print("LEG " + json.dumps(row), flush=True)


def _child(a, leg, cwd, files):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--net", a.net, "--steps", str(a.steps), "--pairs",
           str(a.pairs), "--size", a.size, "--files", files, "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.leg_timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(("LEG ", "SAMPLE "))]
    if p.returncode != 0 or not lines:
        print(p.stdout[-3000:])
        raise SystemExit("leg %s failed with status %d" % (leg, p.returncode))
    return [json.loads(ln.split(" ", 1)[1]) for ln in lines]


def drive(a):
    files = a.keep or tempfile.mkdtemp(prefix="dataset_load_")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    try:
        t0 = time.perf_counter()
        write_files(files, a.pairs, a.size)
        print("files written in %.1f s under %s" % (time.perf_counter() - t0, files), flush=True)
        for row in _child(a, "sample", REPO, files):
            emit(row)
        legs = (["parent"] if a.parent else []) + ["synthetic", "files"]
        for rnd in range(a.rounds):
            for leg in legs:
                cwd = os.path.abspath(a.parent) if leg == "parent" else REPO
                for row in _child(a, "synthetic" if leg == "parent" else leg, cwd, files):
                    emit(dict(row, leg=leg, round=rnd))
        for leg in legs if a.rounds else []:
            v = sorted(r["pair_steps_per_s"] for r in rows if r.get("leg") == leg)
            print("SUMMARY %s %s: median %.3f pair-steps/s, min %.3f, max %.3f (spread %.2f %%)"
                  % (a.net, leg, v[len(v) // 2], v[0], v[-1], 100 * (v[-1] - v[0]) / v[len(v) // 2]), flush=True)
    finally:
        if not a.keep:
            shutil.rmtree(files, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="PWCNet")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--size", default="436x1024")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20, help="timed runs per part of the sample leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (its own synthetic leg)")
    ap.add_argument("--out", default="")
    ap.add_argument("--keep", default="", help="write the files here and keep them")
    ap.add_argument("--files", default="", help="(legs) where the driver wrote the files")
    ap.add_argument("--leg", default="", choices=["", "sample", "files", "synthetic"],
                    help="run ONE leg in this process, tree = the working directory")
    ap.add_argument("--leg_timeout", type=int, default=300)
    a = ap.parse_args()
    if a.leg == "sample":
        sample_leg(a)
    elif a.leg:
        run_leg(a)
    else:
        drive(a)


if __name__ == "__main__":
    main()
