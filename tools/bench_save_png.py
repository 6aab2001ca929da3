"""What saving costs: pair-steps/s of the per-pair PCFA driver with artefacts on, `.npy` only against `--save_png`.

    python tools/bench_save_png.py --net RAFT --rounds 3 [--parent DIR] [--out FILE.jsonl]

Every leg is a fresh process that runs `attack_PCFA.attack_l2` on synthetic pairs (436x1024, 20 steps, 8 pairs by default)
into a temporary folder and reports (pairs - 1) * steps / (time from the end of the first pair to the end of the last):
the first pair pays for warm-up and graph capture, every later one for its steps and its save().  Legs are alternated,
round after round: `parent` (a built checkout of the parent commit given with --parent, saving on), `npy` (this tree,
saving on) and `png` (this tree, --save_png).  Prints one JSON line per leg and a summary with each leg's spread.
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


def run_leg(a):
    sys.path.insert(0, os.getcwd())
    import torch
    from pcfa_amd import attack_PCFA
    from pcfa_amd.helper_functions import parsing_file
    out = tempfile.mkdtemp(prefix="save_png_")
    argv = ["--net", a.net, "--dataset", "Synthetic", "--weights", "random:1234", "--steps", str(a.steps),
            "--synthetic_pairs", str(a.pairs), "--synthetic_size", a.size, "--output_folder", out]
    if a.leg == "png":
        argv += ["--save_png", "--png_flow_scale", a.flow_scale]
    args = parsing_file.create_parser(stage="training", attack_type="pcfa").parse_args(argv)
    ends = []
    inner = attack_PCFA.pcfa_attack

    def timed(*p, **kw):
        res = inner(*p, **kw)
        torch.cuda.synchronize()
        ends.append(time.perf_counter())
        return res
    attack_PCFA.pcfa_attack = timed
    try:
        attack_PCFA.attack_l2(args)
        files = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs]
        row = {"leg": a.leg, "net": a.net, "size": a.size, "steps": a.steps, "pairs": a.pairs,
               "pair_steps_per_s": (a.pairs - 1) * a.steps / (ends[-1] - ends[0]),
               "s_per_pair": (ends[-1] - ends[0]) / (a.pairs - 1),
               "files": len(files), "png_files": sum(f.endswith(".png") for f in files),
               "png_bytes": sum(os.path.getsize(f) for f in files if f.endswith(".png")),
               "npy_bytes": sum(os.path.getsize(f) for f in files if f.endswith(".npy"))}
    finally:
        shutil.rmtree(out, ignore_errors=True)
    print("LEG " + json.dumps(row), flush=True)


def drive(a):
    legs = (["parent"] if a.parent else []) + ["npy", "png"]
    rows = []
    for rnd in range(a.rounds):
        for leg in legs:
            cwd = os.path.abspath(a.parent) if leg == "parent" else REPO
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "npy" if leg == "parent" else leg, "--net", a.net,
                   "--steps", str(a.steps), "--pairs", str(a.pairs), "--size", a.size, "--flow_scale", a.flow_scale]
            p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.leg_timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-3000:])
                raise SystemExit("leg %s failed with status %d" % (leg, p.returncode))
            row = dict(json.loads(line[-1][4:]), leg=leg, round=rnd)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
    for leg in legs:
        v = sorted(r["pair_steps_per_s"] for r in rows if r["leg"] == leg)
        print("SUMMARY %s %s: median %.3f pair-steps/s, min %.3f, max %.3f (spread %.2f %%)"
              % (a.net, leg, v[len(v) // 2], v[0], v[-1], 100 * (v[-1] - v[0]) / v[len(v) // 2]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="RAFT")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--size", default="436x1024")
    ap.add_argument("--flow_scale", default="own")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (its own leg)")
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="", choices=["", "npy", "png"], help="run ONE leg in this process, tree = the working directory")
    ap.add_argument("--leg_timeout", type=int, default=240)
    a = ap.parse_args()
    if a.leg:
        run_leg(a)
    else:
        drive(a)


if __name__ == "__main__":
    main()
