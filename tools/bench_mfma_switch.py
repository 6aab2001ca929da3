#!/usr/bin/env python3
"""Config.mfma = "f32" against "bf16x3" at closure level: median device time of one eager closure of a seeded attack
pair, for GMA and RAFT, for the builds

    default                                  (gma_gemm = conv1x1 = "lib", mfma = "f32")
    hip/f32      gma_gemm = conv1x1 = "hip",  mfma = "f32"
    hip/bf16x3   gma_gemm = conv1x1 = "hip",  mfma = "bf16x3"
    lib/bf16x3   the default with mfma = "bf16x3" (only the pyramid forward changes)
    parent       the default build of ANOTHER checkout of this repository (--parent-tree DIR, built there)

ALTERNATED rep by rep in one session and timed with device events after one warm-up closure each, the way
tools/bench_gma_attention.py takes its closure times.  The other checkout cannot share a process with this one (same
package name, another library), so every tree gets one worker process that keeps its models resident; the driver asks
the workers for one closure at a time, in turn.

    python tools/bench_mfma_switch.py [--nets GMA,RAFT] [--size 436x1024] [--reps 9] [--parent-tree DIR] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"default": {},
          "hip/f32": dict(gma_gemm="hip", conv1x1="hip", mfma="f32"),
          "hip/bf16x3": dict(gma_gemm="hip", conv1x1="hip", mfma="bf16x3"),
          "lib/bf16x3": dict(mfma="bf16x3")}


def worker(tree):
    """Serve 'load <net> <h> <w> <build>' and 'run <net> <build>' lines from stdin; one JSON line per answer."""
    sys.path.insert(0, tree)
    os.chdir(tree)
    import torch
    import bench
    from pcfa_amd import config as pcfa_config
    dev = torch.device("cuda")
    steppers = {}
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "load":
            net, h, w, build = cmd[1], int(cmd[2]), int(cmd[3]), cmd[4]
            config = dataclasses.replace(pcfa_config.DEFAULT, **BUILDS.get(build, {}))
            model = bench.load_model(net, dev, True, config)
            st = bench.AttackStepper(net, h, w, dev, 0, use_graph=False, model=model)
            st.optimizer.zero_grad()
            st.closure_body()          # warm-up
            torch.cuda.synchronize()
            steppers[(net, build)] = st
            print(json.dumps({"ok": True}), flush=True)
        elif cmd[0] == "run":
            st = steppers[(cmd[1], cmd[2])]
            st.optimizer.zero_grad()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.closure_body()
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({"ms": e0.elapsed_time(e1)}), flush=True)


class Worker:
    def __init__(self, tree):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        while True:
            out = self.p.stdout.readline()
            if not out:
                raise RuntimeError("worker ended (exit %s) on: %s" % (self.p.poll(), line))
            if out.startswith("{"):
                return json.loads(out)

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.close()
        except OSError:
            pass
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default="")
    ap.add_argument("--nets", default="GMA,RAFT")
    ap.add_argument("--size", default="436x1024")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    h, w = (int(v) for v in a.size.split("x"))
    mine = Worker(HERE)
    parent = Worker(os.path.abspath(a.parent_tree)) if a.parent_tree else None
    lines = []
    try:
        for net in a.nets.split(","):
            plan = [(mine, b) for b in BUILDS] + ([(parent, "parent")] if parent else [])
            for wk, b in plan:
                wk.ask("load %s %d %d %s" % (net, h, w, b))
            ms = {b: [] for _, b in plan}
            for _ in range(a.reps):            # the builds alternate rep by rep
                for wk, b in plan:
                    ms[b].append(wk.ask("run %s %s" % (net, b))["ms"])
            base = sorted(ms["default"])[len(ms["default"]) // 2]
            for b, v in ms.items():
                v = sorted(v)
                rec = {"net": net, "size": a.size, "build": b, "reps": len(v), "closure_ms_median": round(v[len(v) // 2], 3),
                       "closure_ms_min": round(v[0], 3), "closure_ms_max": round(v[-1], 3),
                       "ratio_to_default": round(v[len(v) // 2] / base, 4)}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        mine.close()
        if parent:
            parent.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
