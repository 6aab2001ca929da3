#!/usr/bin/env python
"""Pair-steps/s of the per-pair PCFA attack with several pairs on one GPU, leg against leg in ONE process.

The model is built once per network; one rep of every leg follows one rep of the next (A B C D A B C D ...), so clock and
thermal drift fall on all legs alike.  A rep attacks whole pairs the way the driver does -- construction (upload, unattacked
flow, target; the graph set is captured by an untimed first rep and adopted afterwards, as by every later pair of a
dataset), `--steps` attack steps, a device synchronisation; pair-steps/s = pairs x steps / wall time.  Legs:

    solo      one PairAttack (the default path)
    lanes N   N pairs in flight (attack_PCFA.PairsInFlight: one host thread, stream and graph set per pair); a build that
              lanes refuse is reported as refused
    B = N     N pairs in one batched closure (attack_PCFA.PairBatch, --pairs_per_closure N)

Prints (and with --out appends) one JSON line per (network, leg): median, min and max of pair-steps/s over the reps, every
rep's figure, and how much torch.cuda.max_memory_allocated grew over the leg's first (capturing) rep.

    python tools/bench_pairs_per_closure.py --nets RAFT PWCNet --lanes 2 --batches 2 4 --out bench.jsonl
    python tools/bench_pairs_per_closure.py --nets GMA --lanes 2 --batches 2 --out bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nets", nargs="+", default=["RAFT", "PWCNet"])
    ap.add_argument("--size", default="436x1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lanes", type=int, nargs="*", default=[2])
    ap.add_argument("--batches", type=int, nargs="*", default=[2, 4])
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    opt = ap.parse_args(argv)
    if max(opt.lanes, default=1) >= 4:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")     # before the runtime starts (attack_PCFA._hardware_queues_for)

    import torch
    import bench
    from pcfa_amd import attack_PCFA
    from pcfa_amd.helper_functions import datasets
    dev = torch.device("cuda")
    h, w = (int(v) for v in opt.size.lower().split("x"))
    nmax = max([1] + opt.lanes + opt.batches)
    pairs = []
    for seed in range(nmax):
        i1, i2, _ = datasets.synthetic_pair(seed, h, w)
        pairs.append((i1[None], i2[None]))

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if opt.out:
            with open(opt.out, "a") as f:
                f.write(text + "\n")

    for net in opt.nets:
        args = bench.attack_args(net, steps=opt.steps)
        model = bench.load_model(net, dev, True)
        mu = attack_PCFA.default_mu(args)

        def attack(k):
            return attack_PCFA.PairAttack(model, pairs[k][0], pairs[k][1], None, k, attack_PCFA.EPS_BOX, dev, False, mu, args)

        def solo():
            st = attack(0)
            for _ in range(opt.steps):
                st.step()
            return 1

        def flight(n):
            attack_PCFA.PairsInFlight(attack, n, dev).run(opt.steps)
            return n

        def batch(n):
            pb = attack_PCFA.PairBatch(model, [(k, pairs[k][0], pairs[k][1], None) for k in range(n)], attack_PCFA.EPS_BOX,
                                       dev, False, mu, args)
            for _ in range(opt.steps):
                pb.step()
            return n

        legs = [("solo", solo)]
        legs += [("lanes %d" % n, (lambda n=n: flight(n))) for n in opt.lanes if n > 1]
        legs += [("B = %d" % n, (lambda n=n: batch(n))) for n in opt.batches if n > 1]
        grew, live = {}, []
        for name, fn in legs:                      # untimed: first-call work, weight packs, graph capture
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            try:
                fn()
            except ValueError as e:                # a build that cannot run several pairs in flight
                emit({"net": net, "size": opt.size, "steps": opt.steps, "leg": name, "refused": str(e)})
                continue
            torch.cuda.synchronize()
            grew[name] = torch.cuda.max_memory_allocated() - base
            live.append((name, fn))
        rates = {name: [] for name, _ in live}
        for _ in range(opt.reps):
            for name, fn in live:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = fn()
                torch.cuda.synchronize()
                rates[name].append(n * opt.steps / (time.perf_counter() - t0))
        for name, _ in live:
            r = rates[name]
            emit({"net": net, "size": opt.size, "steps": opt.steps, "leg": name,
                  "pair_steps_per_s_median": round(statistics.median(r), 3), "pair_steps_per_s_min": round(min(r), 3),
                  "pair_steps_per_s_max": round(max(r), 3), "reps": [round(v, 3) for v in r],
                  "max_memory_allocated_growth_mb": round(grew[name] / 2 ** 20, 1)})
        for name in ("_pcfa_pair_graphs", "_pcfa_pair_batch_graphs"):
            getattr(model, name, {}).clear()
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
