#!/usr/bin/env python
"""I-FGSM iterations/s of the product loop (attack_FGSM.FgsmAttack), leg against leg in ONE session.

The model is built once per network; one rep of every leg follows one rep of the next (A B C D A B C D ...), so clock and
thermal drift fall on all legs alike.  A rep attacks whole pairs the way the driver does -- construction (upload, forward at
the clean images, target), `--steps` iterations, the final read of the metrics -- and ends with a device synchronisation;
iterations/s = pairs x steps / wall time.  Legs:

    parent    fgsm_attack of ANOTHER checkout's pcfa_amd/attack_FGSM.py (`--parent FILE`, e.g. the file as of the parent
              commit): the comparison point.  It is loaded next to this checkout's modules and runs on this checkout's
              kernels, so the leg measures the loop, not the network.
    eager     this checkout's loop with PCFA_HIP_GRAPH=0 semantics (`use_graph=False`): the step kernel, no graphs
    graph     captured forward / backward; the graph set is captured by an untimed first pair and adopted by every rep,
              as by every later pair of a dataset
    lanes N   N pairs in flight (attack_PCFA.PairsInFlight), graph sets adopted likewise
    l2        `graph` with `--step_norm l2` (ops.pgd_l2_step: three launches between the replays instead of one) under
              `--delta_bound`; a graph set of its own, adopted likewise.  Another attack, so `same_result_as_graph` is
              null for it; its line carries the final `l2_delta-avg` next to the bound instead

`--legs` restricts the run to some of them (the order of the table above is kept).

Prints one JSON line per (network, leg): median, min and max of iterations/s over the reps, and every rep's figure.

    python tools/bench_fgsm.py --nets RAFT PWCNet --size 436x1024 --steps 20 --reps 7 --lanes 2 4 --parent old_attack_FGSM.py
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
from argparse import Namespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _load_parent(path):
    """Another checkout's attack_FGSM.py as the module pcfa_amd._bench_parent_attack_FGSM (its relative imports resolve to
    THIS checkout's package)."""
    import pcfa_amd  # noqa: F401
    spec = importlib.util.spec_from_file_location("pcfa_amd._bench_parent_attack_FGSM", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nets", nargs="+", default=["RAFT", "PWCNet"])
    ap.add_argument("--size", default="436x1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lanes", type=int, nargs="*", default=[2])
    ap.add_argument("--loss", default="aee")
    ap.add_argument("--joint", action="store_true")
    ap.add_argument("--weights", default="random:1234")
    ap.add_argument("--parent", default=None, help="attack_FGSM.py of the checkout to compare with")
    ap.add_argument("--delta_bound", type=float, default=0.005, help="the budget of the l2 leg")
    ap.add_argument("--legs", nargs="+", default=None, help="run only these legs (parent, eager, graph, lanes, l2)")
    opt = ap.parse_args(argv)
    if max(opt.lanes, default=1) >= 4:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")     # before the runtime starts (attack_PCFA._hardware_queues_for)

    import torch
    from pcfa_amd import attack_FGSM, attack_PCFA
    from pcfa_amd.helper_functions import datasets
    parent = _load_parent(opt.parent) if opt.parent else None
    dev = torch.device("cuda")
    h, w = (int(v) for v in opt.size.lower().split("x"))
    nmax = max([1] + opt.lanes)
    pairs = []
    for seed in range(nmax):
        i1, i2, flow = datasets.synthetic_pair(seed, h, w)
        pairs.append((i1[None], i2[None], flow[None]))

    for net in opt.nets:
        args = Namespace(net=net, weights=opt.weights, steps=opt.steps, joint_perturbation=opt.joint, epsilon=0.00025,
                         target="zero", custom_target_path="", loss=opt.loss, no_save=True, small_save=False,
                         save_frequency=1, output_folder="experiment_data", pairs_in_flight=1)
        model = attack_PCFA._load_model(args, dev, variable_change=False)

        args_l2 = Namespace(**dict(vars(args), step_norm="l2", delta_bound=opt.delta_bound))

        def solo(use_graph, args=args):
            st = attack_FGSM.FgsmAttack(model, *pairs[0], 0, dev, True, args, use_graph=use_graph)
            for _ in range(opt.steps):
                st.step()
            return 1, st.result()

        def flight(n):
            fl = attack_PCFA.PairsInFlight(
                lambda k: attack_FGSM.FgsmAttack(model, *pairs[k], k, dev, True, args, use_graph=True), n, dev)
            fl.run(opt.steps)
            return n, [st.result() for st in fl.attacks]

        legs = []
        if parent is not None:
            legs.append(("parent", lambda: (1, parent.fgsm_attack(model, *pairs[0], dev, True, args))))
        legs += [("eager", lambda: solo(False)), ("graph", lambda: solo(True))]
        legs += [("lanes %d" % n, (lambda n=n: flight(n))) for n in opt.lanes if n > 1]
        legs.append(("l2", lambda: solo(True, args_l2)))
        if opt.legs is not None:
            legs = [(name, fn) for name, fn in legs if name.split()[0] in opt.legs]
        results = {}
        for name, fn in legs:                      # untimed: first-call work, weight packs, graph capture
            _, results[name] = fn()
            torch.cuda.synchronize()
        rates = {name: [] for name, _ in legs}
        for _ in range(opt.reps):
            for name, fn in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n, _ = fn()
                torch.cuda.synchronize()
                rates[name].append(n * opt.steps / (time.perf_counter() - t0))
        final = results.get("graph")
        for name, _ in legs:
            r = rates[name]
            res = results[name][0] if isinstance(results[name], list) else results[name]   # pair 0 in every leg
            same = None if (final is None or name == "l2") else all(res[k] == final[k] for k in final if k != "history")
            extra = {"l2_delta_avg": res["l2_delta-avg"], "delta_bound": opt.delta_bound} if name == "l2" else {}
            print(json.dumps({"net": net, "size": opt.size, "steps": opt.steps, "loss": opt.loss, "joint": opt.joint,
                              "leg": name, "iters_per_s_median": round(statistics.median(r), 3),
                              "iters_per_s_min": round(min(r), 3), "iters_per_s_max": round(max(r), 3),
                              "reps": [round(v, 3) for v in r], "same_result_as_graph": same, **extra}), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
