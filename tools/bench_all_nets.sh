#!/bin/bash
# One bench line per network of BASELINE.json's configs (N = 1, --full: with the CPU baseline), appended to
# <dir>/<tag>_bench_nets.jsonl (dir: second argument, default bench_outputs).  RAFT is the headline line bench.py
# prints by default.
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r01}
OUT=${2:-bench_outputs}
cd $R
mkdir -p $OUT
: > $OUT/${TAG}_bench_nets.jsonl
for spec in "GMA 436x1024" "PWCNet 375x1242" "SpyNet 436x1024" "FlowNet2 436x1024"; do
  set -- $spec
  timeout -k 10 400 python bench.py --full --net $1 --size $2 --steps 3 --warmup 1 --cpu-closures 4 >> $OUT/${TAG}_bench_nets.jsonl 2>> $OUT/${TAG}_bench_nets.err || exit 1
done
python - <<PY
import json
for line in open("$OUT/${TAG}_bench_nets.jsonl"):
    d = json.loads(line)
    c = d.get("cpu_baseline") or {}
    print("%-70s %7.3f steps/s  %8.1f ms/step  closures/s %.1f  cpu port %.4f steps/s on %s threads" % (d["config"]["workload"][:70], d["value"], d["ms_per_step"], d["closure_evals_per_sec"], c.get("value", float("nan")), c.get("cores", "?")))
PY
