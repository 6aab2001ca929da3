#!/bin/bash
# HBM traffic of the pcfa_amd kernels from rocprofv3 PMC counters, as MI355X_MICROARCH.md prescribes:
# separate --pmc passes (FETCH_SIZE and WRITE_SIZE do not fit one pass), no tracing domains besides
# --kernel-trace, program directly after `--`.  The bench runs with --full: the un-fused lookup kernel
# only runs in its extra eager step.  Run on the GPU box:  bash tools/pmc_traffic.sh <tag> [dir]
# (dir under the repository, default bench_outputs)
export TMPDIR=/tmp
export PCFA_BENCH_NO_TRACER=1  # rocprofv3 owns the tracer in these runs
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r01}
OUT=$R/${2:-bench_outputs}
mkdir -p $OUT
cd /tmp
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 900 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/pmc_${TAG}_$C -- \
      python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $OUT/pmc_${TAG}_$C.log 2>&1
done
cd $R
python3 tools/pmc_traffic.py $OUT/pmc_${TAG}_FETCH_SIZE $OUT/pmc_${TAG}_WRITE_SIZE > $OUT/pmc_${TAG}_traffic.json
cat $OUT/pmc_${TAG}_traffic.json
find $OUT/pmc_${TAG}_FETCH_SIZE $OUT/pmc_${TAG}_WRITE_SIZE -name "*.csv" -size +8M -delete
