#!/bin/bash
# Round evidence: smoke, all GPU tests, bench, rocprofv3 kernel stats, PMC HBM traffic passes.
# Logs and profiles go to $PAMG_OUT (default: out/ in the repository).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-run}
O=${PAMG_OUT:-$R/out}
cd $R && mkdir -p $O
timeout -k 10 240 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 && \
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/gpu_tests.log 2>&1 && \
timeout -k 10 400 python bench.py --full > $O/bench_$TAG.log 2>&1 && \
cd /tmp && export TMPDIR=/tmp && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o run -- python3 $R/bench.py --no-cpu-baseline --no-extra > $O/prof_$TAG.log 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_${TAG}_fetch -o run -- python3 $R/bench.py --steps 20 --warmup 1 --no-cpu-baseline --no-extra > $O/pmc_${TAG}_fetch.log 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_${TAG}_write -o run -- python3 $R/bench.py --steps 20 --warmup 1 --no-cpu-baseline --no-extra > $O/pmc_${TAG}_write.log 2>&1
rc=$?
echo "exit $rc"
exit $rc
