#!/bin/bash
# One GPU session: parity tests (error statistics logged), smoke, bench --full (C2 headline
# with its secondary measurements, and the C4 unit on one GPU), kernel-trace profile.
# Stops at the first fault/abort/timeout (exit codes other than 0 or 1 from pytest).
# Results under $OUT (default: bench_out/ in the tree).
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
cd $R
mkdir -p $OUT
export TMPDIR=/tmp
STEPS=${STEPS:-10}
rm -f $OUT/parity_errors.jsonl
PFB_PARITY_LOG=$OUT/parity_errors.jsonl timeout -k 10 900 \
    python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread -rf \
    > $OUT/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -15 $OUT/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping after pytest rc=$rc"; exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -3 $OUT/smoke.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup 3 > $OUT/bench.json 2> $OUT/bench.err
rc=$?; echo "bench rc=$rc"; cat $OUT/bench.json; tail -3 $OUT/bench.err
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --full --steps $STEPS --warmup 3 --workload c4 --no-cpu-baseline > $OUT/bench_c4.json 2> $OUT/bench_c4.err
rc=$?; echo "bench c4 rc=$rc"; cat $OUT/bench_c4.json; tail -3 $OUT/bench_c4.err
if [ $rc -ne 0 ]; then exit $rc; fi
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run \
    -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --inflight 1 > $OUT/prof.log 2>&1
rc=$?; echo "rocprof rc=$rc"
exit $rc
