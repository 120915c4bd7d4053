#!/usr/bin/env bash
# Full GPU check + profile snapshot: gpu tests, smoke, bench, rocprofv3 kernel stats,
# one SQ counter pass on the AE bench.  Each GPU step is time-limited; a failure stops.
# Logs and profiles go to $OUT (default: bench_out/ in the repository).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
R=$(pwd)
O=${OUT:-$R/bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
step() { local n=$1 t=$2; shift 2; echo "== $n"; timeout -k 10 "$t" "$@" > "$O/$n.log" 2>&1; local rc=$?;
         tail -n 3 "$O/$n.log"; [ $rc -eq 0 ] || { echo "FAILED $n rc=$rc"; exit $rc; }; }
step pytest_gpu 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider
step smoke 300 python -c "import __graft_entry__ as g; g.smoke()"
step bench 600 python bench.py --full
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o run \
   -- python3 "$R/bench.py" --full --steps 50 --warmup 5 --infer-events 100 > "$O/rocprof.log" 2>&1 \
   || { echo "rocprof failed"; tail -20 "$O/rocprof.log"; exit 1; }
timeout -s KILL 120 rocprofv3 --kernel-trace --output-format csv -d "$O/pmc" -o run \
   --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_ACTIVE_INST_VALU \
   -- python3 "$R/bench.py" --steps 20 --warmup 2 > "$O/pmc.log" 2>&1 \
   || { echo "pmc failed"; tail -20 "$O/pmc.log"; exit 1; }
cd "$R"
step bench_lstm 600 python bench/bench_lstm.py
step bench_infer 600 python bench/bench_infer.py
step bench_minibatch 300 python bench/bench_minibatch.py
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_lstm" -o run \
   -- python3 "$R/bench/bench_lstm.py" --steps 10 --warmup 2 > "$O/rocprof_lstm.log" 2>&1 \
   || { echo "rocprof lstm failed"; exit 1; }
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_mb" -o run \
   -- python3 "$R/bench/bench_minibatch.py" --launches 2 > "$O/rocprof_mb.log" 2>&1 \
   || { echo "rocprof minibatch failed"; exit 1; }
echo "== done"
