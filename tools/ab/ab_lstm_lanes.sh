#!/usr/bin/env bash
# same-box A/B of one-lane wide LSTM serving (bench_lstm_serve_lanes.py --ab-child, host p50 at
# 1 000 events/s): tree _C.so vs tools/ab/_C_old.so (tools/ab/build_old.sh), four runs each,
# alternating; one JSON line per run in the file given as $1 (default
# bench_out/ab_lstm_lanes.jsonl).  Stops at the first failure.  The tree's own _C.so is put
# back however the script ends: a failure, or a signal such as the caller's time limit (each
# run is a background child that the script waits for, so a signal is handled at once).
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
P="$R/hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd"
OUT="${1:-$R/bench_out/ab_lstm_lanes.jsonl}"
mkdir -p "$(dirname "$OUT")"
: > "$OUT"
T=$(mktemp -d)
cp "$P/_C.so" "$T/_C_new.so"
cp "$R/tools/ab/_C_old.so" "$T/_C_old.so"
child=
trap 'cp "$T/_C_new.so" "$P/_C.so"; rm -rf "$T"' EXIT
trap '[ -n "$child" ] && kill "$child" 2>/dev/null; exit 130' INT TERM HUP
for v in old new old new old new old new; do
  cp "$T/_C_$v.so" "$P/_C.so"
  for stack in 0 1; do
    timeout -k 10 120 python "$R/bench/bench_lstm_serve_lanes.py" --ab-child "$stack" > "$T/run.txt" 2>/dev/null &
    child=$!
    wait "$child" && line=$(grep '^RESULT ' "$T/run.txt") || { echo "$v stack $stack failed"; exit 1; }
    child=
    echo "${line#RESULT }" | sed "s/^{/{\"build\": \"$v\", /" | tee -a "$OUT"
  done
done
