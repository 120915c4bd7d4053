#!/usr/bin/env python3
"""Throughput of the wide per-event LSTM forecaster (csrc/kernels/lstm_serve_wide.hip) against
its number of resident lanes (``LSTMScoringServer(model, lanes=R)``: key k on lane k % R).

Per stack and lane count, in a child process under its own timeout (the first failure ends
the run: nothing more is started on a device that may be hung):
  saturated -- ``forecast()`` on batches of 4 096 events over 4 096 keys once every key's
               window is full (the windows are filled, one batch is run unmeasured, then
               ``--batches`` batches are timed): events/s and the server's ``lane_events``;
  latency   -- at 1 and 8 lanes, 2 000 events of 8 interleaved keys at 1 000 events/s through
               ``latency_us``: host round trip p50 / p99 over the events that ran the stack.

``--ab-child I`` is one run of the one-lane regression check: the host p50 of stack I on the
native ``LSTMServe`` class with the arguments the parent commit's build also takes, so
``tools/ab/ab_lstm_lanes.sh`` can alternate the two builds; ``--ab-file`` folds that
script's output into the summary.

Writes ``SUMMARY.md`` and ``results.json`` into ``--out`` and prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOOK_BACK = 50
STACKS = [
    ("LSTM(256) -> Dense(18)", [("lstm", 256, False, "tanh"), ("dense", 18, False)]),
    ("LSTM(512) -> Dense(18)", [("lstm", 512, False, "tanh"), ("dense", 18, False)]),
]
LANES = [1, 2, 4, 8, 16, 32]
LATENCY_LANES = (1, 8)
BATCH = 4096          # events per forecast() call, one per key
LAT_KEYS = 8             # as bench_lstm_serve_wide.py: at 8 lanes one key per lane
TARGET = 10_000.0     # events/s: 100 000 cars at one message per 10 s


def _model(idx):
    import torch

    from streamml.models.lstm import LSTMPredictor
    return LSTMPredictor(look_back=LOOK_BACK, stack=STACKS[idx][1], device=torch.device("cuda", 0), seed=1)


def child(idx: int, lanes: int, batches: int, lat_events: int, qps: float) -> dict:
    import numpy as np

    from streamml.ops.serve import LSTMScoringServer

    m = _model(idx)
    rng = np.random.default_rng(2)
    rows = rng.uniform(0, 40, size=(BATCH, 18)).astype(np.float32)
    keys = np.arange(BATCH, dtype=np.int64)
    out = {"stack": STACKS[idx][0], "look_back": LOOK_BACK, "lanes": lanes, "batch": BATCH, "batches": batches}
    with LSTMScoringServer(m, nkeys=BATCH, idle_seconds=5.0, lanes=lanes) as srv:
        out["kernel"] = srv.kernel
        for _ in range(LOOK_BACK - 1):          # fill every key's window (no stack runs yet)
            srv.forecast(rows, keys)
        pred, _, _ = srv.forecast(rows, keys)   # the first batch that runs the stack: unmeasured
        assert pred.any(axis=1).all()
        before = srv.lane_events.copy()
        ts = []
        for _ in range(batches):
            t0 = time.perf_counter()
            _, _, flag = srv.forecast(rows, keys)
            ts.append(time.perf_counter() - t0)
            assert not (flag == 2).any()
        out["lane_events"] = (srv.lane_events - before).tolist()
        out["launches"] = srv.launches
    out["batch_s"] = ts
    out["events_per_s"] = BATCH / float(np.median(ts))
    if lanes in LATENCY_LANES:
        n = lat_events
        lrows = rng.uniform(0, 40, size=(n, 18)).astype(np.float32)
        lkeys = (np.arange(n) % LAT_KEYS).astype(np.int64)
        with LSTMScoringServer(m, nkeys=LAT_KEYS, idle_seconds=5.0, lanes=lanes) as srv:
            host = srv.latency_us(lrows, lkeys, qps=qps)
        ran = np.arange(n) >= LAT_KEYS * (LOOK_BACK - 1)
        out.update(latency_qps=qps, latency_events_scored=int(ran.sum()),
                   host_p50_us=float(np.percentile(host[ran], 50)), host_p99_us=float(np.percentile(host[ran], 99)))
    return out


def ab_child(idx: int, events: int, qps: float) -> dict:
    """Host p50 of one-lane serving through the native class, called with the arguments that
    the parent commit's build takes too (no ``lanes``)."""
    import numpy as np

    from streamml.data.cardata import normalize_affine
    from streamml.ops import load_c
    from streamml.ops.serve import lstm_layer_table

    m = _model(idx)
    flat, table = lstm_layer_table(m)
    sc, sh = (np.asarray(a, np.float32) for a in normalize_affine())
    s = load_c().LSTMServe(0, 4096, flat, [list(t) for t in table], 18, LOOK_BACK, 8, sc, sh, 5.0, 5.0)
    rng = np.random.default_rng(2)
    rows = rng.uniform(0, 40, size=(events, 18)).astype(np.float32)
    keys = (np.arange(events) % 8).astype(np.int64)
    try:
        host = s.latency_run(rows, int(1e9 / qps), keys)[:, 0] / 1e3
    finally:
        s.stop()
    ran = np.arange(events) >= 8 * (LOOK_BACK - 1)
    return {"stack": STACKS[idx][0], "host_p50_us": float(np.percentile(host[ran], 50)),
            "host_p99_us": float(np.percentile(host[ran], 99))}


def _ab_section(path: str) -> list:
    """tools/ab/ab_lstm_lanes.sh writes one JSON line per run: {"build": "old" | "new", ...}."""
    runs = [json.loads(ln) for ln in open(path) if ln.strip()]
    out = ["", "## One-lane regression check against the parent commit", "",
           "The parent's build and this build alternated in one job (`tools/ab/ab_lstm_lanes.sh`), each run a fresh",
           "process: 2 000 events of 8 keys at 1 000 events/s on the native one-lane server, host p50 over the events",
           "that ran the stack.  Spread = (max - min) / median of a build's own runs.", "",
           "| stack | parent p50 us (runs) | this build p50 us (runs) | ratio of medians | parent spread | spread |",
           "|---|---|---|---:|---:|---:|"]
    import statistics
    for name, _ in STACKS:
        col = {}
        for b in ("old", "new"):
            col[b] = [r["host_p50_us"] for r in runs if r["build"] == b and r["stack"] == name]
        if not col["old"] or not col["new"]:
            continue
        med = {b: statistics.median(v) for b, v in col.items()}
        spread = {b: (max(v) - min(v)) / med[b] for b, v in col.items()}
        fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
        out.append(f"| {name} | {fmt(col['old'])} | {fmt(col['new'])} | {med['new'] / med['old']:.4f} | "
                   f"{100 * spread['old']:.2f} % | {100 * spread['new']:.2f} % |")
    return out


def summary(results, ab_file=None) -> str:
    out = ["# Wide LSTM forecaster: events/s against resident lanes (look_back 50, MI355X)", "",
           "`LSTMScoringServer(model, lanes=R)`: R resident workgroups of `lstm_serve_wide.hip` in one launch, key k on",
           "lane k % R.  Saturated stream: `forecast()` on batches of 4 096 events over 4 096 keys, every key's window",
           "full, median batch.  Latency: 2 000 events of 8 keys at 1 000 events/s, host round trip.  The workload's",
           "rate is 10 000 events/s (100 000 cars, one message per 10 s).", "",
           "| stack | lanes | events/s | x one lane | per lane events/s | >= 10 000/s | host p50 us | host p99 us | "
           "lane_events (min..max) |",
           "|---|---:|---:|---:|---:|:---:|---:|---:|---|"]
    one = {}
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['lanes']} | {r['error']} | | | | | | |")
            continue
        if r["lanes"] == 1:
            one[r["stack"]] = r["events_per_s"]
        rel = f"{r['events_per_s'] / one[r['stack']]:.2f}" if r["stack"] in one else ""
        lat = (f"{r['host_p50_us']:.1f} | {r['host_p99_us']:.1f}") if "host_p50_us" in r else " | "
        le = r["lane_events"]
        out.append(f"| {r['stack']} | {r['lanes']} | {r['events_per_s']:.0f} | {rel} | "
                   f"{r['events_per_s'] / r['lanes']:.0f} | {'yes' if r['events_per_s'] >= TARGET else 'no'} | {lat} | "
                   f"{min(le)}..{max(le)} |")
    out.append("")
    for name, _ in STACKS:
        ok = [r for r in results if r["stack"] == name and "error" not in r]
        hit = [r["lanes"] for r in ok if r["events_per_s"] >= TARGET]
        if hit:
            out.append(f"{name} first sustains 10 000 events/s at {min(hit)} lanes.")
        elif ok:
            best = max(ok, key=lambda r: r["events_per_s"])
            out.append(f"{name} does not reach 10 000 events/s: its best is {best['events_per_s']:.0f} events/s at "
                       f"{best['lanes']} lanes.")
    if ab_file and os.path.exists(ab_file):
        out += _ab_section(ab_file)
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, nargs=2, default=None, metavar=("STACK", "LANES"))
    ap.add_argument("--ab-child", type=int, default=-1, metavar="STACK")
    ap.add_argument("--batches", type=int, default=3, help="timed batches per configuration")
    ap.add_argument("--events", type=int, default=2000, help="events of a latency run")
    ap.add_argument("--qps", type=float, default=1000.0)
    ap.add_argument("--lanes", type=int, nargs="*", default=LANES)
    ap.add_argument("--timeout", type=float, default=150.0, help="seconds per configuration")
    ap.add_argument("--ab-file", default=None, help="output of tools/ab/ab_lstm_lanes.sh to fold into the summary")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "lstm_serve_lanes"))
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(child(args.child[0], args.child[1], args.batches, args.events, args.qps)),
              flush=True)
        return 0
    if args.ab_child >= 0:
        print("RESULT " + json.dumps(ab_child(args.ab_child, args.events, args.qps)), flush=True)
        return 0
    results, failed = [], False
    for i, (name, _) in enumerate(STACKS):
        for lanes in args.lanes:
            if failed:
                break
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i), str(lanes), "--batches",
                   str(args.batches), "--events", str(args.events), "--qps", str(args.qps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                results.append({"stack": name, "lanes": lanes, "error": f"timed out after {args.timeout:.0f} s"})
                failed = True   # nothing more on a device that may be hung
                break
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                results.append({"stack": name, "lanes": lanes,
                                "error": f"exit {r.returncode}: {r.stderr.strip()[-300:]}"})
                failed = True
                break
            results.append(json.loads(line[-1][7:]))
            print(json.dumps(results[-1]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "results.json"), "w") as f:
        json.dump(results, f, indent=1)
    with open(os.path.join(args.out, "SUMMARY.md"), "w") as f:
        f.write(summary(results, args.ab_file))
    print(json.dumps({"bench": "lstm_serve_lanes", "results": results}))
    return 0 if not failed else 1


if __name__ == "__main__":
    sys.exit(main())
