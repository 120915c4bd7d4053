#!/usr/bin/env python3
"""Per-event forecasting of LSTM stacks wider than 32 units (csrc/kernels/lstm_serve_wide.hip)
next to the only other way to forecast such a model, ``model.predict`` on one window.

Per stack, in a child process under its own timeout:
  forecaster -- 2 000 events of 8 interleaved car keys at 1 000 events/s through
                ``LSTMScoringServer.latency_us(device_breakdown=True)``: host round trip p50 / p99
                and the device's load / compute split, over the events that ran the stack (their
                key had look_back events);
  baseline   -- ``model.predict`` on one device-resident [1, look_back, 18] window: 200
                synchronised calls after 20 warm-up calls, median.
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
    ("LSTM(64) -> Dense(18)", [("lstm", 64, False, "tanh"), ("dense", 18, False)]),
    ("LSTM(128) -> Dense(18)", [("lstm", 128, False, "tanh"), ("dense", 18, False)]),
    ("LSTM(256) -> Dense(18)", [("lstm", 256, False, "tanh"), ("dense", 18, False)]),
    ("LSTM(512) -> Dense(18)", [("lstm", 512, False, "tanh"), ("dense", 18, False)]),
    ("LSTM(256, seq) -> LSTM(64) -> Dense(18)",
     [("lstm", 256, True, "tanh"), ("lstm", 64, False, "tanh"), ("dense", 18, False)]),
]
NKEYS = 8


def child(idx: int, events: int, qps: float) -> dict:
    import numpy as np
    import torch

    from streamml.models.lstm import LSTMPredictor
    from streamml.ops.serve import LSTMScoringServer

    name, stack = STACKS[idx]
    dev = torch.device("cuda", 0)
    m = LSTMPredictor(look_back=LOOK_BACK, stack=stack, device=dev, seed=1)
    rng = np.random.default_rng(2)
    rows = rng.uniform(0, 40, size=(events, 18)).astype(np.float32)
    keys = (np.arange(events) % NKEYS).astype(np.int64)
    with LSTMScoringServer(m, nkeys=NKEYS, idle_seconds=5.0) as srv:
        kernel = srv.kernel
        host, dev_total, comp = srv.latency_us(rows, keys, qps=qps, device_breakdown=True)
        load = srv.last_device_load_us
        launches = srv.launches
    ran = np.arange(events) >= NKEYS * (LOOK_BACK - 1)   # the key had look_back events: the stack ran
    pct = lambda a, q: float(np.percentile(a[ran], q))
    x = torch.rand(1, LOOK_BACK, 18, device=dev) * 2 - 1
    for _ in range(20):
        m.predict(x)
    torch.cuda.synchronize()
    ts = []
    for _ in range(200):
        t0 = time.perf_counter()
        m.predict(x)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"stack": name, "look_back": LOOK_BACK, "kernel": kernel, "events": events, "events_scored": int(ran.sum()),
            "qps": qps, "launches": int(launches),
            "host_p50_us": pct(host, 50), "host_p99_us": pct(host, 99),
            "device_p50_us": pct(dev_total, 50), "device_p99_us": pct(dev_total, 99),
            "device_load_p50_us": pct(load, 50), "device_compute_p50_us": pct(comp, 50),
            "predict_median_us": float(np.median(ts)), "predict_p99_us": float(np.percentile(ts, 99))}


def summary(results) -> str:
    out = ["# Per-event forecasting of wide LSTM stacks (look_back 50, MI355X)", "",
           "Forecaster: 2 000 events of 8 interleaved keys at 1 000 events/s through the resident kernel",
           "(`lstm_serve_wide.hip`), statistics over the events that ran the stack.  Baseline: `model.predict`",
           "on one device-resident `[1, 50, 18]` window, 200 synchronised calls after 20 warm-up calls.", "",
           "| stack | host p50 us | host p99 us | device load p50 us | device compute p50 us | "
           "`model.predict` median us | predict / forecaster p50 |",
           "|---|---:|---:|---:|---:|---:|---:|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | |")
            continue
        out.append(f"| {r['stack']} | {r['host_p50_us']:.1f} | {r['host_p99_us']:.1f} | {r['device_load_p50_us']:.1f} | "
                   f"{r['device_compute_p50_us']:.1f} | {r['predict_median_us']:.1f} | "
                   f"{r['predict_median_us'] / r['host_p50_us']:.2f}x |")
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--events", type=int, default=2000)
    ap.add_argument("--qps", type=float, default=1000.0)
    ap.add_argument("--timeout", type=float, default=90.0, help="seconds per stack")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "lstm_serve_wide"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child, args.events, args.qps)), flush=True)
        return 0
    results = []
    for i, (name, _) in enumerate(STACKS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i), "--events", str(args.events),
               "--qps", str(args.qps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            results.append({"stack": name, "error": f"timed out after {args.timeout:.0f} s"})
            break   # nothing more on a device that may be hung
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            results.append({"stack": name, "error": f"exit {r.returncode}: {r.stderr.strip()[-300:]}"})
            break
        results.append(json.loads(line[-1][7:]))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "results.json"), "w") as f:
        json.dump(results, f, indent=1)
    with open(os.path.join(args.out, "SUMMARY.md"), "w") as f:
        f.write(summary(results))
    print(json.dumps({"bench": "lstm_serve_wide", "results": results}))
    return 0 if all("error" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
