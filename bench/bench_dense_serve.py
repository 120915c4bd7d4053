#!/usr/bin/env python3
"""Per-event scoring of Dense autoencoders wider or deeper than the reference's
(csrc/kernels/dense_serve.hip) next to the only other way to score such a model,
``nn.Model.predict`` on one row.

Per stack, in a child process under its own timeout:
  latency    -- 2 000 events at 1 000 events/s through
                ``DenseScoringServer.latency_us(device_breakdown=True)``: host round trip p50 / p99
                and the device's row-load / compute split (p50);
  throughput -- saturated ``score()`` on 4 096-row calls, median of three after one warm-up call,
                with the mean pass size (events / passes over the three calls);
  baseline   -- ``model.predict`` on one device-resident [1, D] row: 200 synchronised calls after
                20 warm-up calls, median.
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

#          name, features, widths, activations
STACKS = [
    ("18-64-16-64-18", 18, [64, 16, 64, 18], ["tanh", "relu", "tanh", "relu"]),
    ("30-128-32-128-30", 30, [128, 32, 128, 30], ["tanh", "relu", "tanh", "relu"]),
    ("18-512-128-512-18", 18, [512, 128, 512, 18], ["tanh", "relu", "tanh", "relu"]),
    ("18-512-512-512-18", 18, [512, 512, 512, 18], ["tanh", "relu", "tanh", "relu"]),
]
CALL_ROWS = 4096


def child(idx: int, events: int, qps: float) -> dict:
    import numpy as np
    import torch

    from streamml import nn
    from streamml.nn.layers import Dense
    from streamml.ops.serve import DenseScoringServer

    name, feat, widths, acts = STACKS[idx]
    dev = torch.device("cuda", 0)
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=1)
    m.compile(fused=False)
    rng = np.random.default_rng(2)
    rows = rng.uniform(0, 40, size=(max(events, CALL_ROWS), feat)).astype(np.float32)
    with DenseScoringServer(m, idle_seconds=5.0, normalizer="cardata" if feat == 18 else None) as srv:
        kernel = srv.kernel
        srv.score(rows[:64])
        host, dev_total, load, comp = srv.latency_us(rows[:events], qps=qps, device_breakdown=True)
        srv.score(rows[:CALL_ROWS])
        p0, e0, ts = srv.passes, srv.events, []
        for _ in range(3):
            t0 = time.perf_counter()
            srv.score(rows[:CALL_ROWS])
            ts.append(time.perf_counter() - t0)
        pass_size = (srv.events - e0) / max(srv.passes - p0, 1)
        launches = srv.launches
    x = torch.rand(1, feat, device=dev) * 2 - 1
    for _ in range(20):
        m.predict(x)
    torch.cuda.synchronize()
    tp = []
    for _ in range(200):
        t0 = time.perf_counter()
        m.predict(x)
        torch.cuda.synchronize()
        tp.append((time.perf_counter() - t0) * 1e6)
    pct = lambda a, q: float(np.percentile(a, q))
    return {"stack": name, "kernel": kernel, "events": events, "qps": qps, "launches": int(launches),
            "host_p50_us": pct(host, 50), "host_p99_us": pct(host, 99),
            "device_p50_us": pct(dev_total, 50), "device_load_p50_us": pct(load, 50),
            "device_compute_p50_us": pct(comp, 50),
            "saturated_events_per_s": CALL_ROWS / float(np.median(ts)), "mean_pass_size": float(pass_size),
            "predict_median_us": float(np.median(tp)), "predict_p99_us": float(np.percentile(tp, 99))}


def summary(results) -> str:
    out = ["# Per-event scoring of wide / deep Dense autoencoders (MI355X)", "",
           "Server: `DenseScoringServer` on the resident kernel of `dense_serve.hip`; 2 000 events at",
           "1 000 events/s for the latencies, saturated `score()` on 4 096-row calls (median of three) for",
           "the throughput.  Baseline: `nn.Model.predict` on one device-resident `[1, D]` row, 200",
           "synchronised calls after 20 warm-up calls.", "",
           "| stack | kernel | host p50 us | host p99 us | device load p50 us | device compute p50 us | "
           "saturated events/s | mean pass size | `predict` median us | predict / server p50 |",
           "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | | | | |")
            continue
        out.append(f"| {r['stack']} | {r['kernel']} | {r['host_p50_us']:.1f} | {r['host_p99_us']:.1f} | "
                   f"{r['device_load_p50_us']:.1f} | {r['device_compute_p50_us']:.1f} | "
                   f"{r['saturated_events_per_s']:,.0f} | {r['mean_pass_size']:.2f} | "
                   f"{r['predict_median_us']:.1f} | {r['predict_median_us'] / r['host_p50_us']:.2f}x |")
    slower = [r["stack"] for r in results if "error" not in r and r["predict_median_us"] < r["host_p50_us"]]
    out += ["", "`predict` beats the server's p50 on: " + (", ".join(slower) if slower else "no stack") + "."]
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--events", type=int, default=2000)
    ap.add_argument("--qps", type=float, default=1000.0)
    ap.add_argument("--timeout", type=float, default=90.0, help="seconds per stack")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "dense_serve"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child, args.events, args.qps)), flush=True)
        return 0
    results = []
    for i, (name, _, _, _) in enumerate(STACKS):
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
    print(json.dumps({"bench": "dense_serve", "results": results}))
    return 0 if all("error" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
