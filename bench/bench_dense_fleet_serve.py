#!/usr/bin/env python3
"""Per-event scoring of a FLEET of Dense autoencoders, one model per car key
(csrc/kernels/dense_serve_fleet.hip), next to the single-model server on one member
(csrc/kernels/dense_serve.hip): what does it cost that every event reads its own weight image?

Per stack and fleet size M, all in ONE child process per stack under its own timeout:
  paced      -- 2 000 events at 1 000 events/s through ``DenseFleetScoringServer.latency_us``, the
                model index cycling over all M (with a large M every event finds weights no earlier
                event of the run has read): host round trip p50 / p99, device load / compute p50;
  saturated  -- ``score()`` on 4 096-row calls, index cycling over all M, median of three after one
                warm-up call, with the mean pass size;
  single     -- ``DenseScoringServer`` on member 0, the same two measurements: the single-model cost
                a fleet event is compared with.
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
]
FLEETS = [1, 256, 16384]
CALL_ROWS = 4096


def _measure(latency, score, srv, rows, events, qps):
    import numpy as np
    score(rows[:64])
    host, dev_total, load, comp = latency(rows[:events], qps)
    score(rows[:CALL_ROWS])
    p0, e0, ts = srv.passes, srv.events, []
    for _ in range(3):
        t0 = time.perf_counter()
        score(rows[:CALL_ROWS])
        ts.append(time.perf_counter() - t0)
    pct = lambda a, q: float(np.percentile(a, q))
    return {"kernel": srv.kernel, "launches": int(srv.launches), "host_p50_us": pct(host, 50),
            "host_p99_us": pct(host, 99), "device_p50_us": pct(dev_total, 50), "device_load_p50_us": pct(load, 50),
            "device_compute_p50_us": pct(comp, 50), "saturated_events_per_s": CALL_ROWS / float(np.median(ts)),
            "mean_pass_size": (srv.events - e0) / max(srv.passes - p0, 1)}


def child(idx: int, events: int, qps: float) -> list:
    import numpy as np
    import torch

    from streamml import nn
    from streamml.nn.layers import Dense
    from streamml.ops.serve import DenseFleetScoringServer, DenseScoringServer, dense_layer_table, dense_serve_image

    name, feat, widths, acts = STACKS[idx]
    dev = torch.device("cuda", 0)
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=1)
    layers, weights = dense_layer_table(m)
    flat0 = np.concatenate([a.ravel() for pair in weights for a in pair])
    rng = np.random.default_rng(2)
    rows = rng.uniform(0, 40, size=(max(events, CALL_ROWS), feat)).astype(np.float32)
    norm = "cardata" if feat == 18 else None
    out = []
    with DenseScoringServer(m, idle_seconds=5.0, normalizer=norm) as srv:
        r = _measure(lambda x, q: srv.latency_us(x, qps=q, device_breakdown=True), srv.score, srv, rows, events, qps)
    out.append(dict(r, stack=name, server="single", models=1, image_bytes=4 * int(dense_serve_image(layers, weights)[0].size)))
    for M in FLEETS:
        # member 0 is the model above; the others are its weights scaled, so every image differs
        flats = flat0[None, :] * (1.0 + 1e-3 * (np.arange(M, dtype=np.float32) % 97))[:, None]
        with DenseFleetScoringServer.from_flats(layers, flats, idle_seconds=5.0, normalizer=norm, device=dev) as srv:
            stride = srv.stride
            cyc = lambda n: np.arange(n, dtype=np.int64) % M
            r = _measure(lambda x, q: srv.latency_us(x, cyc(len(x)), qps=q, device_breakdown=True),
                         lambda x: srv.score(x, cyc(len(x))), srv, rows, events, qps)
        out.append(dict(r, stack=name, server="fleet", models=M, image_bytes=4 * stride))
        del flats
    return out


def summary(results) -> str:
    out = ["# Per-event scoring of a fleet of Dense autoencoders, one model per car key (MI355X)", "",
           "`DenseFleetScoringServer` on the resident kernel of `dense_serve_fleet.hip`: one workgroup, M weight",
           "images stacked in device memory, every event reads the image its model index names.  `single` is",
           "`DenseScoringServer` on member 0 in the same job (`dense_serve.hip`: the image in LDS).  Paced: 2 000",
           "events at 1 000 events/s, model index cycling over all M.  Saturated: `score()` on 4 096-row calls,",
           "index cycling, median of three.", "",
           "| stack | server | M | image KiB | host p50 us | host p99 us | device load p50 us | "
           "device compute p50 us | saturated events/s | mean pass size | compute vs single |",
           "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    base = {}
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | | | | | |")
            continue
        if r["server"] == "single":
            base[r["stack"]] = r["device_compute_p50_us"]
        rel = r["device_compute_p50_us"] / base[r["stack"]] if base.get(r["stack"]) else float("nan")
        out.append(f"| {r['stack']} | {r['server']} ({r['kernel']}) | {r['models']} | {r['image_bytes'] / 1024:.1f} | "
                   f"{r['host_p50_us']:.1f} | {r['host_p99_us']:.1f} | {r['device_load_p50_us']:.1f} | "
                   f"{r['device_compute_p50_us']:.1f} | {r['saturated_events_per_s']:,.0f} | "
                   f"{r['mean_pass_size']:.2f} | {rel:.2f}x |")
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--events", type=int, default=2000)
    ap.add_argument("--qps", type=float, default=1000.0)
    ap.add_argument("--timeout", type=float, default=150.0, help="seconds per stack")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "dense_fleet_serve"))
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
        results += json.loads(line[-1][7:])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "results.json"), "w") as f:
        json.dump(results, f, indent=1)
    with open(os.path.join(args.out, "SUMMARY.md"), "w") as f:
        f.write(summary(results))
    print(json.dumps({"bench": "dense_fleet_serve", "results": results}))
    return 0 if all("error" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
