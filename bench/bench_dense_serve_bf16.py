#!/usr/bin/env python3
"""The fp32 and the bf16 per-event Dense scorer (csrc/kernels/dense_serve.hip, dense_serve_bf16.hip) on the
same model in ONE job, alternating: ``DenseScoringServer(precision=...)``.

Per stack (bench_dense_serve.py's four and 18-256-64-256-18), in a child process under its own timeout,
three rounds of {fp32 server, bf16 server}, one server alive at a time:
  latency    -- round 0 only: 2 000 events at 1 000 events/s through ``latency_us(device_breakdown=True)``:
                host round trip p50 / p99 and the device's row-load / compute split (p50);
  throughput -- every round: one saturated ``score()`` on 4 096 rows after one warm-up call; reported as
                the median (min .. max) of the three windows, with the mean pass size over them.
A precision counts as faster on a stack only when its slowest window beats the other's fastest.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dense_serve import CALL_ROWS, STACKS as _STACKS   # noqa: E402

STACKS = _STACKS + [("18-256-64-256-18", 18, [256, 64, 256, 18], ["tanh", "relu", "tanh", "relu"])]
PRECISIONS = ("fp32", "bf16")
ROUNDS = 3
# VGPRs of the resident kernels, from the code object's metadata ({lds, stream} instantiations)
VGPRS = {"lds": 122, "stream": 128, "bf16-lds": 105, "bf16-stream": 106}


def lds_bytes(feat, widths, kernel) -> int:
    """Dynamic LDS of the resident kernel: the activation (and partial-sum) buffers, plus the image when it
    lives there (sml_dense_fleet_serve.h / sml_dense_serve_bf16.h)."""
    dims = [feat] + widths
    pad = lambda n, m: (n + m - 1) // m * m
    if kernel.startswith("bf16"):
        fixed = 2 * 16 * (max(pad(k, 32) for k in dims[:-1]) + 8) * 2
        image = sum(2 * pad(i, 32) * pad(o, 16) + 4 * pad(o, 16) for i, o in zip(dims[:-1], dims[1:]))
    else:
        fixed = (2 * 8 * 512 + 8 * 1024) * 4
        image = sum(4 * (pad(i, 4) + 1) * pad(o, 32) for i, o in zip(dims[:-1], dims[1:]))
    return fixed + (image if kernel.endswith("lds") else 0)


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
    rows = np.random.default_rng(2).uniform(0, 40, size=(max(events, CALL_ROWS), feat)).astype(np.float32)
    pct = lambda a, q: float(np.percentile(a, q))
    out = {p: {"windows": [], "passes": 0, "events": 0} for p in PRECISIONS}
    for rnd in range(ROUNDS):
        for p in PRECISIONS:
            r = out[p]
            with DenseScoringServer(m, idle_seconds=5.0, normalizer="cardata" if feat == 18 else None,
                                    precision=p) as srv:
                r["kernel"] = srv.kernel
                srv.score(rows[:64])
                if rnd == 0:
                    host, _, load, comp = srv.latency_us(rows[:events], qps=qps, device_breakdown=True)
                    r.update(host_p50_us=pct(host, 50), host_p99_us=pct(host, 99),
                             device_load_p50_us=pct(load, 50), device_compute_p50_us=pct(comp, 50))
                srv.score(rows[:CALL_ROWS])
                p0, e0 = srv.passes, srv.events
                t0 = time.perf_counter()
                srv.score(rows[:CALL_ROWS])
                r["windows"].append(CALL_ROWS / (time.perf_counter() - t0))
                r["passes"] += srv.passes - p0
                r["events"] += srv.events - e0
    for p in PRECISIONS:
        r = out[p]
        r["mean_pass_size"] = r["events"] / max(r["passes"], 1)
        r["vgprs"] = VGPRS[r["kernel"]]
        r["lds_bytes"] = lds_bytes(feat, widths, r["kernel"])
    return {"stack": name, "events": events, "qps": qps, **out}


def verdict(r) -> str:
    f, b = r["fp32"]["windows"], r["bf16"]["windows"]
    if min(b) > max(f):
        return f"bf16 faster ({min(b) / max(f):.2f}x at least)"
    if min(f) > max(b):
        return f"fp32 faster ({min(f) / max(b):.2f}x at least)"
    return "windows overlap: no difference shown"


def summary(results) -> str:
    out = ["# Per-event Dense scoring: fp32 (`dense_serve.hip`) and bf16 MFMA (`dense_serve_bf16.hip`) (MI355X)", "",
           "`DenseScoringServer(precision=...)` on the same model in one job, three rounds of {fp32, bf16}, one",
           "server alive at a time.  Latencies: 2 000 events at 1 000 events/s (round 0).  Throughput: one",
           "saturated `score()` on 4 096 rows per round, median (min .. max) of the three windows.  A precision",
           "counts as faster only when its slowest window beats the other's fastest.  LDS: dynamic bytes.", "",
           "| stack | precision | kernel | host p50 us | host p99 us | device load p50 us | device compute p50 us | "
           "saturated events/s | mean pass size | VGPRs | LDS bytes |",
           "|---|---|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | | | | | |")
            continue
        for p in PRECISIONS:
            q = r[p]
            w = sorted(q["windows"])
            out.append(f"| {r['stack']} | {p} | {q['kernel']} | {q['host_p50_us']:.1f} | {q['host_p99_us']:.1f} | "
                       f"{q['device_load_p50_us']:.1f} | {q['device_compute_p50_us']:.1f} | "
                       f"{w[len(w) // 2]:,.0f} ({w[0]:,.0f} .. {w[-1]:,.0f}) | {q['mean_pass_size']:.2f} | "
                       f"{q['vgprs']} | {q['lds_bytes']:,} |")
    out += ["", "Saturated throughput, by the rule above:", ""]
    out += [f"- {r['stack']}: {verdict(r)}" for r in results if "error" not in r]
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--events", type=int, default=2000)
    ap.add_argument("--qps", type=float, default=1000.0)
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per stack")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "dense_serve_bf16"))
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
    print(json.dumps({"bench": "dense_serve_bf16", "results": results}))
    return 0 if all("error" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
