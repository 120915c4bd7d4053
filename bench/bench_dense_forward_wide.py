#!/usr/bin/env python3
"""Bulk inference of WIDE Dense stacks: the wide fused forward (csrc/kernels/dense_forward_wide.hip, the
whole stack in one launch on bf16 MFMAs) next to the layer loop (one GEMM launch per layer), through the
public interface.

Per stack, in a child process under its own timeout, on device-resident fp32 rows: ``Model.score``
(scores to the host) and ``Model.predict`` (reconstructions to the host) with ``engine="wide"`` and
``engine="layers"``, one warm-up call each, then ``--runs`` timed calls per engine, the engines
alternating.  A call's time is a host clock around the call, which ends in the device-to-host copy of
its result; both engines run the same ``--rows`` rows.  The layer loop runs in batches of 65536 rows.
Reported: rows/s (median, min .. max) and, from the shapes, the FLOP/s the wide engine's rate amounts to.
The wide engine "wins" a row when its median time per row is below the layer loop's by more than the
layer loop's own spread.  The comparison is against the layer loop, never against the kernel itself.

A third pair of columns times ``ops.dense_forward_wide.forward`` alone (scores left on the device, a
synchronise at the end, weight image rebuilt per call as always) with 64- and with 128-row tiles: the
figures behind the tile size the kernel picks for itself.

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
    ("18-512-128-512-18", 18, [512, 128, 512, 18], ["tanh", "relu", "tanh", "linear"]),
    ("18-512-512-512-18", 18, [512, 512, 512, 18], ["tanh", "relu", "tanh", "linear"]),
]
KERNEL = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd",
                      "csrc", "kernels", "dense_forward_wide.hip")
PEAK_BF16_MFMA = 2.5e15   # FLOP/s, MI355X dense matrix bf16


def flop_per_row(idx: int) -> int:
    _, feat, widths, _ = STACKS[idx]
    dims = [feat] + widths
    return 2 * sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def _stats(t) -> dict:
    import numpy as np
    return {"rows_per_s": 1 / float(np.median(t)), "rows_per_s_min": 1 / max(t), "rows_per_s_max": 1 / min(t),
            "s_per_row": float(np.median(t)), "spread": max(t) - min(t)}


def child(idx: int, rows: int, runs: int) -> list:
    import torch

    from streamml import nn
    from streamml.nn.layers import Dense
    from streamml.ops import dense_forward_wide as dfww
    name, feat, widths, acts = STACKS[idx]
    dev = torch.device("cuda", 0)
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=1)
    x = torch.rand(rows, feat, device=dev) - 0.5
    out = []
    for mode in ("score", "predict"):
        call = {"score": lambda xs, eng: m.score(xs, batch_size=1 << 20 if eng == "wide" else 65536, engine=eng),
                "predict": lambda xs, eng: m.predict(xs, batch_size=65536, engine=eng)}[mode]
        times = {"wide": [], "layers": []}
        for r in range(runs + 1):                      # run 0 warms both engines up
            for eng in ("wide", "layers"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(x, eng)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert (m.last_score_engine if mode == "score" else m.last_predict_engine) == eng
                if r:
                    times[eng].append(dt / rows)
        row = {"stack": name, "mode": mode, "rows": rows, "wide": _stats(times["wide"]), "layers": _stats(times["layers"])}
        w, l = row["wide"], row["layers"]
        row.update(flop_per_row=flop_per_row(idx), flop_per_s=flop_per_row(idx) * w["rows_per_s"],
                   speedup=l["s_per_row"] / w["s_per_row"], wide_wins=bool(l["s_per_row"] - w["s_per_row"] > l["spread"]),
                   gain_inside_wide_spread=bool(l["s_per_row"] - w["s_per_row"] <= w["spread"]))
        out.append(row)
    # the kernel's launch alone, per tile size, the tile sizes alternating
    times = {64: [], 128: []}
    for r in range(runs + 1):
        for tile in (64, 128):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dfww.forward(m, x, rec=False, score=True, tile=tile)
            torch.cuda.synchronize()
            if r:
                times[tile].append((time.perf_counter() - t0) / rows)
    out.append({"stack": name, "mode": "tiles", "rows": rows, "flop_per_row": flop_per_row(idx),
                "tile64": _stats(times[64]), "tile128": _stats(times[128])})
    return out


def kernel_resources() -> str:
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), KERNEL, "dense_fwdw"],
                           capture_output=True, text=True, timeout=300)
        return r.stdout.strip()
    except Exception as e:   # noqa: BLE001 (the table is an extra)
        return f"(tools/kernel_resources.py did not run: {e})"


def _rate(s: dict) -> str:
    return f"{s['rows_per_s']:,.0f} ({s['rows_per_s_min']:,.0f} .. {s['rows_per_s_max']:,.0f})"


def summary(results, resources) -> str:
    rows = next((r["rows"] for r in results if "rows" in r), 0)
    out = ["# Bulk inference of wide Dense stacks: wide fused forward vs layer loop (MI355X)", "",
           "`engine=\"wide\"` is one launch of `dense_forward_wide.hip` per 1 Mi rows; `engine=\"layers\"` is one GEMM",
           f"launch per layer and 65536 rows.  {rows:,} device-resident fp32 rows per call for both engines, the engines",
           "alternating; a call is timed by a host clock and ends in the device-to-host copy of its result (scores, or",
           "reconstructions); median (min .. max) over the timed calls.  These are END-TO-END rates of the public call,",
           "copy included, not kernel times; FLOP/s is what the wide rate amounts to from the shapes (2 in out per layer).",
           "", "| stack | mode | wide rows/s | layers rows/s | speed-up | wide FLOP/s | beats the layer loop by more than "
           "its spread |", "|---|---|---:|---:|---:|---:|---|"]
    calls = [r for r in results if r.get("mode") in ("score", "predict")]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | |")
    for r in calls:
        out.append(f"| {r['stack']} | {r['mode']} | {_rate(r['wide'])} | {_rate(r['layers'])} | {r['speedup']:.2f}x | "
                   f"{r['flop_per_s'] / 1e12:.1f} TFLOP/s | {'yes' if r['wide_wins'] else 'NO'} |")
    lost = [f"{r['stack']} {r['mode']}" for r in calls if not r["wide_wins"]]
    shaky = [f"{r['stack']} {r['mode']}" for r in calls if r["wide_wins"] and r["gain_inside_wide_spread"]]
    out += ["", "Rows the wide engine does not win: " + (", ".join(lost) if lost else "none") + ".",
            "Rows it wins by less than its OWN spread (max - min of its calls), so the size of the gain is not "
            "established: " + (", ".join(shaky) if shaky else "none") + ".", "",
            "The launch alone (`ops.dense_forward_wide.forward`, scores left on the device, image rebuilt per call), by "
            "tile size, the two alternating:", "",
            "| stack | 64-row tiles rows/s | 128-row tiles rows/s | FLOP/s of the faster | share of the bf16 MFMA peak |",
            "|---|---:|---:|---:|---:|"]
    for r in results:
        if r.get("mode") == "tiles":
            best = max(r["tile64"]["rows_per_s"], r["tile128"]["rows_per_s"]) * r["flop_per_row"]
            out.append(f"| {r['stack']} | {_rate(r['tile64'])} | {_rate(r['tile128'])} | {best / 1e12:.1f} TFLOP/s | "
                       f"{best / PEAK_BF16_MFMA:.1%} |")
    from streamml.ops import dense_forward_wide as dfww
    lds = "; ".join(f"{name}: {dfww.plan([feat] + widths, 64)['lds_bytes']:,} / {dfww.plan([feat] + widths, 128)['lds_bytes']:,}"
                    for name, feat, widths, _ in STACKS)
    out += ["", "That share is a whole-call rate over the peak (image gather and launch included), not the kernel's own "
            "time from a trace: not measured.", "",
            "Tile size: left to itself (as in the first table) the kernel takes 128-row tiles when the rows fill every CU "
            "with them (n >= 128 x CUs) and 64-row tiles below; one workgroup of 8 waves per CU either way.  Dynamic LDS "
            f"in bytes at 64 / 128 rows (the activation tile; plus 1 / 2 KiB static): {lds}.", "",
            "Kernel resources (`tools/kernel_resources.py`; spillV 0: no scratch):", "", "```", resources, "```"]
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--rows", type=int, default=2 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=200.0, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "dense_forward_wide"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child, args.rows, max(args.runs, 3))), flush=True)
        return 0
    results, ok = [], True
    for i, (name, _, _, _) in enumerate(STACKS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i), "--rows", str(args.rows), "--runs",
               str(args.runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            err = "" if r.returncode == 0 and line else f"exit {r.returncode}: {r.stderr.strip()[-300:]}"
        except subprocess.TimeoutExpired:
            err = f"timed out after {args.timeout:.0f} s"
        if err:
            results.append({"stack": name, "error": err})
            ok = False
            break   # nothing more on a device that may be hung
        results += json.loads(line[-1][7:])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "results.json"), "w") as f:
        json.dump(results, f, indent=1)
    with open(os.path.join(args.out, "SUMMARY.md"), "w") as f:
        f.write(summary(results, kernel_resources()))
    print(json.dumps({"bench": "dense_forward_wide", "results": results}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
