#!/usr/bin/env python3
"""Bulk inference of Dense stacks: the fused forward (csrc/kernels/dense_forward.hip, the whole stack
in one launch) next to the layer loop (one K1 launch per layer), through the public interface.

Per stack, in a child process under its own timeout, on device-resident fp32 rows: ``Model.score``
(scores to the host) and ``Model.predict`` (reconstructions to the host) with ``engine="fused"`` and
``engine="layers"``, one warm-up call each, then ``--runs`` timed calls per engine, the engines
alternating.  A call's time is a host clock around the call, which ends in the device-to-host copy of
its result; both engines run the same ``--rows`` rows.  The layer loop runs in batches of 65536 rows
(``predict``'s default batch of 32 would measure launches only).  Reported: rows/s (median, min .. max) and, from the shapes, the bytes/s and FLOP/s the fused engine's rate amounts to.
The fused engine "wins" a row when its median time per row is below the layer loop's by more than the
layer loop's own spread.

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
    ("18-64-16-64-18", 18, [64, 16, 64, 18], ["tanh", "relu", "tanh", "linear"]),
    ("30-128-32-128-30", 30, [128, 32, 128, 30], ["tanh", "relu", "tanh", "linear"]),
]
KERNEL = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd",
                      "csrc", "kernels", "dense_forward.hip")
PEAK_FP32_MFMA = 157.3e12   # FLOP/s, MI355X matrix fp32
PEAK_HBM = 8.0e12           # bytes/s


def counts(idx: int, mode: str) -> tuple:
    """(bytes, FLOP) a row needs: the row in, the score or the reconstruction out; 2 in * out per layer."""
    _, feat, widths, _ = STACKS[idx]
    dims = [feat] + widths
    return 4 * (feat + (1 if mode == "score" else widths[-1])), 2 * sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def child(idx: int, rows: int, runs: int) -> list:
    import numpy as np
    import torch

    from streamml import nn
    from streamml.nn.layers import Dense
    name, feat, widths, acts = STACKS[idx]
    dev = torch.device("cuda", 0)
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=1)
    x = torch.rand(rows, feat, device=dev) - 0.5
    out = []
    for mode in ("score", "predict"):
        call = {"score": lambda xs, eng: m.score(xs, batch_size=1 << 20 if eng == "fused" else 65536, engine=eng),
                "predict": lambda xs, eng: m.predict(xs, batch_size=65536, engine=eng)}[mode]
        times = {"fused": [], "layers": []}
        for r in range(runs + 1):                      # run 0 warms both engines up
            for eng in ("fused", "layers"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(x, eng)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert (m.last_score_engine if mode == "score" else m.last_predict_engine) == eng
                if r:
                    times[eng].append(dt / rows)
        row = {"stack": name, "mode": mode, "rows": rows}
        for eng, t in times.items():
            row[eng] = {"rows_per_s": 1 / float(np.median(t)), "rows_per_s_min": 1 / max(t),
                        "rows_per_s_max": 1 / min(t), "s_per_row": float(np.median(t)), "spread": max(t) - min(t)}
        nbytes, flop = counts(idx, mode)
        f, l = row["fused"], row["layers"]
        row.update(bytes_per_row=nbytes, flop_per_row=flop, bytes_per_s=nbytes * f["rows_per_s"],
                   flop_per_s=flop * f["rows_per_s"], speedup=l["s_per_row"] / f["s_per_row"],
                   fused_wins=bool(l["s_per_row"] - f["s_per_row"] > l["spread"]),
                   gain_inside_fused_spread=bool(l["s_per_row"] - f["s_per_row"] <= f["spread"]))
        out.append(row)
    return out


def kernel_resources() -> str:
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), KERNEL, "dense_fwd"],
                           capture_output=True, text=True, timeout=300)
        return r.stdout.strip()
    except Exception as e:   # noqa: BLE001 (the table is an extra)
        return f"(tools/kernel_resources.py did not run: {e})"


def summary(results, resources) -> str:
    out = ["# Bulk inference of Dense stacks: fused forward vs layer loop (MI355X)", "",
           "`engine=\"fused\"` is one launch of `dense_forward.hip` per 1 Mi rows; `engine=\"layers\"` is one K1 launch",
           "per layer and 65536 rows.  " + (f"{results[0].get('rows', 0):,}" if results else "") +
           " device-resident fp32 rows per call for both engines, the engines alternating; a call is timed by a host",
           "clock and ends in the device-to-host copy of its result (scores, or reconstructions); median",
           "(min .. max) over the timed calls.  These are END-TO-END rates of the public call, copy included, not",
           "kernel times: bytes/s and FLOP/s are what the fused rate amounts to from the shapes (the row in, the result",
           "out; 2 in out per layer).", "",
           "| stack | mode | fused rows/s | layers rows/s | speed-up | fused bytes/s | fused FLOP/s | "
           "beats the layer loop by more than its spread |", "|---|---|---:|---:|---:|---:|---:|---|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | | |")
            continue
        f, l = r["fused"], r["layers"]
        out.append(f"| {r['stack']} | {r['mode']} | {f['rows_per_s']:,.0f} ({f['rows_per_s_min']:,.0f} .. "
                   f"{f['rows_per_s_max']:,.0f}) | {l['rows_per_s']:,.0f} ({l['rows_per_s_min']:,.0f} .. "
                   f"{l['rows_per_s_max']:,.0f}) | {r['speedup']:.1f}x | {r['bytes_per_s'] / 1e9:.1f} GB/s | "
                   f"{r['flop_per_s'] / 1e12:.2f} TFLOP/s | {'yes' if r['fused_wins'] else 'NO'} |")
    lost = [f"{r['stack']} {r['mode']}" for r in results if "error" not in r and not r["fused_wins"]]
    shaky = [f"{r['stack']} {r['mode']}" for r in results if "error" not in r and r["fused_wins"]
             and r["gain_inside_fused_spread"]]
    out += ["", "Rows the fused engine does not win: " + (", ".join(lost) if lost else "none") + ".",
            "Rows it wins by less than its OWN spread (max - min of its calls), so the size of the gain is not "
            "established: " + (", ".join(shaky) if shaky else "none") + ".", "",
            "The kernel's share of the larger of its two bounds (fp32 MFMA rate, HBM bandwidth): not measured.  It",
            "needs the kernel's own time from a trace, and the calls above are dominated by the copy of the result to",
            "the host.  As a whole-call rate over the peaks the best row above stands at "
            + (f"{max(r['flop_per_s'] for r in results if 'error' not in r) / PEAK_FP32_MFMA:.1%} of the fp32 MFMA "
               f"rate and {max(r['bytes_per_s'] for r in results if 'error' not in r) / PEAK_HBM:.1%} of the HBM "
               "bandwidth." if any("error" not in r for r in results) else "(no result)."),
            "", "Kernel resources (`tools/kernel_resources.py`; spillV 0: no scratch):", "", "```", resources, "```"]
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--rows", type=int, default=4 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=150.0, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "dense_forward"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child, args.rows, max(args.runs, 3))),
              flush=True)
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
    print(json.dumps({"bench": "dense_forward", "results": results}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
