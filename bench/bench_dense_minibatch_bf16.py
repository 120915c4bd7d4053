#!/usr/bin/env python3
"""The persistent Dense trainer's two kernels side by side: ``compile(minibatch_precision="bf16")``
(csrc/kernels/dense_minibatch_bf16.hip, contractions on bf16 MFMAs) next to the default fp32 kernel
(csrc/kernels/dense_minibatch.hip), both through ``nn.Model.fit(engine="persistent")``.

Per stack of ``bench_dense_minibatch.STACKS``, in a child process under its own timeout, at Keras
batches 32 and 100: one warm-up ``fit`` per precision, then ``--runs`` timed one-epoch fits per
precision, the two alternating (shuffle off, device-resident rows, ``verbose=0``, ``--steps`` steps
per epoch).  Reported: us per step and rows/s (median, min, max over the runs).  bf16 "wins" a row
when its median step time is below fp32's by more than fp32's own spread (max - min), the rule of
bench_dense_minibatch.py.

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

from bench_dense_minibatch import BATCHES, STACKS  # noqa: E402

KERNEL = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd",
                      "csrc", "kernels", "dense_minibatch_bf16.hip")
PRECISIONS = ("fp32", "bf16")


def _model(idx, dev, precision):
    from streamml import nn
    from streamml.nn.layers import Dense
    _, feat, widths, acts = STACKS[idx]
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=1)
    m.compile(loss="mse", metrics=["accuracy"], minibatch_precision=precision)
    return m


def child(idx: int, steps: int, runs: int) -> list:
    import numpy as np
    import torch

    name, feat, _, _ = STACKS[idx]
    dev = torch.device("cuda", 0)
    out = []
    for batch in BATCHES:
        x = torch.rand(steps * batch, feat, device=dev)
        models = {p: _model(idx, dev, p) for p in PRECISIONS}
        times = {p: [] for p in PRECISIONS}
        for r in range(runs + 1):                      # run 0 warms both kernels up
            for p in PRECISIONS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                models[p].fit(x, batch_size=batch, epochs=1, shuffle=False, verbose=0, engine="persistent")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert models[p].last_fit_engine == "persistent" and models[p].last_fit_precision == p
                if r:
                    times[p].append(dt / steps * 1e6)
        row = {"stack": name, "batch": batch, "params": models["fp32"].count_params(), "steps_per_epoch": steps}
        for p, t in times.items():
            row[p] = {"us_per_step": float(np.median(t)), "us_per_step_min": float(min(t)),
                      "us_per_step_max": float(max(t)), "rows_per_s": batch / float(np.median(t)) * 1e6}
        f, b = row["fp32"], row["bf16"]
        row["speedup"] = f["us_per_step"] / b["us_per_step"]
        row["bf16_wins"] = bool(f["us_per_step"] - b["us_per_step"] > f["us_per_step_max"] - f["us_per_step_min"])
        out.append(row)
    return out


def kernel_resources() -> str:
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), KERNEL, "dense_mb"],
                           capture_output=True, text=True, timeout=300)
        return r.stdout.strip()
    except Exception as e:   # noqa: BLE001 (the table is an extra)
        return f"(tools/kernel_resources.py did not run: {e})"


def summary(results, resources) -> str:
    out = ["# Persistent Dense trainer: bf16-MFMA kernel vs fp32 kernel (MI355X)", "",
           "`compile(minibatch_precision=\"bf16\")` runs `dense_minibatch_bf16.hip` (every contraction on",
           "`v_mfma_f32_16x16x32_bf16`, fp32 master weights and Adam in the owners' registers); the default is",
           "`dense_minibatch.hip` (fp32 `fmaf` tiles).  One-epoch `fit(engine=\"persistent\")` calls on",
           "device-resident rows, shuffle off, the two precisions alternating; median (min .. max) over the timed",
           "runs.  A step's time is the whole `fit()` call divided by its steps.", "",
           "| stack | params | batch | fp32 us/step | fp32 rows/s | bf16 us/step | bf16 rows/s | bf16 speed-up | "
           "bf16 beats fp32 by more than fp32's spread |",
           "|---|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | | | |")
            continue
        f, b = r["fp32"], r["bf16"]
        out.append(f"| {r['stack']} | {r['params']:,} | {r['batch']} | {f['us_per_step']:.1f} "
                   f"({f['us_per_step_min']:.1f} .. {f['us_per_step_max']:.1f}) | {f['rows_per_s']:,.0f} | "
                   f"{b['us_per_step']:.1f} ({b['us_per_step_min']:.1f} .. {b['us_per_step_max']:.1f}) | "
                   f"{b['rows_per_s']:,.0f} | {r['speedup']:.2f}x | {'yes' if r['bf16_wins'] else 'NO'} |")
    lost = [f"{r['stack']} at batch {r['batch']}" for r in results if "error" not in r and not r["bf16_wins"]]
    out += ["", "Rows bf16 does not win (use fp32 there): " + (", ".join(lost) if lost else "none") + "."]
    out += ["", "Kernel resources (`tools/kernel_resources.py`; spillV / spillS are the registers spilled to",
            "scratch / to VGPR lanes -- a kernel with spillV 0 has no private segment):", "", "```", resources, "```"]
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--steps", type=int, default=2000, help="steps per epoch")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=150.0, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "dense_minibatch_bf16"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child, args.steps, max(args.runs, 3))), flush=True)
        return 0
    results, ok = [], True
    for i, (name, _, _, _) in enumerate(STACKS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i), "--steps", str(args.steps), "--runs",
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
        json.dump({"stacks": results}, f, indent=1)
    with open(os.path.join(args.out, "SUMMARY.md"), "w") as f:
        f.write(summary(results, kernel_resources()))
    print(json.dumps({"bench": "dense_minibatch_bf16", "results": results}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
