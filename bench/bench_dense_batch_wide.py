#!/usr/bin/env python3
"""Large-batch training of WIDE Dense stacks: ``fit(engine="wide")`` (csrc/kernels/dense_batch_wide.hip,
four launches per step) next to ``fit(engine="layers")`` (the layer loop), the only other trainer these
stacks have.

Per stack of STACKS, in a child process under its own timeout, at batches 1 024, 8 192 and 65 536: one
warm-up ``fit`` per engine, then three timed one-epoch fits per engine, the two alternating (shuffle
off, device-resident rows, ``verbose=0``, STEPS[batch] steps per epoch).  Reported: us per step, median
(min .. max) of the three; a step's time is the whole ``fit()`` call, ended by a device synchronise,
divided by its steps.  Wide "wins" a row when its SLOWEST call beats the layer loop's FASTEST.

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

KERNEL = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd",
                      "csrc", "kernels", "dense_batch_wide.hip")
STACKS = [("18-512-128-512-18", 18, (512, 128, 512, 18)), ("18-512-512-512-18", 18, (512, 512, 512, 18))]
ACTS = ("tanh", "relu", "tanh", "relu")
STEPS = {1024: 200, 8192: 60, 65536: 12}   # steps per epoch: a timed window of some 0.1 s on the layer loop
ENGINES = ("layers", "wide")
RUNS = 3


def _model(idx, dev):
    from streamml import nn
    from streamml.nn.layers import Dense
    _, feat, widths = STACKS[idx]
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, ACTS))], device=dev, seed=1)
    m.compile(loss="mse", metrics=["accuracy"])
    return m


def child(idx: int) -> list:
    import numpy as np
    import torch

    name, feat, _ = STACKS[idx]
    dev = torch.device("cuda", 0)
    out = []
    for batch, steps in STEPS.items():
        x = torch.rand(steps * batch, feat, device=dev)
        models = {e: _model(idx, dev) for e in ENGINES}
        times = {e: [] for e in ENGINES}
        for r in range(RUNS + 1):                      # run 0 warms both engines up
            for e in ENGINES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                models[e].fit(x, batch_size=batch, epochs=1, shuffle=False, verbose=0, engine=e)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert models[e].last_fit_engine == e
                if r:
                    times[e].append(dt / steps * 1e6)
        row = {"stack": name, "batch": batch, "params": models["layers"].count_params(), "steps_per_epoch": steps}
        for e, t in times.items():
            row[e] = {"us_per_step": float(np.median(t)), "us_per_step_min": float(min(t)),
                      "us_per_step_max": float(max(t)), "rows_per_s": batch / float(np.median(t)) * 1e6}
        row["speedup"] = row["layers"]["us_per_step"] / row["wide"]["us_per_step"]
        row["wide_wins"] = bool(row["wide"]["us_per_step_max"] < row["layers"]["us_per_step_min"])
        out.append(row)
    return out


def kernel_resources() -> str:
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), KERNEL, "dense_batchw"],
                           capture_output=True, text=True, timeout=300)
        return r.stdout.strip()
    except Exception as e:   # noqa: BLE001 (the table is an extra)
        return f"(tools/kernel_resources.py did not run: {e})"


def summary(results, resources) -> str:
    out = ["# Large-batch training of wide Dense stacks: the fused four-launch step vs the layer loop (MI355X)", "",
           "`fit(engine=\"wide\")` runs `dense_batch_wide.hip`: the two bf16 weight images, a persistent forward +",
           "backward grid over 64-row tiles on `v_mfma_f32_16x16x32_bf16`, one grouped weight-gradient launch, then",
           "`dense_batch.hip`'s reduce + Adam launch.  `fit(engine=\"layers\")` is the layer loop.  One-epoch `fit()`",
           "calls on device-resident rows, shuffle off, the two engines alternating; median (min .. max) of three.",
           "A step's time is the whole `fit()` call divided by its steps.", "",
           "| stack | params | batch | layers us/step | wide us/step | wide rows/s | speed-up (medians) | "
           "wide's slowest call beats layers' fastest |",
           "|---|---:|---:|---:|---:|---:|---:|---|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | | |")
            continue
        a, b = r["layers"], r["wide"]
        out.append(f"| {r['stack']} | {r['params']:,} | {r['batch']} | {a['us_per_step']:.1f} "
                   f"({a['us_per_step_min']:.1f} .. {a['us_per_step_max']:.1f}) | "
                   f"{b['us_per_step']:.1f} ({b['us_per_step_min']:.1f} .. {b['us_per_step_max']:.1f}) | "
                   f"{b['rows_per_s']:,.0f} | {r['speedup']:.2f}x | {'yes' if r['wide_wins'] else 'NO'} |")
    lost = [f"{r['stack']} at batch {r['batch']}" for r in results if "error" not in r and not r["wide_wins"]]
    out += ["", "Rows where wide does not win: " + (", ".join(lost) if lost else "none") + "."]
    out += ["", "Kernel resources (`tools/kernel_resources.py`; spillV / spillS are the registers spilled to",
            "scratch / to VGPR lanes -- a kernel with spillV 0 has no private segment; occ is waves per SIMD, of",
            "which the 512-thread forward + backward workgroup takes two; its LDS column is the static part, the",
            "dynamic part is 64 x (widest padded row + 8) x 2 + bias sums + 10 240 bytes: 81 KiB for 18-512-512-512-18):", "",
            "```", resources, "```"]
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "dense_batch_wide"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child)), flush=True)
        return 0
    results, ok = [], True
    for i, (name, _, _) in enumerate(STACKS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i)]
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
    print(json.dumps({"bench": "dense_batch_wide", "results": results}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
