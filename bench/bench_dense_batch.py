#!/usr/bin/env python3
"""Large-batch training of Dense stacks: ``fit(engine="throughput")`` (csrc/kernels/dense_batch.hip, two
launches per step) next to ``fit(engine="layers")`` (the layer loop, about twenty launches per step).

Per stack of ``bench_dense_minibatch.STACKS``, in a child process under its own timeout, at batches
256, 1024, 4096 and 65 536: one warm-up ``fit`` per engine, then ``--runs`` timed one-epoch fits per
engine, the two alternating (shuffle off, device-resident rows, ``verbose=0``, STEPS[batch] steps per
epoch).  Reported: us per step and rows/s (median, min, max over the runs); a step's time is the whole
``fit()`` call, ended by a device synchronise, divided by its steps.  Throughput "wins" a row when its
median step time is below the layer loop's by more than the layer loop's own spread (max - min).

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

from bench_dense_minibatch import STACKS  # noqa: E402

KERNEL = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd",
                      "csrc", "kernels", "dense_batch.hip")
STEPS = {256: 400, 1024: 400, 4096: 200, 65536: 32}   # steps per epoch: a timed window of 0.1 s or more
ENGINES = ("layers", "throughput")


def _model(idx, dev):
    from streamml import nn
    from streamml.nn.layers import Dense
    _, feat, widths, acts = STACKS[idx]
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=1)
    m.compile(loss="mse", metrics=["accuracy"])
    return m


def child(idx: int, runs: int) -> list:
    import numpy as np
    import torch

    from streamml.ops import dense_persistent as dpers

    name, feat, widths, _ = STACKS[idx]
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    out = []
    for batch, steps in STEPS.items():
        x = torch.rand(steps * batch, feat, device=dev)
        models = {e: _model(idx, dev) for e in ENGINES}
        times = {e: [] for e in ENGINES}
        for r in range(runs + 1):                      # run 0 warms both engines up
            for e in ENGINES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                models[e].fit(x, batch_size=batch, epochs=1, shuffle=False, verbose=0, engine=e)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert models[e].last_fit_engine == e
                if r:
                    times[e].append(dt / steps * 1e6)
        row = {"stack": name, "batch": batch, "params": models["layers"].count_params(), "steps_per_epoch": steps,
               "groups": min(cus, -(-batch // dpers.CHUNK)),
               "lds_bytes": dpers.lds_bytes([feat] + list(widths), False, "bf16")}
        for e, t in times.items():
            row[e] = {"us_per_step": float(np.median(t)), "us_per_step_min": float(min(t)),
                      "us_per_step_max": float(max(t)), "rows_per_s": batch / float(np.median(t)) * 1e6}
        lay, thr = row["layers"], row["throughput"]
        row["speedup"] = lay["us_per_step"] / thr["us_per_step"]
        row["throughput_wins"] = bool(lay["us_per_step"] - thr["us_per_step"] >
                                      lay["us_per_step_max"] - lay["us_per_step_min"])
        out.append(row)
    return out


def kernel_resources() -> str:
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), KERNEL, "dense_batch"],
                           capture_output=True, text=True, timeout=300)
        return r.stdout.strip()
    except Exception as e:   # noqa: BLE001 (the table is an extra)
        return f"(tools/kernel_resources.py did not run: {e})"


def summary(results, resources) -> str:
    out = ["# Large-batch Dense training: the fused two-launch step vs the layer loop (MI355X)", "",
           "`fit(engine=\"throughput\")` runs `dense_batch.hip`: a gradient launch of G workgroups (one per CU, at",
           "most one per 32-row chunk) on `v_mfma_f32_16x16x32_bf16`, then a reduce + Adam launch.",
           "`fit(engine=\"layers\")` is the layer loop.  One-epoch `fit()` calls on device-resident rows, shuffle",
           "off, the two engines alternating; median (min .. max) over the timed runs.  A step's time is the whole",
           "`fit()` call divided by its steps.", "",
           "| stack | params | batch | G | layers us/step | layers rows/s | throughput us/step | throughput rows/s | "
           "speed-up | throughput beats layers by more than layers' spread |",
           "|---|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['error']} | | | | | | | | |")
            continue
        a, b = r["layers"], r["throughput"]
        out.append(f"| {r['stack']} | {r['params']:,} | {r['batch']} | {r['groups']} | {a['us_per_step']:.1f} "
                   f"({a['us_per_step_min']:.1f} .. {a['us_per_step_max']:.1f}) | {a['rows_per_s']:,.0f} | "
                   f"{b['us_per_step']:.1f} ({b['us_per_step_min']:.1f} .. {b['us_per_step_max']:.1f}) | "
                   f"{b['rows_per_s']:,.0f} | {r['speedup']:.2f}x | {'yes' if r['throughput_wins'] else 'NO'} |")
    good = [r for r in results if "error" not in r]
    lost = [f"{r['stack']} at batch {r['batch']}" for r in good if not r["throughput_wins"]]
    out += ["", "Rows throughput does not win (it stops winning there): " + (", ".join(lost) if lost else "none") + "."]
    lds = sorted({(r["stack"], r["lds_bytes"]) for r in good})
    out += ["", "LDS of the gradient kernel's plan (dynamic + static): " +
            ", ".join(f"{s} {b:,} bytes ({'two workgroups' if b <= 80 * 1024 else 'one workgroup'} per CU)"
                      for s, b in lds) + "."]
    out += ["", "Kernel resources (`tools/kernel_resources.py`; spillV / spillS are the registers spilled to",
            "scratch / to VGPR lanes -- a kernel with spillV 0 has no private segment; occ is waves per SIMD, of",
            "which a 512-thread workgroup takes two):", "", "```", resources, "```"]
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "dense_batch"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child, max(args.runs, 3))), flush=True)
        return 0
    results, ok = [], True
    for i, (name, _, _, _) in enumerate(STACKS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i), "--runs", str(args.runs)]
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
    print(json.dumps({"bench": "dense_batch", "results": results}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
