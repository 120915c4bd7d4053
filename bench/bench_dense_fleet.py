#!/usr/bin/env python3
"""Fleets of Dense stacks (``ops.dense_fleet.DenseFleet``: one launch, one persistent workgroup per
model) at growing fleet sizes, next to the only other way to train M such models: M sequential
single-model ``dense_persistent.train_steps`` launches.

Per stack of ``bench_dense_minibatch.STACKS`` and precision, in a child process under its own
timeout, at Keras batch 32: fleets of M in {1, 64, #CUs, 2 x #CUs} models, every model on ``--steps``
steps of its own device-resident rows.  One warm-up launch, then ``--runs`` timed one-epoch launches
(``train_epoch``: host descriptors, upload, launch, synchronize).  Reported: the fleet's rows/s, and
the per-model rate relative to M = 1 (1.0 = the fleet costs a model nothing), each as median
(min .. max) over the runs.  The same child times 64 sequential single-model launches of the same
steps (models and rows resident, one synchronize at the end).

Writes ``SUMMARY.md`` and ``results.json`` into ``--out`` and prints one JSON line.  If
``bench/ab_dense_single.py`` (the single-model path on the parent's build and on this one) left its
table in ``--out``, the summary ends with it.
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

KERNELS = [os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd",
                        "csrc", "kernels", f) for f in ("dense_minibatch.hip", "dense_minibatch_bf16.hip")]
PRECISIONS = ("fp32", "bf16")
BATCH = 32
SEQUENTIAL_M = 64


def _model(idx, dev, precision, seed):
    from streamml import nn
    from streamml.nn.layers import Dense
    _, feat, widths, acts = STACKS[idx]
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=seed)
    m.compile(loss="mse", metrics=["accuracy"], fused=False if str(dev) == "cpu" else None, minibatch_precision=precision)
    return m


def _stats(ts):
    import numpy as np
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def child(idx: int, precision: str, steps: int, runs: int) -> dict:
    import torch

    from streamml.ops import dense_persistent as dpers
    from streamml.ops.dense_fleet import DenseFleet

    name, feat, _, _ = STACKS[idx]
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sizes = sorted({1, SEQUENTIAL_M, cus, 2 * cus})
    rows_per_model = steps * BATCH
    out = {"stack": name, "precision": precision, "batch": BATCH, "steps": steps, "cus": cus, "fleets": [],
           "lds_bytes": dpers.lds_bytes([feat] + list(STACKS[idx][2]), False, precision)}
    members = [_model(idx, "cpu", precision, seed) for seed in range(max(sizes))]
    x = torch.rand(max(sizes), rows_per_model, feat, device=dev)
    for M in sizes:
        fleet = DenseFleet(members[:M], dev, precision=precision)
        fleet.attach_rows(x[:M], BATCH)
        times = []
        for r in range(runs + 1):                        # run 0 warms the kernel up
            fleet.reset_metrics()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fleet.train_epoch()
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
        assert int(fleet.iter.min().item()) == int(fleet.iter.max().item()) == (runs + 1) * steps
        out["fleets"].append({"models": M, "seconds": _stats(times),
                              "rows_per_s": _stats([M * rows_per_model / t for t in times])})
    one = out["fleets"][0]["seconds"]["median"]
    for f in out["fleets"]:
        # a model's rate in the fleet over its rate alone; (min .. max) from the fleet's slowest and fastest run
        f["per_model_rate_vs_alone"] = {"median": one / f["seconds"]["median"], "min": one / f["seconds"]["max"],
                                        "max": one / f["seconds"]["min"]}
    # the other way to train SEQUENTIAL_M models today: one single-model launch each, back to back
    alone = [_model(idx, dev, precision, seed) for seed in range(SEQUENTIAL_M)]
    times = []
    for r in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, mdl in enumerate(alone):
            dpers.train_steps(mdl, x[i], None, BATCH, steps, precision=precision)
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    out["sequential"] = {"models": SEQUENTIAL_M, "seconds": _stats(times),
                         "rows_per_s": _stats([SEQUENTIAL_M * rows_per_model / t for t in times])}
    return out


def kernel_resources() -> str:
    text = []
    for k in KERNELS:
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), k, "dense_mb"],
                               capture_output=True, text=True, timeout=300)
            lines = r.stdout.strip().splitlines()
            text += lines if not text else lines[1:]
        except Exception as e:   # noqa: BLE001 (the table is an extra)
            text.append(f"(tools/kernel_resources.py did not run on {os.path.basename(k)}: {e})")
    return "\n".join(text)


def _mmm(s, fmt):
    return f"{s['median']:{fmt}} ({s['min']:{fmt}} .. {s['max']:{fmt}})"


def summary(results, resources) -> str:
    out = ["# Fleets of Dense stacks: one persistent workgroup per model (MI355X)", "",
           "`DenseFleet.train_epoch()` is ONE launch of the fleet entry of `dense_minibatch.hip` (fp32) or",
           "`dense_minibatch_bf16.hip` (bf16): workgroup b trains model `sched[b]` on its own device-resident rows,",
           f"batch {BATCH}.  Times are whole `train_epoch()` calls (host descriptors, upload, launch, synchronize); median",
           "(min .. max) over the timed runs.  \"per-model rate vs alone\" is a member's rows/s over the rows/s of the",
           "M = 1 fleet: 1.0 means a model trains as fast among M - 1 others as alone.  A workgroup fills a CU (8 waves at",
           "about 250 VGPRs), so a fleet of more models than CUs runs in rounds.", "",
           "| stack | precision | models | steps each | seconds | fleet rows/s | per-model rate vs alone |",
           "|---|---|---:|---:|---:|---:|---:|"]
    for r in results:
        if "error" in r:
            out.append(f"| {r['stack']} | {r['precision']} | {r['error']} | | | | |")
            continue
        for f in r["fleets"]:
            out.append(f"| {r['stack']} | {r['precision']} | {f['models']} | {r['steps']} | {_mmm(f['seconds'], '.4f')} | "
                       f"{_mmm(f['rows_per_s'], ',.0f')} | {_mmm(f['per_model_rate_vs_alone'], '.2f')} |")
    out += ["", f"The same {SEQUENTIAL_M} models as {SEQUENTIAL_M} sequential single-model `dense_persistent.train_steps` "
            "launches (one CU busy at a time):", "",
            "| stack | precision | models | seconds | rows/s | the fleet of as many models is faster by |", "|---|---|---:|---:|---:|---:|"]
    for r in results:
        if "error" in r:
            continue
        s = r["sequential"]
        f = [f for f in r["fleets"] if f["models"] == s["models"]][0]
        out.append(f"| {r['stack']} | {r['precision']} | {s['models']} | {_mmm(s['seconds'], '.3f')} | "
                   f"{_mmm(s['rows_per_s'], ',.0f')} | {s['seconds']['median'] / f['seconds']['median']:.1f}x |")
    out += ["", "Kernel resources (`tools/kernel_resources.py`; spillV / spillS are the registers spilled to scratch / to",
            "VGPR lanes -- a kernel with spillV 0 has no private segment; LDS is the static part, the layer tables):", "",
            "```", resources, "```", "",
            "LDS per workgroup with the plan of each stack (`dense_persistent.lds_bytes`, the same for both entries of a kernel): "
            + ", ".join(f"{r['stack']} {r['precision']} {r['lds_bytes']:,} bytes" for r in results if "error" not in r) + "."]
    return "\n".join(out) + "\n"


def _run_child(args, idx, precision):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(idx), "--precision", precision, "--steps",
           str(args.steps), "--runs", str(args.runs)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        return None, f"timed out after {args.timeout:.0f} s"
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        return None, f"exit {r.returncode}: {r.stderr.strip()[-300:]}"
    return json.loads(line[-1][7:]), ""


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--precision", default="fp32", choices=PRECISIONS)
    ap.add_argument("--steps", type=int, default=2000, help="steps per model per launch")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--resources", default=None, help="a file holding the kernel-resource table (default: compile now)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "dense_fleet"))
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child, args.precision, args.steps, max(args.runs, 3))), flush=True)
        return 0
    results, ok = [], True
    for i, (name, _, _, _) in enumerate(STACKS):
        for p in PRECISIONS:
            if not ok:
                break
            res, err = _run_child(args, i, p)
            if res is None:
                results.append({"stack": name, "precision": p, "error": err})
                ok = False   # nothing more on a device that may be hung
            else:
                results.append(res)
    if args.resources:
        with open(args.resources) as f:
            resources = f.read().strip()
    else:
        resources = kernel_resources()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "results.json"), "w") as f:
        json.dump({"fleets": results}, f, indent=1)
    text = summary(results, resources)
    ab = os.path.join(args.out, "SINGLE_MODEL_AB.md")     # bench/ab_dense_single.py, run into the same directory
    if os.path.exists(ab):
        with open(ab) as f:
            text += "\n" + f.read()
    with open(os.path.join(args.out, "SUMMARY.md"), "w") as f:
        f.write(text)
    print(json.dumps({"bench": "dense_fleet", "results": results}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
