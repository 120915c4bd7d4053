#!/usr/bin/env python3
"""Training the MNIST classifier at the reference's batches: ``fit(engine="fused")`` (the two-launch fp32
step of csrc/kernels/mlp_step.hip) next to ``fit(engine="layers")`` (eight launches per step).

Four cells: batch 1 and batch 32, for Dense(128) and for Dense(512) + Dropout(0.2), on ``uint8`` rows.  Per
cell: one warm-up ``fit`` per engine, then RUNS timed fits per engine, the two alternating; a fit is STEPS
steps (whole epochs over at most 8192 rows, shuffled) and its time is the whole ``fit()`` call, ended by a
device synchronise.  Reported: steps per second, median (min .. max).  Then the sweep of the backward
launch's workgroups: ``ops.mlp_step.train_steps(groups=g)`` for STEPS steps per call, same statistics
(0 = the default, one workgroup per ROWS_PER_GROUP rows of W1).

Prints one JSON line; ``--out`` also writes ``results.json`` there.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = [(128, 0.0, 1), (128, 0.0, 32), (512, 0.2, 1), (512, 0.2, 32)]   # hidden, dropout, batch
STEPS = 2048
RUNS = 5
ENGINES = ("layers", "fused")
GROUPS = (0, 4, 8, 16, 32, 49, 64, 98, 128, 196, 256)


def _stats(v):
    import numpy as np
    return {"steps_per_s": float(np.median(v)), "steps_per_s_min": float(min(v)), "steps_per_s_max": float(max(v))}


def cell(hidden: int, rate: float, batch: int, sweep: bool) -> dict:
    import numpy as np
    import torch
    from streamml.models.mlp import MLPClassifier
    from streamml.ops import mlp_step

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    n = min(8192, STEPS * batch)
    epochs = STEPS * batch // n
    x = rng.integers(0, 256, (n, 28, 28), dtype=np.uint8)
    y = rng.integers(0, 10, n).astype(np.int64)
    models = {e: MLPClassifier(hidden=hidden, dropout=rate, device=dev, seed=1) for e in ENGINES}
    times = {e: [] for e in ENGINES}
    for r in range(RUNS + 1):                      # run 0 warms both engines up
        for e in ENGINES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            models[e].fit(x, y, batch_size=batch, epochs=epochs, verbose=0, seed=r, engine=e)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert models[e].last_fit_engine == e
            if r:
                times[e].append(STEPS / dt)
    row = {"hidden": hidden, "dropout": rate, "batch": batch, "steps": STEPS, "runs": RUNS}
    for e in ENGINES:
        row[e] = _stats(times[e])
    row["speedup"] = row["fused"]["steps_per_s"] / row["layers"]["steps_per_s"]
    if sweep:
        xd = torch.as_tensor(x).to(dev).reshape(n, -1)
        yd = torch.as_tensor(y).to(dev)
        order = torch.randperm(STEPS * batch, device=dev) % n
        model = models["fused"]
        row["groups"] = {}
        for r in range(RUNS + 1):
            for g in GROUPS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mlp_step.train_steps(model, xd, yd, order, batch, STEPS, groups=g)
                torch.cuda.synchronize()
                if r:
                    row["groups"].setdefault(str(g), []).append(STEPS / (time.perf_counter() - t0))
        row["groups"] = {g: _stats(v) for g, v in row["groups"].items()}
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-sweep", action="store_true", help="skip the sweep of the backward's workgroups")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    results = [cell(h, r, b, not args.no_sweep) for h, r, b in CELLS]
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "results.json"), "w") as f:
            json.dump({"cells": results}, f, indent=1)
    print(json.dumps({"bench": "mlp_step", "results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
