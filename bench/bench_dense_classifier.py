#!/usr/bin/env python3
"""Training softmax classifiers: ``fit(engine="wide")`` (the softmax head of csrc/kernels/dense_batch_wide.hip,
four launches per step) next to ``fit(engine="layers")`` (a GEMM launch per layer and direction, the
cross-entropy kernel or eager log_softmax, one Adam launch), the only other trainer such a model has.

Per stack of STACKS, in a child process under its own timeout, at batch 4096: one warm-up ``fit`` per
engine, then RUNS timed one-epoch fits per engine, the two alternating (shuffle off, device-resident rows
and labels, ``verbose=0``, STEPS steps per epoch).  Reported: rows per second, median (min .. max); a fit's
time is the whole ``fit()`` call, ended by a device synchronise.  No threshold: the ratio is recorded.

Prints one JSON line; ``--out`` also writes ``results.json`` there.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STACKS = [("18-64-2", 18, (64, 2), ("tanh", "softmax")), ("30-512-512-10", 30, (512, 512, 10), ("tanh", "relu", "softmax"))]
BATCH = 4096
STEPS = 60
ENGINES = ("layers", "wide")
RUNS = 5


def child(idx: int) -> dict:
    import numpy as np
    import torch
    from streamml import nn
    from streamml.nn.layers import Dense

    name, feat, widths, acts = STACKS[idx]
    dev = torch.device("cuda", 0)
    x = torch.rand(STEPS * BATCH, feat, device=dev)
    y = torch.randint(0, widths[-1], (STEPS * BATCH,), device=dev)
    models, times = {}, {e: [] for e in ENGINES}
    for e in ENGINES:
        models[e] = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                                   for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=1)
        models[e].compile(loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    for r in range(RUNS + 1):                      # run 0 warms both engines up
        for e in ENGINES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            models[e].fit(x, y, batch_size=BATCH, epochs=1, shuffle=False, verbose=0, engine=e)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert models[e].last_fit_engine == e
            if r:
                times[e].append(STEPS * BATCH / dt)
    row = {"stack": name, "batch": BATCH, "steps_per_epoch": STEPS, "runs": RUNS}
    for e, t in times.items():
        row[e] = {"rows_per_s": float(np.median(t)), "rows_per_s_min": float(min(t)), "rows_per_s_max": float(max(t))}
    row["speedup"] = row["wide"]["rows_per_s"] / row["layers"]["rows_per_s"]
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child >= 0:
        print("RESULT " + json.dumps(child(args.child)), flush=True)
        return 0
    results, ok = [], True
    for i, stack in enumerate(STACKS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            err = "" if r.returncode == 0 and line else f"exit {r.returncode}: {r.stderr.strip()[-300:]}"
        except subprocess.TimeoutExpired:
            err = f"timed out after {args.timeout:.0f} s"
        if err:
            results.append({"stack": stack[0], "error": err})
            ok = False
            break   # nothing more on a device that may be hung
        results.append(json.loads(line[-1][7:]))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "results.json"), "w") as f:
            json.dump({"stacks": results}, f, indent=1)
    print(json.dumps({"bench": "dense_classifier", "results": results}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
