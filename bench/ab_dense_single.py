#!/usr/bin/env python3
"""Does a change to the persistent Dense trainer slow the single-model path down?  Alternates two
builds of the extension (``--parent-so``: ``_C.so`` built from the parent commit, ``--new-so``: the
one built from this tree) under the children of ``bench_dense_minibatch.py`` and
``bench_dense_minibatch_bf16.py`` in ONE job: ``--rounds`` rounds of parent, new, each child with its
own three timed one-epoch ``fit(engine="persistent")`` calls of 2 000 steps.

A row passes when the new build's median us/step exceeds the parent's by no more than the parent's
own spread (max - min over all its runs of the job): the only noise figure there is for these kernels.

The build under test is copied over the package's ``_C.so`` for the duration of a child and the new
build is put back at the end.  Writes ``single_model_ab.json`` and ``SINGLE_MODEL_AB.md`` into
``--out`` (``bench_dense_fleet.py`` appends the latter to its summary) and prints the table.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd")
SO = os.path.join(PKG, "_C.so")
CHILD = {
    "bench_dense_minibatch": "import json, sys; sys.path.insert(0, 'bench'); import bench_dense_minibatch as b; "
                             "print('RESULT ' + json.dumps(b.child(%d, 2000, 300, 3)))",
    "bench_dense_minibatch_bf16": "import json, sys; sys.path.insert(0, 'bench'); import bench_dense_minibatch_bf16 as b; "
                                  "print('RESULT ' + json.dumps(b.child(%d, 2000, 3)))",
}
KERNELS = ("persistent", "fp32", "bf16")     # the rows' keys that time the persistent trainer


def table(runs) -> str:
    import numpy as np
    cells = {}
    for r in runs:
        for row in r["rows"]:
            for k in KERNELS:
                if k in row:
                    key = (r["bench"], row["stack"], row["batch"], k)
                    c = cells.setdefault(key, {"parent": {"med": [], "lo": [], "hi": []}, "new": {"med": [], "lo": [], "hi": []}})
                    c[r["build"]]["med"].append(row[k]["us_per_step"])
                    c[r["build"]]["lo"].append(row[k]["us_per_step_min"])
                    c[r["build"]]["hi"].append(row[k]["us_per_step_max"])
    out = ["| bench | stack | batch | kernel | parent us/step | new us/step | new - parent | parent's spread | within it |",
           "|---|---|---:|---|---:|---:|---:|---:|---|"]
    for (bench, stack, batch, k), c in cells.items():
        p, n = c["parent"], c["new"]
        pm, nm = float(np.median(p["med"])), float(np.median(n["med"]))
        spread = max(p["hi"]) - min(p["lo"])
        out.append(f"| {bench} | {stack} | {batch} | {k} | {pm:.2f} ({min(p['lo']):.2f} .. {max(p['hi']):.2f}) | "
                   f"{nm:.2f} ({min(n['lo']):.2f} .. {max(n['hi']):.2f}) | {nm - pm:+.2f} | {spread:.2f} | "
                   f"{'yes' if nm - pm <= spread else 'NO'} |")
    return "\n".join(out)


def alternate(builds, rounds, timeout):
    """(runs, ok); stops at the first child that fails: nothing more on a device that may be in trouble."""
    runs = []
    for rnd in range(rounds):
        for build, path in builds.items():
            shutil.copyfile(path, SO)
            for bench, code in CHILD.items():
                for idx in (0, 1):
                    try:
                        r = subprocess.run([sys.executable, "-c", code % idx], cwd=ROOT, capture_output=True, text=True,
                                           timeout=timeout, env=dict(os.environ, SML_NO_AUTOBUILD="1"))
                    except subprocess.TimeoutExpired:
                        print(f"{build} {bench} stack {idx}: timed out after {timeout:.0f} s", flush=True)
                        return runs, False
                    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                    if r.returncode != 0 or not line:
                        print(f"{build} {bench} stack {idx}: exit {r.returncode}: {r.stderr.strip()[-600:]}", flush=True)
                        return runs, False
                    runs.append({"round": rnd, "build": build, "bench": bench, "rows": json.loads(line[-1][7:])})
                    print(f"round {rnd} {build} {bench} stack {idx} done", flush=True)
    return runs, True


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-so", required=True)
    ap.add_argument("--new-so", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=200.0, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "dense_fleet"))
    args = ap.parse_args()
    builds = {"parent": os.path.abspath(args.parent_so), "new": os.path.abspath(args.new_so)}
    os.makedirs(args.out, exist_ok=True)
    try:
        runs, ok = alternate(builds, args.rounds, args.timeout)
    finally:
        shutil.copyfile(builds["new"], SO)
    with open(os.path.join(args.out, "single_model_ab.json"), "w") as f:
        json.dump(runs, f, indent=1)
    text = ("## The single-model path, parent build and new build alternating in one job\n\n"
            f"`bench/ab_dense_single.py`, {args.rounds} rounds of (parent, new); per build the median of the children's median "
            "us/step and (min .. max) over all their timed runs.\n\n" + table(runs) + "\n")
    with open(os.path.join(args.out, "SINGLE_MODEL_AB.md"), "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
