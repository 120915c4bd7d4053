"""Bulk scoring of a Dense fleet: ``DenseFleet.score`` (one fused launch, dense_forward_fleet.hip) against
the loop it replaces, ``ops.dense_forward.forward`` once per member on that member's slice of the same
device-resident rows.

The loop's members are eight ``fleet.model(i)`` objects built once and taken in turn: a call costs what
it would for 4 096 distinct models (the image gather and the launch), without 4 096 model objects.  The
fleet launch is timed with both ways of bringing the next image into LDS (global-to-LDS loads; a copy
through registers).  The three paths alternate in one process; each figure is the median and min .. max
of ``--rounds`` windows that end in a device synchronise.

  python bench/bench_dense_fleet_forward.py [--out SUMMARY.md] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from streamml import nn  # noqa: E402
from streamml.nn.layers import Dense  # noqa: E402
from streamml.nn.model import Adam  # noqa: E402
from streamml.ops import dense_fleet_forward as dff  # noqa: E402
from streamml.ops import dense_forward as dfw  # noqa: E402
from streamml.ops.dense_fleet import DenseFleet  # noqa: E402

STACKS = {"18-64-16-64-18": (18, [64, 16, 64, 18]), "30-128-32-128-30": (30, [128, 32, 128, 30])}
ACTS = ["tanh", "relu", "tanh", "linear"]


def template(features, widths, dev):
    m = nn.Sequential([Dense(u, a, input_shape=(features,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, ACTS))], device=dev, seed=1)
    m.compile(optimizer=Adam(learning_rate=1e-3), loss="mean_squared_error", metrics=["accuracy"])
    return m


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(name, M, rows, rounds, dev):
    features, widths = STACKS[name]
    fleet = DenseFleet([template(features, widths, dev)] * M, dev)
    fleet.flat.copy_(torch.randn(fleet.flat.shape, generator=torch.Generator(dev).manual_seed(M), device=dev) * 0.1)
    x = torch.rand((M * rows, features), device=dev)
    table = np.stack([np.arange(M, dtype=np.int64) * rows, np.full(M, rows, np.int64)], axis=1)
    members = [fleet.model(i) for i in range(min(M, 8))]
    for i, mdl in enumerate(members):      # the loop's members carry the weights of fleet members 0 .. 7
        assert torch.equal(mdl.fp.flat[:fleet.nflat], fleet.flat[i, :fleet.nflat])

    def loop():
        for i in range(M):
            dfw.forward(members[i % len(members)], x[i * rows:(i + 1) * rows], rec=False, score=True)

    def fused(async_copy):
        def run():
            dff.ASYNC_COPY = async_copy
            fleet.score(x, table)
        return run

    paths = {"fleet": fused(True), "fleet_plain_copy": fused(False), "loop": loop}
    # the same scores, bit for bit, on the members both paths hold
    s = fleet.score(x, table)
    for i in range(len(members)):
        one = dfw.forward(members[i], x[i * rows:(i + 1) * rows], rec=False, score=True)[1]
        assert torch.equal(one.view(torch.int32), s[i * rows:(i + 1) * rows].view(torch.int32))
    reps = {k: max(1, min(200, int(0.25 / max(window(fn, 1), 1e-5)))) for k, fn in paths.items()}   # also the warm-up
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(window(fn, reps[k]))
    dff.ASYNC_COPY = True
    out = {"stack": name, "models": M, "rows_per_model": rows, "launches": fleet.last_forward_launches}
    for k, v in times.items():
        out[k + "_ms"] = [round(1e3 * t, 4) for t in (float(np.median(v)), min(v), max(v))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table as markdown here")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="M = 1 and 64 only")
    ns = ap.parse_args()
    dev = torch.device("cuda", 0)
    shapes = [(1, 4096), (64, 4096)] if ns.quick else [(1, 4096), (64, 4096), (256, 4096), (4096, 4096), (16384, 256)]
    lines = ["| stack | models x rows | launches | fleet ms (min .. max) | fleet, plain copy ms | loop ms (min .. max) | loop / fleet |",
             "|---|---|---|---|---|---|---|"]
    for name in STACKS:
        for M, rows in shapes:
            r = measure(name, M, rows, ns.rounds, dev)
            print(json.dumps(r), flush=True)
            f, p, l = r["fleet_ms"], r["fleet_plain_copy_ms"], r["loop_ms"]
            lines.append(f"| {name} | {M} x {rows} | {r['launches']} | {f[0]} ({f[1]} .. {f[2]}) | {p[0]} ({p[1]} .. {p[2]}) | "
                         f"{l[0]} ({l[1]} .. {l[2]}) | {l[0] / f[0]:.2f} |")
            if ns.out:
                os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
                with open(ns.out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
