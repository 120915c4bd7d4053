"""lstm() forward + backward at widths above 128: the torch-op path (``lstm_reference`` under
autograd, what ``ops.lstm.lstm`` ran for these widths before the streamed-weight kernels and
still runs beyond 512 units) against the device kernels.  tanh, 5 warm-up + 20 timed iterations,
device-synchronised wall time, four alternating runs per shape (profiles/r09/lstm_wide).

    python tools/lstm_wide_bench.py [out.json]      # U = 256 / 512 at B = 4096 / 64, T = 50
    python tools/lstm_wide_bench.py --trace          # device kernels only, few iterations:
                                                     #   run under rocprofv3 --kernel-trace --stats
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from streamml.ops.lstm import lstm, lstm_reference  # noqa: E402

TRACE = "--trace" in sys.argv[1:]
WARM, ITERS, RUNS = (2, 3, 1) if TRACE else (5, 20, 4)
dev = torch.device("cuda", 0)


def make(u, B, T=50, inp=18):
    rng = np.random.default_rng(u + B)
    x = torch.tensor(rng.uniform(-1, 1, (B, T, inp)), dtype=torch.float32, device=dev)
    W, U, b = (torch.tensor(a, dtype=torch.float32, device=dev).requires_grad_(True) for a in (
        rng.standard_normal((inp, 4 * u)) * 0.25, rng.standard_normal((u, 4 * u)) * 0.25 / (u / 32) ** 0.5,
        rng.standard_normal(4 * u) * 0.1))
    gy = torch.tensor(rng.standard_normal((B, T, u)), dtype=torch.float32, device=dev)
    return x, W, U, b, gy


def one(path, x, W, U, b, gy):
    for p in (W, U, b):
        p.grad = None
    y = lstm_reference(x, W, U, b, "tanh") if path == "torch" else lstm(x, W, U, b, "tanh")
    (y * gy).sum().backward()


def timed(path, args):
    for _ in range(WARM):
        one(path, *args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        one(path, *args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e3


def main():
    out = {}
    for u, B in ((256, 4096), (512, 4096)) if TRACE else ((256, 4096), (256, 64), (512, 4096), (512, 64)):
        args = make(u, B)
        res = {"torch": [], "kernels": []}
        for _ in range(RUNS):
            if not TRACE:
                res["torch"].append(timed("torch", args))
            res["kernels"].append(timed("kernels", args))
        out["U%d_B%d" % (u, B)] = res
        print(u, B, {k: ["%.3f" % v for v in vs] for k, vs in res.items()}, flush=True)
        del args
        torch.cuda.empty_cache()
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
