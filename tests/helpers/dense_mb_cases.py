"""The cases of tests/test_dense_minibatch_gpu.py: models, data and their float64 reference.

A case is a Dense stack with ordinary weights (Glorot kernels, biases drawn from +-0.2), a batch
size and 24-40 steps of rows, trained at the default learning rate.  The per-step ``correct``
count is an exact check, so every row needs a margin between its top two outputs and between its
top two targets (a near tie would make the count depend on rounding).  The margin is per row:

* the largest element of every target row is raised by ``TARGET_BOOST``;
* the rows of step s are chosen while the float64 reference runs: candidates are drawn from the
  case's generator and a row is kept only if, under the reference's weights at step s, its top two
  outputs differ by more than ``OUTPUT_MARGIN``.  Nothing else about a row is selected, so the
  predicted class varies from row to row as the data does (the acceptance test asserts it).
"""
import functools

import numpy as np

from helpers.dense_mb_ref import DenseRef, Layer

TARGET_BOOST = 0.05
OUTPUT_MARGIN = 5e-3       # five times the 1e-3 the checks need

# name -> (widths, activations, batch, n rows, dict of extras)
#   extras: seed, bias (per layer, default True), l1 / l2 (per layer), own_y, order
CASES = {
    "ragged_sigmoid_18-33-18": ([18, 33, 18], ["sigmoid", "linear"], 32, 32 * 24, {}),
    "18-64-16-64-18": ([18, 64, 16, 64, 18], ["tanh", "relu", "tanh", "relu"], 32, 32 * 24, {}),
    "30-128-32-128-30_b32": ([30, 128, 32, 128, 30], ["tanh", "relu", "tanh", "relu"], 32, 32 * 24, {}),
    "30-128-32-128-30_b100": ([30, 128, 32, 128, 30], ["tanh", "relu", "tanh", "relu"], 100, 100 * 24, {}),
    "eight_layers": ([18, 24, 16, 12, 8, 12, 16, 24, 18], ["tanh"] * 7 + ["linear"], 32, 32 * 24, {}),
    "one_layer": ([18, 18], ["tanh"], 32, 32 * 24, {}),
    "no_bias_layer": ([18, 20, 18], ["tanh", "linear"], 32, 32 * 24, {"bias": [False, True]}),
    "l1_first_l2_middle": ([18, 16, 8, 16, 18], ["tanh", "tanh", "tanh", "linear"], 32, 32 * 24,
                           {"l1": [1e-3, 0, 0, 0], "l2": [0, 1e-3, 0, 0]}),
    "own_targets_18-8-3": ([18, 8, 3], ["tanh", "linear"], 32, 32 * 24, {"own_y": True}),
    "four_activations": ([18, 12, 10, 14, 18], ["relu", "tanh", "sigmoid", "linear"], 32, 32 * 24, {}),
    "batch_1": ([18, 20, 18], ["tanh", "sigmoid"], 1, 40, {}),
    "batch_7": ([18, 20, 18], ["tanh", "sigmoid"], 7, 7 * 30, {}),
    "batch_33": ([18, 20, 18], ["tanh", "sigmoid"], 33, 33 * 24, {}),
    "batch_128": ([18, 20, 18], ["tanh", "sigmoid"], 128, 128 * 24, {}),
    "partial_last_step": ([18, 20, 18], ["tanh", "linear"], 32, 32 * 24 + 13, {}),
    "order_given": ([18, 20, 18], ["relu", "linear"], 32, 32 * 24, {"order": True}),
}
# accepted by tests/test_dense_minibatch_gpu.py::test_case_seed_is_acceptable (see there)
SEEDS = {name: 0 for name in CASES}


def steps_of(name):
    _, _, batch, n, _ = CASES[name]
    return -(-n // batch)


def _layers(name, ws):
    widths, acts, _, _, ex = CASES[name]
    nl = len(widths) - 1
    bias, l1, l2 = ex.get("bias", [True] * nl), ex.get("l1", [0] * nl), ex.get("l2", [0] * nl)
    ws = list(ws)
    layers = []
    for l in range(nl):
        W = ws.pop(0)
        b = ws.pop(0) if bias[l] else None
        layers.append(Layer(W, b, acts[l], l1[l], l2[l]))
    return layers


@functools.lru_cache(maxsize=None)
def _case(name):
    """Builds the case and runs its float64 reference, once: the rows of a step are selected
    against the reference's weights at that step (module docstring)."""
    widths, acts, batch, n, ex = CASES[name]
    rng = np.random.default_rng([SEEDS[name], len(widths), n])
    nl = len(widths) - 1
    bias = ex.get("bias", [True] * nl)
    ws = []
    for l in range(nl):
        fin, fout = widths[l], widths[l + 1]
        lim = np.sqrt(6.0 / (fin + fout))
        ws.append(rng.uniform(-lim, lim, size=(fin, fout)).astype(np.float32))
        b = rng.uniform(-0.2, 0.2, size=fout).astype(np.float32)
        if bias[l]:
            ws.append(b)
    own = bool(ex.get("own_y"))
    order = rng.permutation(n).astype(np.int32) if ex.get("order") else None
    ref = DenseRef(_layers(name, ws))
    x = np.zeros((n, widths[0]), np.float32)
    y = np.zeros((n, widths[-1]), np.float32) if own else None
    out = []
    for s in range(steps_of(name)):
        pos = np.arange(s * batch, min((s + 1) * batch, n))
        rows = pos if order is None else order[pos]
        filled = 0
        while filled < len(rows):
            cx = rng.uniform(0.0, 1.0, size=(2 * len(rows), widths[0])).astype(np.float32)
            cy = rng.uniform(0.0, 1.0, size=(2 * len(rows), widths[-1])).astype(np.float32) if own else None
            t = cy if own else cx
            t[np.arange(len(t)), t.argmax(-1)] += np.float32(TARGET_BOOST)
            yp = np.sort(ref.forward(cx)[-1], axis=-1)
            keep = np.nonzero(yp[:, -1] - yp[:, -2] > OUTPUT_MARGIN)[0][:len(rows) - filled]
            x[rows[filled:filled + len(keep)]] = cx[keep]
            if own:
                y[rows[filled:filled + len(keep)]] = cy[keep]
            filled += len(keep)
        out.append(ref.step(x[rows], y[rows] if own else None))
    return ws, x, y, order, ref, np.asarray(out, np.float64)


def arrays(name):
    """(weights list in FlatParams order, x, y or None, order or None) of a case, all fp32."""
    return _case(name)[:4]


def build_model(name, device):
    """The case's nn.Sequential on ``device`` with the case's weights, compiled for MSE."""
    from streamml import nn
    from streamml.nn.layers import L1L2, Dense
    widths, acts, _, _, ex = CASES[name]
    nl = len(widths) - 1
    bias, l1, l2 = ex.get("bias", [True] * nl), ex.get("l1", [0] * nl), ex.get("l2", [0] * nl)
    layers = []
    for l in range(nl):
        reg = L1L2(l1[l], l2[l]) if (l1[l] or l2[l]) else None
        layers.append(Dense(widths[l + 1], acts[l], use_bias=bias[l], activity_regularizer=reg,
                            input_shape=(widths[0],) if l == 0 else None))
    model = nn.Sequential(layers, device=device, seed=1)
    model.compile(loss="mse", metrics=["accuracy"], fused=False if str(device) == "cpu" else None)
    model.set_weights(arrays(name)[0])
    return model


def reference(name):
    """The float64 run of the whole case, computed once: (DenseRef after the steps, [nsteps, 2])."""
    return _case(name)[4:]


def flat_of(arrs):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in arrs])


# (widths, batch, own targets) on which the Python limits must agree with the C++ check
SHAPES = [
    ([18, 64, 16, 64, 18], 1, False), ([18, 64, 16, 64, 18], 32, False), ([18, 64, 16, 64, 18], 100, False),
    ([18, 64, 16, 64, 18], 128, False), ([30, 128, 32, 128, 30], 1, False), ([30, 128, 32, 128, 30], 32, False),
    ([30, 128, 32, 128, 30], 100, True), ([30, 128, 32, 128, 30], 128, True),
    ([18] + [20] * 8 + [18], 32, False),            # nine layers
    ([18, 129, 18], 32, False),                     # too wide
    ([129, 18, 129], 32, False),                    # input too wide
    ([18, 33, 18], 129, False), ([18, 33, 18], 0, False),
    ([128, 128, 128], 32, False),                   # 32 768 kernel elements
    ([128, 124, 128], 32, False),                   # 31 744
    ([64, 128, 64], 32, False),                     # 16 384: MAX_PARAMS exactly
    ([64, 128, 65], 32, True),                      # 68 pads to 68: 16 896
    ([128, 16, 128, 16, 128, 16, 128, 16, 128], 32, True),   # 16 384 elements, but the LDS plan does not fit
    ([18, 8, 3], 32, False), ([18, 8, 3], 32, True),      # y = x needs O == D
    ([18, 33, 18], 32, False), ([1, 1], 1, False),
]
