"""The cases of tests/test_dense_minibatch_bf16_gpu.py: those of helpers/dense_mb_cases (imported,
not edited) plus ``64-128-64_b32``, which sits exactly on the bf16 kernel's MAX_PARAMS_BF16.

The extra case is built like the others: Glorot kernels, biases in +-0.2, target rows with their
largest element raised by TARGET_BOOST, and the rows of step s kept only if their top two outputs
under the float64 reference's weights at step s differ by more than OUTPUT_MARGIN.
"""
import functools

import numpy as np

from helpers import dense_mb_cases as base
from helpers.dense_mb_bf16_ref import Spec
from helpers.dense_mb_ref import DenseRef, Layer

EXTRA = {
    "64-128-64_b32": ([64, 128, 64], ["tanh", "relu"], 32, 32 * 24, {}),
}
EXTRA_SEEDS = {"64-128-64_b32": 0}
NAMES = list(base.CASES) + list(EXTRA)


def case(name):
    return base.CASES[name] if name in base.CASES else EXTRA[name]


def batch_of(name):
    return case(name)[2]


def steps_of(name):
    _, _, batch, n, _ = case(name)
    return -(-n // batch)


def spec(name):
    widths, acts, _, _, ex = case(name)
    return Spec(widths, acts, ex.get("bias"), ex.get("l1"), ex.get("l2"))


@functools.lru_cache(maxsize=None)
def _extra(name):
    widths, acts, batch, n, _ = EXTRA[name]
    rng = np.random.default_rng([EXTRA_SEEDS[name], len(widths), n])
    ws = []
    for fin, fout in zip(widths[:-1], widths[1:]):
        lim = np.sqrt(6.0 / (fin + fout))
        ws.append(rng.uniform(-lim, lim, size=(fin, fout)).astype(np.float32))
        ws.append(rng.uniform(-0.2, 0.2, size=fout).astype(np.float32))
    ref = DenseRef([Layer(ws[2 * l], ws[2 * l + 1], acts[l]) for l in range(len(acts))])
    x = np.zeros((n, widths[0]), np.float32)
    for s in range(-(-n // batch)):
        rows = np.arange(s * batch, min((s + 1) * batch, n))
        filled = 0
        while filled < len(rows):
            cx = rng.uniform(0.0, 1.0, size=(2 * len(rows), widths[0])).astype(np.float32)
            cx[np.arange(len(cx)), cx.argmax(-1)] += np.float32(base.TARGET_BOOST)
            yp = np.sort(ref.forward(cx)[-1], axis=-1)
            keep = np.nonzero(yp[:, -1] - yp[:, -2] > base.OUTPUT_MARGIN)[0][:len(rows) - filled]
            x[rows[filled:filled + len(keep)]] = cx[keep]
            filled += len(keep)
        ref.step(x[rows])
    return ws, x, None, None


def arrays(name):
    """(weights list in FlatParams order, x, y or None, order or None) of a case, all fp32."""
    return base.arrays(name) if name in base.CASES else _extra(name)


def build_model(name, device, minibatch_precision=None):
    """The case's nn.Sequential on ``device`` with the case's weights, compiled for MSE."""
    from streamml import nn
    from streamml.nn.layers import L1L2, Dense
    widths, acts, _, _, ex = case(name)
    nl = len(widths) - 1
    bias, l1, l2 = ex.get("bias", [True] * nl), ex.get("l1", [0] * nl), ex.get("l2", [0] * nl)
    layers = []
    for l in range(nl):
        reg = L1L2(l1[l], l2[l]) if (l1[l] or l2[l]) else None
        layers.append(Dense(widths[l + 1], acts[l], use_bias=bias[l], activity_regularizer=reg,
                            input_shape=(widths[0],) if l == 0 else None))
    model = nn.Sequential(layers, device=device, seed=1)
    model.compile(loss="mse", metrics=["accuracy"], fused=False if str(device) == "cpu" else None,
                  minibatch_precision=minibatch_precision)
    model.set_weights(arrays(name)[0])
    return model
