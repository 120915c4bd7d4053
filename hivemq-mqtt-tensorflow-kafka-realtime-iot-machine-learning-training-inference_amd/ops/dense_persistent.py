"""Persistent small-batch trainer for Dense stacks of any depth (``dense_minibatch.hip``).

``train_steps`` runs ``nsteps`` Keras steps (forward, MSE + activity penalties, categorical
accuracy, backward, Adam) of an ``nn.Model`` made of Dense layers in ONE launch: one
workgroup, fp32 weights in LDS, gradients and Adam moments in registers.  ``precision="bf16"``
runs the sibling kernel (``dense_minibatch_bf16.hip``): every contraction on bf16 MFMAs, fp32
master weights, gradients and Adam moments in the registers of the wave that owns a 16x16 tile,
one bf16 weight image in LDS; its limits are its own (``MAX_PARAMS_BF16``).  The model's
:class:`~streamml.ops.adam.FlatParams` (``flat / m / v / iter``) are updated in place and the
per-step ``[loss, correct]`` come back as a device tensor, as ``ops.lstm_persistent`` does for
the reference LSTM stack.

``supports`` needs no device and no built extension: it mirrors the C++ checks and LDS plans
(``dense_mb_check``, ``dense_mb_plan``, ``dense_mb_plan_bf16`` of ``csrc/include/sml_dense_mb_plan.h``)
and names the limit a model exceeds.  ``tests/test_dense_mb_plan.py`` holds the two copies together on
the CPU, through a host program over that header.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from ._ext import load_c

ACT = {"linear": 0, "relu": 1, "tanh": 2, "sigmoid": 3}
MAX_BATCH = 128
MAX_LAYERS = 8
MAX_WIDTH = 128
THREADS = 512                # of the workgroup
TILES_PER_THREAD = 2         # 4x4 parameter tiles whose state a thread keeps in registers
MAX_PARAMS = THREADS * TILES_PER_THREAD * 16   # kernel elements with both widths rounded up to 4
TILES_BF16 = 64              # 16x16 parameter tiles of the bf16 kernel: 8 per wave
MAX_PARAMS_BF16 = TILES_BF16 * 256             # kernel elements with both widths rounded up to 16
PRECISION = {"fp32": 0, "bf16": 1}
CHUNK = 32                   # rows of a batch in LDS at a time
LDS_BYTES = 160 * 1024
_STATIC_LDS = 1024           # the kernel's own copy of the layer table


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def _pad16(n: int) -> int:
    return (n + 15) // 16 * 16


def _precision(precision: str) -> int:
    if precision not in PRECISION:
        raise ValueError(f"precision must be 'fp32' or 'bf16', not {precision!r}")
    return PRECISION[precision]


def dense_layers(model) -> Tuple[Optional[list], str]:
    """The model's Dense layers, or (None, reason) if another kind of layer takes part."""
    from ..nn.layers import Dense, Dropout, InputLayer
    out = []
    for lyr in model.layers:
        if isinstance(lyr, InputLayer):
            continue
        if isinstance(lyr, Dropout):
            if lyr.rate > 0:
                return None, f"Dropout with rate {lyr.rate:g} (only rate 0 is a no-op the trainer can skip)"
            continue
        if not isinstance(lyr, Dense):
            return None, f"layer {lyr.name or lyr.class_name!r} is a {lyr.class_name}, not Dense"
        out.append(lyr)
    return out, ""


def _lds_bytes_bf16(widths: List[int], own_targets: bool) -> int:
    """The plan of ``dense_mb_plan_bf16``: fp32 and bf16 input rows, per layer the unit-major bf16
    weight image [up][ip + 8], four fp32 bias arrays, the fp32 output [CHUNK][up + 4] and the bf16
    gradient [CHUNK][up + 8], a bf16 output image for every layer but the last, targets, the
    per-row statistics and the tile table."""
    dp = _pad16(widths[0])
    n = CHUNK * (dp + 4) * 4 + CHUNK * (dp + 8) * 2
    prev = dp
    ups = []
    for u in widths[1:]:
        up = _pad16(u)
        n += up * (prev + 8) * 2 + 16 * up
        ups.append(up)
        prev = up
    n += sum(CHUNK * (up + 4) * 4 for up in ups)
    n += sum(CHUNK * (up + 8) * 2 for up in ups[:-1])
    n += sum(CHUNK * (up + 8) * 2 for up in ups)
    if own_targets:
        n += CHUNK * (prev + 4) * 4
    n += 4 * CHUNK * 4 + TILES_BF16 * 4
    return n + _STATIC_LDS


def lds_bytes(widths: List[int], own_targets: bool, precision: str = "fp32") -> int:
    """LDS the kernel needs for a stack ``widths[0] -> widths[1] -> ...`` (the plan of
    ``dense_mb_plan``): input rows, weight image, every layer's output and gradient, targets."""
    if _precision(precision):
        return _lds_bytes_bf16(widths, own_targets)
    dp = _pad4(widths[0])
    floats = CHUNK * dp
    prev = dp
    ups = []
    for u in widths[1:]:
        up = _pad4(u)
        ws = up if (up // 4) % 2 else up + 4
        floats += prev * ws + up
        ups.append(up)
        prev = up
    floats += CHUNK * sum(ups)              # outputs
    floats += CHUNK * sum(ups[:-1])         # gradients (the last layer's share its output's buffer)
    if own_targets:
        floats += CHUNK * prev
    floats += 4 * CHUNK
    return floats * 4 + _STATIC_LDS


def check_shape(widths: List[int], batch_size: int, own_targets: bool = False, precision: str = "fp32") -> str:
    """Empty if the kernel of this precision takes a stack of these widths at this batch size,
    else the reason."""
    bf16 = bool(_precision(precision))
    pad = _pad16 if bf16 else _pad4
    nl = len(widths) - 1
    if nl < 1 or nl > MAX_LAYERS:
        return f"{nl} Dense layers: the persistent trainer takes 1..{MAX_LAYERS} (MAX_LAYERS)"
    if batch_size < 1 or batch_size > MAX_BATCH:
        return f"batch {batch_size} is outside 1..{MAX_BATCH} (MAX_BATCH)"
    if widths[0] < 1 or widths[0] > MAX_WIDTH:
        return f"input width {widths[0]} is outside 1..{MAX_WIDTH} (MAX_WIDTH)"
    for l, u in enumerate(widths[1:]):
        if u < 1 or u > MAX_WIDTH:
            return f"layer {l} has {u} units: the limit is {MAX_WIDTH} (MAX_WIDTH)"
    padded = sum(pad(a) * pad(b) for a, b in zip(widths[:-1], widths[1:]))
    if bf16 and padded > MAX_PARAMS_BF16:
        return (f"{padded} kernel elements (widths rounded up to 16): the limit is {MAX_PARAMS_BF16} "
                "(MAX_PARAMS_BF16)")
    if not bf16 and padded > MAX_PARAMS:
        return f"{padded} kernel elements (widths rounded up to 4): the limit is {MAX_PARAMS} (MAX_PARAMS)"
    if not own_targets and widths[-1] != widths[0]:
        return "y = x needs as many output units as inputs"
    need = lds_bytes(widths, own_targets, precision)
    if need > LDS_BYTES:
        return f"{need} bytes of LDS: the limit is {LDS_BYTES} (LDS_BYTES)"
    return ""


def supports(model, batch_size: int = 32, own_targets: bool = False, precision: str = "fp32") -> Tuple[bool, str]:
    """(True, "") if ``train_steps`` can train ``model`` at ``batch_size`` in this precision, else
    (False, reason).  ``own_targets``: ``y`` is given (it costs LDS); otherwise ``y = x``."""
    _precision(precision)
    layers, why = dense_layers(model)
    if layers is None:
        return False, why
    if not layers:
        return False, "the model has no Dense layer"
    if model.loss != "mean_squared_error":
        return False, f"loss {model.loss!r}: the persistent trainer implements mean_squared_error"
    shape = tuple(model._input_shape())
    if len(shape) != 1:
        return False, f"input shape {shape}: the persistent trainer takes 1-D rows"
    for lyr in layers:
        if lyr.activation == "softmax":
            return False, f"layer {lyr.name or 'dense'!r} has a softmax activation"
        if lyr.activation not in ACT:
            return False, f"activation {lyr.activation!r} is not one of {sorted(ACT)}"
    why = check_shape([int(shape[0])] + [l.units for l in layers], int(batch_size), own_targets, precision)
    return (not why), why


def table(model) -> List[Tuple[float, ...]]:
    """Rows (in, units, act, has_bias, l1, l2, w_off, b_off) of the built model's Dense layers."""
    layers, why = dense_layers(model)
    if layers is None:
        raise ValueError(why)
    model.build()
    fp = model.fp
    rows, width = [], int(model._input_shape()[0])
    for lyr in layers:
        r = lyr.activity_regularizer
        w_off = int(fp.offsets[lyr.param_slots[0]])
        b_off = int(fp.offsets[lyr.param_slots[1]]) if lyr.use_bias else 0
        rows.append((width, lyr.units, ACT[lyr.activation], int(bool(lyr.use_bias)), float(r.l1) if r else 0.0,
                     float(r.l2) if r else 0.0, w_off, b_off))
        width = lyr.units
    return rows


def train_steps(model, x: torch.Tensor, y: Optional[torch.Tensor], batch: int, nsteps: int, row0: int = 0,
                order: Optional[torch.Tensor] = None, precision: str = "fp32") -> torch.Tensor:
    """``nsteps`` Keras steps of ``batch`` rows each from sample ``row0`` on (the last one partial
    if the samples run out).  ``x``: [n, D] fp32 rows on the device (any row stride); ``y``:
    [n, O] or None for ``y = x``; ``order``: int32 [n] permutation of the samples.  Returns the
    device tensor [nsteps, 2] = (mean loss incl. penalties, rows whose argmax matches).
    ``precision="bf16"`` runs the bf16-MFMA kernel; a model outside its limits is a ``ValueError``
    (``nn.Model.fit`` falls back to fp32 itself, this function never does)."""
    ok, why = supports(model, batch, own_targets=y is not None, precision=precision)
    if not ok:
        raise ValueError(f"persistent Dense trainer: {why}")
    fp, hp = model.fp, model.hp
    return load_c().dense_mb_train(fp.flat, fp.m, fp.v, fp.iter, table(model), x, y, order, int(row0), int(batch),
                                   int(nsteps), hp["lr"], hp["beta_1"], hp["beta_2"], hp["epsilon"],
                                   PRECISION[precision])
