"""Large-batch train step for WIDE Dense stacks (``dense_batch_wide.hip``): ``fit(engine="wide")``.

A Keras step of a stack of 1..``MAX_LAYERS`` Dense layers, every width up to ``MAX_WIDTH``, is four
launches and no host synchronisation: the two bf16 weight images from the fp32 masters; a persistent
grid that runs forward and backward over 64-row tiles on bf16 MFMAs (weights stream from L2, the
tile's activation stays in LDS) and leaves the bf16 operands of the weight gradients in a per-step
workspace; one grouped weight-gradient launch over ``splits`` row splits; and ``dense_batch.hip``'s
apply launch, which sums the splits' slabs in ascending order and applies Adam in place on the
model's :class:`~streamml.ops.adam.FlatParams`.  The rounding points are the bf16 trainers', so a
model trained here gets the forward that ``predict(engine="wide")`` runs.  Both splits are static: a
result's bits depend on the batch, ``groups`` and ``splits`` alone.

``supports`` needs no device and no built extension: it mirrors ``dense_batchw_check`` of
``csrc/include/sml_dense_batchw.h``.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import dense_persistent as dpers
from ._ext import load_c

MAX_LAYERS = 8
MAX_WIDTH = 512
MAX_BATCH = 1 << 24          # a chosen bound, the narrow step's
TILE_ROWS = 64               # rows of a forward / backward tile; the workspace holds whole tiles
WS_BYTES = 1 << 30           # the budget of a step's activation workspace


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def workspace_bytes(widths: List[int], batch_size: int) -> int:
    """bf16 input and pre-activation gradient of every layer, rows rounded up to whole tiles."""
    rows = -(-batch_size // TILE_ROWS) * TILE_ROWS
    return 2 * rows * sum(_pad32(a) + _pad32(b) for a, b in zip(widths[:-1], widths[1:]))


def check_shape(widths: List[int], batch_size: int, own_targets: bool = False) -> str:
    """Empty if the step takes a stack of these widths at this batch size, else the reason."""
    nl = len(widths) - 1
    if nl < 1 or nl > MAX_LAYERS:
        return f"{nl} Dense layers: the wide trainer takes 1..{MAX_LAYERS} (MAX_LAYERS)"
    if widths[0] < 1 or widths[0] > MAX_WIDTH:
        return f"input width {widths[0]} is outside 1..{MAX_WIDTH} (MAX_WIDTH)"
    for l, u in enumerate(widths[1:]):
        if u < 1 or u > MAX_WIDTH:
            return f"layer {l} has {u} units: the limit is {MAX_WIDTH} (MAX_WIDTH)"
    if not own_targets and widths[-1] != widths[0]:
        return "y = x needs as many output units as inputs"
    if batch_size < 1 or batch_size > MAX_BATCH:
        return f"batch {batch_size} is outside 1..{MAX_BATCH} (MAX_BATCH)"
    need = workspace_bytes(widths, batch_size)
    if need > WS_BYTES:
        return f"{need} bytes of activation workspace at batch {batch_size}: the budget is {WS_BYTES} (WS_BYTES)"
    return ""


def supports(model, batch_size: int, own_targets: bool = False) -> Tuple[bool, str]:
    """(True, "") if ``train_steps`` can train ``model`` at ``batch_size``, else (False, reason).
    ``own_targets``: ``y`` is given; otherwise ``y = x``."""
    layers, why = dpers.dense_layers(model)
    if layers is None:
        return False, why
    if not layers:
        return False, "the model has no Dense layer"
    if model.loss != "mean_squared_error":
        return False, f"loss {model.loss!r}: the wide trainer implements mean_squared_error"
    shape = tuple(model._input_shape())
    if len(shape) != 1:
        return False, f"input shape {shape}: the wide trainer takes 1-D rows"
    for lyr in layers:
        if lyr.activation not in dpers.ACT:
            return False, f"activation {lyr.activation!r} is not one of {sorted(dpers.ACT)}"
    why = check_shape([int(shape[0])] + [l.units for l in layers], int(batch_size), own_targets)
    return (not why), why


def _checked(model, batch: int, own_targets: bool) -> None:
    ok, why = supports(model, batch, own_targets=own_targets)
    if not ok:
        raise ValueError(f"wide large-batch Dense trainer: {why}")


def train_steps(model, x: torch.Tensor, y: Optional[torch.Tensor], batch: int, nsteps: int, row0: int = 0,
                order: Optional[torch.Tensor] = None, groups: Optional[int] = None,
                splits: Optional[int] = None) -> torch.Tensor:
    """``nsteps`` Keras steps of ``batch`` rows each from sample ``row0`` on (the last one partial if
    the samples run out), ``4 * nsteps`` launches on the current stream.  Arguments and the returned
    device tensor [nsteps, 2] are those of ``dense_batch.train_steps``; ``groups``: forward / backward
    workgroups of a step (None: one per CU); ``splits``: row splits of the weight gradients (None:
    enough to fill the CUs)."""
    _checked(model, int(batch), y is not None)
    fp, hp = model.fp, model.hp
    return load_c().dense_batchw_train(fp.flat, fp.m, fp.v, fp.iter, dpers.table(model), x, y, order, int(row0),
                                       int(batch), int(nsteps), hp["lr"], hp["beta_1"], hp["beta_2"], hp["epsilon"],
                                       int(groups or 0), int(splits or 0))


def grad_step(model, x: torch.Tensor, y: Optional[torch.Tensor] = None, groups: Optional[int] = None,
              splits: Optional[int] = None) -> Tuple[torch.Tensor, float, int]:
    """One step over all rows of ``x`` without the update: (flat gradient in the order of
    ``model.fp.flat``, mean loss incl. penalties, rows whose argmax matches)."""
    batch = int(x.shape[0])
    _checked(model, batch, y is not None)
    grad, out = load_c().dense_batchw_grad(model.fp.flat, dpers.table(model), x, y, None, 0, batch, int(groups or 0),
                                           int(splits or 0))
    loss, correct = out.tolist()
    return grad, float(loss), int(correct)
