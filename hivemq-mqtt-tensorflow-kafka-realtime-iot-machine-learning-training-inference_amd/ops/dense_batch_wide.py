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

Two losses.  ``mean_squared_error`` on the last layer's own activation, or, for a model whose last Dense
layer is ``softmax`` under ``sparse_categorical_crossentropy``, the kernel's softmax head: that layer
enters the table as linear, ``y`` is an integer tensor of classes, and the last-layer epilogue forms
``dz = (softmax(z) - onehot) / batch`` with the mean cross-entropy and the argmax matches, in the same
four launches.  A softmax anywhere else, under another loss, with a regulariser of its own or with
``y = x`` is refused with the reason; so is every other loss.

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


HEAD_LOSS = "sparse_categorical_crossentropy"


def has_head(model) -> bool:
    """The model trains on the softmax head: its loss is ``HEAD_LOSS`` and its last Dense layer softmax."""
    layers, _ = dpers.dense_layers(model)
    return bool(layers) and model.loss == HEAD_LOSS and layers[-1].activation == "softmax"


def _check_head(model, layers, own_targets: bool) -> str:
    """Empty if loss and softmax layers go together (either no softmax under mean_squared_error, or
    ``HEAD_LOSS`` with the one softmax head), else the combination that does not."""
    soft = [l for l, lyr in enumerate(layers) if lyr.activation == "softmax"]
    if model.loss == "mean_squared_error":
        if soft:
            return (f"layer {soft[0]} is softmax under mean_squared_error: the softmax head goes with {HEAD_LOSS}")
        return ""
    if model.loss != HEAD_LOSS:
        return (f"loss {model.loss!r}: the wide trainer implements mean_squared_error, and {HEAD_LOSS} "
                "with a softmax head")
    last = layers[-1]
    if last.activation != "softmax":
        return f"loss {HEAD_LOSS} needs a softmax head: the last Dense layer is {last.activation!r}"
    if soft[0] != len(layers) - 1:
        return f"layer {soft[0]} is a softmax in the middle of the stack: only the last layer can be the head"
    if last.units < 2:
        return f"a softmax head of {last.units} unit: it needs 2..{MAX_WIDTH}"
    r = last.activity_regularizer
    if r is not None and (float(r.l1) or float(r.l2)):
        return "an activity regularizer on the softmax head"
    if not own_targets:
        return f"{HEAD_LOSS} needs labels: y = x has none"
    return ""


def supports(model, batch_size: int, own_targets: bool = False) -> Tuple[bool, str]:
    """(True, "") if ``train_steps`` can train ``model`` at ``batch_size``, else (False, reason).
    ``own_targets``: ``y`` is given (the labels, for a softmax head); otherwise ``y = x``."""
    layers, why = dpers.dense_layers(model)
    if layers is None:
        return False, why
    if not layers:
        return False, "the model has no Dense layer"
    why = _check_head(model, layers, own_targets)
    if why:
        return False, why
    shape = tuple(model._input_shape())
    if len(shape) != 1:
        return False, f"input shape {shape}: the wide trainer takes 1-D rows"
    for lyr in layers[:-1] if model.loss == HEAD_LOSS else layers:
        if lyr.activation not in dpers.ACT:
            return False, f"activation {lyr.activation!r} is not one of {sorted(dpers.ACT)}"
    why = check_shape([int(shape[0])] + [l.units for l in layers], int(batch_size), own_targets)
    return (not why), why


def _checked(model, batch: int, own_targets: bool) -> None:
    ok, why = supports(model, batch, own_targets=own_targets)
    if not ok:
        raise ValueError(f"wide large-batch Dense trainer: {why}")


def _targets(model, x: torch.Tensor, y: Optional[torch.Tensor]):
    """(y, labels, head) as the bindings take them: under the softmax head ``y`` [n] or [n, 1] of any
    integer type becomes contiguous int32 [n] labels (no copy when it is that already)."""
    if not has_head(model):
        return y, None, 0
    if y is None or y.is_floating_point() or y.dtype == torch.bool or y.numel() != x.shape[0] or y.dim() > 2:
        raise ValueError(f"wide large-batch Dense trainer: a softmax head takes y as an integer tensor [{x.shape[0]}] or "
                         f"[{x.shape[0]}, 1] of classes")
    return None, y.reshape(-1).to(device=x.device, dtype=torch.int32).contiguous(), 1


def train_steps(model, x: torch.Tensor, y: Optional[torch.Tensor], batch: int, nsteps: int, row0: int = 0,
                order: Optional[torch.Tensor] = None, groups: Optional[int] = None,
                splits: Optional[int] = None) -> torch.Tensor:
    """``nsteps`` Keras steps of ``batch`` rows each from sample ``row0`` on (the last one partial if
    the samples run out), ``4 * nsteps`` launches on the current stream.  Arguments and the returned
    device tensor [nsteps, 2] are those of ``dense_batch.train_steps``; ``groups``: forward / backward
    workgroups of a step (None: one per CU); ``splits``: row splits of the weight gradients (None:
    enough to fill the CUs).  For a softmax head ``y`` holds the classes (integers, [n] or [n, 1]) and
    a step's loss is the mean cross-entropy.  The kernel compares labels and never indexes with them:
    a class outside the head's units counts as a unit no row has (``fit`` refuses such labels)."""
    _checked(model, int(batch), y is not None)
    y, labels, head = _targets(model, x, y)
    fp, hp = model.fp, model.hp
    return load_c().dense_batchw_train(fp.flat, fp.m, fp.v, fp.iter, dpers.table(model, head=bool(head)), x, y, order,
                                       int(row0), int(batch), int(nsteps), hp["lr"], hp["beta_1"], hp["beta_2"],
                                       hp["epsilon"], int(groups or 0), int(splits or 0), labels, head)


def grad_step(model, x: torch.Tensor, y: Optional[torch.Tensor] = None, groups: Optional[int] = None,
              splits: Optional[int] = None) -> Tuple[torch.Tensor, float, int]:
    """One step over all rows of ``x`` without the update: (flat gradient in the order of
    ``model.fp.flat``, mean loss incl. penalties, rows whose argmax matches)."""
    batch = int(x.shape[0])
    _checked(model, batch, y is not None)
    y, labels, head = _targets(model, x, y)
    grad, out = load_c().dense_batchw_grad(model.fp.flat, dpers.table(model, head=bool(head)), x, y, None, 0, batch,
                                           int(groups or 0), int(splits or 0), labels, head)
    loss, correct = out.tolist()
    return grad, float(loss), int(correct)
