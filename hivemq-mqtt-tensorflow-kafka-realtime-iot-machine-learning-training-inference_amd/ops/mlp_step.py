"""Fused fp32 train step of the MNIST classifier (``mlp_step.hip``): ``MLPClassifier.fit(engine="fused")``.

A Keras step of ``Flatten -> Dense(H, relu) -> [Dropout] -> Dense(C, softmax)`` at batch 1..32 is two
launches and no host synchronisation.  ``mlp_step_fwd_kernel`` gathers the step's rows through the
epoch's permutation, scales ``uint8`` by 1/255 and computes ``h`` on fp32 MFMAs, one workgroup per 64
hidden units with k split over its eight waves.  ``mlp_step_bwd_kernel`` recomputes the head in every
workgroup and gives every parameter exactly one owner, which forms its gradient as a chain over the
batch rows and applies Adam in place on the model's :class:`~streamml.ops.adam.FlatParams`.  The
split is static and no sum depends on it, so a result's bits depend on neither ``groups`` nor the device.

``supports`` needs no device and no built extension; the constants and the check mirror
``csrc/include/sml_mlp_step.h``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._ext import load_c

MAX_BATCH = 32
MAX_IN = 1024
MAX_HIDDEN = 512
MIN_CLASSES = 2
MAX_CLASSES = 64
UNITS_PER_BLOCK = 64      # hidden units a workgroup of the forward owns
ROWS_PER_GROUP = 8        # default: one backward workgroup per 8 rows of W1
MAX_GROUPS = 1024


def _outside(what: str, v: int, lo: int, hi: int, name: str) -> str:
    return f"{what} {v} is outside {lo}..{hi} ({name})"


def check(batch: int, in_features: int, hidden: int, classes: int, rate: float = 0.0, world: int = 1) -> str:
    """``mlp_step_check`` of the header: empty, or the limit exceeded."""
    if batch < 1 or batch > MAX_BATCH:
        return _outside("batch", batch, 1, MAX_BATCH, "MLS_MAXBATCH")
    if in_features < 1 or in_features > MAX_IN:
        return _outside("in_features", in_features, 1, MAX_IN, "MLS_MAXIN")
    if hidden < 1 or hidden > MAX_HIDDEN:
        return _outside("hidden", hidden, 1, MAX_HIDDEN, "MLS_MAXHIDDEN")
    if classes < MIN_CLASSES or classes > MAX_CLASSES:
        return _outside("classes", classes, MIN_CLASSES, MAX_CLASSES, "MLS_MAXCLASSES")
    if not (0.0 <= rate < 1.0):
        return f"dropout rate {rate:f} is outside [0, 1)"
    if world != 1:
        return f"world size {world}: the fused step trains on one device (MLS_WORLD)"
    return ""


def groups_of(in_features: int, groups: int = 0, cus: int = 256) -> int:
    """Workgroups of the backward launch (``mlp_step_groups``)."""
    want = groups if groups > 0 else min((in_features + ROWS_PER_GROUP - 1) // ROWS_PER_GROUP, cus)
    return max(1, min(want, MAX_GROUPS))


def _world() -> int:
    import torch.distributed as dist

    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def supports(model, batch_size: int, world: Optional[int] = None) -> Tuple[bool, str]:
    """(True, "") if ``train_steps`` can train ``model`` at ``batch_size``, else (False, reason).
    ``world``: the data-parallel world size (None: that of the process)."""
    why = check(int(batch_size), model.in_features, model.hidden, model.classes, model.dropout,
                _world() if world is None else int(world))
    if not why and model.device.type != "cuda":
        why = f"the model is on {model.device}, not on a ROCm device"
    return not why, why


def train_steps(model, x: torch.Tensor, y: torch.Tensor, order: Optional[torch.Tensor], batch: int, steps: int,
                groups: int = 0) -> None:
    """``steps`` Keras steps of ``batch`` samples each, ``2 * steps`` launches on the current stream.
    Step ``s`` takes the samples ``s * batch .. (s + 1) * batch - 1``; sample ``i`` is row ``order[i]`` of
    ``x`` ([n, in] uint8 or float32 on the model's device; ``y`` int64 [n]), or row ``i`` without
    ``order``.  The model's parameters, Adam state and metric buffer are updated in place and its
    Dropout counter advances by ``steps``."""
    ok, why = supports(model, int(batch))
    if not ok:
        raise ValueError(f"fused MLP train step: {why}")
    fp, hp = model.fp, model.hp
    load_c().mlp_train_steps(fp.flat, fp.m, fp.v, fp.iter, x, y, order, model._acc, model.hidden, model.classes,
                             int(batch), int(steps), model.dropout, model._seed, model._step & 0xffffffff,
                             hp["lr"], hp["beta_1"], hp["beta_2"], hp["epsilon"], int(groups))
    model._step += int(steps)
