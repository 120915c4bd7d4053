"""Large-batch train step for Dense stacks (``dense_batch.hip``): ``fit(engine="throughput")``.

A Keras step at any batch from 1 to ``MAX_BATCH`` is two launches and no host synchronisation.
``dense_batch_grad_kernel`` spreads the step's 32-row chunks over ``groups`` workgroups (one per CU
unless told otherwise, never more than there are chunks); each runs the bf16 persistent trainer's
chunk -- every contraction on bf16 MFMAs, everything else fp32 -- over its contiguous span and writes
one gradient slab.  ``dense_batch_apply_kernel`` sums the slabs in ascending order and applies Adam in
place on the model's :class:`~streamml.ops.adam.FlatParams`.  The split is static, so a result's bits
depend on the batch and ``groups`` alone; with ``groups=1`` they are those of
``dense_persistent.train_steps(precision="bf16")``.

``supports`` needs no device and no built extension: the stack's limits are the bf16 persistent
trainer's (``dense_persistent.check_shape``), the batch's is ``MAX_BATCH``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import dense_persistent as dpers
from ._ext import load_c

MAX_BATCH = 1 << 24          # a chosen bound: a step's row indices stay in int32


def supports(model, batch_size: int, own_targets: bool = False) -> Tuple[bool, str]:
    """(True, "") if ``train_steps`` can train ``model`` at ``batch_size``, else (False, reason).
    ``own_targets``: ``y`` is given (it costs LDS); otherwise ``y = x``."""
    ok, why = dpers.supports(model, 1, own_targets=own_targets, precision="bf16")
    if not ok:
        return False, why
    if batch_size < 1 or batch_size > MAX_BATCH:
        return False, f"batch {batch_size} is outside 1..{MAX_BATCH} (MAX_BATCH)"
    return True, ""


def _checked(model, batch: int, own_targets: bool) -> None:
    ok, why = supports(model, batch, own_targets=own_targets)
    if not ok:
        raise ValueError(f"large-batch Dense trainer: {why}")


def train_steps(model, x: torch.Tensor, y: Optional[torch.Tensor], batch: int, nsteps: int, row0: int = 0,
                order: Optional[torch.Tensor] = None, groups: Optional[int] = None) -> torch.Tensor:
    """``nsteps`` Keras steps of ``batch`` rows each from sample ``row0`` on (the last one partial if
    the samples run out), ``2 * nsteps`` launches on the current stream.  Arguments and the returned
    device tensor [nsteps, 2] are those of ``dense_persistent.train_steps``; ``groups``: workgroups of
    a step (None: one per CU)."""
    _checked(model, int(batch), y is not None)
    fp, hp = model.fp, model.hp
    return load_c().dense_batch_train(fp.flat, fp.m, fp.v, fp.iter, dpers.table(model), x, y, order, int(row0),
                                      int(batch), int(nsteps), hp["lr"], hp["beta_1"], hp["beta_2"], hp["epsilon"],
                                      int(groups or 0))


def grad_step(model, x: torch.Tensor, y: Optional[torch.Tensor] = None,
              groups: Optional[int] = None) -> Tuple[torch.Tensor, float, int]:
    """One step over all rows of ``x`` without the update: (flat gradient in the order of
    ``model.fp.flat``, mean loss incl. penalties, rows whose argmax matches)."""
    batch = int(x.shape[0])
    _checked(model, batch, y is not None)
    grad, out = load_c().dense_batch_grad(model.fp.flat, dpers.table(model), x, y, None, 0, batch, int(groups or 0))
    loss, correct = out.tolist()
    return grad, float(loss), int(correct)
