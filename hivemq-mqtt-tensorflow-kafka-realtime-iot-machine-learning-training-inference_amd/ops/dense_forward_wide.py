"""Fused bulk forward of a wide Dense stack (``csrc/kernels/dense_forward_wide.hip``).

One launch runs a whole stack of 1 .. ``MAX_LAYERS`` Dense layers, every width (input included) up to
``MAX_WIDTH`` = 512, over all rows, with the rounding points of the bf16 trainers' forward: every
contraction is ``bf16(h) . bf16(W)`` on ``v_mfma_f32_16x16x32_bf16`` with fp32 accumulation; bias,
activation, scores and sums stay fp32.  Weights stream from a bf16 image in device memory, a tile's
activations stay in LDS.  ``forward`` and ``evaluate_sums`` return what ``ops.dense_forward``'s do;
``nn.Model.predict / score / detect / reconstruct_and_score / evaluate`` come here under ``engine="wide"``.

``supports`` needs no device and no built extension: it mirrors ``dense_fwdw_check`` of
``csrc/include/sml_dense_fwdw_plan.h``.  This module holds what is the wide kernel's own: the bf16 rounding
of the image, the LDS plan and ``tile``.  The check's rules, ``supports``, the fragment order, the cached
state and the drivers of ``forward`` / ``evaluate_sums`` are ``ops/dense_forward.py``'s, over ``WIDE``.

The softmax head.  ``head=True`` (``nn.Model.predict / evaluate(engine="wide")`` of a classifier) makes a
final softmax layer the kernel's head: it enters the table as linear, ``forward`` returns the probabilities
and ``evaluate_sums(labels=...)`` the cross-entropy sum and the rows whose argmax is the label.  Scores are
refused with a head, and without ``head`` a softmax layer is refused as before; ``dense_forward.ACT`` has
no softmax, so the narrow forward, the fleets and the scorers keep refusing it.

The image.  ``pack_image`` is the layout, in numpy (``uint16`` words).  For an ``nn.Model`` the VALUES are
never cached (kernels update ``model.fp.flat`` in place where no Python hook sees it): what is cached on
the model is the image's gather index into the flat buffer, and ``image`` is one device gather, one
rounding to bf16 and one concatenation per call.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import dense_forward as dfw
from .dense_forward import ACT, MAX_LAYERS, _is_nn, _pad   # noqa: F401  (ACT, MAX_LAYERS: this module's names too)
from .serve import dense_layer_table

MAX_WIDTH = 512
WAVES = 8
ROWS = (64, 128)             # rows of a workgroup's tile
LDS_BYTES = 160 * 1024
_ROW_PAD = 8
_PART_WORDS = 5

WIDE = dfw.Variant("wide fused", MAX_WIDTH, 32, (4, 8), 2, True, "_dense_fwdw_state", "dense_forward_wide",
                   (("DFWW_MAXLAYERS", MAX_LAYERS), ("DFWW_MAXW", MAX_WIDTH)))


def image_table(layers) -> Tuple[list, int]:
    """(table of ``(in, units, activation code, w_off, b_off)``, 16-bit words of the image) for ``layers`` =
    ``[(in, units, activation name, use_bias)]``: per layer ``pad32(in) * pad16(units)`` bf16 weights, then
    ``pad16(units)`` fp32 biases (two words each)."""
    return dfw._table(WIDE, layers)


def plan(widths, rows: int = 64) -> dict:
    """``dense_fwdw_plan``: the stride of an activation row in LDS (words) and the dynamic LDS bytes."""
    stride = max(_pad(w, 32) for w in widths[:-1]) + _ROW_PAD
    return {"rows": rows, "stride": stride, "lds_bytes": max(rows * stride * 2, WAVES * rows * _PART_WORDS * 4)}


WHY_HEAD_SCORE = "scores need a reconstruction, not a softmax head"


def check_shape(widths, activations, score: bool = False, head: bool = False) -> str:
    """Empty if the kernel takes a stack ``widths[0] -> widths[1] -> ...`` with these activation names
    (``score``: against the input row; ``head``: the last one is the softmax head), else the limit it
    exceeds -- ``dense_fwdw_check``'s words.  The LDS plan fits at every width inside the limit."""
    if not head:
        return dfw._check_rows(WIDE, widths, activations, score)
    if score:
        return WHY_HEAD_SCORE
    activations = list(activations)
    if not activations or activations[-1] != "softmax":
        return "a softmax head needs a final softmax layer"
    why = dfw._check_rows(WIDE, widths, activations[:-1] + ["linear"], False)
    if not why and widths[-1] < 2:
        why = f"a softmax head needs 2..{MAX_WIDTH} units in the last layer and a linear last entry in the table"
    return why


def supports(model, score: bool = False, head: bool = False) -> Tuple[bool, str]:
    """(True, "") if the kernel can run ``model`` (``score``: with scores against the input row; ``head``:
    with its final softmax layer as the head), else (False, the limit it exceeds).  Needs no device."""
    return dfw._supports(lambda: dfw._layers(model, WIDE), lambda w, a: check_shape(w, a, score, head))


def to_bf16(a) -> np.ndarray:
    """fp32 -> bf16 words, round to nearest even."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) >> np.uint32(16)).astype(np.uint16)


def pack_image(layers, weights) -> Tuple[np.ndarray, list]:
    """Pack ``weights`` = ``[(W [in, units], b [units] or None)]`` into the kernel's image (``uint16``): per
    layer the bf16 weights in fragment order (a lane's eight k-values of a 32-k by 16-unit block in 16
    bytes), zero past ``in`` / ``units``, then the fp32 bias padded to 16 with zeros (all zero without a
    bias), two little-endian words each.  Returns (image, table of ``image_table``)."""
    parts = []
    for (n_in, n_out, _, _), (W, b) in zip(layers, weights):
        wf, bp = dfw._fragments(WIDE, n_in, n_out, W, b, np.float32, 0)
        parts += [to_bf16(wf), bp.view(np.uint16)]
    return np.ascontiguousarray(np.concatenate(parts)), image_table(layers)[0]


def image(model) -> Tuple[torch.Tensor, list]:
    """(device image of the model's current weights as int16 words, table)."""
    if not _is_nn(model):
        layers, weights = dense_layer_table(model)
        img, table = pack_image(layers, weights)
        return torch.from_numpy(img.view(np.int16)).to(model.device), [list(t) for t in table]
    g, st = dfw._gather(model, WIDE)   # every kernel, then every bias
    w16, b16 = g[:st["nw"]].to(torch.bfloat16).view(torch.int16), g[st["nw"]:].view(torch.int16)
    parts, wo, bo = [], 0, 0
    for n_in, n_out, _, _, _ in st["table"]:
        nw, nb = _pad(n_in, 32) * _pad(n_out, 16), 2 * _pad(n_out, 16)
        parts += [w16[wo:wo + nw], b16[bo:bo + nb]]
        wo, bo = wo + nw, bo + nb
    return torch.cat(parts), st["table"]


def _head_image(model) -> Tuple[torch.Tensor, list]:
    """``image`` with the final softmax layer linear in the table (a copy: the cached table keeps -1)."""
    img, table = image(model)
    return img, [list(t) for t in table[:-1]] + [list(table[-1][:2]) + [ACT["linear"]] + list(table[-1][3:])]


def _head_supports(model, score: bool = False) -> Tuple[bool, str]:
    return supports(model, score=score, head=True)


def forward(model, x: torch.Tensor, rec: bool = True, score: bool = False, threshold: Optional[float] = None,
            normalizer=None, max_blocks: int = 0, tile: int = 0, head: bool = False):
    """The stack over device rows ``x`` [n, D] fp32 (any row stride) in one launch.  Returns
    ``(reconstructions [n, out] | None, scores [n] | None, flags [n] bool | None)`` as device tensors;
    flags (``score > threshold``) come with ``score`` and a threshold.  ``tile``: rows of a workgroup's
    tile (64 or 128; 0: 128 when that still fills every CU).  ``head``: the final softmax layer is the
    kernel's head and the reconstructions are its probabilities; scores are refused then.  A model outside
    the kernel's limits is a ``ValueError``: this function never falls back."""
    if head:
        return dfw._forward(WIDE, _head_supports, _head_image, model, x, rec, score, threshold, normalizer, int(max_blocks),
                            int(tile), None, 1)
    return dfw._forward(WIDE, supports, image, model, x, rec, score, threshold, normalizer, int(max_blocks), int(tile))


def evaluate_sums(model, x: torch.Tensor, y: Optional[torch.Tensor] = None, normalizer=None,
                  max_blocks: int = 0, tile: int = 0, labels: Optional[torch.Tensor] = None) -> Tuple[float, float]:
    """(sum over rows of the row's mean squared error, rows whose argmax matches the target's) over device
    rows ``x`` against ``y`` [n, out] (or, without ``y``, the normalised row): one launch, one host read,
    the per-workgroup partials added in index order.  ``labels`` (integers, [n] or [n, 1], instead of
    ``y``): the final softmax layer is the head, and the sums are (cross-entropy, rows whose argmax is the
    label)."""
    if labels is None:
        return dfw._evaluate_sums(WIDE, supports, image, model, x, y, normalizer, int(max_blocks), int(tile))
    if y is not None or labels.is_floating_point() or labels.numel() != x.shape[0]:
        raise ValueError(f"wide fused Dense forward: a softmax head takes integer labels [{x.shape[0]}] and no y")
    lab = labels.reshape(-1).to(device=x.device, dtype=torch.int32).contiguous()
    part = dfw._launch(WIDE, _head_supports, _head_image, model, x, False, normalizer,
                       lambda n, out_w: (None, None, None, 0.0, True, None), (int(max_blocks), int(tile), lab, 1))[1]
    return dfw._sum_parts(part)
