"""Fused bulk forward of a Dense stack (``csrc/kernels/dense_forward.hip``).

One launch runs a whole stack of 1 .. ``MAX_LAYERS`` Dense layers, every width (input included) up to
``MAX_WIDTH``, over all rows: rows are read once, activations chain from layer to layer in registers on
fp32 MFMAs.  ``forward`` gives reconstructions, per-row scores (``mean((y - xn)^2)``,
``xn = x * scale + shift``: ``DenseScoringServer``'s convention) and flags; ``evaluate_sums`` the loss
and accuracy sums of ``nn.Model.evaluate``.  ``nn.Model.predict / score / detect /
reconstruct_and_score / evaluate`` come here under ``engine="fused"`` (and ``"auto"``).

``supports`` needs no device and no built extension: it mirrors ``dense_fwd_check`` and ``dense_fwd_plan``
of ``csrc/include/sml_dense_fwd_plan.h``.

The image.  ``pack_image`` is the layout, in numpy.  For an ``nn.Model`` the VALUES are not cached: six
kernels (the trainers, Adam, the data-parallel all-reduce) update ``model.fp.flat`` in place where no
Python hook sees it, so a cached copy could not be invalidated reliably.  What is cached on the model is
the image's gather index into the flat buffer (it depends on the architecture only); ``image`` is then one
16 K-element device gather (and a fill of the padding) per call, always current, with no host copy.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ._ext import load_c
from .serve import _resolve_normalizer, dense_layer_table

ACT = {"linear": 0, "relu": 1, "tanh": 2, "sigmoid": 3}
MAX_LAYERS = 8
MAX_WIDTH = 128
LDS_BYTES = 160 * 1024
WAVE_TILES = 2               # 16-row tiles a wave runs at once
MAX_WAVES = 8                # 4 for the widest kernel instance
_STATIC_LDS = 1024
_STAGE_PAD = 4


def _pad16(n: int) -> int:
    return (n + 15) // 16 * 16


def image_table(layers) -> Tuple[list, int]:
    """(table of ``(in, units, activation code, w_off, b_off)``, floats of the image) for ``layers`` =
    ``[(in, units, activation name, use_bias)]``: per layer ``pad16(in) * pad16(units)`` weights, then
    ``pad16(units)`` biases."""
    table, off = [], 0
    for n_in, n_out, act, _ in layers:
        kp, npad = _pad16(n_in), _pad16(n_out)
        table.append((n_in, n_out, ACT.get(act, -1), off, off + kp * npad))   # -1: the check names it
        off += kp * npad + npad
    return table, off


def plan(widths) -> dict:
    """``dense_fwd_plan``: the kernel instance (``mb`` 16-wide blocks), the staging stride, the waves of
    a workgroup that fit (0: none) and the dynamic LDS bytes."""
    dp = _pad16(widths[0])
    pads = [_pad16(u) for u in widths[1:]]
    off = sum(a * b + b for a, b in zip([dp] + pads[:-1], pads)) + 2 * dp
    blocks = max([dp] + pads) // 16
    mb = 2 if blocks <= 2 else 4 if blocks <= 4 else 8
    stride = max(dp, pads[-1]) + _STAGE_PAD
    wave_floats = WAVE_TILES * 16 * stride
    waves = MAX_WAVES // 2 if mb == 8 else MAX_WAVES
    while waves > 0 and (off + waves * wave_floats) * 4 + _STATIC_LDS > LDS_BYTES:
        waves >>= 1
    return {"mb": mb, "stride": stride, "waves": waves, "lds_bytes": (off + waves * wave_floats) * 4,
            "one_wave_bytes": (off + wave_floats) * 4 + _STATIC_LDS}


def check_shape(widths, activations, score: bool = False) -> str:
    """Empty if the kernel takes a stack ``widths[0] -> widths[1] -> ...`` with these activation names
    (``score``: against the input row), else the limit it exceeds -- ``dense_fwd_check``'s words."""
    nl = len(widths) - 1
    if nl < 1 or nl > MAX_LAYERS:
        return f"{nl} Dense layers: the fused forward takes 1..{MAX_LAYERS} (MAX_LAYERS)"
    if widths[0] < 1 or widths[0] > MAX_WIDTH:
        return f"input width {widths[0]} is outside 1..{MAX_WIDTH} (MAX_WIDTH)"
    for l, (u, act) in enumerate(zip(widths[1:], activations)):
        if u < 1 or u > MAX_WIDTH:
            return f"layer {l} has {u} units: the limit is {MAX_WIDTH} (MAX_WIDTH)"
        if act not in ACT:
            return f"layer {l}: unknown activation"
    if score and widths[-1] != widths[0]:
        return (f"scores against the input row need as many output units as inputs ({widths[-1]} units, "
                f"{widths[0]} inputs)")
    p = plan(widths)
    if p["waves"] < 1:
        return f"{p['one_wave_bytes']} bytes of LDS: the limit is {LDS_BYTES} (LDS_BYTES)"
    return ""


def _is_nn(model) -> bool:
    return hasattr(model, "layers") and hasattr(model, "_input_shape")


def _layers(model) -> list:
    """``dense_layer_table``'s layer list; for an ``nn.Model`` the cached one (no copy of the weights)."""
    return _state(model)["layers"] if _is_nn(model) else dense_layer_table(model)[0]


def supports(model, score: bool = False) -> Tuple[bool, str]:
    """(True, "") if the kernel can run ``model`` (``score``: with scores against the input row), else
    (False, the limit it exceeds).  Needs no device."""
    try:
        layers = _layers(model)
    except ValueError as e:
        return False, str(e)
    if not layers:
        return False, "the model has no Dense layer"
    why = check_shape([layers[0][0]] + [l[1] for l in layers], [l[2] for l in layers], score)
    return (not why), why


def pack_image(layers, weights, dtype=np.float32, fill=0) -> Tuple[np.ndarray, list]:
    """Pack ``weights`` = ``[(W [in, units], b [units] or None)]`` into the kernel's image: per layer
    ``img[kb][ub][lane][r] = W[16 kb + 4 (lane // 16) + r][16 ub + lane % 16]`` (a lane's four A values of
    a block pair in 16 bytes), ``fill`` past ``in`` / ``units``, then the bias padded to 16 with ``fill``
    (all ``fill`` without a bias).  Returns (image, table of ``image_table``)."""
    parts = []
    for (n_in, n_out, _, _), (W, b) in zip(layers, weights):
        W = np.asarray(W, dtype)
        if W.shape != (n_in, n_out):
            raise ValueError(f"kernel of shape {W.shape} for a {n_in} -> {n_out} layer")
        kp, npad = _pad16(n_in), _pad16(n_out)
        wp = np.full((kp, npad), fill, dtype)
        wp[:n_in, :n_out] = W
        bp = np.full(npad, fill, dtype)
        if b is not None:
            bp[:n_out] = np.asarray(b, dtype).reshape(n_out)
        # [kb, g, r, ub, c] -> [kb, ub, g, c, r]
        parts += [wp.reshape(kp // 16, 4, 4, npad // 16, 16).transpose(0, 3, 1, 4, 2).ravel(), bp]
    return np.ascontiguousarray(np.concatenate(parts), dtype), image_table(layers)[0]


def _state(model) -> dict:
    """What is cached on a built ``nn.Model``: the layer list, the table, the image's gather index into
    ``fp.flat`` and the mask of its padding, on the device the parameters are on now."""
    st = getattr(model, "_dense_fwd_state", None)
    if st is not None and st["fp"] is model.fp and st["index"].device == model.fp.flat.device:
        return st
    layers, _ = dense_layer_table(model)   # builds the model
    fp = model.fp
    from ..nn.layers import Dense
    dense = [l for l in model.layers if isinstance(l, Dense)]
    idx = []
    for (n_in, n_out, _, _), lyr in zip(layers, dense):
        w0 = int(fp.offsets[lyr.param_slots[0]])
        W = w0 + np.arange(n_in * n_out, dtype=np.int64).reshape(n_in, n_out)
        b = int(fp.offsets[lyr.param_slots[1]]) + np.arange(n_out, dtype=np.int64) if lyr.use_bias else None
        idx.append((W, b))
    index, table = pack_image(layers, idx, np.int64, fill=-1)
    dev = fp.flat.device
    st = {"fp": fp, "layers": layers, "table": [list(t) for t in table],
          "index": torch.from_numpy(np.maximum(index, 0)).to(dev), "pad": torch.from_numpy(index < 0).to(dev), "norm": {}}
    model._dense_fwd_state = st
    return st


def image(model) -> Tuple[torch.Tensor, list]:
    """(fp32 device image of the model's current weights, table)."""
    if _is_nn(model):
        st = _state(model)
        return st["fp"].flat.index_select(0, st["index"]).masked_fill_(st["pad"], 0.0), st["table"]
    layers, weights = dense_layer_table(model)
    img, table = pack_image(layers, weights)
    return torch.from_numpy(img).to(model.device), [list(t) for t in table]


def _normalizer(model, normalizer, D: int, dev):
    """(scale, shift) tensors on ``dev`` or (None, None); the two named normalisers are cached on the
    model, per device."""
    cacheable = _is_nn(model) and (normalizer is None or isinstance(normalizer, str))
    cache = _state(model)["norm"] if cacheable else {}
    key = (normalizer, str(dev)) if cacheable else None
    if cacheable and key in cache:
        return cache[key]
    sc, sh = _resolve_normalizer(normalizer, D, model, "the model has")
    out = (None, None) if sc is None else (torch.from_numpy(sc).to(dev), torch.from_numpy(sh).to(dev))
    if cacheable:
        cache[key] = out
    return out


def _check_limits(C) -> None:
    assert (C.DFW_MAXLAYERS, C.DFW_MAXW, C.DFW_LDS_BYTES) == (MAX_LAYERS, MAX_WIDTH, LDS_BYTES)


def forward(model, x: torch.Tensor, rec: bool = True, score: bool = False, threshold: Optional[float] = None,
            normalizer=None, max_blocks: int = 0):
    """The stack over device rows ``x`` [n, D] fp32 (any row stride) in one launch.  Returns
    ``(reconstructions [n, out] | None, scores [n] | None, flags [n] bool | None)`` as device tensors;
    flags (``score > threshold``) come with ``score`` and a threshold.  A model outside the kernel's limits
    is a ``ValueError``: this function never falls back."""
    ok, why = supports(model, score=score)
    if not ok:
        raise ValueError(f"fused Dense forward: {why}")
    C = load_c()
    _check_limits(C)
    img, table = image(model)
    n, out_w = int(x.shape[0]), table[-1][1]
    sc, sh = _normalizer(model, normalizer, table[0][0], x.device)
    r = torch.empty((n, out_w), device=x.device) if rec else None
    s = torch.empty(n, device=x.device) if score else None
    f = torch.empty(n, dtype=torch.bool, device=x.device) if score and threshold is not None else None
    if n:
        C.dense_forward(x, img, table, sc, sh, r, s, f, 0.0 if threshold is None else float(threshold), False, None,
                        int(max_blocks))
    return r, s, f


def evaluate_sums(model, x: torch.Tensor, y: Optional[torch.Tensor] = None, normalizer=None,
                  max_blocks: int = 0) -> Tuple[float, float]:
    """(sum over rows of the row's mean squared error, rows whose argmax matches the target's) over device
    rows ``x`` against ``y`` [n, out] (or, without ``y``, the normalised row): one launch, one host read,
    the per-workgroup partials added in index order."""
    ok, why = supports(model, score=y is None)
    if not ok:
        raise ValueError(f"fused Dense forward: {why}")
    C = load_c()
    _check_limits(C)
    img, table = image(model)
    if int(x.shape[0]) == 0:
        return 0.0, 0.0
    sc, sh = _normalizer(model, normalizer, table[0][0], x.device)
    part = C.dense_forward(x, img, table, sc, sh, None, None, None, 0.0, True, y, int(max_blocks)).cpu().numpy()
    tot = np.cumsum(part, axis=0)[-1]   # sequential: index order
    return float(tot[0]), float(tot[1])
