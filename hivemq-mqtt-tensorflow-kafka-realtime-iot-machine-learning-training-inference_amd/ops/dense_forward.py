"""Fused bulk forward of a Dense stack (``csrc/kernels/dense_forward.hip``).

One launch runs a whole stack of 1 .. ``MAX_LAYERS`` Dense layers, every width (input included) up to
``MAX_WIDTH``, over all rows: rows are read once, activations chain from layer to layer in registers on
fp32 MFMAs.  ``forward`` gives reconstructions, per-row scores (``mean((y - xn)^2)``,
``xn = x * scale + shift``: ``DenseScoringServer``'s convention) and flags; ``evaluate_sums`` the loss
and accuracy sums of ``nn.Model.evaluate``.  ``nn.Model.predict / score / detect /
reconstruct_and_score / evaluate`` come here under ``engine="fused"`` (and ``"auto"``).

``supports`` needs no device and no built extension: it mirrors ``dense_fwd_check`` and ``dense_fwd_plan``
of ``csrc/include/sml_dense_fwd_plan.h``.  tests/test_dense_forward_check.py holds the mirror and the
header together on the CPU, through ``csrc/tests/dense_fwd_check.cpp``.

Shared.  What this kernel's host side has in common with the wide one's (``ops/dense_forward_wide.py``) and
the fleet's (``ops/dense_fleet_forward.py``) is written once, here, over a ``Variant`` record: the rules of
``check_shape``, ``supports``, the padded matrix in fragment order behind every image and gather index,
the state cached on an ``nn.Model``, the normaliser cache and the ``forward`` / ``evaluate_sums`` drivers.

The image.  ``pack_image`` is the layout, in numpy.  For an ``nn.Model`` the VALUES are not cached: six
kernels (the trainers, Adam, the data-parallel all-reduce) update ``model.fp.flat`` in place where no
Python hook sees it, so a cached copy could not be invalidated reliably.  What is cached on the model is
the image's gather index into the flat buffer (it depends on the architecture only); ``image`` is then one
16 K-element device gather (and a fill of the padding) per call, always current, with no host copy.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

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


class Variant(NamedTuple):
    """What the host side of a fused forward kernel has of its own."""
    who: str                 # in the check's words and in front of forward's errors
    max_width: int
    kpad: int                # inputs of a weight block (units: 16)
    frag: Tuple[int, int]    # a block's fragment: (lane groups, values of a lane)
    bias_words: int          # image units of a bias entry
    split: bool              # the gather index holds every kernel, then every bias (they are rounded apart)
    state: str               # the attribute of an nn.Model that caches ``_state``
    binding: str
    limits: tuple            # (constant of the extension, its value here)


NARROW = Variant("fused", MAX_WIDTH, 16, (4, 4), 1, False, "_dense_fwd_state", "dense_forward",
                 (("DFW_MAXLAYERS", MAX_LAYERS), ("DFW_MAXW", MAX_WIDTH), ("DFW_LDS_BYTES", LDS_BYTES)))


def _pad(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _pad16(n: int) -> int:
    return _pad(n, 16)


def _table(v: Variant, layers) -> Tuple[list, int]:
    table, off = [], 0
    for n_in, n_out, act, _ in layers:
        kp, npad = _pad(n_in, v.kpad), _pad16(n_out)
        table.append((n_in, n_out, ACT.get(act, -1), off, off + kp * npad))   # -1: the check names it
        off += kp * npad + v.bias_words * npad
    return table, off


def image_table(layers) -> Tuple[list, int]:
    """(table of ``(in, units, activation code, w_off, b_off)``, floats of the image) for ``layers`` =
    ``[(in, units, activation name, use_bias)]``: per layer ``pad16(in) * pad16(units)`` weights, then
    ``pad16(units)`` biases."""
    return _table(NARROW, layers)


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


def _check_rows(v: Variant, widths, activations, score: bool) -> str:
    """``dense_fwd_check_rows``: the rules every fused forward has, in its words."""
    nl = len(widths) - 1
    if nl < 1 or nl > MAX_LAYERS:
        return f"{nl} Dense layers: the {v.who} forward takes 1..{MAX_LAYERS} (MAX_LAYERS)"
    if widths[0] < 1 or widths[0] > v.max_width:
        return f"input width {widths[0]} is outside 1..{v.max_width} (MAX_WIDTH)"
    for l, (u, act) in enumerate(zip(widths[1:], activations)):
        if u < 1 or u > v.max_width:
            return f"layer {l} has {u} units: the limit is {v.max_width} (MAX_WIDTH)"
        if act not in ACT:
            return f"layer {l}: unknown activation"
    if score and widths[-1] != widths[0]:
        return (f"scores against the input row need as many output units as inputs ({widths[-1]} units, "
                f"{widths[0]} inputs)")
    return ""


def check_shape(widths, activations, score: bool = False) -> str:
    """Empty if the kernel takes a stack ``widths[0] -> widths[1] -> ...`` with these activation names
    (``score``: against the input row), else the limit it exceeds -- ``dense_fwd_check``'s words."""
    why = _check_rows(NARROW, widths, activations, score)
    if why:
        return why
    p = plan(widths)
    if p["waves"] < 1:
        return f"{p['one_wave_bytes']} bytes of LDS: the limit is {LDS_BYTES} (LDS_BYTES)"
    return ""


def _is_nn(model) -> bool:
    return hasattr(model, "layers") and hasattr(model, "_input_shape")


def _state(model, v: Variant = NARROW) -> dict:
    """What is cached on a built ``nn.Model``: the layer list, the table, the normalisers and (once
    ``_indexed`` was asked) the image's gather index into ``fp.flat`` with the mask of its padding, on the
    device the parameters are on now."""
    st = getattr(model, v.state, None)
    if st is not None and st["fp"] is model.fp and (st["index"] is None or st["index"].device == model.fp.flat.device):
        return st
    layers, _ = dense_layer_table(model)   # builds the model
    st = {"fp": model.fp, "layers": layers, "table": [list(t) for t in _table(v, layers)[0]], "index": None, "norm": {}}
    setattr(model, v.state, st)
    return st


def _layers(model, v: Variant = NARROW) -> list:
    """``dense_layer_table``'s layer list; for an ``nn.Model`` the cached one (no copy of the weights)."""
    return _state(model, v)["layers"] if _is_nn(model) else dense_layer_table(model)[0]


def _supports(layers_of, check) -> Tuple[bool, str]:
    """``supports`` of every variant: ``check(widths, activation names)`` of the layers ``layers_of()`` gives."""
    try:
        layers = layers_of()
    except ValueError as e:
        return False, str(e)
    if not layers:
        return False, "the model has no Dense layer"
    why = check([layers[0][0]] + [l[1] for l in layers], [l[2] for l in layers])
    return (not why), why


def supports(model, score: bool = False) -> Tuple[bool, str]:
    """(True, "") if the kernel can run ``model`` (``score``: with scores against the input row), else
    (False, the limit it exceeds).  Needs no device."""
    return _supports(lambda: _layers(model), lambda w, a: check_shape(w, a, score))


def _fragments(v: Variant, n_in, n_out, W, b, dtype, fill) -> list:
    """[a layer's kernel ``W [in, units]`` padded with ``fill`` to whole blocks, in MFMA-fragment order
    (``out[kb][ub][lane][j] = wp[kpad kb + J (lane // 16) + j][16 ub + lane % 16]``, J values per lane);
    its bias ``b [units]`` or None padded to 16 with ``fill``]."""
    W = np.asarray(W, dtype)
    if W.shape != (n_in, n_out):
        raise ValueError(f"kernel of shape {W.shape} for a {n_in} -> {n_out} layer")
    kp, npad = _pad(n_in, v.kpad), _pad16(n_out)
    wp = np.full((kp, npad), fill, dtype)
    wp[:n_in, :n_out] = W
    bp = np.full(npad, fill, dtype)
    if b is not None:
        bp[:n_out] = np.asarray(b, dtype).reshape(n_out)
    # [kb, g, j, ub, c] -> [kb, ub, g, c, j]
    return [wp.reshape(kp // v.kpad, *v.frag, npad // 16, 16).transpose(0, 3, 1, 4, 2).ravel(), bp]


def pack_image(layers, weights, dtype=np.float32, fill=0) -> Tuple[np.ndarray, list]:
    """Pack ``weights`` = ``[(W [in, units], b [units] or None)]`` into the kernel's image: per layer
    ``img[kb][ub][lane][r] = W[16 kb + 4 (lane // 16) + r][16 ub + lane % 16]`` (a lane's four A values of
    a block pair in 16 bytes), ``fill`` past ``in`` / ``units``, then the bias padded to 16 with ``fill``
    (all ``fill`` without a bias).  Returns (image, table of ``image_table``)."""
    parts = []
    for (n_in, n_out, _, _), (W, b) in zip(layers, weights):
        parts += _fragments(NARROW, n_in, n_out, W, b, dtype, fill)
    return np.ascontiguousarray(np.concatenate(parts), dtype), image_table(layers)[0]


def _indexed(model, v: Variant = NARROW) -> dict:
    """``_state`` with the gather index: the image's element order (``v.split``: every kernel, then every
    bias; ``st["nw"]`` elements are kernels'), -1 where the image is padding."""
    st = _state(model, v)
    if st["index"] is None:
        from ..nn.layers import Dense
        fp = model.fp
        ws, bs = [], []
        for (n_in, n_out, _, _), lyr in zip(st["layers"], [l for l in model.layers if isinstance(l, Dense)]):
            W = int(fp.offsets[lyr.param_slots[0]]) + np.arange(n_in * n_out, dtype=np.int64).reshape(n_in, n_out)
            b = int(fp.offsets[lyr.param_slots[1]]) + np.arange(n_out, dtype=np.int64) if lyr.use_bias else None
            wf, bp = _fragments(v, n_in, n_out, W, b, np.int64, -1)
            ws.append(wf)
            bs.append(bp)
        index = np.concatenate(ws + bs if v.split else [p for wb in zip(ws, bs) for p in wb])
        dev = fp.flat.device
        st["nw"] = int(sum(len(w) for w in ws))
        st["pad"] = torch.from_numpy(index < 0).to(dev)
        st["index"] = torch.from_numpy(np.maximum(index, 0)).to(dev)
    return st


def _gather(model, v: Variant = NARROW) -> Tuple[torch.Tensor, dict]:
    """(the model's current parameters in the gather index's order, zero in the padding; the state)."""
    st = _indexed(model, v)
    return st["fp"].flat.index_select(0, st["index"]).masked_fill_(st["pad"], 0.0), st


def image(model) -> Tuple[torch.Tensor, list]:
    """(fp32 device image of the model's current weights, table)."""
    if _is_nn(model):
        g, st = _gather(model)
        return g, st["table"]
    layers, weights = dense_layer_table(model)
    img, table = pack_image(layers, weights)
    return torch.from_numpy(img).to(model.device), [list(t) for t in table]


def _cached_normalizer(cache, key, normalizer, D: int, template, whose: str, dev):
    """(scale, shift) tensors on ``dev`` or (None, None) for ``template``'s normaliser, kept in ``cache``
    (None: not to be cached) under ``key``."""
    if cache is not None and key in cache:
        return cache[key]
    sc, sh = _resolve_normalizer(normalizer, D, template, whose)
    out = (None, None) if sc is None else (torch.from_numpy(sc).to(dev), torch.from_numpy(sh).to(dev))
    if cache is not None:
        cache[key] = out
    return out


def _normalizer(model, normalizer, D: int, dev, v: Variant = NARROW):
    """The two named normalisers are cached on the model, per device."""
    cacheable = _is_nn(model) and (normalizer is None or isinstance(normalizer, str))
    return _cached_normalizer(_state(model, v)["norm"] if cacheable else None, (normalizer, str(dev)), normalizer, D, model,
                              "the model has", dev)


def _launch(v: Variant, supports_, image_, model, x, score: bool, normalizer, outputs, tail):
    """What ``forward`` and ``evaluate_sums`` of a variant do around the binding: refuse a model outside
    the limits, take the current image and the normaliser, and call ``v.binding`` with ``outputs(n, out
    width)`` = ``(rec, score, flag, threshold, sums, y)`` between them and ``tail``.  Without rows nothing
    is launched.  Returns (outputs, what the binding returned)."""
    ok, why = supports_(model, score=score)
    if not ok:
        raise ValueError(f"{v.who} Dense forward: {why}")
    C = load_c()
    assert all(getattr(C, name) == value for name, value in v.limits)
    img, table = image_(model)
    n = int(x.shape[0])
    out = outputs(n, table[-1][1])
    if not n and out[4]:   # sums of no rows: the normaliser is not asked for
        return out, None
    sc, sh = _normalizer(model, normalizer, table[0][0], x.device, v)
    return out, getattr(C, v.binding)(x, img, table, sc, sh, *out, *tail) if n else None


def _forward(v, supports_, image_, model, x, rec, score, threshold, normalizer, *tail):
    def outputs(n, out_w):
        return (torch.empty((n, out_w), device=x.device) if rec else None,
                torch.empty(n, device=x.device) if score else None,
                torch.empty(n, dtype=torch.bool, device=x.device) if score and threshold is not None else None,
                0.0 if threshold is None else float(threshold), False, None)

    return _launch(v, supports_, image_, model, x, score, normalizer, outputs, tail)[0][:3]


def _evaluate_sums(v, supports_, image_, model, x, y, normalizer, *tail) -> Tuple[float, float]:
    return _sum_parts(_launch(v, supports_, image_, model, x, y is None, normalizer,
                              lambda n, out_w: (None, None, None, 0.0, True, y), tail)[1])


def _sum_parts(part) -> Tuple[float, float]:
    """The per-workgroup pairs a sums launch returned (None: no rows), added in index order: one host read."""
    if part is None:
        return 0.0, 0.0
    tot = np.cumsum(part.cpu().numpy(), axis=0)[-1]   # sequential: index order
    return float(tot[0]), float(tot[1])


def forward(model, x: torch.Tensor, rec: bool = True, score: bool = False, threshold: Optional[float] = None,
            normalizer=None, max_blocks: int = 0):
    """The stack over device rows ``x`` [n, D] fp32 (any row stride) in one launch.  Returns
    ``(reconstructions [n, out] | None, scores [n] | None, flags [n] bool | None)`` as device tensors;
    flags (``score > threshold``) come with ``score`` and a threshold.  A model outside the kernel's limits
    is a ``ValueError``: this function never falls back."""
    return _forward(NARROW, supports, image, model, x, rec, score, threshold, normalizer, int(max_blocks))


def evaluate_sums(model, x: torch.Tensor, y: Optional[torch.Tensor] = None, normalizer=None,
                  max_blocks: int = 0) -> Tuple[float, float]:
    """(sum over rows of the row's mean squared error, rows whose argmax matches the target's) over device
    rows ``x`` against ``y`` [n, out] (or, without ``y``, the normalised row): one launch, one host read,
    the per-workgroup partials added in index order."""
    return _evaluate_sums(NARROW, supports, image, model, x, y, normalizer, int(max_blocks))
