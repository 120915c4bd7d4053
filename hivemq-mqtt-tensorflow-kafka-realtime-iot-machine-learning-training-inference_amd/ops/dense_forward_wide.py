"""Fused bulk forward of a wide Dense stack (``csrc/kernels/dense_forward_wide.hip``).

One launch runs a whole stack of 1 .. ``MAX_LAYERS`` Dense layers, every width (input included) up to
``MAX_WIDTH`` = 512, over all rows, with the rounding points of the bf16 trainers' forward: every
contraction is ``bf16(h) . bf16(W)`` on ``v_mfma_f32_16x16x32_bf16`` with fp32 accumulation; bias,
activation, scores and sums stay fp32.  Weights stream from a bf16 image in device memory, a tile's
activations stay in LDS.  ``forward`` and ``evaluate_sums`` return what ``ops.dense_forward``'s do;
``nn.Model.predict / score / detect / reconstruct_and_score / evaluate`` come here under ``engine="wide"``.

``supports`` needs no device and no built extension: it mirrors ``dense_fwdw_check`` of
``csrc/include/sml_dense_fwdw_plan.h``.

The image.  ``pack_image`` is the layout, in numpy (``uint16`` words).  For an ``nn.Model`` the VALUES are
never cached (kernels update ``model.fp.flat`` in place where no Python hook sees it): what is cached on
the model is the image's gather index into the flat buffer, and ``image`` is one device gather, one
rounding to bf16 and one concatenation per call.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ._ext import load_c
from .dense_forward import ACT, _is_nn
from .serve import _resolve_normalizer, dense_layer_table

MAX_LAYERS = 8
MAX_WIDTH = 512
WAVES = 8
ROWS = (64, 128)             # rows of a workgroup's tile
LDS_BYTES = 160 * 1024
_ROW_PAD = 8
_PART_WORDS = 5


def _pad(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def image_table(layers) -> Tuple[list, int]:
    """(table of ``(in, units, activation code, w_off, b_off)``, 16-bit words of the image) for ``layers`` =
    ``[(in, units, activation name, use_bias)]``: per layer ``pad32(in) * pad16(units)`` bf16 weights, then
    ``pad16(units)`` fp32 biases (two words each)."""
    table, off = [], 0
    for n_in, n_out, act, _ in layers:
        kp, npad = _pad(n_in, 32), _pad(n_out, 16)
        table.append((n_in, n_out, ACT.get(act, -1), off, off + kp * npad))   # -1: the check names it
        off += kp * npad + 2 * npad
    return table, off


def plan(widths, rows: int = 64) -> dict:
    """``dense_fwdw_plan``: the stride of an activation row in LDS (words) and the dynamic LDS bytes."""
    stride = max(_pad(w, 32) for w in widths[:-1]) + _ROW_PAD
    return {"rows": rows, "stride": stride, "lds_bytes": max(rows * stride * 2, WAVES * rows * _PART_WORDS * 4)}


def check_shape(widths, activations, score: bool = False) -> str:
    """Empty if the kernel takes a stack ``widths[0] -> widths[1] -> ...`` with these activation names
    (``score``: against the input row), else the limit it exceeds -- ``dense_fwdw_check``'s words.  The LDS
    plan fits at every width inside the limit."""
    nl = len(widths) - 1
    if nl < 1 or nl > MAX_LAYERS:
        return f"{nl} Dense layers: the wide fused forward takes 1..{MAX_LAYERS} (MAX_LAYERS)"
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
    return ""


def _layers(model) -> list:
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


def _fragments(wp: np.ndarray) -> np.ndarray:
    """A padded ``[kp, np]`` matrix in MFMA-fragment order: ``out[kb][ub][lane][j] =
    wp[32 kb + 8 (lane // 16) + j][16 ub + lane % 16]``."""
    kp, npad = wp.shape
    # [kb, g, j, ub, c] -> [kb, ub, g, c, j]
    return wp.reshape(kp // 32, 4, 8, npad // 16, 16).transpose(0, 3, 1, 4, 2).ravel()


def to_bf16(a) -> np.ndarray:
    """fp32 -> bf16 words, round to nearest even."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) >> np.uint32(16)).astype(np.uint16)


def _padded(n_in, n_out, W, b, dtype, fill):
    kp, npad = _pad(n_in, 32), _pad(n_out, 16)
    wp = np.full((kp, npad), fill, dtype)
    wp[:n_in, :n_out] = W
    bp = np.full(npad, fill, dtype)
    if b is not None:
        bp[:n_out] = np.asarray(b, dtype).reshape(n_out)
    return wp, bp


def pack_image(layers, weights) -> Tuple[np.ndarray, list]:
    """Pack ``weights`` = ``[(W [in, units], b [units] or None)]`` into the kernel's image (``uint16``): per
    layer the bf16 weights in fragment order (a lane's eight k-values of a 32-k by 16-unit block in 16
    bytes), zero past ``in`` / ``units``, then the fp32 bias padded to 16 with zeros (all zero without a
    bias), two little-endian words each.  Returns (image, table of ``image_table``)."""
    parts = []
    for (n_in, n_out, _, _), (W, b) in zip(layers, weights):
        W = np.asarray(W, np.float32)
        if W.shape != (n_in, n_out):
            raise ValueError(f"kernel of shape {W.shape} for a {n_in} -> {n_out} layer")
        wp, bp = _padded(n_in, n_out, W, b, np.float32, 0)
        parts += [to_bf16(_fragments(wp)), bp.view(np.uint16)]
    return np.ascontiguousarray(np.concatenate(parts)), image_table(layers)[0]


def _state(model) -> dict:
    """What is cached on a built ``nn.Model``: the layer list, the table, and the image's gather index into
    ``fp.flat`` (all weights in image order, then all biases) with the mask of its padding, on the device
    the parameters are on now."""
    st = getattr(model, "_dense_fwdw_state", None)
    if st is not None and st["fp"] is model.fp and (st["index"] is None or st["index"].device == model.fp.flat.device):
        return st
    layers, _ = dense_layer_table(model)   # builds the model
    st = {"fp": model.fp, "layers": layers, "table": [list(t) for t in image_table(layers)[0]], "index": None, "norm": {}}
    model._dense_fwdw_state = st
    return st


def _index(model) -> dict:
    st = _state(model)
    if st["index"] is None:
        from ..nn.layers import Dense
        fp = model.fp
        ws, bs = [], []
        for (n_in, n_out, _, _), lyr in zip(st["layers"], [l for l in model.layers if isinstance(l, Dense)]):
            W = int(fp.offsets[lyr.param_slots[0]]) + np.arange(n_in * n_out, dtype=np.int64).reshape(n_in, n_out)
            b = int(fp.offsets[lyr.param_slots[1]]) + np.arange(n_out, dtype=np.int64) if lyr.use_bias else None
            wp, bp = _padded(n_in, n_out, W, b, np.int64, -1)
            ws.append(_fragments(wp))
            bs.append(bp)
        index = np.concatenate(ws + bs)
        dev = fp.flat.device
        st["nw"] = int(sum(len(w) for w in ws))
        st["pad"] = torch.from_numpy(index < 0).to(dev)
        st["index"] = torch.from_numpy(np.maximum(index, 0)).to(dev)
    return st


def image(model) -> Tuple[torch.Tensor, list]:
    """(device image of the model's current weights as int16 words, table)."""
    if not _is_nn(model):
        layers, weights = dense_layer_table(model)
        img, table = pack_image(layers, weights)
        return torch.from_numpy(img.view(np.int16)).to(model.device), [list(t) for t in table]
    st = _index(model)
    g = st["fp"].flat.index_select(0, st["index"]).masked_fill_(st["pad"], 0.0)
    w16, b16 = g[:st["nw"]].to(torch.bfloat16).view(torch.int16), g[st["nw"]:].view(torch.int16)
    parts, wo, bo = [], 0, 0
    for n_in, n_out, _, _, _ in st["table"]:
        nw, nb = _pad(n_in, 32) * _pad(n_out, 16), 2 * _pad(n_out, 16)
        parts += [w16[wo:wo + nw], b16[bo:bo + nb]]
        wo, bo = wo + nw, bo + nb
    return torch.cat(parts), st["table"]


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


def _ext():
    C = load_c()
    assert (C.DFWW_MAXLAYERS, C.DFWW_MAXW) == (MAX_LAYERS, MAX_WIDTH)
    return C


def forward(model, x: torch.Tensor, rec: bool = True, score: bool = False, threshold: Optional[float] = None,
            normalizer=None, max_blocks: int = 0, tile: int = 0):
    """The stack over device rows ``x`` [n, D] fp32 (any row stride) in one launch.  Returns
    ``(reconstructions [n, out] | None, scores [n] | None, flags [n] bool | None)`` as device tensors;
    flags (``score > threshold``) come with ``score`` and a threshold.  ``tile``: rows of a workgroup's
    tile (64 or 128; 0: 128 when that still fills every CU).  A model outside the kernel's limits is a
    ``ValueError``: this function never falls back."""
    ok, why = supports(model, score=score)
    if not ok:
        raise ValueError(f"wide fused Dense forward: {why}")
    C = _ext()
    img, table = image(model)
    n, out_w = int(x.shape[0]), table[-1][1]
    sc, sh = _normalizer(model, normalizer, table[0][0], x.device)
    r = torch.empty((n, out_w), device=x.device) if rec else None
    s = torch.empty(n, device=x.device) if score else None
    f = torch.empty(n, dtype=torch.bool, device=x.device) if score and threshold is not None else None
    if n:
        C.dense_forward_wide(x, img, table, sc, sh, r, s, f, 0.0 if threshold is None else float(threshold), False, None,
                             int(max_blocks), int(tile))
    return r, s, f


def evaluate_sums(model, x: torch.Tensor, y: Optional[torch.Tensor] = None, normalizer=None,
                  max_blocks: int = 0, tile: int = 0) -> Tuple[float, float]:
    """(sum over rows of the row's mean squared error, rows whose argmax matches the target's) over device
    rows ``x`` against ``y`` [n, out] (or, without ``y``, the normalised row): one launch, one host read,
    the per-workgroup partials added in index order."""
    ok, why = supports(model, score=y is None)
    if not ok:
        raise ValueError(f"wide fused Dense forward: {why}")
    C = _ext()
    img, table = image(model)
    if int(x.shape[0]) == 0:
        return 0.0, 0.0
    sc, sh = _normalizer(model, normalizer, table[0][0], x.device)
    part = C.dense_forward_wide(x, img, table, sc, sh, None, None, None, 0.0, True, y, int(max_blocks),
                                int(tile)).cpu().numpy()
    tot = np.cumsum(part, axis=0)[-1]   # sequential: index order
    return float(tot[0]), float(tot[1])
