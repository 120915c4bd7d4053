"""Fused bulk forward of a fleet of Dense stacks (``csrc/kernels/dense_forward_fleet.hip``).

M stacks of one shape, stacked as ``fleet.flat [M, stride]``, each over its own slice ``table[m] =
{first row, rows}`` of one flat row array, in ONE launch: the arithmetic of ``ops.dense_forward`` (a
row's reconstruction and score bits are those ``dense_forward.forward(fleet.model(m), rows)`` gives),
split over a persistent grid by tile pairs aligned to the models' first rows.  ``forward`` gives
reconstructions, scores and flags against per-model thresholds; ``evaluate_sums`` the per-model loss and
correct-row sums.  ``DenseFleet.score / detect / evaluate / calibrate_thresholds`` come here.

``supports`` and ``plan`` need no device: they mirror ``csrc/include/sml_dense_fleet_fwd.h``.

Images.  ``images`` is one gather of ``fleet.flat`` along dim 1 through the architecture's cached index
(and a fill of the padding): always current, no host copy.  A launch covers at most ``IMAGE_BUDGET``
bytes of images; a larger fleet goes in consecutive launches over consecutive members.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import dense_forward as dfw
from ._ext import load_c
from .serve import dense_layer_table

IMG_ALIGN = 256               # floats: image stride and LDS image buffers are whole 1 KiB chunks
MAX_MODELS = (1 << 24) - 1
PAIR_ROWS = 32
IMAGE_BUDGET = 512 << 20      # bytes of stacked images per launch
ASYNC_COPY = True             # the next image by global-to-LDS loads (False: through registers)


def _img_pad(floats: int) -> int:
    return (floats + IMG_ALIGN - 1) // IMG_ALIGN * IMG_ALIGN


def plan(widths) -> dict:
    """``dense_fleet_fwd_plan``: the single-model plan's ``mb`` and ``stride``, the image buffers in LDS
    (``nbuf``), the second one's float offset, the waves that fit and the dynamic LDS bytes."""
    one = dfw.plan(widths)
    dp = dfw._pad16(widths[0])
    pads = [dfw._pad16(u) for u in widths[1:]]
    buf = _img_pad(sum(a * b + b for a, b in zip([dp] + pads[:-1], pads)))
    wave_floats = dfw.WAVE_TILES * 16 * one["stride"]
    maxw = dfw.MAX_WAVES // 2 if one["mb"] == 8 else dfw.MAX_WAVES

    def fits(nbuf, waves):
        return (nbuf * buf + 2 * dp + waves * wave_floats) * 4 + dfw._STATIC_LDS <= dfw.LDS_BYTES

    nbuf = 2 if fits(2, maxw // 2) else 1
    waves = maxw
    while waves > 0 and not fits(nbuf, waves):
        waves >>= 1
    return {"mb": one["mb"], "nbuf": nbuf, "img2_off": buf if nbuf == 2 else 0, "waves": waves, "stride": one["stride"],
            "lds_bytes": (nbuf * buf + 2 * dp + waves * wave_floats) * 4}


def check_shape(widths, activations, score: bool, n_models: int) -> str:
    """``dense_fleet_fwd_check`` without slices: empty, or the limit exceeded."""
    why = dfw.check_shape(widths, activations, score)
    if why:
        return why
    if plan(widths)["waves"] < 1:
        return f"an image in whole 1 KiB chunks leaves no staging: the limit is {dfw.LDS_BYTES} (LDS_BYTES)"
    if not 1 <= int(n_models) <= MAX_MODELS:
        return f"a fleet of {int(n_models)} models: the fused fleet forward takes 1..{MAX_MODELS}"
    return ""


def supports(model, n_models: int = 1, score: bool = False) -> Tuple[bool, str]:
    """(True, "") if the kernel runs a fleet of ``n_models`` stacks shaped like ``model``, else (False, the
    limit it exceeds).  Needs no device."""
    return dfw._supports(lambda: dense_layer_table(model)[0], lambda w, a: check_shape(w, a, score, n_models))


def _state(fleet) -> dict:
    """Cached on the fleet: the layer table of the image, its gather index into a row of ``fleet.flat``
    (padded to the image stride), the padding mask, normalisers and device copies of row tables."""
    st = getattr(fleet, "_fleet_fwd_state", None)
    if st is not None:
        return st
    layers = dense_layer_table(fleet._template)[0]
    idx = []
    for (n_in, n_out, _, use_bias), row in zip(layers, fleet.table):
        W = int(row[6]) + np.arange(n_in * n_out, dtype=np.int64).reshape(n_in, n_out)
        idx.append((W, int(row[7]) + np.arange(n_out, dtype=np.int64) if use_bias else None))
    index, table = dfw.pack_image(layers, idx, np.int64, fill=-1)
    index = np.concatenate([index, np.full(_img_pad(index.size) - index.size, -1, np.int64)])
    dev = fleet.device
    st = {"layers": layers, "table": [list(t) for t in table], "index": torch.from_numpy(np.maximum(index, 0)).to(dev),
          "pad": torch.from_numpy(index < 0).to(dev), "norm": {}, "tables": {}, "supports": {}}
    fleet._fleet_fwd_state = st
    return st


def images(fleet, m0: int = 0, m1: Optional[int] = None) -> Tuple[torch.Tensor, list]:
    """(fp32 device images [m1 - m0, stride] of members m0 .. m1 - 1 as they stand, layer table)."""
    st = _state(fleet)
    flat = fleet.flat if m0 == 0 and m1 in (None, fleet.n_models) else fleet.flat[m0:m1]
    return flat.index_select(1, st["index"]).masked_fill_(st["pad"], 0.0), st["table"]


def _rows_tables(fleet, table, n_rows: int, per_row: bool):
    """The checked table and its launches, cached for the latest table: ``{"table", "covers" (every row
    lies in exactly one slice), "disjoint", "launches": [(first member, end, host table, device table,
    device pair_base)]}``; a launch without rows is left out."""
    st = _state(fleet)
    M = fleet.n_models
    table = np.asarray(table)
    if table.shape != (M, 2) or not np.issubdtype(table.dtype, np.integer):
        raise ValueError(f"table must be [{M}, 2] integers {{first row, rows}}")
    table = np.ascontiguousarray(table, np.int64)
    key = (table.tobytes(), int(n_rows))
    got = st["tables"].get(key)
    if got is None:
        outside = (table < 0).any(1) | (table[:, 0] + table[:, 1] > n_rows)
        if outside.any():
            bad = int(np.flatnonzero(outside)[0])
            raise ValueError(f"model {bad}: rows {table[bad, 0]} .. {table[bad, 0]} + {table[bad, 1]} lie outside the "
                             f"{n_rows} rows")
        t = table[table[:, 1] > 0]
        o = np.argsort(t[:, 0], kind="stable")
        disjoint = not (t[o[1:], 0] < t[o[:-1], 0] + t[o[:-1], 1]).any()
        per = max(1, IMAGE_BUDGET // (int(st["index"].numel()) * 4))
        launches = []
        for m0 in range(0, M, per):
            t = np.ascontiguousarray(table[m0:m0 + per])
            if int(t[:, 1].sum()) == 0:
                continue
            pb = np.concatenate([[0], np.cumsum(-(-t[:, 1] // PAIR_ROWS))]).astype(np.int64)
            launches.append((m0, m0 + len(t), torch.from_numpy(t), torch.from_numpy(t).to(fleet.device),
                             torch.from_numpy(pb).to(fleet.device)))
        got = {"table": table, "disjoint": disjoint, "covers": disjoint and int(table[:, 1].sum()) == n_rows,
               "launches": launches}
        st["tables"] = {key: got}    # the latest table only
    if per_row and not got["disjoint"]:
        raise ValueError("per-row outputs need row slices that do not overlap")
    return got


def _normalizer(fleet, normalizer, D: int):
    """The two named normalisers are cached on the fleet (it has one device)."""
    named = normalizer is None or isinstance(normalizer, str)
    return dfw._cached_normalizer(_state(fleet)["norm"] if named else None, normalizer, normalizer, D, fleet._template,
                                  "the models have", fleet.device)


def _prepare(fleet, x, table, score: bool, per_row: bool):
    st = _state(fleet)
    if score not in st["supports"]:
        st["supports"][score] = supports(fleet._template, fleet.n_models, score=score)
    ok, why = st["supports"][score]
    if not ok:
        raise ValueError(f"fused Dense fleet forward: {why}")
    D = st["table"][0][0]
    if (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.size(1) != D or x.device != fleet.device
            or x.dtype != torch.float32 or (D > 1 and x.stride(1) != 1)):
        raise ValueError(f"the rows must be a float32 [N, {D}] tensor with unit column stride on {fleet.device}")
    C = load_c()
    assert C.DFF_IMG_ALIGN == IMG_ALIGN
    return C, _rows_tables(fleet, table, int(x.size(0)), per_row), int(x.size(0))


def forward(fleet, x: torch.Tensor, table, rec: bool = True, score: bool = False, thresholds=None, normalizer=None,
            max_blocks: int = 0):
    """Every member over its own rows of ``x`` [N, D] (device fp32).  Returns ``(reconstructions [N, out]
    | None, scores [N] | None, flags [N] bool | None)``; flags (``score > thresholds[m]``, one number or
    [M]) come with ``score`` and thresholds.  Rows no slice covers hold NaN and False.  ``fleet.
    last_forward_launches`` counts the launches.  Never falls back: a fleet outside the limits is a ``ValueError``."""
    C, rt, n = _prepare(fleet, x, table, score, True)
    st = _state(fleet)
    M, out_w = fleet.n_models, st["table"][-1][1]
    sc, sh = _normalizer(fleet, normalizer, st["table"][0][0])
    dev = x.device
    new = torch.empty if rt["covers"] else (lambda *a, **k: torch.full(*a, float("nan"), **k))   # NaN where no slice covers
    r = new((n, out_w), device=dev) if rec else None
    s = new((n,), device=dev) if score else None
    f = thr = None
    if score and thresholds is not None:
        thr = np.asarray(thresholds, np.float32)
        thr = np.full(M, float(thr), np.float32) if thr.ndim == 0 else thr.reshape(-1)
        if thr.shape != (M,):
            raise ValueError(f"thresholds must be one number or [{M}], one per model")
        thr = torch.from_numpy(np.ascontiguousarray(thr)).to(dev)
        f = torch.zeros(n, dtype=torch.bool, device=dev)
    fleet.last_forward_launches = 0
    for m0, m1, host, tdev, pb in rt["launches"]:
        img, ltable = images(fleet, m0, m1)
        C.dense_forward_fleet(x, img, ltable, host, tdev, pb, sc, sh, r, s, f, None if thr is None else thr[m0:m1],
                              False, None, int(max_blocks), not ASYNC_COPY)
        fleet.last_forward_launches += 1
    return r, s, f


def evaluate_sums(fleet, x: torch.Tensor, table, y: Optional[torch.Tensor] = None, normalizer=None,
                  max_blocks: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Per member (sum over its rows of the row's mean squared error, rows whose argmax matches the
    target's), float64 [M] each, against ``y`` [N, out] or the normalised row: one host read per launch,
    the slots folded in slot order."""
    C, rt, n = _prepare(fleet, x, table, y is None, False)
    st = _state(fleet)
    M = fleet.n_models
    sc, sh = _normalizer(fleet, normalizer, st["table"][0][0])
    loss, correct = np.zeros(M), np.zeros(M)
    fleet.last_forward_launches = 0
    for m0, m1, host, tdev, pb in rt["launches"]:
        img, ltable = images(fleet, m0, m1)
        part, model = C.dense_forward_fleet(x, img, ltable, host, tdev, pb, sc, sh, None, None, None, None, True, y,
                                            int(max_blocks), not ASYNC_COPY)
        part, model = part.cpu().numpy(), model.cpu().numpy()
        used = model >= 0
        np.add.at(loss, m0 + model[used], part[used, 0])      # unbuffered: in slot order
        np.add.at(correct, m0 + model[used], part[used, 1])
        fleet.last_forward_launches += 1
    return loss, correct


def quantile_index(rows: np.ndarray, q: float) -> np.ndarray:
    """Index, in a member's ascending scores, of ``np.quantile(scores, q, method="higher")``: numpy's own
    virtual index ``n q + (1 - q) - 1`` in float64, rounded up."""
    n = rows.astype(np.float64)
    q = np.float64(q)
    virt = n * q + (1.0 + q * (1.0 - 1.0 - 1.0)) - 1.0
    return np.clip(np.ceil(virt).astype(np.int64), 0, np.maximum(rows - 1, 0))


def segmented_quantiles(scores: torch.Tensor, table: np.ndarray, q: float) -> np.ndarray:
    """``[M]`` float32: member m's ``q`` order statistic of ``scores[first : first + rows]``, by a
    segmented sort on the device (sort by score, then a stable sort by member)."""
    dev = scores.device
    rows = torch.from_numpy(table[:, 1].copy()).to(dev)
    first = torch.from_numpy(table[:, 0].copy()).to(dev)
    start = torch.cumsum(rows, 0) - rows
    total = int(table[:, 1].sum())
    seg = torch.repeat_interleave(torch.arange(len(table), device=dev), rows, output_size=total)
    idx = first[seg] + (torch.arange(total, device=dev) - start[seg])
    vals, o1 = torch.sort(scores[idx])
    o2 = torch.sort(seg[o1], stable=True)[1]
    grouped = vals[o2]                                   # member by member, ascending inside each
    k = torch.from_numpy(quantile_index(table[:, 1], q)).to(dev)
    return grouped[start + k].cpu().numpy().astype(np.float32)
