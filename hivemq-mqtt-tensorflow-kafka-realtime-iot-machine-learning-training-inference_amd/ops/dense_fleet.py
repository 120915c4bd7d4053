"""Fleet training of Dense stacks: many models of ONE architecture, one persistent workgroup each.

The persistent Dense trainer (``ops/dense_persistent.py``, ``dense_minibatch.hip`` and
``dense_minibatch_bf16.hip``) is one workgroup, so a single model uses one CU.  A per-car, ensemble
or learning-rate-sweep workload trains M such models; the fleet entries of the two kernels run them
in ONE launch of M workgroups.  Workgroup ``b`` trains model ``sched[b]``: its arguments are rebased
once from a per-model descriptor and the single-model body runs unchanged, so a fleet member is bit
for bit the model trained alone with ``dense_persistent.train_steps``.  No workgroup waits on
another: models take different numbers of steps and a fleet larger than the CU count runs in rounds.

State is stacked: ``flat / m / v [M, stride]`` (each row laid out as ``FlatParams.flat`` of the single
model), ``iter [M]``.  Rows live in one flat array ``x[N, D]``; model ``b`` owns the slice
``table[b] = {first row, rows}`` (``ops.ae_fleet.ragged_rings_by_key`` builds such a table) and
keeps a cursor into it, so a pass can be split over several launches.

The surface follows ``ops.ae_fleet.AEFleet`` as far as the different state allows.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dense_persistent as dpers
from ._ext import load_c

# one row per model, read by the kernels as DenseMBFleetModel (sml_ops.h)
DESCRIPTOR = np.dtype([("first_row", "<i8"), ("rows", "<i8"), ("row0", "<i8"), ("nsteps", "<i4"), ("lr", "<f4")])
SCHEDULES = ("longest_first", "index")


def _structure(model) -> List[Tuple[str, object]]:
    """What every member of a fleet must share, as (name, value) pairs in the order they are compared."""
    layers, why = dpers.dense_layers(model)
    if layers is None:
        raise ValueError(why)
    if not layers:
        raise ValueError("the model has no Dense layer")
    if not model.compiled:
        raise ValueError("fleet members must be compiled")
    out: List[Tuple[str, object]] = [("input shape", tuple(model._input_shape())), ("depth", len(layers))]
    for l, lyr in enumerate(layers):
        r = lyr.activity_regularizer
        out += [(f"layer {l} units", int(lyr.units)), (f"layer {l} activation", lyr.activation),
                (f"layer {l} use_bias", bool(lyr.use_bias)),
                (f"layer {l} activity regulariser (l1, l2)", (float(r.l1), float(r.l2)) if r else (0.0, 0.0))]
    out.append(("loss", model.loss))
    out += [(k, float(model.hp[k])) for k in ("beta_1", "beta_2", "epsilon")]
    out.append(("parameter layout", dpers.table(model)))
    return out


def first_difference(models) -> str:
    """Empty if the models can share a fleet, else the first thing in which one differs from model 0."""
    ref = _structure(models[0])
    for i, mdl in enumerate(models[1:], start=1):
        for (name, a), (_, b) in zip(ref, _structure(mdl)):
            if a != b:
                return f"model {i} differs from model 0 in {name}: {b!r} != {a!r}"
    return ""


class DenseFleet:
    """M Dense stacks of one architecture, trained concurrently (one workgroup per model)."""

    def __init__(self, models: Sequence, device, precision: str = "fp32", lr=None, stride: Optional[int] = None,
                 schedule: str = "longest_first"):
        models = list(models)
        if not models:
            raise ValueError("a fleet needs at least one model")
        if precision not in dpers.PRECISION:
            raise ValueError(f"precision must be 'fp32' or 'bf16', not {precision!r}")
        if schedule not in SCHEDULES:
            raise ValueError(f"schedule must be one of {SCHEDULES}, not {schedule!r}")
        why = first_difference(models)
        if why:
            raise ValueError(why)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DenseFleet runs on a ROCm device only")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.C = load_c()
        self._precision = precision
        self.schedule = schedule
        self._template = models[0]
        self._n_models = M = len(models)
        self.table = dpers.table(models[0])
        self.hp = dict(models[0].hp)
        fp = models[0].fp
        self.nflat = n = int(fp.n)
        self.stride = int(fp.n_pad if stride is None else stride)
        if self.stride < n:
            raise ValueError(f"stride {self.stride} is below the {n} parameters of a model")
        if lr is None:
            lrs = np.array([float(mdl.hp["lr"]) for mdl in models], np.float32)
        elif np.ndim(lr) == 0:
            lrs = np.full(M, float(lr), np.float32)
        else:
            lrs = np.asarray(lr, dtype=np.float32)
            if lrs.shape != (M,):
                raise ValueError(f"lr must be None, a scalar or [{M}] per-model rates")
        self.lrs = lrs
        dev = self.device
        self.flat = torch.zeros(M, self.stride, device=dev)
        self.m = torch.zeros(M, self.stride, device=dev)
        self.v = torch.zeros(M, self.stride, device=dev)
        self.iter = torch.zeros(M, dtype=torch.int64, device=dev)
        for i, mdl in enumerate(models):
            self.flat[i, :n].copy_(mdl.fp.flat[:n])
            self.m[i, :n].copy_(mdl.fp.m[:n])
            self.v[i, :n].copy_(mdl.fp.v[:n])
            self.iter[i:i + 1].copy_(mdl.fp.iter)
        self.x: Optional[torch.Tensor] = None
        self.y: Optional[torch.Tensor] = None
        self.batch = 0
        self._rows_table: Optional[np.ndarray] = None
        self._cursor = np.zeros(M, np.int64)
        self._pending: list = []          # (out [M, S, 2], steps [M], rows of each model's last step [M])
        self._launches = 0
        self.last_out: Optional[torch.Tensor] = None    # [M, S, 2] of the latest launch: per step (loss, correct rows)

    @classmethod
    def from_seeds(cls, build, seeds: Sequence[int], device, **kw) -> "DenseFleet":
        """``build(seed) -> compiled model``, one member per seed."""
        return cls([build(int(s)) for s in seeds], device, **kw)

    @staticmethod
    def supports(model, batch_size: int, n_models: int, precision: str = "fp32",
                 own_targets: bool = False) -> Tuple[bool, str]:
        """(True, "") if a fleet of ``n_models`` copies of ``model`` can train at ``batch_size`` in this
        precision, else (False, reason).  Needs no device."""
        ok, why = dpers.supports(model, batch_size, own_targets=own_targets, precision=precision)
        if not ok:
            return False, why
        if int(n_models) < 1:
            return False, f"a fleet of {int(n_models)} models: it needs at least one"
        if int(n_models) >= 1 << 24:
            return False, f"a fleet of {int(n_models)} models: the limit is {(1 << 24) - 1}"
        return True, ""

    # -- properties --------------------------------------------------------------------
    @property
    def n_models(self) -> int:
        return self._n_models

    @property
    def precision(self) -> str:
        return self._precision

    @property
    def launches(self) -> int:
        return self._launches

    # -- data --------------------------------------------------------------------------
    def attach_ragged(self, flat_rows: torch.Tensor, batch: int, table, y: Optional[torch.Tensor] = None) -> None:
        """Models of different sizes in one flat row array: model b's rows are
        ``flat_rows[table[b, 0] : table[b, 0] + table[b, 1]]`` (and the same rows of ``y`` when the
        models have targets of their own).  Row counts need not be multiples of ``batch``: the last
        step of a pass is then partial."""
        M = self.n_models
        table = np.asarray(table)
        if table.shape != (M, 2) or not np.issubdtype(table.dtype, np.integer):
            raise ValueError(f"table must be [{M}, 2] integers {{first row, rows}}")
        table = table.astype(np.int64)
        D, O = int(self.table[0][0]), int(self.table[-1][1])
        if not isinstance(flat_rows, torch.Tensor) or flat_rows.dim() != 2 or flat_rows.size(1) != D:
            raise ValueError(f"the rows must be a [N, {D}] tensor")
        if (table[:, 1] < 1).any():
            raise ValueError(f"models {np.flatnonzero(table[:, 1] < 1)[:8].tolist()} have no rows")
        if table[:, 0].min() < 0 or (table[:, 0] + table[:, 1]).max() > flat_rows.size(0):
            raise ValueError("table rows outside the flat array")
        if flat_rows.device != self.device or flat_rows.dtype != torch.float32 or flat_rows.stride(1) != 1:
            raise ValueError("the rows must be float32 with unit column stride on " + str(self.device))
        if y is not None:
            if (not isinstance(y, torch.Tensor) or y.dim() != 2 or y.size(0) != flat_rows.size(0) or y.size(1) != O
                    or y.device != self.device or y.dtype != torch.float32 or y.stride(1) != 1):
                raise ValueError(f"y must be a float32 [{flat_rows.size(0)}, {O}] tensor on {self.device}")
        ok, why = self.supports(self._template, int(batch), M, self._precision, own_targets=y is not None)
        if not ok:
            raise ValueError(f"persistent Dense trainer: {why}")
        self.x, self.y, self.batch = flat_rows, y, int(batch)
        self._rows_table = table
        self._cursor[:] = 0

    def attach_rows(self, rows: torch.Tensor, batch: int, y: Optional[torch.Tensor] = None) -> None:
        """``rows [M, n, D]``: model b trains on ``rows[b]`` (``y [M, n, O]`` likewise)."""
        M = self.n_models
        if not isinstance(rows, torch.Tensor) or rows.dim() != 3 or rows.size(0) != M or rows.size(1) < 1:
            raise ValueError(f"rows must be a [{M}, n, D] tensor")
        n = int(rows.size(1))
        if y is not None:
            if not isinstance(y, torch.Tensor) or y.dim() != 3 or tuple(y.shape[:2]) != (M, n):
                raise ValueError(f"y must be a [{M}, {n}, O] tensor")
            y = y.contiguous().view(M * n, y.size(2))
        table = np.stack([np.arange(M, dtype=np.int64) * n, np.full(M, n, np.int64)], axis=1)
        self.attach_ragged(rows.contiguous().view(M * n, rows.size(2)), batch, table, y=y)

    def epoch_steps(self) -> np.ndarray:
        """Steps of one pass over each model's own rows (the last one partial where they run out)."""
        self._need_rows()
        return -(-self._rows_table[:, 1] // self.batch)

    # -- training ----------------------------------------------------------------------
    def train_epoch(self, epochs: int = 1, shuffle: bool = False, seed: int = 0) -> None:
        """Every model passes ``epochs`` times over its OWN rows, one launch per epoch.  ``shuffle``:
        each model walks its rows in a permutation of its own, drawn from (seed, epoch, model)."""
        self._need_rows()
        for ep in range(int(epochs)):
            order = None
            if shuffle:
                t = self._rows_table
                if (np.sort(t[:, 0])[1:] < np.sort(t[:, 0] + t[:, 1])[:-1]).any():
                    raise ValueError("shuffle needs models whose row slices do not overlap")
                local = np.zeros(int(self.x.size(0)), np.int32)
                for i, (first, rows) in enumerate(t):
                    local[first:first + rows] = np.random.default_rng([seed, ep, i]).permutation(int(rows))
                order = torch.from_numpy(local).to(self.device)
            self._cursor[:] = 0
            self._launch(self.epoch_steps(), order)

    def train_steps(self, nsteps, order: Optional[torch.Tensor] = None) -> None:
        """``nsteps`` (a number, or one per model) further steps of every model from its own cursor, in
        one launch; a model whose rows run out stops there, and starts its next pass with the next call.
        ``order``: int32 ``[N]`` on the device, position ``table[b, 0] + p`` holding the index, local to
        model b's slice, of the row model b reads at position ``p``."""
        self._need_rows()
        steps = np.broadcast_to(np.asarray(nsteps, np.int64), (self.n_models,)).copy()
        if (steps < 1).any() or (steps >= 1 << 30).any():
            raise ValueError("nsteps must be in 1 .. 2^30 - 1 for every model")
        self._cursor[self._cursor >= self._rows_table[:, 1]] = 0
        self._launch(steps, order)

    def _need_rows(self) -> None:
        if self._rows_table is None:
            raise RuntimeError("attach_ragged() or attach_rows() first")

    def _launch(self, steps: np.ndarray, order: Optional[torch.Tensor]) -> None:
        t, B = self._rows_table, self.batch
        left = t[:, 1] - self._cursor
        taken = np.minimum(steps, -(-left // B))
        desc = np.zeros(self.n_models, DESCRIPTOR)
        desc["first_row"], desc["rows"], desc["row0"] = t[:, 0], t[:, 1], self._cursor
        desc["nsteps"], desc["lr"] = steps, self.lrs
        if self.schedule == "longest_first":
            sched = np.argsort(-taken, kind="stable").astype(np.int32)
        else:
            sched = np.arange(self.n_models, dtype=np.int32)
        hp = self.hp
        out = self.C.dense_mb_train_fleet(self.flat, self.m, self.v, self.iter, self.table, self.x, self.y, order,
                                          torch.from_numpy(desc.view(np.int64).reshape(-1, 4)),
                                          torch.from_numpy(sched), B, hp["beta_1"], hp["beta_2"], hp["epsilon"],
                                          dpers.PRECISION[self._precision])
        last = np.minimum(left - (taken - 1) * B, B)
        self._pending.append((out, taken, last))
        self._cursor = np.minimum(self._cursor + taken * B, t[:, 1])
        self._launches += 1
        self.last_out = out

    # -- metrics -----------------------------------------------------------------------
    def reset_metrics(self) -> None:
        self._pending = []

    def read_metrics(self) -> List[dict]:
        """Per-model ``loss`` (row-weighted mean of the steps' losses, penalties included),
        ``accuracy`` and ``rows`` over the launches since ``reset_metrics`` (one host sync)."""
        M = self.n_models
        if not self._pending:
            return [{"loss": 0.0, "accuracy": 0.0, "rows": 0.0} for _ in range(M)]
        outs = torch.cat([o.reshape(M, -1) for o, _, _ in self._pending], dim=1).double().cpu().numpy()
        loss, corr, rows = np.zeros(M), np.zeros(M), np.zeros(M)
        col = 0
        for o, taken, last in self._pending:
            S = int(o.size(1))
            r = outs[:, col:col + 2 * S].reshape(M, S, 2)
            col += 2 * S
            s = np.arange(S)[None, :]
            w = np.where(s < taken[:, None] - 1, self.batch, np.where(s == taken[:, None] - 1, last[:, None], 0))
            loss += (r[:, :, 0] * w).sum(1)
            corr += (r[:, :, 1] * (w > 0)).sum(1)
            rows += w.sum(1)
        d = np.maximum(rows, 1.0)
        return [{"loss": float(loss[i] / d[i]), "accuracy": float(corr[i] / d[i]), "rows": float(rows[i])}
                for i in range(M)]

    # -- state -------------------------------------------------------------------------
    def _check_index(self, i: int) -> int:
        if not 0 <= int(i) < self.n_models:
            raise IndexError(f"model {i} of a fleet of {self.n_models}")
        return int(i)

    def get_weights(self, i: int) -> List[np.ndarray]:
        return self._template.fp.split(self.flat[self._check_index(i)])

    def set_weights(self, i: int, weights: Sequence[np.ndarray]) -> None:
        fp = self._template.fp
        weights = [np.asarray(w, np.float32) for w in weights]
        if [w.shape for w in weights] != list(fp.shapes):
            raise ValueError(f"weights of shapes {[w.shape for w in weights]}, not {list(fp.shapes)}")
        buf = np.concatenate([w.ravel() for w in weights])
        self.flat[self._check_index(i), :self.nflat].copy_(torch.from_numpy(buf))

    def server(self, **kw):
        """A :class:`~streamml.ops.serve.DenseFleetScoringServer` over this fleet's weights as they stand."""
        from .serve import DenseFleetScoringServer
        return DenseFleetScoringServer.from_fleet(self, **kw)

    def model(self, i: int, device=None):
        """Model ``i`` as a standalone ``nn`` model of the fleet's architecture with its weights, Adam
        moments, iteration and learning rate: it can go on training with ``fit`` (the fleet's
        precision is its ``minibatch_precision``), be saved, or be served."""
        from ..nn.layers import layer_from_config
        from ..nn.model import Adam, Model, Sequential
        i = self._check_index(i)
        t = self._template
        cfg = t.model_config()["config"]
        layers = [layer_from_config(l["class_name"], l["config"]) for l in cfg["layers"]]
        dev = self.device if device is None else device
        if t.functional:
            for a, b in zip(layers[:-1], layers[1:]):
                b.inbound = [a]
            mdl = Model(inputs=layers[0], outputs=layers[-1], name=t.name, device=dev)
        else:
            mdl = Sequential(layers, name=t.name, device=dev)
        mdl.compile(optimizer=Adam(learning_rate=float(self.lrs[i]), beta_1=self.hp["beta_1"], beta_2=self.hp["beta_2"],
                                   epsilon=self.hp["epsilon"]), loss=t.loss, metrics=list(t.metrics),
                    fused=t._fused_arg, minibatch_precision=self._precision)
        n = self.nflat
        with torch.no_grad():
            mdl.fp.flat[:n].copy_(self.flat[i, :n])
            mdl.fp.m[:n].copy_(self.m[i, :n])
            mdl.fp.v[:n].copy_(self.v[i, :n])
            mdl.fp.iter.copy_(self.iter[i:i + 1])
        if mdl._fused is not None:     # the recognised autoencoder trains on its fused backend
            mdl._sync_to_fused()
        return mdl
