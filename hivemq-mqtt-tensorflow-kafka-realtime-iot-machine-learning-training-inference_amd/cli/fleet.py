"""``fleet``: one anomaly autoencoder per car (or per key group), trained concurrently.

The reference trains a single model on the whole stream (cardata-v3.py:187-203,
``fit(batch_size=32)``).  ``fleet`` keys the same rows by car id (the CSV's ``car``
column / the record key that the KSQL REKEY step produces) and trains one model per
key with the same Keras-batch semantics, all models at once on one GPU
(``ops/ae_fleet.py``).  It then writes every model as a Keras HDF5 file plus an
``index.json`` {name -> file, keys, final loss}.

``--layers 64,16,64`` trains the Dense stack ``cardata-v3 --layers`` builds (18 in, 18 out, tanh /
relu alternating, relu last) instead, one persistent workgroup per model (``ops/dense_fleet.py``),
on rows normalised once on the host; every ``.h5`` is one ``serve --model dense`` accepts,
``index.json`` also records ``layers``, ``engine`` and ``precision``, and the whole directory is what
``serve --model dense-fleet <dir>`` scores the live stream with, every car by its own model.

  fleet <csv|synthetic> [--models N] [--epochs E] [--batch 32] [--lr 1e-3] [--out DIR]
        [--layers 64,16,64 [--precision fp32|bf16]]
"""
from __future__ import annotations

import argparse
import json
import os
import re
from typing import Sequence


def parse_args(argv: Sequence[str]):
    p = argparse.ArgumentParser(prog="fleet", description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("source", help="car-sensor CSV (time,car,...) or 'synthetic'")
    p.add_argument("--models", type=int, default=None, help="hash keys onto N models (default: one per key)")
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--out", default="fleet_models")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--synthetic-rows", type=int, default=1 << 20)
    p.add_argument("--synthetic-devices", type=int, default=1000)
    p.add_argument("--layers", default=None,
                   help="hidden widths of a Dense stack, e.g. 64,16,64 (18 in, 18 out; tanh / relu alternate, relu "
                        "last): trains a fleet of such stacks on the persistent Dense trainer")
    p.add_argument("--precision", default=None, choices=["fp32", "bf16"],
                   help="with --layers: the trainer's contractions, fp32 (default) or bf16 MFMAs")
    ns = p.parse_args(list(argv))
    if ns.precision is not None and ns.layers is None:
        p.error("--precision goes with --layers")
    return ns


def model_name(members, i: int, used=None) -> str:
    """File stem of model ``i``: its key when it owns exactly one, else ``modelNNNNN``.
    ``used`` (a set) de-duplicates stems that sanitise alike (``car/1`` vs ``car_1``, or a
    key literally named ``model00003``): a later collision gets ``-<i>`` appended."""
    stem = re.sub(r"[^A-Za-z0-9_.-]", "_", str(members[i][0])) if len(members[i]) == 1 else f"model{i:05d}"
    if used is not None:
        if stem in used:
            stem = f"{stem}-{i}"
        used.add(stem)
    return stem


def training_rows(ns):
    """(raw rows, car keys) of NORMAL events only: the reference trains its anomaly model on
    ``failure_occurred == "false"`` rows (cardata-v3.py:211-212); the CSV has no failure
    column, so every CSV row counts as normal."""
    import numpy as np

    from ..data.cardata import SyntheticCarSource, load_csv
    if ns.source == "synthetic":
        src = SyntheticCarSource(seed=ns.seed, n_devices=ns.synthetic_devices)
        raw, fail, dev_id, _ = src.generate(ns.synthetic_rows)
        raw, dev_id = raw[~fail], dev_id[~fail]
        return raw, np.array([f"electric-vehicle-{d:05d}" for d in dev_id])
    raw, _, keys = load_csv(ns.source)
    return raw, keys


INDEX_META = ("layers", "engine", "precision")   # keys of index.json beside the models' names (--layers)


def build_index(names, members, losses, layers=None, precision=None) -> dict:
    """``index.json``: name -> {file, keys, loss}; for a ``--layers`` fleet also the stack's hidden
    widths, the engine that trained it and its precision."""
    index = {name: {"file": name + ".h5", "keys": [str(k) for k in members[i]], "loss": losses[i]}
             for i, name in enumerate(names)}
    if layers is not None:
        index.update(layers=[int(w) for w in layers], engine="persistent", precision=precision or "fp32")
    return index


def dense_stack(hidden, seed: int, lr: float, device="cpu", precision=None, features: int = 18):
    """The ``cardata-v3 --layers`` stack: features -> hidden widths -> features, tanh / relu
    alternating, relu last, compiled for MSE."""
    from .. import nn
    from ..nn.model import Adam
    widths = list(hidden) + [features]
    acts = ["tanh" if i % 2 == 0 else "relu" for i in range(len(widths))]
    acts[-1] = "relu"
    model = nn.Sequential([nn.Dense(u, activation=a, input_shape=(features,) if i == 0 else None)
                           for i, (u, a) in enumerate(zip(widths, acts))], device=device, seed=seed)
    model.compile(optimizer=Adam(learning_rate=lr), loss="mean_squared_error", metrics=["accuracy"],
                  minibatch_precision=precision)
    return model


def _main_layers(ns) -> int:
    import numpy as np
    import torch

    from ..data.cardata import normalize_affine
    from ..ops.ae_fleet import ragged_rings_by_key
    from ..ops.dense_fleet import DenseFleet
    from .cardata_autoencoder import _hidden_widths

    hidden = _hidden_widths(ns.layers)
    precision = ns.precision or "fp32"
    raw, keys = training_rows(ns)
    scale, shift = normalize_affine()
    rows = (raw.astype(np.float64) * scale + shift).astype(np.float32)     # normalize_fn, once
    flat, table, members = ragged_rings_by_key(rows, keys, batch=ns.batch, n_models=ns.models)
    M = len(members)
    ok, why = DenseFleet.supports(dense_stack(hidden, ns.seed, ns.lr, features=raw.shape[1]), ns.batch, M, precision)
    if not ok:
        raise SystemExit(f"fleet --layers {ns.layers}: {why}")
    dev = torch.device(ns.device)
    fleet = DenseFleet.from_seeds(lambda s: dense_stack(hidden, s, ns.lr, features=raw.shape[1]),
                                  [ns.seed + i for i in range(M)], dev, precision=precision)
    fleet.attach_ragged(torch.from_numpy(flat).to(dev), ns.batch, table)
    steps = fleet.epoch_steps()
    D = raw.shape[1]
    print(f"fleet: {M} models {D}-{'-'.join(str(w) for w in hidden)}-{D} ({precision}), {len(flat)} rows, "
          f"{int(steps.min())}-{int(steps.max())} steps of {ns.batch} rows per model per epoch", flush=True)
    ms = []
    for ep in range(ns.epochs):
        fleet.reset_metrics()
        fleet.train_epoch()
        ms = fleet.read_metrics()
        losses = np.array([m["loss"] for m in ms])
        print(f"Epoch {ep + 1}/{ns.epochs} - loss mean {losses.mean():.4f} min {losses.min():.4f} "
              f"max {losses.max():.4f}", flush=True)
    os.makedirs(ns.out, exist_ok=True)
    used = set(INDEX_META)
    names = [model_name(members, i, used) for i in range(M)]
    for i, name in enumerate(names):
        fleet.model(i, device="cpu").save(os.path.join(ns.out, name + ".h5"))
    index = build_index(names, members, [ms[i]["loss"] if ms else None for i in range(M)], hidden, precision)
    with open(os.path.join(ns.out, "index.json"), "w") as f:
        json.dump(index, f, indent=1)
    print(f"wrote {M} models to {ns.out}", flush=True)
    return 0


def main(argv: Sequence[str]) -> int:
    ns = parse_args(argv)
    if ns.layers:
        return _main_layers(ns)
    import numpy as np
    import torch

    from ..data.cardata import normalize_affine
    from ..models.autoencoder import Autoencoder
    from ..ops.ae import AESpec
    from ..ops.ae_fleet import AEFleet, ragged_rings_by_key

    raw, keys = training_rows(ns)
    flat, table, members = ragged_rings_by_key(raw, keys, batch=ns.batch, n_models=ns.models)
    M = len(members)
    spec = AESpec(input_dim=raw.shape[1])
    scale, shift = normalize_affine()
    dev = torch.device(ns.device)
    fleet = AEFleet.from_seeds(spec, [ns.seed + i for i in range(M)], dev, lr=ns.lr, scale=scale, shift=shift)
    fleet.attach_ragged(torch.from_numpy(flat).to(dev), ns.batch, table)
    steps = fleet.epoch_steps()
    print(f"fleet: {M} models, {len(flat)} rows, {int(steps.min())}-{int(steps.max())} steps of {ns.batch} rows "
          f"per model per epoch", flush=True)
    ms = []
    for ep in range(ns.epochs):
        fleet.reset_metrics()
        fleet.train_epoch()
        ms = fleet.read_metrics()
        losses = np.array([m["loss"] for m in ms])
        print(f"Epoch {ep + 1}/{ns.epochs} - loss mean {losses.mean():.4f} min {losses.min():.4f} "
              f"max {losses.max():.4f}", flush=True)
    os.makedirs(ns.out, exist_ok=True)
    index, used = {}, set()
    for i in range(M):
        name = model_name(members, i, used)
        path = os.path.join(ns.out, name + ".h5")
        am = Autoencoder(input_dim=spec.input_dim, device="cpu")
        am.compile(learning_rate=ns.lr)   # the saved training_config records the rate actually used
        am.set_weights(fleet.get_weights(i))
        am.save(path, include_optimizer=False)
        index[name] = {"file": os.path.basename(path), "keys": [str(k) for k in members[i]],
                       "loss": ms[i]["loss"] if ms else None}
    with open(os.path.join(ns.out, "index.json"), "w") as f:
        json.dump(index, f, indent=1)
    print(f"wrote {M} models to {ns.out}", flush=True)
    return 0
