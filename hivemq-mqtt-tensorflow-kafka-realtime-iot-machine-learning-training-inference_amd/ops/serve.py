"""Persistent per-event scoring on the GPU (``csrc/kernels/ae_serve.hip``, ``dense_serve.hip``,
``dense_serve_fleet.hip``, ``lstm_serve.hip``, ``lstm_serve_wide.hip``).

``ScoringServer(model)`` keeps one wave resident on the device that polls a
host-mapped request ring; ``score(rows)`` publishes rows and spins on the
completion counter -- no kernel launch, no hipMemcpy per event.  This is the
low-latency path of BASELINE config 5 (the launch-per-event path is
``Autoencoder.score``).  The kernel exits by itself after ``idle_seconds``
without requests and is relaunched transparently on the next request.

``DenseScoringServer(model)`` has the same surface for Dense stacks of any depth (1..8 layers
up to 512 wide: an ``nn.Sequential`` / ``nn.Model`` or an ``Autoencoder``) on a resident
1024-thread workgroup that serves up to 8 events of a backlog per pass.

``DenseFleetScoringServer(models)`` serves M such stacks of one shape from ONE resident workgroup
(``dense_serve_fleet.hip``): every row names the member that scores it -- one model per car, as
``ops.dense_fleet.DenseFleet`` / ``fleet --layers`` train them.

``LSTMScoringServer(model)`` serves an :class:`~streamml.models.lstm.LSTMPredictor` the
same way, per car key: the device keeps each key's last ``look_back`` normalised events
and its latest forecast; every event is scored against the key's previous forecast (MSE)
and a forecast of the key's next event is returned (the reference's per-event LSTM
prediction stream, LSTM-TensorFlow-IO-Kafka/cardata-v2.py:220-273).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ._ext import load_c


class _Server:
    """What the scoring servers share: the life of the native server ``_s`` (``close`` tolerates an
    object whose construction failed before ``_s`` was set) and the columns of a latency run."""

    @staticmethod
    def _latency_columns(out, device_breakdown: bool):
        if device_breakdown:   # (host round trip, device total, device row-load, device compute)
            return out[:, 0], out[:, 1], out[:, 2], out[:, 3]
        return out[:, 0]

    @property
    def launches(self) -> int:
        return int(self._s.launches)

    def close(self) -> None:
        if getattr(self, "_s", None) is not None:
            self._s.stop()
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DenseServer(_Server):
    """The counters both Dense scorers read from their kernel's stats word."""

    @property
    def kernel(self) -> str:
        """Where the resident kernel reads the weights: "lds" | "stream", or "fleet" (always, for a
        fleet: the images stay in device memory)."""
        return str(self._s.kernel)

    @property
    def passes(self) -> int:
        """Passes the kernel ran since construction (one pass serves 1 .. ``MAX_PASS`` events)."""
        return int(self._s.passes)

    @property
    def events(self) -> int:
        """Events those passes served."""
        return int(self._s.events)


def _resolve_normalizer(normalizer, D: int, model, what: str):
    """(scale, shift) as fp32 ``[D]`` arrays, or (None, None): ``normalizer`` is None (``model``'s own,
    if it has one), ``"cardata"``, ``"none"`` or a ``(scale, shift)`` pair.  ``what``: "the model has"
    / "the models have", for the message."""
    sc = sh = None
    if normalizer is None:
        if hasattr(model, "_normalizer"):   # an Autoencoder's own input normaliser
            sc, sh = model._normalizer()
    elif isinstance(normalizer, str) and normalizer == "cardata":
        from ..data.cardata import normalize_affine
        if D != 18:
            raise ValueError(f"the cardata normaliser needs 18 features ({what} {D})")
        sc, sh = normalize_affine()
    elif not (isinstance(normalizer, str) and normalizer == "none"):
        if isinstance(normalizer, str) or len(normalizer) != 2:
            raise ValueError(f"unknown normalizer {normalizer!r}")
        sc, sh = normalizer
    if sc is not None:
        sc, sh = np.asarray(sc, np.float32).reshape(-1), np.asarray(sh, np.float32).reshape(-1)
        if sc.size != D or sh.size != D:
            raise ValueError(f"normalizer scale / shift must have {D} entries")
    return sc, sh


class ScoringServer(_Server):
    def __init__(self, model, threshold: float = 5.0, slots: int = 4096, idle_seconds: float = 2.0,
                 device: Optional[torch.device] = None):
        dev = torch.device(device) if device is not None else model.device
        if dev.type != "cuda":
            raise RuntimeError("ScoringServer needs a ROCm device (use Autoencoder.score on CPU)")
        spec = model.spec
        ws = model.get_weights()
        flat = np.concatenate([np.asarray(w, np.float32).ravel() for w in ws])
        sc, sh = model._normalizer()
        self.D = spec.input_dim
        self.threshold = float(threshold)
        self._s = load_c().AEServe(dev.index if dev.index is not None else torch.cuda.current_device(), int(slots),
                                   flat, [spec.input_dim, spec.encoding_dim, spec.hidden_dim], list(spec.act_codes),
                                   None if sc is None else np.asarray(sc, np.float32),
                                   None if sh is None else np.asarray(sh, np.float32), float(threshold),
                                   float(idle_seconds))

    def score(self, rows) -> Tuple[np.ndarray, np.ndarray]:
        """(scores [k], anomaly flags [k]) for raw rows [k, D]."""
        s, f, _ = self._s.infer(np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, self.D)), False, 10.0)
        return s, f.astype(bool)

    def infer(self, rows) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(scores, flags, reconstructions [k, D])."""
        s, f, r = self._s.infer(np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, self.D)), True, 10.0)
        return s, f.astype(bool), r

    def latency_us(self, rows, qps: float = 10000.0, device_breakdown: bool = False):
        """Per-event latency (us) of rows submitted one at a time at ``qps`` (C++ timing loop);
        with ``device_breakdown`` also the on-device processing time of each event (us)."""
        gap = int(1e9 / qps) if qps > 0 else 0
        out = self._s.latency_run(np.ascontiguousarray(np.asarray(rows, np.float32)), gap) / 1e3
        return self._latency_columns(out, device_breakdown)


def dense_layer_table(model) -> Tuple[list, list]:
    """(layers, weights) of a Dense stack: ``layers`` is a list of ``(in, units, activation name,
    use_bias)``, ``weights`` the matching list of ``(W [in, units], b [units] or None)`` fp32 arrays.

    Accepts an ``nn.Model`` / ``nn.Sequential`` made of ``InputLayer``, ``Dense`` and ``Dropout``
    (identity at inference) over a 1-D input, or a ``models.Autoencoder`` (its four Dense layers).
    Raises ``ValueError`` naming the layer it cannot take."""
    if hasattr(model, "spec") and hasattr(model.spec, "layer_sizes"):
        ws = [np.asarray(w, np.float32) for w in model.get_weights()]
        layers = [(int(i), int(o), a or "linear", True) for (i, o), a in zip(model.spec.layer_sizes,
                                                                             model.spec.activations)]
        return layers, [(ws[2 * k], ws[2 * k + 1]) for k in range(len(layers))]
    from ..nn.layers import Dense, Dropout, InputLayer
    if not hasattr(model, "layers") or not hasattr(model, "_input_shape"):
        raise ValueError(f"expected an nn.Model of Dense layers or an Autoencoder, got {type(model).__name__}")
    for lyr in model.layers:
        if not isinstance(lyr, (InputLayer, Dense, Dropout)):
            raise ValueError(f"only Dense (and InputLayer / Dropout) layers are served, found {lyr.class_name}")
    shape = tuple(model._input_shape())
    if len(shape) != 1:
        raise ValueError(f"the input must be one row of features, not shape {shape}")
    arrays = [np.asarray(a, np.float32) for a in model.get_weights()]
    dim, layers, weights = int(shape[0]), [], []
    for lyr in model.layers:
        if not isinstance(lyr, Dense):
            continue
        W = arrays[lyr.param_slots[0]]
        b = arrays[lyr.param_slots[1]] if lyr.use_bias else None
        layers.append((dim, int(lyr.units), lyr.activation or "linear", bool(lyr.use_bias)))
        weights.append((W, b))
        dim = int(lyr.units)
    return layers, weights


DENSE_SERVE_TILE = 32   # output widths are zero-padded to this, input widths to 4


def _dense_image_floats(layers) -> int:
    """Floats of the packed image of ``layers``: per layer ``Kp * Np`` weights and ``Np`` biases."""
    t = DENSE_SERVE_TILE
    return sum(((i + 3) // 4 * 4 + 1) * ((o + t - 1) // t * t) for i, o, _, _ in layers)


def dense_serve_image(layers, weights) -> Tuple[np.ndarray, list]:
    """Pack the weight image of ``dense_serve.hip``: per layer ``float4 img[Kp / 4][Np]`` with
    ``img[g][o] = W[4g .. 4g + 3][o]`` (``Kp`` = in rounded up to 4, ``Np`` = units rounded up to
    32, zero-padded), then the padded bias ``[Np]`` (zeros for a layer without bias).  Returns
    (fp32 image, table of ``(in, units, activation code, w_off, b_off)``, offsets in floats)."""
    from .dense import ACT
    parts, table, off = [], [], 0
    for (n_in, n_out, act, _), (W, b) in zip(layers, weights):
        W = np.asarray(W, np.float32)
        if W.shape != (n_in, n_out):
            raise ValueError(f"kernel of shape {W.shape} for a {n_in} -> {n_out} layer")
        kp, npad = (n_in + 3) // 4 * 4, (n_out + DENSE_SERVE_TILE - 1) // DENSE_SERVE_TILE * DENSE_SERVE_TILE
        wp = np.zeros((kp, npad), np.float32)
        wp[:n_in, :n_out] = W
        bp = np.zeros(npad, np.float32)
        if b is not None:
            bp[:n_out] = np.asarray(b, np.float32).reshape(n_out)
        # [Kp, Np] -> [Kp / 4][Np][4]: 16 bytes hold rows 4g .. 4g + 3 of one column
        parts += [wp.reshape(kp // 4, 4, npad).transpose(0, 2, 1).ravel(), bp]
        table.append((n_in, n_out, ACT[act], off, off + kp * npad))
        off += kp * npad + npad
    image = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    return np.ascontiguousarray(image, np.float32), table


class DenseScoringServer(_DenseServer):
    """Persistent per-event scorer for a Dense stack of any depth (``dense_serve.hip``): 1 ..
    ``MAX_LAYERS`` Dense layers, every width up to ``MAX_WIDTH``, rows of up to ``MAX_FEATURES``
    features, the last layer one unit per feature.  Same surface and semantics as
    :class:`ScoringServer` (``xn = x * scale + shift``, ``score = mean((y - xn)^2)``, fp32).

    One resident workgroup serves up to ``MAX_PASS`` events per pass; an event's result bits do
    not depend on how the ring batched it.  ``kernel`` is ``"lds"`` when the packed weights fit
    the CU's LDS (``LDS_IMAGE_BYTES``), else ``"stream"``; ``passes`` / ``events`` count what the
    kernel ran.  ``normalizer``: None, ``"cardata"`` (18 features) or a ``(scale, shift)`` pair;
    for an ``Autoencoder`` the default is the model's own."""

    MAX_WIDTH = 512
    MAX_FEATURES = 32    # a request slot holds 32 words
    MAX_LAYERS = 8
    MAX_PASS = 8
    LDS_IMAGE_BYTES = 92 * 1024
    ACTIVATIONS = ("linear", "relu", "tanh", "sigmoid")

    @staticmethod
    def supports(model) -> Tuple[bool, str]:
        """(True, "") if the scorer can serve ``model``, else (False, the limit it exceeds).
        Mirrors the checks of ``DenseServe``'s constructor; needs no device."""
        S = DenseScoringServer
        try:
            layers, _ = dense_layer_table(model)
        except ValueError as e:
            return False, str(e)
        if not 1 <= len(layers) <= S.MAX_LAYERS:
            return False, f"the stack must have 1..{S.MAX_LAYERS} Dense layers (it has {len(layers)})"
        D = layers[0][0]
        if not 1 <= D <= S.MAX_FEATURES:
            return False, f"rows must have 1..{S.MAX_FEATURES} features (a request slot holds 32 words; it has {D})"
        for n_in, n_out, act, _ in layers:
            if not 1 <= n_out <= S.MAX_WIDTH:
                return False, f"Dense layers must have 1..{S.MAX_WIDTH} units (one has {n_out})"
            if act not in S.ACTIVATIONS:
                return False, f"activations must be linear, relu, tanh or sigmoid (found {act})"
        if layers[-1][1] != D:
            return False, f"the last layer must have one unit per feature ({layers[-1][1]} units, {D} features)"
        return True, ""

    @staticmethod
    def kernel_for(model) -> str:
        """"lds" | "stream": where the resident kernel will keep the weights of ``model``."""
        layers, _ = dense_layer_table(model)
        return "lds" if 4 * _dense_image_floats(layers) <= DenseScoringServer.LDS_IMAGE_BYTES else "stream"

    def __init__(self, model, threshold: float = 5.0, slots: int = 4096, idle_seconds: float = 2.0,
                 normalizer=None, device: Optional[torch.device] = None):
        dev = torch.device(device) if device is not None else model.device
        if dev.type != "cuda":
            raise RuntimeError("DenseScoringServer needs a ROCm device (use model.predict on CPU)")
        ok, why = self.supports(model)
        if not ok:
            raise ValueError(f"DenseScoringServer cannot serve this model: {why}")
        layers, weights = dense_layer_table(model)
        image, table = dense_serve_image(layers, weights)
        self.D = int(layers[0][0])
        sc, sh = _resolve_normalizer(normalizer, self.D, model, "the model has")
        self.threshold = float(threshold)
        C = load_c()
        assert (C.DSV_MAXW, C.DSV_MAXLAYERS, C.DSV_EB, C.DSV_LDS_IMAGE_BYTES) == (
            self.MAX_WIDTH, self.MAX_LAYERS, self.MAX_PASS, self.LDS_IMAGE_BYTES)
        self._s = C.DenseServe(dev.index if dev.index is not None else torch.cuda.current_device(), int(slots),
                               image, [list(t) for t in table], self.D, sc, sh, float(threshold),
                               float(idle_seconds))

    def score(self, rows) -> Tuple[np.ndarray, np.ndarray]:
        """(scores [k], anomaly flags [k]) for raw rows [k, D]."""
        s, f, _ = self._s.infer(np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, self.D)), False, 10.0)
        return s, f.astype(bool)

    def infer(self, rows) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(scores, flags, reconstructions [k, D])."""
        s, f, r = self._s.infer(np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, self.D)), True, 10.0)
        return s, f.astype(bool), r

    def latency_us(self, rows, qps: float = 10000.0, device_breakdown: bool = False):
        """Per-event latency (us) of rows submitted one at a time at ``qps`` (C++ timing loop);
        with ``device_breakdown`` also the on-device processing time of each event (us)."""
        gap = int(1e9 / qps) if qps > 0 else 0
        out = self._s.latency_run(np.ascontiguousarray(np.asarray(rows, np.float32)), gap) / 1e3
        return self._latency_columns(out, device_breakdown)


def _dense_flat_offsets(layers) -> list:
    """(w_off, b_off) of each layer in a flat parameter vector that holds every kernel ``[in, units]``
    followed by its bias (layers without a bias have none), one layer after the other."""
    offs, off = [], 0
    for n_in, n_out, _, use_bias in layers:
        offs.append((off, off + n_in * n_out))
        off += n_in * n_out + (n_out if use_bias else 0)
    return offs


def dense_fleet_serve_images(layers, flats_or_weight_lists, offsets=None) -> Tuple[np.ndarray, list]:
    """Pack the stacked weight images of ``dense_serve_fleet.hip`` for M models of ONE layer table:
    ``images [M, stride]`` fp32 whose row i equals ``dense_serve_image(layers, weights_i)[0]``,
    zero-padded to ``stride`` (the image's length rounded up to 4 floats), and the one table of
    ``(in, units, activation code, w_off, b_off)`` with offsets relative to a model's image.

    ``flats_or_weight_lists``: a ``[M, n]`` array of flat parameters (layer k's kernel at
    ``offsets[k][0]``, its bias at ``offsets[k][1]``; default: kernels and biases one after the
    other, as ``FlatParams.flat`` and ``DenseFleet.flat`` hold them), or a sequence of M weight
    lists as ``dense_layer_table`` returns them.  The packing is numpy over the model axis."""
    from .dense import ACT
    layers = list(layers)
    if isinstance(flats_or_weight_lists, np.ndarray):
        flats = np.asarray(flats_or_weight_lists, np.float32)
        if flats.ndim != 2:
            raise ValueError("flat parameters must be [M, n]")
    else:
        if offsets is not None:
            raise ValueError("offsets go with flat parameters")
        rows = []
        for weights in flats_or_weight_lists:   # gathers M separate objects; the packing below has no such loop
            parts = []
            for (n_in, n_out, _, use_bias), (W, b) in zip(layers, weights):
                W = np.asarray(W, np.float32)
                if W.shape != (n_in, n_out):
                    raise ValueError(f"kernel of shape {W.shape} for a {n_in} -> {n_out} layer")
                parts.append(W.ravel())
                if use_bias:
                    parts.append(np.asarray(b, np.float32).reshape(n_out))
            rows.append(np.concatenate(parts))
        flats = np.stack(rows) if rows else np.zeros((0, 0), np.float32)
    offsets = _dense_flat_offsets(layers) if offsets is None else list(offsets)
    M, t = flats.shape[0], DENSE_SERVE_TILE
    geo = [((i + 3) // 4 * 4, (o + t - 1) // t * t) for i, o, _, _ in layers]
    img_floats = _dense_image_floats(layers)
    stride = (img_floats + 3) // 4 * 4
    images = np.zeros((M, stride), np.float32)
    table, off = [], 0
    for (n_in, n_out, act, use_bias), (kp, npad), (w_off, b_off) in zip(layers, geo, offsets):
        if w_off + n_in * n_out > flats.shape[1] or (use_bias and b_off + n_out > flats.shape[1]):
            raise ValueError("a layer's parameters lie outside the flat vector")
        wp = np.zeros((M, kp, npad), np.float32)
        wp[:, :n_in, :n_out] = flats[:, w_off:w_off + n_in * n_out].reshape(M, n_in, n_out)
        # [M, Kp, Np] -> [M][Kp / 4][Np][4]: 16 bytes hold rows 4g .. 4g + 3 of one column
        images[:, off:off + kp * npad] = wp.reshape(M, kp // 4, 4, npad).transpose(0, 1, 3, 2).reshape(M, kp * npad)
        if use_bias:
            images[:, off + kp * npad:off + kp * npad + n_out] = flats[:, b_off:b_off + n_out]
        table.append((n_in, n_out, ACT[act], off, off + kp * npad))
        off += kp * npad + npad
    return images, table


class DenseFleetScoringServer(_DenseServer):
    """Persistent per-event scorer for a FLEET of Dense stacks of one shape (``dense_serve_fleet.hip``):
    every row names the member that scores it, ``score(rows, models)``.  One resident workgroup holds
    the whole fleet: the members' weight images are stacked in device memory and each event reads its
    own; an event's result bits are those :class:`DenseScoringServer` gives for that member alone.

    ``models``: a sequence of ``nn`` models (or ``Autoencoder``) whose ``dense_layer_table(...)[0]`` are
    equal.  ``thresholds``: one number or one per member (``flag = score > thresholds[model]``).
    ``normalizer``: None, ``"cardata"`` or a ``(scale, shift)`` pair, ONE for the whole fleet, the way
    the fleet trainer normalises.  Limits as :class:`DenseScoringServer`, but rows have at most
    ``MAX_FEATURES`` = 31 features: request word 31 carries the model index."""

    MAX_WIDTH = DenseScoringServer.MAX_WIDTH
    MAX_FEATURES = 31    # request word 31 carries the model index
    MAX_LAYERS = DenseScoringServer.MAX_LAYERS
    MAX_PASS = DenseScoringServer.MAX_PASS
    MAX_MODELS = (1 << 24) - 1
    ACTIVATIONS = DenseScoringServer.ACTIVATIONS

    @staticmethod
    def supports(model, n_models: int = 1) -> Tuple[bool, str]:
        """(True, "") if a fleet of ``n_models`` members shaped like ``model`` can be served, else
        (False, the limit it exceeds).  ``model`` may be a sequence of members: then their layer
        tables must be equal.  Mirrors ``dense_fleet_serve_check``; needs no device."""
        S = DenseFleetScoringServer
        members = list(model) if isinstance(model, (list, tuple)) else [model]
        if not members:
            return False, "a fleet must have 1..16777215 models (it has 0)"
        try:
            layers, _ = dense_layer_table(members[0])
        except ValueError as e:
            return False, str(e)
        D = layers[0][0] if layers else 0
        if layers and not 1 <= D <= S.MAX_FEATURES:
            return False, (f"rows must have 1..{S.MAX_FEATURES} features (request word 31 carries the model index); "
                           f"it has {D}")
        ok, why = DenseScoringServer.supports(members[0])
        if not ok:
            return False, why
        why = S.first_difference(members)
        if why:
            return False, why
        if not 1 <= int(n_models) <= S.MAX_MODELS:
            return False, f"a fleet must have 1..{S.MAX_MODELS} models (it has {int(n_models)})"
        return True, ""

    @staticmethod
    def first_difference(models) -> str:
        """Empty if the members share one layer table, else the first model and layer that differ."""
        ref, _ = dense_layer_table(models[0])
        for i, mdl in enumerate(models[1:], start=1):
            try:
                layers, _ = dense_layer_table(mdl)
            except ValueError as e:
                return f"model {i}: {e}"
            if len(layers) != len(ref):
                return f"model {i} has {len(layers)} Dense layers, model 0 has {len(ref)}"
            for l, (a, b) in enumerate(zip(ref, layers)):
                if a != b:
                    return (f"model {i} differs from model 0 in layer {l}: (in, units, activation, use_bias) = "
                            f"{b} != {a}")
        return ""

    def __init__(self, models, thresholds=5.0, slots: int = 4096, idle_seconds: float = 2.0, normalizer=None,
                 device: Optional[torch.device] = None):
        models = list(models)
        if not models:
            raise ValueError("a fleet needs at least one model")
        ok, why = self.supports(models, len(models))
        if not ok:
            raise ValueError(f"DenseFleetScoringServer cannot serve this fleet: {why}")
        layers, _ = dense_layer_table(models[0])
        images, table = dense_fleet_serve_images(layers, [dense_layer_table(m)[1] for m in models])
        dev = device if device is not None else models[0].device
        self._open(layers, images, table, thresholds, slots, idle_seconds, normalizer, dev)

    def _open(self, layers, images, table, thresholds, slots, idle_seconds, normalizer, device) -> None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("DenseFleetScoringServer needs a ROCm device (use model.predict on CPU)")
        self.layers = list(layers)
        self.D = int(layers[0][0])
        M = int(images.shape[0])
        thr = np.asarray(thresholds, np.float32)
        thr = np.full(M, float(thr), np.float32) if thr.ndim == 0 else np.ascontiguousarray(thr.reshape(-1))
        if thr.shape != (M,):
            raise ValueError(f"thresholds must be one number or [{M}], one per model")
        self.thresholds = thr
        sc, sh = _resolve_normalizer(normalizer, self.D, None, "the models have")
        C = load_c()
        assert (C.DSV_FLEET_MAXD, C.DSV_FLEET_MAXMODELS - 1) == (self.MAX_FEATURES, self.MAX_MODELS)
        self._s = C.DenseFleetServe(dev.index if dev.index is not None else torch.cuda.current_device(), int(slots),
                                    np.ascontiguousarray(images, np.float32), _dense_image_floats(layers),
                                    [list(r) for r in table], self.D, sc, sh, thr, float(idle_seconds))

    @classmethod
    def from_fleet(cls, fleet, **kw) -> "DenseFleetScoringServer":
        """Serve a :class:`~streamml.ops.dense_fleet.DenseFleet` as it stands: ``fleet.flat`` is read once."""
        self = cls.__new__(cls)
        layers, images, table = cls._fleet_images(fleet)
        ok, why = cls.supports(fleet._template, fleet.n_models)
        if not ok:
            raise ValueError(f"DenseFleetScoringServer cannot serve this fleet: {why}")
        self._open(layers, images, table, kw.pop("thresholds", 5.0), kw.pop("slots", 4096),
                   kw.pop("idle_seconds", 2.0), kw.pop("normalizer", None), kw.pop("device", fleet.device))
        if kw:
            raise TypeError(f"unexpected arguments {sorted(kw)}")
        return self

    @classmethod
    def from_flats(cls, layers, flats, offsets=None, thresholds=5.0, slots: int = 4096, idle_seconds: float = 2.0,
                   normalizer=None, device=None) -> "DenseFleetScoringServer":
        """Serve M members given as flat parameter vectors ``flats [M, n]`` of the layer table ``layers``
        (``dense_layer_table(model)[0]``), without building M model objects; ``offsets`` as in
        :func:`dense_fleet_serve_images`."""
        self = cls.__new__(cls)
        images, table = dense_fleet_serve_images(layers, np.asarray(flats, np.float32), offsets=offsets)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self._open(list(layers), images, table, thresholds, slots, idle_seconds, normalizer, device)
        return self

    @staticmethod
    def _fleet_images(fleet):
        layers, _ = dense_layer_table(fleet._template)
        offsets = [(int(r[6]), int(r[7])) for r in fleet.table]   # (w_off, b_off) in a member's flat
        flats = fleet.flat.detach().cpu().numpy()                  # one device -> host copy
        images, table = dense_fleet_serve_images(layers, flats, offsets=offsets)
        return layers, images, table

    @classmethod
    def from_dir(cls, path, **kw) -> "DenseFleetScoringServer":
        """Serve the directory ``fleet --layers`` wrote: ``index.json`` names the members' files and
        the car keys each one owns.  ``names[i]`` is member i's name and ``key_to_model`` maps a car
        key to its member's index."""
        models, names, key_to_model = cls.load_dir(path)
        if kw.get("device", None) is None:
            kw["device"] = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self = cls(models, **kw)
        self.names, self.key_to_model = names, key_to_model
        return self

    @classmethod
    def load_dir(cls, path) -> Tuple[list, list, dict]:
        """What ``from_dir`` reads before it opens a device: (members as CPU models, names,
        key_to_model).  Raises ``ValueError`` for a directory without ``layers`` in its index or
        with members ``supports`` rejects."""
        names, files, key_to_model = read_fleet_index(path)
        from ..nn.model import load_model
        models = [load_model(f, device="cpu", compile=False) for f in files]
        ok, why = cls.supports(models, len(models))
        if not ok:
            raise ValueError(f"{path}: the persistent fleet scorer cannot serve these models: {why}")
        return models, names, key_to_model

    def _rows_models(self, rows, models):
        rows = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, self.D))
        idx = np.ascontiguousarray(np.asarray(models, np.int64).reshape(-1))
        if idx.size != rows.shape[0]:
            raise ValueError(f"{idx.size} model indices for {rows.shape[0]} rows")
        return rows, idx

    def score(self, rows, models) -> Tuple[np.ndarray, np.ndarray]:
        """(scores [k], anomaly flags [k]) for raw rows [k, D], row i scored by member ``models[i]``.
        An index outside ``[0, n_models)`` raises ``ValueError`` before anything is published."""
        rows, idx = self._rows_models(rows, models)
        s, f, _ = self._s.infer_models(rows, idx, False, 10.0)
        return s, f.astype(bool)

    def infer(self, rows, models) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(scores, flags, reconstructions [k, D])."""
        rows, idx = self._rows_models(rows, models)
        s, f, r = self._s.infer_models(rows, idx, True, 10.0)
        return s, f.astype(bool), r

    def latency_us(self, rows, models, qps: float = 10000.0, device_breakdown: bool = False):
        """Per-event latency (us) of rows submitted one at a time at ``qps`` (C++ timing loop);
        with ``device_breakdown`` also the on-device processing time of each event (us)."""
        rows, idx = self._rows_models(rows, models)
        gap = int(1e9 / qps) if qps > 0 else 0
        out = self._s.latency_models(rows, gap, idx) / 1e3
        return self._latency_columns(out, device_breakdown)

    def set_weights(self, i: int, weights) -> None:
        """Replace member i's weights (a Keras-order list as ``model.get_weights()`` gives, or the
        ``(W, b)`` pairs of ``dense_layer_table``): the resident kernel is stopped, the image copied,
        and the next call relaunches it."""
        weights = list(weights)
        if weights and not isinstance(weights[0], (tuple, list)):
            it, pairs = iter(weights), []
            for _, _, _, use_bias in self.layers:
                W = next(it)
                pairs.append((W, next(it) if use_bias else None))
            weights = pairs
        images, _ = dense_fleet_serve_images(self.layers, [weights])
        if not 0 <= int(i) < self.n_models:
            raise ValueError(f"model index {int(i)} is outside [0, {self.n_models})")
        self._s.set_image(int(i), images[0])

    def refresh(self, fleet) -> None:
        """Take every member's weights from ``fleet`` again (after further training)."""
        layers, images, _ = self._fleet_images(fleet)
        if list(layers) != self.layers or images.shape[0] != self.n_models:
            raise ValueError("the fleet's shape differs from the one being served")
        self._s.set_images(images)

    @property
    def n_models(self) -> int:
        return int(self._s.n_models)

    @property
    def stride(self) -> int:
        """Floats between two members' weight images in device memory."""
        return int(self._s.stride)


def read_fleet_index(path) -> Tuple[list, list, dict]:
    """(names, files, key_to_model) of a ``fleet --layers`` directory: the members in ``index.json``'s
    order (its ``INDEX_META`` keys skipped), their ``.h5`` paths and car key -> member index.
    Raises ``ValueError`` for a directory the Dense fleet trainer did not write."""
    import json
    import os
    from ..cli.fleet import INDEX_META
    idx_path = os.path.join(str(path), "index.json")
    if not os.path.isfile(idx_path):
        raise ValueError(f"{path}: no index.json (expected the output directory of fleet --layers)")
    with open(idx_path) as f:
        index = json.load(f)
    if "layers" not in index:
        raise ValueError(f"{path}: index.json has no 'layers' (the directory was not written by fleet --layers)")
    names = [n for n in index if n not in INDEX_META]
    if not names:
        raise ValueError(f"{path}: index.json names no model")
    files = [os.path.join(str(path), index[n]["file"]) for n in names]
    key_to_model = {}
    for i, n in enumerate(names):
        for k in index[n].get("keys", []):
            key_to_model[str(k)] = i
    return names, files, key_to_model


def lstm_layer_table(model) -> Tuple[np.ndarray, list]:
    """(flat weights in Keras order, LstmServeLayer tuples) of an LSTMPredictor."""
    from .lstm import ACT
    arrays = [np.asarray(a, np.float32) for a in model.fp.get()]
    offs = np.cumsum([0] + [a.size for a in arrays])
    flat = np.concatenate([a.ravel() for a in arrays]) if arrays else np.zeros(0, np.float32)
    table = []
    for L in model.layers:
        if L["kind"] == "lstm":
            p = L["params"]
            table.append((0, L["in_dim"], L["units"], ACT[L["activation"]], int(L["return_sequences"]), 0,
                          int(offs[p]), int(offs[p + 1]), int(offs[p + 2])))
        elif L["kind"] == "repeat":
            table.append((1, 0, 0, 0, 0, int(L["n"]), 0, 0, 0))
        else:
            p = L["params"]
            table.append((2, L["in_dim"], L["units"], 0, 0, 0, int(offs[p]), 0, int(offs[p + 1])))
    return flat, table


class LSTMScoringServer(_Server):
    """Persistent per-event LSTM forecaster; ``nkeys`` car keys (ids in [0, nkeys)).

    Stacks whose layers are at most 32 wide run from LDS and registers (``kernel`` is
    ``"ref1"``, ``"pipe"`` or ``"generic"``, fp32 throughout); anything wider, up to
    ``MAX_WIDTH`` units or inputs per layer, runs on the streamed-weight kernel (``"wide"``:
    bf16 weight images, bf16-rounded x and h, fp32 everywhere else; widths zero-padded to
    ``WIDE_TILE``).

    ``lanes`` (wide stacks only, up to ``MAX_LANES``): that many resident workgroups, each a
    complete one-event-at-a-time server with ``slots`` request / result slots of its own; key
    ``k`` is served by lane ``k % lanes``, so a key's events stay in order on one lane and
    every result has the bits the one-lane server gives, while events of different lanes
    run side by side."""

    MAX_WIDTH = 512      # LSTM units, layer inputs, head inputs
    MAX_FEATURES = 31    # request word 31 carries the key
    MAX_LOOK_BACK = 64
    MAX_LAYERS = 8
    WIDE_TILE = 32       # the wide kernel pads every width to a multiple of this
    MAX_LANES = 32       # resident workgroups of the wide kernel (the device also caps it: half its CUs)

    @staticmethod
    def supports(model, lanes: int = 1) -> Tuple[bool, str]:
        """(True, "") if the forecaster can serve ``model`` on ``lanes`` lanes, else (False, the
        limit it exceeds).  Mirrors the checks of ``LSTMServe``'s constructor; needs no device."""
        S = LSTMScoringServer
        if not 1 <= int(lanes) <= S.MAX_LANES:
            return False, f"lanes must be 1..{S.MAX_LANES}"
        if not 1 <= int(model.features) <= S.MAX_FEATURES:
            return False, f"rows must have 1..{S.MAX_FEATURES} features (request word 31 carries the key)"
        if not 1 <= int(model.look_back) <= S.MAX_LOOK_BACK:
            return False, f"look_back must be 1..{S.MAX_LOOK_BACK}"
        layers = model.layers
        if not 1 <= len(layers) <= S.MAX_LAYERS:
            return False, f"1..{S.MAX_LAYERS} layers"
        lstms = [L for L in layers if L["kind"] == "lstm"]
        wide = (len(lstms) > 4 or any(L["units"] > 32 or L["in_dim"] > 32 for L in lstms)
                or any(L["kind"] == "dense" and L["in_dim"] > 32 for L in layers))
        for L in lstms:
            if not 1 <= L["units"] <= S.MAX_WIDTH:
                return False, f"LSTM layers must have 1..{S.MAX_WIDTH} units ({L['name']} has {L['units']})"
            if L["in_dim"] > S.MAX_WIDTH:
                return False, f"layer inputs must be 1..{S.MAX_WIDTH} wide ({L['name']} reads {L['in_dim']})"
        for i, L in enumerate(layers):
            if L["kind"] == "repeat" and not 1 <= L["n"] <= S.MAX_LOOK_BACK:
                return False, f"RepeatVector must repeat 1..{S.MAX_LOOK_BACK} times"
            if L["kind"] == "dense":
                if L["in_dim"] > S.MAX_WIDTH:
                    return False, f"the head's input must be 1..{S.MAX_WIDTH} wide"
                if wide and i != len(layers) - 1:
                    return False, "a stack with layers wider than 32 takes a Dense layer only as its head"
                if not wide and L["units"] > 32:
                    return False, "Dense layers must have 1..32 units"
        if not lstms:
            return False, "the stack needs an LSTM layer"
        if layers[-1]["kind"] != "dense" or layers[-1]["units"] != int(model.features):
            return False, "the stack must end in a Dense head with one output per feature"
        if int(lanes) > 1 and not wide:
            return False, "only the streamed-weight (wide) kernel runs on several lanes"
        return True, ""

    def __init__(self, model, nkeys: int = 100_000, threshold: float = 5.0, slots: int = 4096,
                 idle_seconds: float = 2.0, normalizer: Optional[str] = "cardata", device: Optional[torch.device] = None,
                 lanes: int = 1):
        dev = torch.device(device) if device is not None else model.device
        if dev.type != "cuda":
            raise RuntimeError("LSTMScoringServer needs a ROCm device (use LSTMPredictor.predict on CPU)")
        ok, why = self.supports(model, lanes=lanes)
        if not ok:
            raise ValueError(f"LSTMScoringServer cannot serve this model: {why}")
        flat, table = lstm_layer_table(model)
        sc = sh = None
        if normalizer == "cardata":
            from ..data.cardata import normalize_affine
            sc, sh = (np.asarray(a, np.float32) for a in normalize_affine())
        elif normalizer not in (None, "none"):
            raise ValueError(f"unknown normalizer {normalizer!r}")
        self.D, self.T, self.nkeys = int(model.features), int(model.look_back), int(nkeys)
        self.threshold = float(threshold)
        self._s = load_c().LSTMServe(dev.index if dev.index is not None else torch.cuda.current_device(), int(slots),
                                     flat, [list(t) for t in table], self.D, self.T, self.nkeys, sc, sh,
                                     float(threshold), float(idle_seconds), int(lanes))

    def forecast(self, rows, keys) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Events in order -> (forecast of each key's next event [k, D] (zeros until the key has
        ``look_back`` events), score vs the key's previous forecast [k] (NaN if none),
        flags [k]: 0 normal, 1 score > threshold, 2 no previous forecast)."""
        rows = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, self.D))
        keys = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(-1))
        s, f, r = self._s.infer(rows, True, 10.0, keys)
        return r, s, f

    def latency_us(self, rows, keys, qps: float = 10000.0, device_breakdown: bool = False):
        gap = int(1e9 / qps) if qps > 0 else 0
        out = self._s.latency_run(np.ascontiguousarray(np.asarray(rows, np.float32)), gap,
                                  np.ascontiguousarray(np.asarray(keys, np.int64))) / 1e3
        # device phases of the last run: pick-up -> key state and window gathered ("load"),
        # then the stack over the window ("compute")
        self.last_device_load_us = out[:, 2]
        if device_breakdown:
            return out[:, 0], out[:, 1], out[:, 3]
        return out[:, 0]

    def reset(self) -> None:
        """Forget every key's window and forecast."""
        self._s.reset_keys()

    @property
    def lanes(self) -> int:
        return int(self._s.lanes)

    @property
    def slots(self) -> int:
        """Request / result slots of each lane."""
        return int(self._s.nslots)

    @property
    def lane_events(self) -> np.ndarray:
        """int64 [lanes]: events each lane completed since construction or the last ``reset()``
        (read from the lanes' completion counters)."""
        return np.asarray(self._s.lane_events, np.int64)

    @property
    def kernel(self) -> str:
        """The resident kernel chosen for this stack: "ref1" | "pipe" | "generic" | "wide"."""
        return str(self._s.kernel)
