"""Persistent per-event scoring on the GPU (``csrc/kernels/ae_serve.hip``, ``dense_serve.hip``,
``lstm_serve.hip``, ``lstm_serve_wide.hip``).

``ScoringServer(model)`` keeps one wave resident on the device that polls a
host-mapped request ring; ``score(rows)`` publishes rows and spins on the
completion counter -- no kernel launch, no hipMemcpy per event.  This is the
low-latency path of BASELINE config 5 (the launch-per-event path is
``Autoencoder.score``).  The kernel exits by itself after ``idle_seconds``
without requests and is relaunched transparently on the next request.

``DenseScoringServer(model)`` has the same surface for Dense stacks of any depth (1..8 layers
up to 512 wide: an ``nn.Sequential`` / ``nn.Model`` or an ``Autoencoder``) on a resident
1024-thread workgroup that serves up to 8 events of a backlog per pass.

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


class ScoringServer:
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
        if device_breakdown:   # (host round trip, device total, device row-load, device compute)
            return out[:, 0], out[:, 1], out[:, 2], out[:, 3]
        return out[:, 0]

    @property
    def launches(self) -> int:
        return int(self._s.launches)

    def close(self) -> None:
        if self._s is not None:
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


class DenseScoringServer:
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
        t = DENSE_SERVE_TILE
        nbytes = sum(4 * (((i + 3) // 4 * 4) * ((o + t - 1) // t * t) + (o + t - 1) // t * t) for i, o, _, _ in layers)
        return "lds" if nbytes <= DenseScoringServer.LDS_IMAGE_BYTES else "stream"

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
        sc = sh = None
        if normalizer is None:
            if hasattr(model, "_normalizer"):   # an Autoencoder's own input normaliser
                sc, sh = model._normalizer()
        elif isinstance(normalizer, str) and normalizer == "cardata":
            from ..data.cardata import normalize_affine
            if self.D != 18:
                raise ValueError(f"the cardata normaliser needs 18 features (the model has {self.D})")
            sc, sh = normalize_affine()
        elif not (isinstance(normalizer, str) and normalizer == "none"):
            if isinstance(normalizer, str) or len(normalizer) != 2:
                raise ValueError(f"unknown normalizer {normalizer!r}")
            sc, sh = normalizer
        if sc is not None:
            sc, sh = np.asarray(sc, np.float32).reshape(-1), np.asarray(sh, np.float32).reshape(-1)
            if sc.size != self.D or sh.size != self.D:
                raise ValueError(f"normalizer scale / shift must have {self.D} entries")
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
        if device_breakdown:   # (host round trip, device total, device row-load, device compute)
            return out[:, 0], out[:, 1], out[:, 2], out[:, 3]
        return out[:, 0]

    @property
    def kernel(self) -> str:
        """Where the resident kernel keeps the weight image: "lds" | "stream"."""
        return str(self._s.kernel)

    @property
    def passes(self) -> int:
        """Passes the kernel ran since construction (one pass serves 1 .. ``MAX_PASS`` events)."""
        return int(self._s.passes)

    @property
    def events(self) -> int:
        """Events those passes served."""
        return int(self._s.events)

    @property
    def launches(self) -> int:
        return int(self._s.launches)

    def close(self) -> None:
        if self._s is not None:
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


class LSTMScoringServer:
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

    @property
    def launches(self) -> int:
        return int(self._s.launches)

    def close(self) -> None:
        if self._s is not None:
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
