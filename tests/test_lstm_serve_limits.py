"""Limits of the per-event LSTM forecaster, checked without a device:
``LSTMScoringServer.supports`` and the engine ``cardata-lstm ... predict`` picks under
``--predict-engine auto``."""
import types

import numpy as np
import pytest
import torch

from streamml.models.lstm import LSTMPredictor
from streamml.ops.serve import LSTMScoringServer


def _model(stack, look_back=3, features=18):
    return LSTMPredictor(look_back=look_back, features=features, stack=stack, device="cpu", seed=1)


@pytest.mark.parametrize("u", [1, 32, 33, 512])
def test_supports_every_width_up_to_512(u):
    assert LSTMScoringServer.supports(_model([("lstm", u, False, "tanh"), ("dense", 18, False)])) == (True, "")


def test_supports_wide_inputs_and_the_reference_stacks():
    ok, why = LSTMScoringServer.supports(_model([("lstm", 512, True, "tanh"), ("lstm", 512, False, "relu"),
                                                 ("dense", 18, False)]))   # layer and head inputs of 512
    assert ok, why
    assert LSTMScoringServer.supports(LSTMPredictor.reference(look_back=1, device="cpu"))[0]
    assert LSTMScoringServer.supports(LSTMPredictor.two_layer(look_back=50, device="cpu"))[0]
    assert LSTMScoringServer.supports(_model([("lstm", 8, False, "relu"), ("dense", 18, False)], look_back=64))[0]
    assert LSTMScoringServer.supports(_model([("lstm", 8, False, "relu"), ("dense", 31, False)], features=31))[0]


@pytest.mark.parametrize("build,word", [
    (lambda: _model([("lstm", 513, False, "tanh"), ("dense", 18, False)]), "512"),
    (lambda: _model([("lstm", 16, False, "tanh"), ("dense", 18, False)], look_back=65), "64"),
    (lambda: _model([("lstm", 16, False, "tanh"), ("dense", 32, False)], features=32), "31"),
    (lambda: _model([("lstm", 8, True, "tanh")] * 8 + [("dense", 18, True)]), "8 layers"),
], ids=["u513", "look_back65", "D32", "nine_layers"])
def test_supports_names_the_limit(build, word):
    ok, why = LSTMScoringServer.supports(build())
    assert not ok and word in why, why


class _OnDevice:
    """A CPU model that claims a ROCm device: what ``_predict`` sees on a GPU machine."""

    def __init__(self, model):
        self._m = model
        self.device = torch.device("cuda", 0)

    def __getattr__(self, name):
        return getattr(self._m, name)


def _run_predict(monkeypatch, model, engine="auto"):
    from streamml.cli import cardata_lstm
    used = []
    monkeypatch.setattr(cardata_lstm, "_predict_persistent",
                        lambda m, rows, first, count: used.append("persistent") or
                        np.zeros((count, m.features), np.float32))
    rows = np.random.default_rng(0).uniform(-1, 1, size=(40, 18)).astype(np.float32)
    ns = types.SimpleNamespace(look_back=model.look_back, skip=0, batch_size=4, predict_take=2, predict_engine=engine)
    out = cardata_lstm._predict(ns, None, None, rows, model, None)
    return used, out


def test_predict_auto_resolves_to_batch_without_a_servable_model(monkeypatch):
    import streamml.ops.serve as serve
    stack = [("lstm", 8, False, "tanh"), ("dense", 18, False)]
    cpu = _model(stack)
    used, out = _run_predict(monkeypatch, cpu)             # a CPU model: batch
    assert used == [] and out.shape == (8, 18)
    used, _ = _run_predict(monkeypatch, _OnDevice(cpu))    # servable, on a device: the forecaster
    assert used == ["persistent"]

    class Refuses:
        @staticmethod
        def supports(model):
            return False, "LSTM layers must have 1..512 units"

    monkeypatch.setattr(serve, "LSTMScoringServer", Refuses)
    used, out = _run_predict(monkeypatch, _OnDevice(cpu))  # on a device but not servable: batch
    assert used == [] and out.shape == (8, 18)
    with pytest.raises(SystemExit, match="1..512 units"):  # asked for explicitly: exits with the reason
        _run_predict(monkeypatch, _OnDevice(cpu), engine="persistent")


def test_supports_reports_the_offending_layer():
    too_wide = _model([("lstm", 520, False, "tanh"), ("dense", 18, False)])
    ok, why = LSTMScoringServer.supports(too_wide)
    assert not ok and "lstm has 520" in why
