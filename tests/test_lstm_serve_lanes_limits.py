"""The multi-lane forecaster's limits and its key -> lane sharding, checked without a device:
``LSTMScoringServer.supports(model, lanes=...)``, the partition / gather table the host runtime
shards a batch with (``_io.serve_lane_partition``, csrc/include/sml_serve_shard.h), and the
``--lanes`` flag of ``serve`` and ``cardata-lstm ... predict``."""
import types

import numpy as np
import pytest
import torch

from streamml.cli import common
from streamml.models.lstm import LSTMPredictor
from streamml.ops.serve import LSTMScoringServer

WIDE = [("lstm", 136, True, "tanh"), ("lstm", 40, False, "tanh"), ("dense", 18, False)]
NARROW = [("lstm", 32, False, "tanh"), ("dense", 18, False)]


def _model(stack, look_back=6, features=18):
    return LSTMPredictor(look_back=look_back, features=features, stack=stack, device="cpu", seed=1)


def test_max_lanes_constant():
    assert LSTMScoringServer.MAX_LANES == 32


@pytest.mark.parametrize("lanes", [1, 32])
def test_supports_a_wide_stack_on_lanes(lanes):
    assert LSTMScoringServer.supports(_model(WIDE), lanes=lanes) == (True, "")


@pytest.mark.parametrize("lanes", [0, 33, -1])
def test_supports_refuses_lanes_out_of_range(lanes):
    ok, why = LSTMScoringServer.supports(_model(WIDE), lanes=lanes)
    assert not ok and "lanes must be 1..32" in why, why


def test_supports_narrow_stacks_take_one_lane_only():
    m = _model(NARROW)
    assert LSTMScoringServer.supports(m) == (True, "")
    assert LSTMScoringServer.supports(m, lanes=1) == (True, "")
    ok, why = LSTMScoringServer.supports(m, lanes=2)
    assert not ok and why == "only the streamed-weight (wide) kernel runs on several lanes"
    # the reference stacks are narrow too
    assert not LSTMScoringServer.supports(LSTMPredictor.two_layer(look_back=50, device="cpu"), lanes=2)[0]


def test_supports_reports_the_models_own_limit_before_the_lane_rule():
    ok, why = LSTMScoringServer.supports(_model([("lstm", 513, False, "tanh"), ("dense", 18, False)]), lanes=4)
    assert not ok and "512" in why


def _partition(keys, lanes):
    from streamml.ops import load_io
    order, start = load_io().serve_lane_partition(np.asarray(keys, np.int64), lanes)
    return np.asarray(order), np.asarray(start)


@pytest.mark.parametrize("seed", range(8))
def test_lane_partition_is_stable_and_its_inverse_restores_batch_order(seed):
    rng = np.random.default_rng(seed)
    lanes = int(rng.integers(1, 33))
    k = int(rng.integers(0, 400))
    # few keys (hot lanes, empty lanes) or many, up to the top of uint32
    hi = [3, 50, 1 << 32][seed % 3]
    keys = rng.integers(0, hi, size=k, dtype=np.int64)
    order, start = _partition(keys, lanes)
    assert order.shape == (k,) and start.shape == (lanes + 1,)
    assert start[0] == 0 and start[-1] == k and np.all(np.diff(start) >= 0)
    assert sorted(order.tolist()) == list(range(k))          # a permutation of the batch
    for l in range(lanes):
        mine = order[start[l]:start[l + 1]]
        assert np.all(keys[mine] % lanes == l)                # every row on its key's lane
        assert np.all(np.diff(mine) > 0)                      # in batch order within the lane (stable)
        assert len(mine) == int(np.sum(keys % lanes == l))
    # what the gather does: lane results, concatenated lane by lane, scattered through `order`
    per_lane = np.arange(k)[order] * 10 + 7                   # "result" of the row each lane slot holds
    back = np.empty(k, np.int64)
    back[order] = per_lane
    assert np.array_equal(back, np.arange(k) * 10 + 7)
    inv = np.empty(k, np.int64)
    inv[order] = np.arange(k)
    assert np.array_equal(order[inv], np.arange(k))           # the inverse permutation restores batch order


def test_lane_partition_edges():
    order, start = _partition([], 4)
    assert order.size == 0 and start.tolist() == [0, 0, 0, 0, 0]
    order, start = _partition([5, 5, 5, 1], 4)                 # one hot lane
    assert order.tolist() == [0, 1, 2, 3] and start.tolist() == [0, 0, 4, 4, 4]
    order, start = _partition([3, 2, 1, 0, 7], 4)
    assert order.tolist() == [3, 2, 1, 0, 4] and start.tolist() == [0, 1, 2, 3, 5]
    order, start = _partition([9, 8, 7], 1)                    # one lane: the identity
    assert order.tolist() == [0, 1, 2] and start.tolist() == [0, 3]
    with pytest.raises(ValueError):
        _partition([1], 0)
    with pytest.raises(IndexError):
        _partition([-1], 2)


def test_cli_parses_lanes():
    from streamml.cli import cardata_lstm, serve
    pos = ["servers", "topic", "result_topic", "model_file"]
    ns = common.parse(["s", "t", "r", "m.h5", "--model", "lstm", "--lanes", "8"], serve.USAGE, pos,
                      add_flags=serve._flags)
    assert ns.lanes == 8 and ns.model == "lstm"
    assert common.parse(["s", "t", "r", "m.h5"], serve.USAGE, pos, add_flags=serve._flags).lanes == 1
    pos = ["servers", "topic", "offset", "result_topic", "mode", "model_file"]
    ns = common.parse(["s", "t", "0", "r", "predict", "m.h5", "--lanes", "4"], cardata_lstm.V2_USAGE, pos,
                      add_flags=cardata_lstm._flags)
    assert ns.lanes == 4 and ns.mode == "predict"
    assert common.parse(["s", "t", "0", "r", "predict", "m.h5"], cardata_lstm.V2_USAGE, pos,
                        add_flags=cardata_lstm._flags).lanes == 1


def test_serve_exits_with_the_reason_for_an_unservable_lane_count():
    from streamml.cli import serve
    with pytest.raises(SystemExit, match="only the streamed-weight"):
        serve._require_servable(_model(NARROW), 2)
    with pytest.raises(SystemExit, match="lanes must be 1..32"):
        serve._require_servable(_model(WIDE), 33)
    serve._require_servable(_model(WIDE), 8)
    serve._require_servable(_model(NARROW))


class _OnDevice:
    """A CPU model that claims a ROCm device: what ``_predict`` sees on a GPU machine."""

    def __init__(self, model):
        self._m = model
        self.device = torch.device("cuda", 0)

    def __getattr__(self, name):
        return getattr(self._m, name)


def _run_predict(monkeypatch, model, engine, lanes):
    from streamml.cli import cardata_lstm
    used = []
    monkeypatch.setattr(cardata_lstm, "_predict_persistent",
                        lambda m, rows, first, count, lanes=1: used.append(lanes) or
                        np.zeros((count, m.features), np.float32))
    rows = np.random.default_rng(0).uniform(-1, 1, size=(40, 18)).astype(np.float32)
    ns = types.SimpleNamespace(look_back=model.look_back, skip=0, batch_size=4, predict_take=2, predict_engine=engine,
                               lanes=lanes)
    out = cardata_lstm._predict(ns, None, None, rows, model, None)
    return used, out


def test_predict_passes_lanes_on_and_names_an_unservable_combination(monkeypatch):
    wide, narrow = _OnDevice(_model(WIDE, look_back=3)), _OnDevice(_model(NARROW, look_back=3))
    used, out = _run_predict(monkeypatch, wide, "persistent", 4)
    assert used == [4] and out.shape == (8, 18)
    used, _ = _run_predict(monkeypatch, wide, "auto", 1)
    assert used == [1]
    used, out = _run_predict(monkeypatch, narrow, "auto", 2)       # not servable on 2 lanes: batch
    assert used == [] and out.shape == (8, 18)
    with pytest.raises(SystemExit, match="only the streamed-weight"):   # asked for explicitly: the reason
        _run_predict(monkeypatch, narrow, "persistent", 2)
    with pytest.raises(SystemExit, match="lanes must be 1..32"):
        _run_predict(monkeypatch, wide, "persistent", 33)
