"""The persistent Dense trainer's limits, checked without a device: ``ops.dense_persistent.supports``
answers and reasons, the two stacks it must admit, and the ``--layers`` CLI round trip on the CPU."""
import numpy as np
import pytest

from helpers import dense_mb_cases as cases
from streamml import nn
from streamml.nn.layers import LSTM, Dense, Dropout
from streamml.ops import dense_persistent as dp


def _seq(widths, acts=None, features=18, loss="mse", **first_kw):
    acts = acts or ["tanh"] * (len(widths) - 1) + ["linear"]
    layers = [Dense(u, a, input_shape=(features,) if i == 0 else None, **(first_kw if i == 0 else {}))
              for i, (u, a) in enumerate(zip(widths, acts))]
    model = nn.Sequential(layers, device="cpu", seed=13)
    model.compile(loss=loss)
    return model


def _with_dropout(rate):
    model = nn.Sequential([Dense(40, "relu", input_shape=(18,)), Dropout(rate), Dense(18, "linear")], device="cpu")
    model.compile(loss="mse")
    return model


def _with_lstm():
    model = nn.Sequential([LSTM(8, input_shape=(3, 18)), Dense(18)], device="cpu", seed=1)
    model.compile(loss="mse")
    return model


@pytest.mark.parametrize("build,batch,word", [
    (lambda: _seq([20] * 8 + [18]), 32, "MAX_LAYERS"),
    (lambda: _seq([129, 18]), 32, "MAX_WIDTH"),
    (lambda: _seq([33, 18]), 129, "MAX_BATCH"),
    (lambda: _with_dropout(0.3), 32, "Dropout"),
    (_with_lstm, 32, "LSTM"),
    (lambda: _seq([16, 18], acts=["tanh", "softmax"]), 32, "softmax"),
    (lambda: _seq([16, 18], loss="mae"), 32, "mean_absolute_error"),
    (lambda: _seq([128, 128, 128], features=128), 32, "MAX_PARAMS"),
    (lambda: _seq([16, 17]), 32, "y = x"),
], ids=["nine_layers", "w129", "b129", "dropout", "lstm", "softmax", "mae", "params", "y_is_x"])
def test_supports_names_the_limit(build, batch, word):
    ok, why = dp.supports(build(), batch)
    assert not ok and word in why, why


@pytest.mark.parametrize("widths,features", [([64, 16, 64, 18], 18), ([128, 32, 128, 30], 30)])
@pytest.mark.parametrize("batch", [1, 32, 100, 128])
def test_required_stacks_are_accepted(widths, features, batch):
    model = _seq(widths, acts=["tanh", "relu", "tanh", "relu"], features=features)
    assert dp.supports(model, batch) == (True, "")
    assert dp.supports(model, batch, own_targets=True) == (True, "")


def test_other_accepted_models():
    assert dp.supports(_with_dropout(0.0), 32) == (True, "")
    assert dp.supports(_seq([20, 18], use_bias=False), 7) == (True, "")
    assert dp.supports(_seq([16, 17]), 32, own_targets=True) == (True, "")
    assert _seq([128, 32, 128, 30], features=30).count_params() == 16190


def test_shape_list_covers_both_answers():
    answers = [dp.check_shape(list(w), b, own) for w, b, own in cases.SHAPES]
    assert sum(a == "" for a in answers) >= 8 and sum(a != "" for a in answers) >= 8
    for word in ("MAX_LAYERS", "MAX_WIDTH", "MAX_BATCH", "MAX_PARAMS", "LDS_BYTES", "y = x"):
        assert any(word in a for a in answers), word


def test_table_points_into_the_flat_buffer():
    model = _seq([20, 18], use_bias=False)
    rows = dp.table(model)
    assert rows[0][:4] == (18, 20, dp.ACT["tanh"], 0) and rows[1][:4] == (20, 18, dp.ACT["linear"], 1)
    assert rows[0][6] == 0 and rows[1][6] == 18 * 20 and rows[1][7] == 18 * 20 + 20 * 18
    assert model.fp.n == 18 * 20 + 20 * 18 + 18


def test_fit_engine_argument_on_the_cpu():
    model = _seq([20, 18])
    x = np.random.default_rng(0).uniform(0, 1, (64, 18)).astype(np.float32)
    model.fit(x, batch_size=32, epochs=1, verbose=0)
    assert model.last_fit_engine == "layers"
    with pytest.raises(ValueError, match="ROCm"):
        model.fit(x, batch_size=32, epochs=1, verbose=0, engine="persistent")
    with pytest.raises(ValueError, match="engine"):
        model.fit(x, batch_size=32, epochs=1, verbose=0, engine="fast")


def test_layers_flag_trains_saves_and_reloads_a_dense_stack(tmp_path, monkeypatch):
    from streamml.cli.__main__ import main as cli
    from streamml.ops.serve import DenseScoringServer
    monkeypatch.setenv("SML_MODEL_STORE", str(tmp_path / "store"))
    base = ["synthetic://6000", "CARSL", "0", "predsl"]
    common = ["--device", "cpu", "--workdir", str(tmp_path), "--layers", "64,16,64", "--take", "8", "--skip", "8",
              "--predict-take", "4"]
    assert cli(["cardata-v3", *base, "train", "wide.h5", "proj", "--epochs", "2", *common]) == 0
    model = nn.load_model(str(tmp_path / "wide.h5"), device="cpu")
    dense = [l for l in model.layers if isinstance(l, Dense)]
    assert [l.units for l in dense] == [64, 16, 64, 18]
    assert [l.activation for l in dense] == ["tanh", "relu", "tanh", "relu"]
    assert int(model.fp.iter.item()) == 16                      # 2 epochs x take(8): the Adam state came along
    assert DenseScoringServer.supports(model) == (True, "")     # what `serve --model dense` asks
    assert dp.supports(model, 100) == (True, "")
    x = np.random.default_rng(1).uniform(0, 1, (5, 18)).astype(np.float32)
    assert model.predict(x).shape == (5, 18)
    assert cli(["cardata-v3", *base, "predict", "wide.h5", "proj", *common]) == 0
    assert cli(["cardata-v1", "synthetic://4000", "CARSL1", "0", "predsl1", "--epochs", "1", *common]) == 0


def test_layers_flag_is_refused_under_torchrun(tmp_path, monkeypatch):
    from streamml.cli.__main__ import main as cli
    monkeypatch.setenv("WORLD_SIZE", "2")
    try:
        rc = cli(["cardata-v1", "synthetic://2000", "CARSL2", "0", "p2", "--device", "cpu", "--workdir", str(tmp_path),
                  "--layers", "20", "--epochs", "1", "--take", "2"])
    except SystemExit as e:
        rc = e.code
    assert rc not in (0, None) and not (tmp_path / "path_to_my_model.h5").exists()
