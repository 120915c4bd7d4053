"""The large-batch Dense train step's limits, checked without a device: ``ops.dense_batch.supports``
names the limit a model exceeds, and ``fit(engine="throughput")`` says why it cannot run."""
import numpy as np
import pytest

from streamml import nn
from streamml.nn.layers import Dense
from streamml.ops import dense_batch as db


def _seq(widths, features=18):
    acts = ["tanh"] * (len(widths) - 1) + ["linear"]
    layers = [Dense(u, a, input_shape=(features,) if i == 0 else None) for i, (u, a) in enumerate(zip(widths, acts))]
    model = nn.Sequential(layers, device="cpu", seed=13)
    model.compile(loss="mse")
    return model


@pytest.mark.parametrize("widths,features,batch,word", [
    ([20] * 8 + [18], 18, 1024, "MAX_LAYERS"),
    ([129, 18], 18, 1024, "MAX_WIDTH"),
    ([128, 128, 128], 128, 1024, "MAX_PARAMS_BF16"),
    ([64, 16, 64, 18], 18, db.MAX_BATCH + 1, "MAX_BATCH"),
    ([64, 16, 64, 18], 18, 0, "MAX_BATCH"),
], ids=["nine_layers", "w129", "params", "batch_above", "batch_zero"])
def test_supports_names_the_limit(widths, features, batch, word):
    ok, why = db.supports(_seq(widths, features), batch)
    assert not ok and word in why, why


@pytest.mark.parametrize("batch", [1, 129, 65536, db.MAX_BATCH])
def test_required_stacks_are_accepted_above_the_persistent_batch(batch):
    assert db.MAX_BATCH == 1 << 24
    for widths, features in (([64, 16, 64, 18], 18), ([128, 32, 128, 30], 30)):
        assert db.supports(_seq(widths, features), batch) == (True, "")
        assert db.supports(_seq(widths, features), batch, own_targets=True) == (True, "")


def test_fit_engine_throughput_on_the_cpu():
    model = _seq([20, 18])
    x = np.random.default_rng(0).uniform(0, 1, (64, 18)).astype(np.float32)
    with pytest.raises(ValueError, match="ROCm"):
        model.fit(x, batch_size=256, epochs=1, verbose=0, engine="throughput")
    with pytest.raises(ValueError, match="engine"):
        model.fit(x, batch_size=32, epochs=1, verbose=0, engine="fast")
    model.fit(x, batch_size=32, epochs=1, verbose=0)
    assert model.last_fit_engine == "layers"
