"""The wide large-batch Dense train step's limits, checked without a device:
``ops.dense_batch_wide.supports`` names the limit a model or a batch exceeds, and ``fit(engine="wide")``
says why it cannot run."""
import numpy as np
import pytest

from streamml import nn
from streamml.nn.layers import Dense
from streamml.ops import dense_batch_wide as dbw


def _seq(widths, features=18, loss="mse"):
    acts = ["tanh"] * (len(widths) - 1) + ["linear"]
    layers = [Dense(u, a, input_shape=(features,) if i == 0 else None) for i, (u, a) in enumerate(zip(widths, acts))]
    model = nn.Sequential(layers, device="cpu", seed=13)
    model.compile(loss=loss)
    return model


@pytest.mark.parametrize("widths,loss,batch,word", [
    ([20] * 8 + [18], "mse", 1024, "MAX_LAYERS"),
    ([513, 18], "mse", 1024, "MAX_WIDTH"),
    ([64, 18], "mae", 1024, "mean_squared_error"),
    ([64, 16, 64, 18], "mse", 0, "MAX_BATCH"),
    ([512, 512, 512, 18], "mse", 1 << 20, "WS_BYTES"),
], ids=["nine_layers", "w513", "loss", "batch_zero", "workspace"])
def test_supports_names_the_limit(widths, loss, batch, word):
    ok, why = dbw.supports(_seq(widths, loss=loss), batch)
    assert not ok and word in why, why


@pytest.mark.parametrize("widths", [[512, 512, 512, 18], [64, 16, 64, 18]])
def test_required_stacks_are_accepted(widths):
    for batch in (1, 129, 65536):
        assert dbw.supports(_seq(widths), batch) == (True, "")
        assert dbw.supports(_seq(widths), batch, own_targets=True) == (True, "")
    # the budget is the largest workspace a step may take: 6272 bytes a row for the 512-wide stack
    assert dbw.workspace_bytes([18, 512, 512, 512, 18], 64) == 64 * 6272


def test_fit_engine_wide_on_the_cpu():
    model = _seq([20, 18])
    x = np.random.default_rng(0).uniform(0, 1, (64, 18)).astype(np.float32)
    with pytest.raises(ValueError, match="ROCm"):
        model.fit(x, batch_size=256, epochs=1, verbose=0, engine="wide")
