"""The bf16 persistent Dense trainer's limits and its way through the public interface, checked
without a device: ``ops.dense_persistent.check_shape(..., precision="bf16")``,
``nn.Model.compile(minibatch_precision=)`` and the ``--layers ... --precision`` CLI."""
import numpy as np
import pytest

from streamml import nn
from streamml.nn.layers import Dense
from streamml.ops import dense_persistent as dp


def test_max_params_bf16_is_64_tiles_of_256():
    assert dp.MAX_PARAMS_BF16 == 16384


def test_exactly_max_params_bf16_is_accepted():
    assert dp.check_shape([64, 128, 64], 32, precision="bf16") == ""
    assert dp.check_shape([30, 128, 32, 128, 30], 32, precision="bf16") == ""
    assert dp.check_shape([30, 128, 32, 128, 30], 128, own_targets=True, precision="bf16") == ""
    assert dp.check_shape([18, 64, 16, 64, 18], 100, precision="bf16") == ""
    assert dp.lds_bytes([30, 128, 32, 128, 30], True, precision="bf16") <= dp.LDS_BYTES


def test_one_more_tile_is_refused_while_fp32_accepts():
    why = dp.check_shape([65, 113, 65], 32, precision="bf16")      # 80 x 128 x 2 = 20 480 elements
    assert "MAX_PARAMS_BF16" in why and "20480" in why, why
    assert dp.check_shape([65, 113, 65], 32, precision="fp32") == ""
    assert dp.check_shape([65, 113, 65], 32) == ""


@pytest.mark.parametrize("widths,batch,word", [
    ([18, 129, 18], 32, "MAX_WIDTH"),
    ([18] + [20] * 8 + [18], 32, "MAX_LAYERS"),
    ([18, 33, 18], 0, "MAX_BATCH"),
    ([18, 33, 18], 129, "MAX_BATCH"),
], ids=["w129", "nine_layers", "b0", "b129"])
def test_shared_limits_hold_for_bf16(widths, batch, word):
    assert word in dp.check_shape(widths, batch, precision="bf16")


def test_unknown_precision_is_an_error():
    with pytest.raises(ValueError, match="precision"):
        dp.check_shape([18, 33, 18], 32, precision="fp8")


def _seq(widths=(20, 18)):
    layers = [Dense(u, "tanh", input_shape=(18,) if i == 0 else None) for i, u in enumerate(widths)]
    return nn.Sequential(layers, device="cpu", seed=13)


def test_supports_takes_a_precision():
    model = _seq((64, 16, 64, 18))
    model.compile(loss="mse")
    assert dp.supports(model, 32, precision="bf16") == (True, "")
    wide = nn.Sequential([Dense(113, "tanh", input_shape=(65,)), Dense(65, "linear")], device="cpu", seed=1)
    wide.compile(loss="mse")
    assert dp.supports(wide, 32) == (True, "")
    ok, why = dp.supports(wide, 32, precision="bf16")
    assert not ok and "MAX_PARAMS_BF16" in why


def test_compile_refuses_an_unknown_minibatch_precision():
    with pytest.raises(ValueError, match="minibatch_precision"):
        _seq().compile(loss="mse", minibatch_precision="fp8")


def test_bf16_is_a_no_op_on_a_cpu_model():
    x = np.random.default_rng(0).uniform(0, 1, (64, 18)).astype(np.float32)
    a, b = _seq(), _seq()
    a.compile(loss="mse")
    b.compile(loss="mse", minibatch_precision="bf16")
    assert b.minibatch_precision == "bf16" and a.minibatch_precision is None
    a.fit(x, batch_size=32, epochs=1, verbose=0)
    b.fit(x, batch_size=32, epochs=1, verbose=0)
    assert b.last_fit_engine == "layers" and b.last_fit_precision is None
    for wa, wb in zip(a.get_weights(), b.get_weights()):
        np.testing.assert_array_equal(wa, wb)


@pytest.mark.parametrize("flag,want", [(["--precision", "bf16"], "bf16"), ([], None)], ids=["bf16", "unset"])
def test_layers_cli_hands_the_precision_to_compile(tmp_path, monkeypatch, flag, want):
    from streamml.cli.__main__ import main as cli
    seen = []
    real = nn.Model.compile

    def spy(self, *a, **kw):
        seen.append(kw.get("minibatch_precision", "absent"))
        return real(self, *a, **kw)

    monkeypatch.setattr(nn.Model, "compile", spy)
    monkeypatch.setenv("SML_MODEL_STORE", str(tmp_path / "store"))
    assert cli(["cardata-v3", "synthetic://3000", "CARBF", "0", "predbf", "train", "bf.h5", "proj", "--epochs", "1",
                "--device", "cpu", "--workdir", str(tmp_path), "--layers", "64,16,64", "--take", "4", *flag]) == 0
    assert seen and seen[0] == want, seen
