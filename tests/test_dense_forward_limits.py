"""The fused bulk forward's limits and weight image on the CPU (``ops/dense_forward.py``: the Python
mirror of ``csrc/include/sml_dense_fwd_plan.h``; tests/test_dense_forward_check.py holds the two checks
together on the CPU, tests/test_dense_forward_gpu.py through the extension)."""
import numpy as np
import pytest

from streamml import nn
from streamml.nn.layers import LSTM, Dense, Dropout
from streamml.ops import dense_forward as dfw
from streamml.ops.dense_persistent import MAX_PARAMS_BF16

#        hidden + output widths, activations, features, score, words of the reason ("" = supported)
LIMITS = {
    "cardata_64": ([64, 16, 64, 18], ["tanh", "relu", "tanh", "linear"], 18, True, ""),
    "max_width_64k_image": ([128, 32, 128, 30], ["tanh", "relu", "tanh", "linear"], 30, True, ""),
    "eight_layers": ([24, 16, 12, 8, 12, 16, 24, 18], ["tanh"] * 8, 18, True, ""),
    "nine_layers": ([20] * 8 + [18], ["tanh"] * 9, 18, True, "9 Dense layers: the fused forward takes 1..8 (MAX_LAYERS)"),
    "wide_input": ([16, 129], ["relu", "linear"], 129, True, "input width 129 is outside 1..128 (MAX_WIDTH)"),
    "wide_layer": ([256, 18], ["tanh", "linear"], 18, True, "layer 0 has 256 units: the limit is 128 (MAX_WIDTH)"),
    "softmax": ([32, 18], ["relu", "softmax"], 18, False, "layer 1: unknown activation"),
    "score_needs_square": ([32, 5], ["relu", "linear"], 18, True, "need as many output units as inputs (5 units, 18"),
    "rec_takes_any_head": ([32, 5], ["relu", "linear"], 18, False, ""),
    "lds": ([128] * 4, ["relu"] * 4, 128, True, "bytes of LDS: the limit is 163840 (LDS_BYTES)"),
}


def _model(widths, acts, feat):
    return nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                          for i, (u, a) in enumerate(zip(widths, acts))], device="cpu", seed=3)


@pytest.mark.parametrize("name", list(LIMITS))
def test_supports_names_the_limit(name):
    widths, acts, feat, score, words = LIMITS[name]
    ok, why = dfw.supports(_model(widths, acts, feat), score=score)
    assert ok == (words == "") and words in why, why


def test_supports_refuses_other_layers():
    m = nn.Sequential([LSTM(8, input_shape=(4, 18)), Dense(18)], device="cpu")
    ok, why = dfw.supports(m)
    assert not ok and "LSTM" in why


def test_plan_admits_every_stack_of_the_bf16_trainer():
    """A 64 KiB image (MAX_PARAMS_BF16 padded elements) at the widest staging stride still fits."""
    assert 128 * 128 == MAX_PARAMS_BF16 and dfw.check_shape([128, 128], ["relu"], True) == ""
    p = dfw.plan([128, 128])
    assert p["mb"] == 8 and 1 <= p["waves"] <= 4 and p["lds_bytes"] + 1024 <= dfw.LDS_BYTES
    assert dfw.plan([18, 64, 16, 64, 18])["mb"] == 4 and dfw.plan([18, 64, 16, 64, 18])["waves"] == 8
    assert dfw.plan([18, 33, 18])["mb"] == 4 and dfw.plan([7, 7])["mb"] == 2


def test_image_unpacks_to_the_weights():
    """img[w_off + ((kb * nub + ub) * 64 + lane) * 4 + r] = W[16 kb + 4 (lane // 16) + r][16 ub + lane % 16],
    zeros past in / units; the bias follows, zero past units and for a layer without bias."""
    m = nn.Sequential([Dense(33, "tanh", input_shape=(18,)), Dropout(0.2), Dense(40, "relu", use_bias=False),
                       Dense(18, "sigmoid")], device="cpu", seed=5)
    rng = np.random.default_rng(5)
    m.set_weights([rng.uniform(-1, 1, w.shape).astype(np.float32) for w in m.get_weights()])
    from streamml.ops.serve import dense_layer_table
    layers, weights = dense_layer_table(m)
    img, table = dfw.pack_image(layers, weights)
    assert [t[:3] for t in table] == [(18, 33, 2), (33, 40, 1), (40, 18, 3)]
    assert img.dtype == np.float32 and img.size == dfw.image_table(layers)[1] == 32 * 48 + 48 + 48 * 48 + 48 + 48 * 32 + 32
    lane, r = np.arange(64)[:, None], np.arange(4)[None, :]
    for (n_in, n_out, _, w_off, b_off), (W, b) in zip(table, weights):
        kp, npad = -(-n_in // 16) * 16, -(-n_out // 16) * 16
        Wp = np.full((kp, npad), np.nan, np.float32)
        for kb in range(kp // 16):
            for ub in range(npad // 16):
                blk = img[w_off + (kb * (npad // 16) + ub) * 256:][:256].reshape(64, 4)
                Wp[16 * kb + 4 * (lane // 16) + r, 16 * ub + lane % 16 + 0 * r] = blk
        assert b_off == w_off + kp * npad
        assert np.array_equal(Wp[:n_in, :n_out], W) and not Wp[n_in:].any() and not Wp[:, n_out:].any()
        bp = img[b_off:b_off + npad]
        assert np.array_equal(bp[:n_out], b if b is not None else np.zeros(n_out)) and not bp[n_out:].any()
    # the model's own image is a gather of the flat parameters through the same packing
    dev_img, dev_table = dfw.image(m)
    assert np.array_equal(dev_img.numpy(), img) and [tuple(t) for t in dev_table] == table
    m.fp.flat.mul_(2.0)   # an in-place update no hook sees
    assert np.array_equal(dfw.image(m)[0].numpy(), 2.0 * img)
