"""The wide fused bulk forward's limits and bf16 weight image on the CPU (``ops/dense_forward_wide.py``:
the Python mirror of ``csrc/include/sml_dense_fwdw_plan.h``; tests/test_dense_forward_check.py holds the
two checks together on the CPU, tests/test_dense_forward_wide_gpu.py through the extension)."""
import numpy as np
import pytest

from helpers.dense_mb_bf16_ref import bf
from streamml import nn
from streamml.nn.layers import Dense, Dropout
from streamml.ops import dense_forward_wide as dfww

#        hidden + output widths, activations, features, score, words of the reason ("" = supported)
LIMITS = {
    "nine_layers": ([20] * 8 + [18], ["tanh"] * 9, 18, True, "9 Dense layers: the wide fused forward takes 1..8 (MAX_LAYERS)"),
    "wide_input": ([16, 513], ["relu", "linear"], 513, True, "input width 513 is outside 1..512 (MAX_WIDTH)"),
    "wide_layer": ([513, 18], ["tanh", "linear"], 18, True, "layer 0 has 513 units: the limit is 512 (MAX_WIDTH)"),
    "softmax": ([32, 18], ["relu", "softmax"], 18, False, "layer 1: unknown activation"),
    "score_needs_square": ([32, 5], ["relu", "linear"], 18, True, "need as many output units as inputs (5 units, 18"),
    "18-512-512-512-18": ([512, 512, 512, 18], ["tanh", "relu", "tanh", "linear"], 18, True, ""),
    "eight_512_layers": ([512] * 8, ["relu"] * 8, 512, True, ""),   # LDS holds the widest tile: 133120 bytes
}


@pytest.mark.parametrize("name", list(LIMITS))
def test_supports_names_the_limit(name):
    widths, acts, feat, score, words = LIMITS[name]
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                       for i, (u, a) in enumerate(zip(widths, acts))], device="cpu", seed=3)
    ok, why = dfww.supports(m, score=score)
    assert ok == (words == "") and words in why, why
    if ok:
        assert dfww.plan([feat] + widths, 128)["lds_bytes"] + 2048 <= dfww.LDS_BYTES


def test_image_unpacks_to_the_weights():
    """img[w_off + ((kb * nub + ub) * 64 + lane) * 8 + j] = bf16(W[32 kb + 8 (lane // 16) + j][16 ub + lane % 16]),
    zeros past in / units; the fp32 bias follows, zero past units and for a layer without bias."""
    m = nn.Sequential([Dense(33, "tanh", input_shape=(18,)), Dropout(0.2), Dense(40, "relu", use_bias=False),
                       Dense(18, "sigmoid")], device="cpu", seed=5)
    rng = np.random.default_rng(5)
    m.set_weights([rng.uniform(-1, 1, w.shape).astype(np.float32) for w in m.get_weights()])
    from streamml.ops.serve import dense_layer_table
    layers, weights = dense_layer_table(m)
    img, table = dfww.pack_image(layers, weights)
    assert [t[:3] for t in table] == [(18, 33, 2), (33, 40, 1), (40, 18, 3)]
    assert img.dtype == np.uint16 and img.size == dfww.image_table(layers)[1] == 32 * 48 + 96 + 64 * 48 + 96 + 64 * 32 + 64
    lane, j = np.arange(64)[:, None], np.arange(8)[None, :]
    for (n_in, n_out, _, w_off, b_off), (W, b) in zip(table, weights):
        kp, npad = -(-n_in // 32) * 32, -(-n_out // 16) * 16
        Wp = np.full((kp, npad), np.nan, np.float32)
        for kb in range(kp // 32):
            for ub in range(npad // 16):
                blk = img[w_off + (kb * (npad // 16) + ub) * 512:][:512].reshape(64, 8)
                Wp[32 * kb + 8 * (lane // 16) + j, 16 * ub + lane % 16 + 0 * j] = (blk.astype(np.uint32) << 16).view(np.float32)
        assert b_off == w_off + kp * npad and w_off % 8 == 0 and b_off % 8 == 0
        assert np.array_equal(Wp[:n_in, :n_out], bf(W)) and not Wp[n_in:].any() and not Wp[:, n_out:].any()
        bp = img[b_off:b_off + 2 * npad].view(np.float32)
        assert np.array_equal(bp[:n_out], b if b is not None else np.zeros(n_out)) and not bp[n_out:].any()
    # the model's own image is a gather of the flat parameters through the same packing, always current
    dev_img, dev_table = dfww.image(m)
    assert np.array_equal(dev_img.numpy().view(np.uint16), img) and [tuple(t) for t in dev_table] == table
    m.fp.flat.mul_(2.0)   # an in-place update no hook sees
    assert np.array_equal(dfww.image(m)[0].numpy().view(np.uint16), dfww.pack_image(layers, [(2 * W, None if b is None else 2 * b)
                                                                                           for W, b in weights])[0])
