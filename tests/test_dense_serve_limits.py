"""The persistent Dense scorer's limits, weight image and CLI guards, checked without a device:
``DenseScoringServer.supports`` / ``kernel_for``, ``dense_serve_image`` and ``serve --model dense``; and
``supports`` / ``kernel_for`` against the host program over ``sml_dense_fleet_serve.h``
(``dense_serve_check``, ``dense_serve_in_lds``): the Python mirror and the C++ check must decide
alike and name the same limit."""
import os
import subprocess

import numpy as np
import pytest

import streamml
from helpers.dense_serve_ref import forward, forward_image, unpack_image
from streamml import nn
from streamml.nn.layers import LSTM, Dense, Dropout
from streamml.ops.serve import DenseScoringServer, dense_layer_table, dense_serve_image


def _seq(widths, acts=None, features=18, seed=13, **first_kw):
    acts = acts or ["tanh"] * (len(widths) - 1) + ["linear"]
    layers = [Dense(u, a, input_shape=(features,) if i == 0 else None, **(first_kw if i == 0 else {}))
              for i, (u, a) in enumerate(zip(widths, acts))]
    return nn.Sequential(layers, device="cpu", seed=seed)


def _with_dropout():
    return nn.Sequential([Dense(40, "relu", input_shape=(18,)), Dropout(0.3), Dense(18, "linear")], device="cpu",
                         seed=13)


def _autoencoder():
    from streamml.models.autoencoder import Autoencoder
    return Autoencoder(18, 14, 7, device="cpu", seed=13)


@pytest.mark.parametrize("build", [
    lambda: _seq([33, 18]),
    lambda: _seq([512, 512, 18]),
    lambda: _seq([24, 16, 12, 8, 12, 16, 24, 18]),
    lambda: _seq([32], features=32),
    _with_dropout,
    lambda: _seq([40, 18], use_bias=False),
    _autoencoder,
], ids=["18-33-18", "18-512-512-18", "eight_layers", "one_layer_32", "dropout", "no_bias", "autoencoder"])
def test_supports(build):
    assert DenseScoringServer.supports(build()) == (True, "")


def _functional_with_lstm():
    return nn.Sequential([LSTM(8, input_shape=(3, 18)), Dense(18)], device="cpu", seed=1)


@pytest.mark.parametrize("build,word", [
    (lambda: _seq([513, 18]), "512"),
    (lambda: _seq([20] * 8 + [18]), "8"),
    (lambda: _seq([16, 33], features=33), "32"),
    (lambda: _seq([16, 17]), "one unit per feature"),
    (lambda: _seq([16, 18], acts=["tanh", "softmax"]), "softmax"),
    (_functional_with_lstm, "LSTM"),
], ids=["w513", "nine_layers", "D33", "last_units", "softmax", "lstm"])
def test_supports_names_the_limit(build, word):
    ok, why = DenseScoringServer.supports(build())
    assert not ok and word in why, why


def test_layer_table_of_an_autoencoder_and_of_a_stack_with_dropout():
    layers, weights = dense_layer_table(_autoencoder())
    assert [(i, o) for i, o, _, _ in layers] == [(18, 14), (14, 7), (7, 7), (7, 18)]
    assert [a for _, _, a, _ in layers] == ["tanh", "relu", "tanh", "relu"]
    assert [w.shape for w, _ in weights] == [(18, 14), (14, 7), (7, 7), (7, 18)]
    layers, weights = dense_layer_table(_with_dropout())
    assert [(i, o, a) for i, o, a, _ in layers] == [(18, 40, "relu"), (40, 18, "linear")]
    layers, weights = dense_layer_table(_seq([40, 18], use_bias=False))
    assert layers[0][3] is False and weights[0][1] is None and weights[1][1] is not None


@pytest.mark.parametrize("widths,acts", [([33, 18], ["tanh", "relu"]),
                                         ([130, 40, 130, 18], ["relu", "relu", "relu", "sigmoid"])],
                         ids=["18-33-18", "18-130-40-130-18"])
def test_image_round_trips(widths, acts):
    m = _seq(widths, acts)
    # non-zero biases, so a misplaced bias shows
    ws = m.get_weights()
    rng = np.random.default_rng(5)
    m.set_weights([w if w.ndim == 2 else rng.uniform(-0.5, 0.5, w.shape).astype(np.float32) for w in ws])
    layers, weights = dense_layer_table(m)
    image, table = dense_serve_image(layers, weights)
    assert image.dtype == np.float32
    off = 0
    for (n_in, n_out, act, _), (W, b), (ti, to, ta, w_off, b_off), (Wi, bi, Wp, bp) in zip(
            layers, weights, table, unpack_image(image, table)):
        kp, npad = (n_in + 3) // 4 * 4, (n_out + 31) // 32 * 32
        assert (ti, to, ta) == (n_in, n_out, {"linear": 0, "relu": 1, "tanh": 2, "sigmoid": 3}[act])
        assert (w_off, b_off) == (off, off + kp * npad) and w_off % 4 == 0 and b_off % 4 == 0
        # every W[k][o] and bias where the layout says: float4 img[g][o] = W[4g .. 4g + 3][o], then bias[Np]
        for k in range(n_in):
            for o in range(n_out):
                assert image[w_off + ((k // 4) * npad + o) * 4 + k % 4] == W[k, o]
        assert np.array_equal(image[b_off:b_off + n_out], b)
        # every padded entry is zero
        assert not Wp[n_in:].any() and not Wp[:, n_out:].any() and not bp[n_out:].any()
        assert np.array_equal(Wi, W) and np.array_equal(bi, b)
        off += kp * npad + npad
    assert image.size == off
    xn = np.random.default_rng(13).uniform(-1, 1, (50, 18))
    a, b = forward(layers, weights, xn), forward_image(layers, image, table, xn)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_image_of_a_layer_without_bias_has_a_zero_bias():
    layers, weights = dense_layer_table(_seq([40, 18], use_bias=False))
    image, table = dense_serve_image(layers, weights)
    assert not image[table[0][4]:table[0][4] + 64].any()


def test_kernel_for():
    assert DenseScoringServer.kernel_for(_seq([64, 16, 64, 18])) == "lds"
    assert DenseScoringServer.kernel_for(_seq([512, 512, 18])) == "stream"
    assert DenseScoringServer.kernel_for(_autoencoder()) == "lds"


def test_server_needs_a_rocm_device():
    with pytest.raises(RuntimeError, match="ROCm"):
        DenseScoringServer(_seq([33, 18]), device="cpu")


def _serve(tmp_path, model, name, extra=()):
    from streamml.cli.__main__ import main as cli_main
    model.compile(fused=False)
    model.save(str(tmp_path / name))
    return cli_main(["serve", "synthetic://100", "SENSOR_DENSE_CPU", "preds-dense-cpu", name, "--workdir",
                     str(tmp_path), "--device", "cpu", "--model", "dense", "--idle-timeout", "0.3", *extra])


@pytest.mark.parametrize("extra", [(), ("--low-latency",)], ids=["chunked", "low_latency"])
def test_cli_on_cpu_names_rocm(tmp_path, extra):
    with pytest.raises(SystemExit, match="ROCm"):
        _serve(tmp_path, _seq([64, 16, 64, 18]), "wide_ae.h5", extra)


def test_cli_names_the_limit_of_a_nine_layer_model(tmp_path):
    with pytest.raises(SystemExit, match=r"1\.\.8 Dense layers"):
        _serve(tmp_path, _seq([20] * 8 + [18]), "nine.h5")


def test_cli_names_the_cardata_normaliser(tmp_path, monkeypatch):
    """A servable model without 18 inputs: the error names the normaliser (checked on a model
    that claims a ROCm device, which is where the check is reached)."""
    import torch

    from streamml.cli import serve as serve_cli
    m = _seq([16, 20], features=20)
    m.build()
    m.device = torch.device("cuda", 0)
    with pytest.raises(SystemExit, match="cardata normaliser needs 18"):
        serve_cli._require_dense_servable(m)


# ---- supports / kernel_for and the host checker ------------------------------------------------
PKG = os.path.dirname(os.path.abspath(streamml.__file__))


def _tanh_stack(widths, seed=0):
    return nn.Sequential([Dense(u, "tanh", input_shape=(widths[0],) if i == 0 else None)
                          for i, u in enumerate(widths[1:])], device="cpu", seed=seed)


#          widths, what the refusal names ("" = served)
SHAPES = [
    ([18, 64, 16, 64, 18], ""),
    ([32, 32], ""),                                   # lane 31 is a feature here; the fleet refuses it
    ([33, 33], "1..32 features"),
    ([18, 513, 18], "1..512 units"),
    ([18] + [20] * 8 + [18], "1..8 Dense layers"),    # nine layers
    ([18, 64, 17], "one unit per feature"),
    # the two sides of DSV_LDS_IMAGE_BYTES = 94 208: 21 * 448 + 441 * 32 = 23 520 floats = 94 080 bytes,
    # and 21 * 448 + 445 * 32 = 23 648 floats = 94 592 bytes
    ([20, 440, 20], ""),
    ([20, 441, 20], ""),
]
KERNELS = {(20, 440, 20): ("lds", 23520), (20, 441, 20): ("stream", 23648)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")   # the host compiler the package itself is built with
    exe = str(tmp_path_factory.mktemp("dense_serve_check") / "dense_fleet_serve_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc", "include"),
                    os.path.join(PKG, "csrc", "tests", "dense_fleet_serve_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=120)
    return exe


def test_host_checker_agrees_with_supports_and_kernel_for(checker):
    text = "".join(",".join(map(str, w)) + "\n" for w, _ in SHAPES)
    r = subprocess.run([checker, "-s"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert len(got) == len(SHAPES)
    for (widths, names), (why_c, img_floats, where) in zip(SHAPES, got):
        model = _tanh_stack(widths)
        ok, why_py = DenseScoringServer.supports(model)
        # the decision, and the limit both name (Python adds the offending number to its wording)
        assert ok == (why_c == "") == (names == ""), (widths, why_c, why_py)
        assert names in why_c and names in why_py, (widths, why_c, why_py)
        if ok:
            layers, weights = dense_layer_table(model)
            assert dense_serve_image(layers, weights)[0].size == int(img_floats)
            assert DenseScoringServer.kernel_for(model) == where, (widths, img_floats, where)
        if tuple(widths) in KERNELS:
            assert (where, int(img_floats)) == KERNELS[tuple(widths)]
            assert (4 * int(img_floats) <= DenseScoringServer.LDS_IMAGE_BYTES) == (where == "lds")


def test_the_fleet_check_refuses_the_32nd_feature(checker):
    r = subprocess.run([checker], input="32,32 1\n31,31 1\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    why = [ln.split("\t")[0] for ln in r.stdout.splitlines()]
    assert "1..31 features" in why[0] and why[1] == "", r.stdout
