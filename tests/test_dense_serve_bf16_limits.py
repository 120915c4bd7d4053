"""The bf16 per-event Dense scorer's limits, checked without a device: ``DenseScoringServer.supports`` /
``kernel_for(precision="bf16")`` against the host program over ``sml_dense_serve_bf16.h``
(``dense_serve_bf16_check``, ``dense_serve_bf16_plan``): the Python mirror and the C++ check must decide
alike and name the same limit; the unknown precision; the CLI's ``--precision`` guard."""
import os
import subprocess

import pytest

import streamml
from streamml import nn
from streamml.nn.layers import Dense
from streamml.ops import dense_forward_wide as dfww
from streamml.ops.serve import DenseScoringServer, dense_layer_table

PKG = os.path.dirname(os.path.abspath(streamml.__file__))


def _tanh_stack(widths):
    return nn.Sequential([Dense(u, "tanh", input_shape=(widths[0],) if i == 0 else None)
                          for i, u in enumerate(widths[1:])], device="cpu", seed=0)


#          widths, what the refusal names ("" = served)
SHAPES = [
    ([18, 512, 512, 512, 18], ""),
    ([18, 256, 64, 256, 18], ""),
    ([32, 32], ""),
    ([33, 64, 33], "1..32 features"),
    ([18, 513, 18], "513 units: the limit is 512"),
    ([18] + [20] * 8 + [18], "9 Dense layers"),
    ([18, 64, 17], "one unit per feature"),
    # the two sides of DSVB_LDS_IMAGE_BYTES = 124 928 bytes = 62 464 words: 20-256-h-20 packs into
    # 8 768 + 258 pad16(h) + 32 pad32(h) words
    ([20, 256, 176, 20], ""),
    ([20, 256, 177, 20], ""),
]
KERNELS = {(18, 512, 512, 512, 18): "bf16-stream", (18, 256, 64, 256, 18): "bf16-lds",
           (20, 256, 176, 20): ("bf16-lds", 60320), (20, 256, 177, 20): ("bf16-stream", 64448)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")   # the host compiler the package itself is built with
    exe = str(tmp_path_factory.mktemp("dense_serve_bf16_check") / "dense_serve_bf16_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc", "include"),
                    os.path.join(PKG, "csrc", "tests", "dense_serve_bf16_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=120)
    return exe


def test_host_checker_agrees_with_supports_and_kernel_for(checker):
    text = "".join(",".join(map(str, w)) + "\n" for w, _ in SHAPES)
    r = subprocess.run([checker], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert len(got) == len(SHAPES)
    for (widths, names), (why_c, words, where, lds_bytes) in zip(SHAPES, got):
        model = _tanh_stack(widths)
        ok, why_py = DenseScoringServer.supports(model, precision="bf16")
        # the decision, and the limit both name (Python adds the offending numbers to the serving rules)
        assert ok == (why_c == "") == (names == ""), (widths, why_c, why_py)
        assert names in why_c and names in why_py, (widths, why_c, why_py)
        if ok:
            assert dfww.image_table(dense_layer_table(model)[0])[1] == int(words)
            assert DenseScoringServer.kernel_for(model, precision="bf16") == where, (widths, words, where)
            assert (2 * int(words) <= DenseScoringServer.LDS_IMAGE_BYTES_BF16) == (where == "bf16-lds")
            assert int(lds_bytes) + 5120 <= 160 * 1024   # the plan with DSVB_STATIC_LDS beside it
        want = KERNELS.get(tuple(widths))
        if want is not None:
            assert (where, int(words)) == want or where == want


def test_constants_are_the_headers(checker):
    r = subprocess.run([checker, "-c"], capture_output=True, text=True, timeout=60)
    c = dict(ln.split() for ln in r.stdout.splitlines())
    assert (int(c["DSVB_EB"]), int(c["DSVB_MAXD"]), int(c["DSVB_LDS_IMAGE_BYTES"])) == (
        DenseScoringServer.MAX_PASS_BF16, DenseScoringServer.MAX_FEATURES, DenseScoringServer.LDS_IMAGE_BYTES_BF16)
    assert int(c["DSVB_STATIC_LDS"]) == 5120 and int(c["DSVB_NT"]) == 1024


def test_default_precision_keeps_the_fp32_answers():
    m = _tanh_stack([18, 256, 64, 256, 18])
    assert DenseScoringServer.kernel_for(m) == DenseScoringServer.kernel_for(m, precision="fp32") == "stream"
    assert DenseScoringServer.supports(m) == DenseScoringServer.supports(m, "fp32") == (True, "")


def test_unknown_precision_is_a_value_error():
    m = _tanh_stack([18, 64, 18])
    for call in (lambda: DenseScoringServer.supports(m, precision="fp16"),
                 lambda: DenseScoringServer.kernel_for(m, precision="fp16"),
                 lambda: DenseScoringServer(m, precision="fp16", device="cpu")):
        with pytest.raises(ValueError, match="precision must be 'fp32' or 'bf16'"):
            call()


def test_cli_precision_goes_with_model_dense(tmp_path):
    from streamml.cli.__main__ import main as cli_main
    with pytest.raises(SystemExit, match="--precision goes with --model dense"):
        cli_main(["serve", "synthetic://100", "SENSOR_BF16_CPU", "preds-bf16-cpu", "none.h5", "--workdir", str(tmp_path),
                  "--device", "cpu", "--model", "lstm", "--precision", "bf16"])
