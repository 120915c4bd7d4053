"""The persistent Dense trainer's limits and LDS plans exist twice: in C++
(``csrc/include/sml_dense_mb_plan.h``: ``dense_mb_check``, ``dense_mb_plan``, ``dense_mb_plan_bf16``),
which the launchers and the binding use, and in Python (``ops/dense_persistent.py``), which must
answer without a built extension.  ``csrc/tests/dense_mb_plan_walk.cpp`` is a host program over the
header; this test feeds it shapes and holds the two copies together on the CPU: the same refusal,
byte for byte, the same LDS bytes, the same constants."""
import os
import subprocess

import pytest

from helpers import dense_mb_bf16_cases as bf16_cases
from helpers import dense_mb_cases as cases
from streamml.ops import dense_persistent as dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd")

NINE = [18] + [20] * 8 + [18]
# (widths, batch, own targets)
SHAPES = (
    list(cases.SHAPES)
    # every trained case of the fp32 and the bf16 GPU tests
    + [(bf16_cases.case(n)[0], bf16_cases.case(n)[2], bool(bf16_cases.case(n)[4].get("own_y"))) for n in bf16_cases.NAMES]
    # what test_python_bf16_limits_agree_with_the_cpp_check adds to cases.SHAPES
    + [([64, 128, 64], 32, False), ([65, 113, 65], 32, False), ([18, 129, 18], 32, False), (NINE, 32, False),
       ([18, 33, 18], 0, False), ([18, 33, 18], 129, False), ([30, 128, 32, 128, 30], 128, True)]
    # the limit cases of tests/test_dense_minibatch_bf16_limits.py not yet among them
    + [([30, 128, 32, 128, 30], 32, False), ([18, 64, 16, 64, 18], 100, False), ([30, 128, 32, 128, 30], 128, False)]
)


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")   # the host compiler the package itself is built with
    exe = str(tmp_path_factory.mktemp("dense_mb_plan_walk") / "dense_mb_plan_walk")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(PKG, "csrc", "include"),
                    os.path.join(PKG, "csrc", "tests", "dense_mb_plan_walk.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=120)
    return exe


def test_check_and_lds_bytes_match_python(walker):
    text = "".join("%s %d %d\n" % (",".join(map(str, w)), b, own) for w, b, own in SHAPES)
    r = subprocess.run([walker], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert len(got) == 2 * len(SHAPES)
    answers = {"fp32": [], "bf16": []}
    for i, (widths, batch, own) in enumerate(SHAPES):
        for (prec, why, nbytes), want in zip(got[2 * i:2 * i + 2], ("fp32", "bf16")):
            assert prec == want
            assert why == dp.check_shape(list(widths), batch, own, precision=prec), (widths, batch, own, prec)
            if why == "":
                assert int(nbytes) == dp.lds_bytes(list(widths), own, precision=prec), (widths, own, prec)
            answers[prec].append(why)
    # the walk meets every limit, and stacks that pass, in both precisions
    for word in ("MAX_LAYERS", "MAX_BATCH", "MAX_WIDTH", "MAX_PARAMS)", "LDS_BYTES", "y = x"):
        assert any(word in a for a in answers["fp32"]), word
    for word in ("MAX_LAYERS", "MAX_BATCH", "MAX_WIDTH", "MAX_PARAMS_BF16", "y = x"):
        assert any(word in a for a in answers["bf16"]), word
    assert sum(a == "" for a in answers["fp32"]) >= 8 and sum(a == "" for a in answers["bf16"]) >= 8


def test_constants_match_python(walker):
    out = subprocess.run([walker, "-c"], capture_output=True, text=True, timeout=60, check=True).stdout
    c = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert c == {
        "DMB_MAXLAYERS": dp.MAX_LAYERS, "DMB_MAXW": dp.MAX_WIDTH, "DMB_MAXBATCH": dp.MAX_BATCH, "DMB_NT": dp.THREADS,
        "DMB_TPT": dp.TILES_PER_THREAD, "DMB_CHUNK": dp.CHUNK, "DMB_MAXPARAMS": dp.MAX_PARAMS,
        "DMB_LDS_BYTES": dp.LDS_BYTES, "DMB_STATIC_LDS": dp._STATIC_LDS, "DMB_FP32": dp.PRECISION["fp32"],
        "DMB_BF16": dp.PRECISION["bf16"], "DMB_TILES_BF16": dp.TILES_BF16, "DMB_MAXPARAMS_BF16": dp.MAX_PARAMS_BF16,
    }
