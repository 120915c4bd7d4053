"""Which ``ae_train_kernel`` instance ``ae_train_launch`` picks, checked on the CPU:
``csrc/tests/ae_variant_select.cpp`` walks a fixed grid of launch requests and ``SML_AE_*`` knob
settings through ``ae_train_select`` (``csrc/include/sml_ae_variants.h``) and prints, per case, the
variant's name, its eleven values, the grid it gets and what ``ae_train_last_variant`` reports, or
``REFUSE``.  ``tests/golden/ae_variant_select.txt`` is the same walk recorded from the nested
``if / else`` chain the table replaced (that launcher's text compiled unmodified against host stubs
that print the instance each launch site names), so a changed choice fails here, without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ae_variant_select.txt")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")   # the host compiler the package itself is built with
    exe = str(tmp_path_factory.mktemp("ae_variant_select") / "ae_variant_select")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(PKG, "csrc", "include"),
                    os.path.join(PKG, "csrc", "tests", "ae_variant_select.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


def test_choice_matches_the_recorded_chain(walker):
    r = subprocess.run([walker], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(got) == len(want)
    wrong = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not wrong, "%d lines differ; first (line %d):\nwant %s\ngot  %s" % ((len(wrong),) + wrong[0])


def test_every_table_row_is_chosen(walker):
    table = subprocess.run([walker, "-t"], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    rows = [ln.split()[0] for ln in table]
    assert len(rows) == len(set(rows)) and rows
    values = [ln.split()[1] for ln in table]
    assert len(values) == len(set(values)), "two rows with the same eleven values"
    with open(GOLDEN) as f:
        chosen = set(re.findall(r"-> (\w+) <", f.read()))
    assert chosen == set(rows), "rows no request reaches: %s" % sorted(set(rows) - chosen)
