"""The lane-masked transposed-read address table (``tr_rd_off_half``, ``csrc/include/sml_common.h``)
checked on the CPU: ``csrc/tests/tr_mask_table.cpp`` emulates ``ds_read_b64_tr_b16`` over a
workgroup's transpose slots and the cell area laid out as the ``XP 5`` packed-pair train kernel lays
them out, and holds the reads through the two masked addresses to the selects they replace, for
every lane, the bias cell of the ``xub`` slot included.  A wrong cell address fails here, without a GPU."""
import os
import shutil
import subprocess

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "hivemq-mqtt-tensorflow-kafka-realtime-iot-machine-learning-training-inference_amd")


def test_masked_read_addresses_match_the_selects(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "tr_mask_table")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-I", os.path.join(PKG, "csrc", "include"),
                    os.path.join(PKG, "csrc", "tests", "tr_mask_table.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "PASS tr_mask_table: 0 mismatches, 0 out-of-range" in r.stdout
