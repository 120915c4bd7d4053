"""bench.py's plain run: the headline alone, and ``--dump-outputs``.

A run without ``--full`` times its K steps and prints the headline line with none of the side
measurements; ``--dump-outputs DIR`` writes the state the last timed step left.  The train step has
no float atomics (ae_fused.hip: every slab is written once, reduced in a fixed order) and the dump
run starts its W + K steps from the seeded model, so two runs with the same arguments must write
the same bytes.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("params", "adam_m", "adam_v", "metrics", "counters")
SIDE_KEYS = ("phase_s", "budget", "infer", "p50_infer_us", "keras_batch32", "kafka_e2e", "fit_batch100",
             "stream_e2e", "lstm_seq50", "mqtt_e2e")


def _plain(dump, steps=5, warmup=2):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("SML_SHARE_GPU0", "SML_FORCE_PG", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--batch-per-gpu", "65536", "--dataset-rows", "262144", "--dump-outputs", dump]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    return json.loads(lines[0])


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sml_bench_plain", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_options_default_to_a_plain_run(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_the_step_state(tmp_path):
    """One float32 / float64 ``.npy`` per array of the state, values unchanged (CPU stand-in)."""
    import types

    import torch
    g = torch.Generator().manual_seed(0)
    fused = types.SimpleNamespace(params=torch.randn(600, generator=g), m=torch.randn(600, generator=g),
                                  v=torch.rand(600, generator=g), metrics=torch.tensor([1.5, 2.5, 3.0, 4.0]),
                                  iter=torch.tensor([25]), cursor=torch.tensor([3 << 25]))
    d = str(tmp_path / "new" / "dir")
    _bench().dump_outputs(d, fused)
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    for n, t in (("params", fused.params), ("adam_m", fused.m), ("adam_v", fused.v)):
        assert got[n].dtype == np.float32
        np.testing.assert_array_equal(got[n], t.numpy())
    assert got["metrics"].dtype == np.float64 and got["metrics"].tolist() == [1.5, 2.5, 3.0, 4.0]
    assert got["counters"].dtype == np.float64 and got["counters"].tolist() == [25.0, float(3 << 25)]


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_repeatably(tmp_path, cuda_device):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = _plain(a)
    assert out["steps"] == 5 and out["warmup"] == 2 and out["n_gpus"] == 1
    assert out["unit"] == "rows/s" and out["dtype"] == "bf16" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(65536 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert out["summary"] == {"headline_rows_per_s": float(f"{out['value']:.4g}")}
    assert not [k for k in SIDE_KEYS if k in out], sorted(out)
    _plain(b)
    total = 0
    for name in NAMES:
        x, y = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), (name, x.dtype)
        np.testing.assert_array_equal(x, y, err_msg=name)
        total += x.nbytes
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in NAMES) and total <= 64 << 20
    # W + K optimizer steps from the seeded model, each consuming one batch of the 4-batch ring
    steps, cursor = np.load(os.path.join(a, "counters.npy"))
    assert steps == 7 and cursor == (7 % 4) * 65536
    rows = np.load(os.path.join(a, "metrics.npy"))[3]
    assert rows == 7 * 65536
    assert np.abs(np.load(os.path.join(a, "adam_v.npy"))).max() > 0
