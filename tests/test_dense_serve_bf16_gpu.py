"""The bf16 per-event Dense scorer (dense_serve_bf16.hip, ``DenseScoringServer(precision="bf16")``) on the
wide bulk forward's cases, models and oracle (tests/test_dense_forward_wide_gpu.py: O is the float64
forward with both operands of every contraction rounded to bf16; its 203 rows are shared, computed once).

TOLERANCES.  The reconstruction chains are the bulk kernel's, so TOL_R and TOL_S are that file's, quoted.
A score is an fp32 sum of at most 32 non-negative terms and a divide over the kernel's own fp32 y and xn:
below 34 x 2^-24, about 2e-6, of the float64 value; the bound is 1e-5."""
import json
import time

import numpy as np
import pytest
import torch

from test_dense_forward_wide_gpu import TOL_R, TOL_S, _model, _reference
from helpers.dense_serve_ref import relerr

pytestmark = pytest.mark.gpu

N = 203
CASES = ["18-512-512-512-18", "30-129-30", "32-500-33-144-32", "eight_layers", "7-7", "no_bias_dropout"]
LDS = {"18-512-512-512-18": "bf16-stream", "30-129-30": "bf16-lds", "7-7": "bf16-lds"}


def _server(name, thr=5.0, **kw):
    from streamml.ops.serve import DenseScoringServer
    return DenseScoringServer(_model(name), threshold=thr, slots=256, idle_seconds=0.05,
                              normalizer=_reference(name)[1], precision="bf16", **kw)


@pytest.mark.parametrize("name", CASES)
def test_against_the_bf16_oracle_and_the_bulk_kernels_bits(cuda_device, name):
    from streamml.ops import dense_forward_wide as dfww
    from streamml.ops.serve import DenseScoringServer
    raw, arg, xn, y, ref = (a if isinstance(a, (str, tuple)) else a[:N] for a in _reference(name))
    thr = float(np.median(ref))
    with _server(name, thr) as srv:
        assert srv.precision == "bf16"
        assert srv.kernel == DenseScoringServer.kernel_for(_model(name), precision="bf16") == LDS.get(name, srv.kernel)
        s, f, r = srv.infer(raw)
        assert srv.events == N
    # 1. the oracle
    e_r, e_s = relerr(r, y), float(np.max(np.abs(s - ref) / ref))
    near = np.abs(ref - thr) <= TOL_S * thr
    print(f"{name}: reconstruction {e_r:.2e}, score {e_s:.2e}, flagged {int(f.sum())}/{N}, near {int(near.sum())}")
    assert r.shape == y.shape and e_r <= TOL_R and e_s <= TOL_S
    assert near.sum() <= 0.05 * N and np.array_equal(f[~near], (ref > thr)[~near])
    # 2. the bulk kernel's bits; the score from the kernel's own fp32 y and xn
    rb, _, _ = dfww.forward(_model(name), torch.from_numpy(raw).to(cuda_device), rec=True, normalizer=arg)
    assert np.array_equal(r.view(np.uint32), rb.cpu().numpy().view(np.uint32))
    xn32 = xn.astype(np.float32)   # fmaf(x, scale, shift): the float64 product is exact, one rounding each
    own = ((r.astype(np.float64) - xn32.astype(np.float64)) ** 2).mean(axis=1)
    assert float(np.max(np.abs(s - own) / own)) <= 1e-5


@pytest.mark.parametrize("name", ["18-512-512-512-18", "32-500-33-144-32"])
def test_batching_does_not_change_bits(cuda_device, name):
    """Rows one at a time at a low rate (every pass has E = 1) and the same rows as one backlog picked up by
    a relaunched kernel (16-column passes): the same bits."""
    raw = _reference(name)[0][:N]
    with _server(name) as srv:
        srv.latency_us(raw[:40], qps=2000.0)
        assert srv.passes == 40 and srv.events == 40
        one = [srv.infer(raw[i:i + 1]) for i in range(N)]
        assert srv.passes == 40 + N
        time.sleep(0.5)            # the kernel leaves after 0.05 s without a request
        launches, passes, events = srv.launches, srv.passes, srv.events
        s16, f16, r16 = srv.infer(raw)   # every row and the head are published before the relaunch
        assert srv.launches == launches + 1, "the kernel had not left: the backlog was not forced"
        mean = (srv.events - events) / (srv.passes - passes)
        print(f"{name}: {srv.passes - passes} passes, mean pass size {mean:.1f}")
        assert srv.events - events == N and mean > 8
    s1, f1, r1 = (np.concatenate([o[k] for o in one]) for k in range(3))
    assert np.array_equal(s1.view(np.uint32), s16.view(np.uint32))
    assert np.array_equal(f1, f16)
    assert np.array_equal(r1.view(np.uint32), r16.view(np.uint32))


@pytest.mark.parametrize("mode", ["low_latency", "chunked"])
def test_serve_cli_precision_bf16(cuda_device, tmp_path, capsys, mode):
    """``serve --model dense --precision bf16`` over a synthetic topic: every record's score is the one
    ``DenseScoringServer(precision="bf16").score`` gives the decoded row; the default still reports fp32."""
    from streamml.cli.__main__ import main as cli_main
    from streamml.data.stream import kafka
    from streamml.ops.serve import DenseScoringServer
    from test_dense_serve_gpu import _read_topic, _saved_model
    m = _saved_model(tmp_path, cuda_device)   # 18-64-16-64-18 as wide_ae.h5
    got = {}
    for precision in ("bf16", None):
        topic, out = f"SENSOR_BF16_{mode.upper()}_{precision}", f"preds-bf16-{mode}-{precision}"
        argv = ["serve", "synthetic://300", topic, out, "wide_ae.h5", "--workdir", str(tmp_path), "--device",
                str(cuda_device), "--model", "dense", "--synthetic-partitions", "1", "--idle-timeout", "0.3"]
        argv += ["--low-latency", "--max-wait-ms", "20"] if mode == "low_latency" else []
        argv += ["--precision", precision] if precision else []
        assert cli_main(argv) == 0
        summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert summary["events"] == 300 and summary["model"] == "dense"
        got[precision] = summary["kernel"]
        if precision:
            recs = _read_topic(f"fake://synthetic-{topic}", out)
            src = next(iter(kafka(f"fake://synthetic-{topic}", [f"{topic}:0:0"]).batch(1 << 20)))
            with DenseScoringServer(m, normalizer="cardata", idle_seconds=0.05, precision="bf16") as srv:
                want, _ = srv.score(np.asarray(src.x, np.float32))
            assert len(recs) == 300 and [r["offset"] for r in recs] == list(range(300))
            assert np.array_equal(np.array([r["score"] for r in recs], np.float32).view(np.uint32), want.view(np.uint32))
    assert got == {"bf16": "bf16-lds", None: "lds"}
