"""Persistent Dense scorer (dense_serve.hip) against the float64 reference of
tests/helpers/dense_serve_ref.py, against itself under different batching (bit for bit), and
against the one-wave scorer on the reference shape; then through the low-latency loop and the
``serve --model dense`` command."""
import functools
import json
import time

import numpy as np
import pytest
import torch

from helpers.dense_serve_ref import forward, relerr, score
from streamml import nn
from streamml.data.cardata import normalize_affine
from streamml.nn.layers import Dense, Dropout

pytestmark = pytest.mark.gpu

THR = 90.0      # the float64 scores of these inputs straddle it, so both flags occur
N = 203
TOL = 1e-4      # what tests/test_serve_gpu.py holds the fp32 one-wave scorer to, same act_fwd

#         widths, activations, features
CASES = {
    "18-33-18": ([33, 18], ["tanh", "relu"], 18),                                  # first width past the old limit
    "18-64-16-64-18": ([64, 16, 64, 18], ["tanh", "relu", "tanh", "linear"], 18),  # lds; k slices
    "18-130-40-130-18": ([130, 40, 130, 18], ["relu", "relu", "relu", "sigmoid"], 18),   # ragged widths
    "18-512-18": ([512, 18], ["tanh", "linear"], 18),                              # maximum width
    "18-512-512-18": ([512, 512, 18], ["tanh", "relu", "linear"], 18),             # stream
    "eight_layers": ([24, 16, 12, 8, 12, 16, 24, 18], ["tanh"] * 7 + ["linear"], 18),
    "one_layer_32": ([32], ["linear"], 32),                                        # the slot's last word
    "no_bias_dropout": None,                                                       # bias-less layer; identity Dropout
}


def _model(name, dev):
    if name == "no_bias_dropout":
        m = nn.Sequential([Dense(40, "relu", use_bias=False, input_shape=(18,)), Dropout(0.3), Dense(18, "linear")],
                          device=dev, seed=13)
    else:
        widths, acts, feat = CASES[name]
        m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                           for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=13)
    # Keras initialises biases to zero, which would hide a misplaced bias: draw them
    rng = np.random.default_rng(13)
    m.set_weights([w if w.ndim == 2 else rng.uniform(-0.5, 0.5, w.shape).astype(np.float32)
                   for w in m.get_weights()])
    return m


def _features(name):
    return 32 if name == "one_layer_32" else 18


@functools.lru_cache(maxsize=None)
def _rows(features):
    return np.random.default_rng(13).uniform(0, 40, (N, features)).astype(np.float32)


def _normalised(raw):
    if raw.shape[1] != 18:
        return raw.astype(np.float64)
    sc, sh = normalize_affine()
    return raw.astype(np.float64) * np.float32(sc) + np.float32(sh)


@functools.lru_cache(maxsize=None)
def _run(name):
    """One server per case: (kernel, expected kernel, scores, flags, reconstructions, float64
    reconstructions, float64 scores)."""
    from streamml.ops.serve import DenseScoringServer, dense_layer_table
    m = _model(name, torch.device("cuda", 0))
    raw = _rows(_features(name))
    with DenseScoringServer(m, threshold=THR, slots=256,
                            normalizer="cardata" if raw.shape[1] == 18 else None) as srv:
        kernel = srv.kernel
        s, f, r = srv.infer(raw)
    layers, weights = dense_layer_table(m)
    xn = _normalised(raw)
    y = forward(layers, weights, xn)
    return kernel, DenseScoringServer.kernel_for(m), s, f, r, y, score(y, xn)


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_float64_reference(cuda_device, name):
    kernel, want_kernel, s, f, r, y, ref = _run(name)
    assert kernel == want_kernel
    assert np.all(np.linalg.norm(y, axis=1) > 0)   # the relative error below is defined
    e_r, e_s = relerr(r, y), float(np.max(np.abs(s - ref) / ref))
    print(f"{name}: kernel {kernel}, reconstruction {e_r:.2e}, score {e_s:.2e}, flagged {int(f.sum())}/{N}")
    assert s.shape == (N,) and f.shape == (N,) and r.shape == y.shape
    assert e_r <= TOL
    assert e_s <= TOL
    near = np.abs(ref - THR) <= TOL * THR
    assert np.array_equal(f[~near], (ref > THR)[~near])


def test_kernels_cover_both_placements(cuda_device):
    assert _run("18-64-16-64-18")[0] == "lds" and _run("18-512-512-18")[0] == "stream"


@pytest.mark.parametrize("name", ["18-64-16-64-18", "18-512-512-18"])
def test_batching_does_not_change_bits(cuda_device, name):
    """One row per call (E = 1) against one backlog of 203 rows picked up by a relaunched kernel
    (25 passes of 8 events and one of 3): the same bits."""
    from streamml.ops.serve import DenseScoringServer
    m = _model(name, cuda_device)
    raw = _rows(18)
    with DenseScoringServer(m, threshold=THR, slots=256, idle_seconds=0.05, normalizer="cardata") as srv:
        one = [srv.infer(raw[i:i + 1]) for i in range(N)]
        assert srv.passes == N and srv.events == N
        s1 = np.concatenate([o[0] for o in one])
        f1 = np.concatenate([o[1] for o in one])
        r1 = np.concatenate([o[2] for o in one])
        time.sleep(0.5)            # the kernel leaves after 0.05 s without a request
        launches, passes = srv.launches, srv.passes
        s8, f8, r8 = srv.infer(raw)   # every row and the head are published before the relaunch
        assert srv.launches == launches + 1, "the kernel had not left: the backlog was not forced"
        assert srv.passes - passes == -(-N // 8) == 26
        assert srv.events == 2 * N
    assert np.array_equal(s1.view(np.uint32), s8.view(np.uint32))
    assert np.array_equal(f1, f8)
    assert np.array_equal(r1.view(np.uint32), r8.view(np.uint32))
    # and both equal the cached run of the case (a third batching: whatever the ring did)
    _, _, s, f, r, _, _ = _run(name)
    assert np.array_equal(s.view(np.uint32), s8.view(np.uint32))
    assert np.array_equal(r.view(np.uint32), r8.view(np.uint32))


def test_word_31_is_a_feature_in_every_batching(cuda_device):
    """Rows of 32 features: request word 31 is the last feature here (the fleet scorer reads a model
    index there).  Nine rows one per call and the same nine in one call (a backlog: the other waves
    fetch rows 1..7) give the same bits, within TOL of the float64 reference."""
    from streamml.ops.serve import DenseScoringServer, dense_layer_table
    m = _model("one_layer_32", cuda_device)
    raw = _rows(32)[:9]
    with DenseScoringServer(m, threshold=THR, slots=256) as srv:
        one = [srv.infer(raw[i:i + 1]) for i in range(9)]
        assert srv.passes == 9 and srv.events == 9
        s9, f9, r9 = srv.infer(raw)
        print(f"one_layer_32: 9 rows in one call took {srv.passes - 9} passes")
        assert srv.events == 18
    s1, f1, r1 = (np.concatenate([o[k] for o in one]) for k in range(3))
    assert np.array_equal(s1.view(np.uint32), s9.view(np.uint32))
    assert np.array_equal(f1, f9)
    assert np.array_equal(r1.view(np.uint32), r9.view(np.uint32))
    layers, weights = dense_layer_table(m)
    xn = _normalised(raw)
    y = forward(layers, weights, xn)
    ref = score(y, xn)
    assert np.any(raw[:, 31] != 0) and relerr(r9, y) <= TOL and float(np.max(np.abs(s9 - ref) / ref)) <= TOL


def test_reference_shape_matches_the_one_wave_scorer(cuda_device):
    from streamml.models.autoencoder import Autoencoder
    from streamml.ops.serve import DenseScoringServer, ScoringServer
    m = Autoencoder(18, 14, 7, device=cuda_device, seed=13, input_normalizer="cardata")
    raw = _rows(18)
    with ScoringServer(m, threshold=THR, slots=256) as srv:
        s0, f0, r0 = srv.infer(raw)
    with DenseScoringServer(m, threshold=THR, slots=256) as srv:   # the model's own normaliser
        assert srv.kernel == "lds"
        s1, f1, r1 = srv.infer(raw)
    np.testing.assert_allclose(s1, s0, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r1, r0, rtol=1e-5, atol=1e-6)


def test_low_latency_loop_end_to_end(cuda_device):
    """tests/test_serve_gpu.py::test_low_latency_loop_end_to_end with a wide stack.  Every
    record equals the server's own ``infer`` result for that row exactly: the score bit for bit
    (the record carries its shortest round-trip text) and the whole record, reconstruction
    included, byte for byte against the same formatter over ``infer``'s values."""
    import threading

    from streamml.data import stream as S
    from streamml.data.avro import AvroCodec
    from streamml.data.produce import encode_chunk
    from streamml.kafka import fake_broker
    from streamml.kafka.scoreloop import LowLatencyScorer, paced_produce
    from streamml.ops import load_io
    from streamml.ops.serve import DenseScoringServer

    name = "gpu-lowlat-dense"
    b = fake_broker(name)
    b.create_topic("SENSOR", 1)
    b.create_topic("RESULTS", 1)
    c = next(iter(S.synthetic(600, chunk=600, seed=5, failure_rate=0.05)))
    buf, offs = encode_chunk(AvroCodec("cardata-v1"), c.x, c.label)
    keys = [f"car{i % 17}" for i in range(600)]
    m = _model("18-64-16-64-18", cuda_device)
    with DenseScoringServer(m, threshold=0.5, slots=256, normalizer="cardata") as srv:
        ref_s, ref_f, ref_r = srv.infer(c.x)
        loop = LowLatencyScorer(f"fake://{name}", "SENSOR", "RESULTS", [0], srv, starts=[0], emit_recon=True,
                                max_wait_ms=50, record_latency=True)
        out = {}
        th = threading.Thread(target=lambda: out.update(loop.run(max_events=600, idle_timeout_s=10.0)))
        th.start()
        paced_produce(f"fake://{name}", "SENSOR", 0, bytes(buf), offs, keys=keys, qps=5000.0)
        th.join(60)
    assert not th.is_alive() and out["events"] == 600
    res = b.read("RESULTS", 0, 0)
    assert len(res) == 600
    want = load_io().score_records(keys, 0, np.arange(600, dtype=np.int64), ref_s, ref_f.astype(np.uint8), ref_r)
    for off, key, val in res:
        d = json.loads(val)
        i = d["offset"]
        assert key.decode() == keys[i] == d["car"]
        assert np.float32(d["score"]).view(np.uint32) == ref_s[i].view(np.uint32)
        assert d["anomaly"] == bool(ref_f[i])
        assert bytes(val) == bytes(want[i])
        assert set(d) == {"car", "partition", "offset", "score", "anomaly", "reconstruction"}


def _saved_model(tmp_path, dev):
    m = _model("18-64-16-64-18", dev)
    m.compile(fused=False)
    m.save(str(tmp_path / "wide_ae.h5"))
    return m


def _read_topic(servers, topic):
    from streamml.kafka import KafkaClient
    c = KafkaClient(servers)
    pos, recs = 0, []
    while True:
        b = c.fetch(topic, 0, pos, 1 << 22, 10)
        if len(b["offsets"]) == 0:
            return recs
        vals, vo = b["values"], b["value_offsets"]
        recs += [json.loads(vals[vo[i]:vo[i + 1]]) for i in range(len(vo) - 1)]
        pos = int(b["offsets"][-1]) + 1


@pytest.mark.parametrize("mode", ["low_latency", "chunked"])
def test_serve_cli_scores_a_wide_model(cuda_device, tmp_path, capsys, mode):
    """``serve --model dense`` (``--low-latency``, and the chunked path with ``--emit both``) on an
    ``.h5`` saved from ``nn.Sequential`` 18-64-16-64-18, which ``models.autoencoder.load_model``
    refuses: 600 records, scores within 1e-4 of the float64 reference on the decoded rows."""
    from streamml.cli.__main__ import main as cli_main
    from streamml.data.stream import kafka
    from streamml.ops.serve import dense_layer_table
    m = _saved_model(tmp_path, cuda_device)
    topic, out = f"SENSOR_DENSE_{mode.upper()}", f"preds-dense-{mode}"
    argv = ["serve", "synthetic://600", topic, out, "wide_ae.h5", "--workdir", str(tmp_path), "--device",
            str(cuda_device), "--model", "dense", "--synthetic-partitions", "1", "--idle-timeout", "0.3",
            "--threshold", str(THR)]
    argv += ["--low-latency", "--max-wait-ms", "20"] if mode == "low_latency" else ["--emit", "both"]
    assert cli_main(argv) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["events"] == 600 and summary["model"] == "dense"
    servers = f"fake://synthetic-{topic}"
    recs = _read_topic(servers, out)
    assert len(recs) == 600 and [r["offset"] for r in recs] == list(range(600))
    src = next(iter(kafka(servers, [f"{topic}:0:0"]).batch(1 << 20)))
    layers, weights = dense_layer_table(m)
    xn = _normalised(np.asarray(src.x, np.float32))
    y = forward(layers, weights, xn)
    ref = score(y, xn)
    got = np.array([r["score"] for r in recs])
    assert float(np.max(np.abs(got - ref) / ref)) <= TOL
    near = np.abs(ref - THR) <= TOL * THR
    assert np.array_equal(np.array([r["anomaly"] for r in recs])[~near], (ref > THR)[~near])
    if mode == "chunked":
        rec = np.array([np.array(r["reconstruction"].strip("[]").split(), dtype=np.float64) for r in recs])
        assert np.all(np.linalg.norm(rec - y, axis=1) <= 1e-4 * np.linalg.norm(y, axis=1) + 18 ** 0.5 * 5e-9)


def test_native_constructor_names_the_limit(cuda_device):
    """``_C.DenseServe`` itself (below ``DenseScoringServer.supports``) refuses a 513-unit layer
    and a ninth layer with the limit in the message, before it allocates anything."""
    from streamml.ops import load_c
    from streamml.ops.serve import dense_serve_image
    C = load_c()
    rng = np.random.default_rng(0)

    def build(widths):
        dims = [18] + widths
        layers = [(i, o, "tanh", True) for i, o in zip(dims[:-1], dims[1:])]
        ws = [(rng.uniform(-1, 1, (i, o)).astype(np.float32), np.zeros(o, np.float32)) for i, o, _, _ in layers]
        image, table = dense_serve_image(layers, ws)
        return C.DenseServe(0, 256, image, [list(t) for t in table], 18, None, None, 5.0, 0.5)

    with pytest.raises(Exception, match="512"):
        build([513, 18])
    with pytest.raises(Exception, match="8 Dense layers"):
        build([20] * 8 + [18])
    with pytest.raises(Exception, match="one unit per feature"):
        build([20, 17])
