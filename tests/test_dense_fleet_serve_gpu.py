"""The fleet scorer (dense_serve_fleet.hip, ops.serve.DenseFleetScoringServer): every event is
scored by the member it names.  The oracle is the single-model server (dense_serve.hip, itself held
to float64 by tests/test_dense_serve_gpu.py): the fleet's scores, flags and reconstructions must be
its bits exactly, whatever the ring batched and whichever models shared a pass.  Then per-model
thresholds, weight updates, the index check, the low-latency loop with a preset key table and the
``serve --model dense-fleet`` command."""
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
TOL = 1e-4      # the project's bound for the fp32 scorers against float64

#         widths, activations, features, members
CASES = {
    "18-33-18": ([33, 18], ["tanh", "relu"], 18, 5),
    "18-64-16-64-18": ([64, 16, 64, 18], ["tanh", "relu", "tanh", "linear"], 18, 5),
    "18-130-40-130-18": ([130, 40, 130, 18], ["relu", "relu", "relu", "sigmoid"], 18, 5),     # ragged widths
    "eight_layers": ([24, 16, 12, 8, 12, 16, 24, 18], ["tanh"] * 7 + ["linear"], 18, 5),
    "no_bias_dropout": (None, None, 18, 5),                                                   # bias-less layer
    "18-512-512-18": ([512, 512, 18], ["tanh", "relu", "linear"], 18, 3),                     # long slices
    "31-31": ([31], ["linear"], 31, 5),                    # the last feature sits next to the index word
}


def _member(name, dev, seed):
    widths, acts, feat, _ = CASES[name]
    if name == "no_bias_dropout":
        m = nn.Sequential([Dense(40, "relu", use_bias=False, input_shape=(18,)), Dropout(0.3), Dense(18, "linear")],
                          device=dev, seed=seed)
    else:
        m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                           for i, (u, a) in enumerate(zip(widths, acts))], device=dev, seed=seed)
    # Keras initialises biases to zero, which would hide a misplaced bias: draw them
    rng = np.random.default_rng(seed)
    m.set_weights([w if w.ndim == 2 else rng.uniform(-0.5, 0.5, w.shape).astype(np.float32)
                   for w in m.get_weights()])
    return m


def _members(name, dev=None):
    dev = torch.device("cuda", 0) if dev is None else dev
    return [_member(name, dev, 13 + j) for j in range(CASES[name][3])]


@functools.lru_cache(maxsize=None)
def _rows(features):
    return np.random.default_rng(13).uniform(0, 40, (N, features)).astype(np.float32)


def _index(M, pattern="mixed"):
    i = np.arange(N)
    return (7 * i) % M if pattern == "mixed" else (i // 8) % M   # runs of 8: every full pass names one model


def _normalizer(features):
    return "cardata" if features == 18 else None


def _normalised(raw):
    if raw.shape[1] != 18:
        return raw.astype(np.float64)
    sc, sh = normalize_affine()
    return raw.astype(np.float64) * np.float32(sc) + np.float32(sh)


def _single(model, raw, threshold=THR):
    """The oracle: one single-model server, opened and closed."""
    from streamml.ops.serve import DenseScoringServer
    with DenseScoringServer(model, threshold=threshold, slots=256, normalizer=_normalizer(raw.shape[1])) as srv:
        return srv.infer(raw)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _run(name):
    """One fleet server per case, then the single-model servers one after another: (scores, flags,
    reconstructions) of the fleet, the same assembled from the single servers, the float64
    reconstructions and scores, the index."""
    from streamml.ops.serve import DenseFleetScoringServer, dense_layer_table
    models = _members(name)
    M = len(models)
    raw = _rows(CASES[name][2])
    idx = _index(M)
    with DenseFleetScoringServer(models, thresholds=THR, slots=256, normalizer=_normalizer(raw.shape[1])) as srv:
        assert srv.kernel == "fleet" and srv.n_models == M
        s, f, r = srv.infer(raw, idx)
    s1, f1, r1 = np.empty_like(s), np.empty_like(f), np.empty_like(r)
    xn = _normalised(raw)
    y = np.empty(r.shape, np.float64)
    for j, m in enumerate(models):
        rows = np.flatnonzero(idx == j)
        s1[rows], f1[rows], r1[rows] = _single(m, raw[rows])
        layers, weights = dense_layer_table(m)
        y[rows] = forward(layers, weights, xn[rows])
    return (s, f, r), (s1, f1, r1), y, score(y, xn), idx


@pytest.mark.parametrize("name", list(CASES))
def test_bit_for_bit_against_the_single_model_server(cuda_device, name):
    (s, f, r), (s1, f1, r1), _, _, idx = _run(name)
    assert s.shape == (N,) and f.shape == (N,) and r.shape == (N, CASES[name][2])
    assert len(set(idx[:8].tolist())) > 1          # the passes mix models
    assert _bits_equal(s, s1)
    assert np.array_equal(f, f1)
    assert _bits_equal(r, r1)


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_float64_reference(cuda_device, name):
    (s, f, r), _, y, ref, _ = _run(name)
    assert np.all(np.linalg.norm(y, axis=1) > 0)   # the relative error below is defined
    e_r, e_s = relerr(r, y), float(np.max(np.abs(s - ref) / ref))
    print(f"{name}: reconstruction {e_r:.2e}, score {e_s:.2e}, flagged {int(f.sum())}/{N}")
    assert e_r <= TOL
    assert e_s <= TOL
    near = np.abs(ref - THR) <= TOL * THR
    assert np.array_equal(f[~near], (ref > THR)[~near])


@pytest.mark.parametrize("name,pattern", [("18-64-16-64-18", "mixed"), ("18-64-16-64-18", "runs"),
                                          ("18-512-512-18", "mixed"), ("18-130-40-130-18", "runs")])
def test_batching_does_not_change_bits(cuda_device, name, pattern):
    """One row per call (E = 1) against one backlog of 203 rows picked up by a relaunched kernel
    (25 passes of 8 events and one of 3): the same bits, with passes that mix models and with
    passes that each name one model."""
    from streamml.ops.serve import DenseFleetScoringServer
    models = _members(name, cuda_device)
    raw = _rows(18)
    idx = _index(len(models), pattern)
    with DenseFleetScoringServer(models, thresholds=THR, slots=256, idle_seconds=0.05, normalizer="cardata") as srv:
        one = [srv.infer(raw[i:i + 1], idx[i:i + 1]) for i in range(N)]
        assert srv.passes == N and srv.events == N
        s1 = np.concatenate([o[0] for o in one])
        f1 = np.concatenate([o[1] for o in one])
        r1 = np.concatenate([o[2] for o in one])
        time.sleep(0.5)            # the kernel leaves after 0.05 s without a request
        launches, passes = srv.launches, srv.passes
        s8, f8, r8 = srv.infer(raw, idx)   # every row and the head are published before the relaunch
        assert srv.launches == launches + 1, "the kernel had not left: the backlog was not forced"
        assert srv.passes - passes == -(-N // 8) == 26
        assert srv.events == 2 * N
    assert _bits_equal(s1, s8)
    assert np.array_equal(f1, f8)
    assert _bits_equal(r1, r8)
    if pattern == "mixed":   # and both equal the cached run of the case, whatever the ring did there
        (s, f, r), _, _, _, _ = _run(name)
        assert _bits_equal(s, s8) and _bits_equal(r, r8)


def test_per_model_thresholds(cuda_device):
    from streamml.ops.serve import DenseFleetScoringServer
    name = "18-64-16-64-18"
    _, _, _, ref, idx = _run(name)
    models = _members(name, cuda_device)
    M = len(models)
    raw = _rows(18)
    # each member's threshold is the median float64 score of its own rows
    thr = np.array([np.median(ref[idx == j]) for j in range(M)])
    assert len(set(thr.tolist())) == M
    with DenseFleetScoringServer(models, thresholds=thr, slots=256, normalizer="cardata") as srv:
        s, f = srv.score(raw, idx)
        # one row, every member: thresholds from that row's float64 score under each member
        from streamml.ops.serve import dense_layer_table
        xn = _normalised(raw[:1])
        own = np.array([score(forward(*dense_layer_table(m), xn), xn)[0] for m in models])
    near = np.abs(ref - thr[idx]) <= TOL * thr[idx]
    assert np.array_equal(f[~near], (ref > thr[idx])[~near])
    assert 0 < int(f.sum()) < N
    factor = np.where(np.arange(M) % 2 == 0, 0.5, 2.0)      # flags under members 0, 2, 4 and not under 1, 3
    with DenseFleetScoringServer(models, thresholds=own * factor, slots=256, normalizer="cardata") as srv:
        s, f = srv.score(np.repeat(raw[:1], M, axis=0), np.arange(M))
    assert np.max(np.abs(s - own) / own) <= TOL
    assert f.tolist() == [True, False, True, False, True]


def test_set_weights_and_refresh(cuda_device):
    from streamml.nn.model import Adam
    from streamml.ops.dense_fleet import DenseFleet
    from streamml.ops.serve import DenseFleetScoringServer
    name = "18-64-16-64-18"
    models = _members(name, cuda_device)
    raw = _rows(18)
    idx = _index(len(models))
    other = _member(name, cuda_device, 99)
    with DenseFleetScoringServer(models, thresholds=THR, slots=256, normalizer="cardata") as srv:
        s0, f0, r0 = srv.infer(raw, idx)
        launches = srv.launches
        srv.set_weights(2, other.get_weights())
        s1, f1, r1 = srv.infer(raw, idx)
        assert srv.launches == launches + 1      # stopped for the copy, relaunched by the next call
        assert srv.events == 2 * N
    keep = idx != 2
    assert _bits_equal(s0[keep], s1[keep]) and _bits_equal(r0[keep], r1[keep]) and np.array_equal(f0[keep], f1[keep])
    so, fo, ro = _single(other, raw[~keep])
    assert _bits_equal(s1[~keep], so) and _bits_equal(r1[~keep], ro) and np.array_equal(f1[~keep], fo)
    assert not _bits_equal(s0[~keep], s1[~keep])

    # refresh: a DenseFleet goes on training, the server takes its weights again
    for m in models:
        m.compile(optimizer=Adam(learning_rate=1e-2), loss="mse", metrics=["accuracy"], fused=False)
    fleet = DenseFleet(models, cuda_device)
    x = torch.rand((len(models), 64, 18), device=cuda_device, generator=None)
    fleet.attach_rows(x, 32)
    with fleet.server(thresholds=THR, slots=256, normalizer="cardata") as srv:
        sa, _, ra = srv.infer(raw, idx)
        assert _bits_equal(sa, s0) and _bits_equal(ra, r0)     # the fleet's flat is the members' weights
        fleet.train_steps(2)
        torch.cuda.synchronize()
        srv.refresh(fleet)
        sb, fb, rb = srv.infer(raw, idx)
    with DenseFleetScoringServer.from_fleet(fleet, thresholds=THR, slots=256, normalizer="cardata") as fresh:
        sc, fc, rc = fresh.infer(raw, idx)
    assert _bits_equal(sb, sc) and _bits_equal(rb, rc) and np.array_equal(fb, fc)
    assert not _bits_equal(sa, sb)


def test_index_out_of_range_is_refused_before_anything_is_published(cuda_device):
    from streamml.ops.serve import DenseFleetScoringServer
    name = "18-33-18"
    models = _members(name, cuda_device)
    M = len(models)
    raw = _rows(18)[:16]
    with DenseFleetScoringServer(models, thresholds=THR, slots=256, normalizer="cardata") as srv:
        good = srv.infer(raw, np.arange(16) % M)
        events = srv.events
        assert events == 16
        for bad in (M, 1 << 31, -1):
            idx = np.arange(16) % M
            idx[11] = bad
            with pytest.raises(ValueError, match=f"model index {bad} of row 11"):
                srv.infer(raw, idx)
            with pytest.raises(ValueError, match="model index"):
                srv.latency_us(raw, idx, qps=0)
        assert srv.events == events
        again = srv.infer(raw, np.arange(16) % M)
        assert srv.events == events + 16
    assert _bits_equal(good[0], again[0]) and _bits_equal(good[2], again[2])


def test_low_latency_loop_end_to_end(cuda_device):
    """tests/test_dense_serve_gpu.py::test_low_latency_loop_end_to_end on a fleet: 17 car keys mapped
    onto 5 members by a preset table, one unknown car dropped.  Every record is byte for byte the
    formatter over the fleet server's own ``infer``."""
    import threading

    from streamml.data import stream as S
    from streamml.data.avro import AvroCodec
    from streamml.data.produce import encode_chunk
    from streamml.kafka import fake_broker
    from streamml.kafka.scoreloop import LowLatencyScorer, paced_produce
    from streamml.ops import load_io
    from streamml.ops.serve import DenseFleetScoringServer

    name = "gpu-lowlat-dense-fleet"
    b = fake_broker(name)
    b.create_topic("SENSOR", 1)
    b.create_topic("RESULTS", 1)
    c = next(iter(S.synthetic(600, chunk=600, seed=5, failure_rate=0.05)))
    buf, offs = encode_chunk(AvroCodec("cardata-v1"), c.x, c.label)
    keys = [f"car{i % 18}" for i in range(600)]            # car17 is in no table
    table = {f"car{j}": (3 * j + 2) % 5 for j in range(17)}
    known = np.array([k in table for k in keys])
    n_known = int(known.sum())
    midx = np.array([table.get(k, 0) for k in keys])
    models = _members("18-64-16-64-18", cuda_device)
    with DenseFleetScoringServer(models, thresholds=0.5, slots=256, normalizer="cardata") as srv:
        ref_s, ref_f, ref_r = srv.infer(c.x, midx)
        loop = LowLatencyScorer(f"fake://{name}", "SENSOR", "RESULTS", [0], srv, starts=[0], emit_recon=True,
                                max_wait_ms=50, record_latency=True, key_table=table, unknown_key_id=-1)
        out = {}
        th = threading.Thread(target=lambda: out.update(loop.run(max_events=n_known, idle_timeout_s=10.0)))
        th.start()
        paced_produce(f"fake://{name}", "SENSOR", 0, bytes(buf), offs, keys=keys, qps=5000.0)
        th.join(60)
    assert not th.is_alive() and out["events"] == n_known
    assert out["keys_dropped"] >= 600 - n_known - 1      # the loop may stop before the last unknown record
    res = b.read("RESULTS", 0, 0)
    assert len(res) == n_known
    want = load_io().score_records(keys, 0, np.arange(600, dtype=np.int64), ref_s, ref_f.astype(np.uint8), ref_r)
    seen = []
    for off, key, val in res:
        d = json.loads(val)
        i = d["offset"]
        seen.append(i)
        assert key.decode() == keys[i] == d["car"] and known[i]
        assert np.float32(d["score"]).view(np.uint32) == ref_s[i].view(np.uint32)
        assert d["anomaly"] == bool(ref_f[i])
        assert bytes(val) == bytes(want[i])
    assert seen == np.flatnonzero(known).tolist()


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


@pytest.fixture(scope="module")
def fleet_dir(tmp_path_factory):
    """``fleet synthetic --layers 16 --models 4 --epochs 1`` on a few thousand rows."""
    from streamml.cli.__main__ import main as cli_main
    out = str(tmp_path_factory.mktemp("fleet_dir") / "fleet")
    assert cli_main(["fleet", "synthetic", "--layers", "16", "--models", "4", "--epochs", "1", "--synthetic-rows",
                     "4096", "--synthetic-devices", "400", "--out", out, "--device", "cuda:0"]) == 0
    return out


@pytest.mark.parametrize("mode", ["low_latency", "chunked"])
def test_serve_cli_scores_every_car_by_its_own_model(cuda_device, tmp_path, capsys, fleet_dir, mode):
    from streamml.cli.__main__ import main as cli_main
    from streamml.data.stream import kafka
    from streamml.nn.model import load_model
    from streamml.ops.serve import dense_layer_table, read_fleet_index
    capsys.readouterr()
    names, files, key_to_model = read_fleet_index(fleet_dir)
    assert len(names) == 4 and len(key_to_model) >= 4
    topic, out = f"SENSOR_FLEET_{mode.upper()}", f"preds-fleet-{mode}"
    argv = ["serve", "synthetic://600", topic, out, fleet_dir, "--workdir", str(tmp_path), "--device",
            str(cuda_device), "--model", "dense-fleet", "--synthetic-partitions", "1", "--idle-timeout", "0.3",
            "--threshold", str(THR)]
    argv += ["--low-latency", "--max-wait-ms", "20"] if mode == "low_latency" else ["--emit", "both"]
    assert cli_main(argv) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["model"] == "dense-fleet" and summary["models"] == 4 and "keys_dropped" in summary
    servers = f"fake://synthetic-{topic}"
    recs = _read_topic(servers, out)
    src = next(iter(kafka(servers, [f"{topic}:0:0"]).batch(1 << 20)))
    cars = [k.decode() if isinstance(k, bytes) else k for k in src.keys]
    known = np.array([k in key_to_model for k in cars])
    assert summary["events"] == len(recs) == int(known.sum()) and summary["keys_dropped"] == int((~known).sum())
    assert summary["events"] > 0
    assert [r["offset"] for r in recs] == np.flatnonzero(known).tolist()
    # every record against the float64 reference of the member that owns the car
    members = [load_model(f, device="cpu", compile=False) for f in files]
    xn = _normalised(np.asarray(src.x, np.float32))
    got = np.array([r["score"] for r in recs])
    ref = np.empty(len(recs))
    for n, r in enumerate(recs):
        i = r["offset"]
        assert r["car"] == cars[i]
        layers, weights = dense_layer_table(members[key_to_model[cars[i]]])
        ref[n] = score(forward(layers, weights, xn[i:i + 1]), xn[i:i + 1])[0]
    assert float(np.max(np.abs(got - ref) / ref)) <= TOL
    near = np.abs(ref - THR) <= TOL * THR
    assert np.array_equal(np.array([r["anomaly"] for r in recs])[~near], (ref > THR)[~near])


def test_serve_cli_fallback_model_scores_unknown_cars(cuda_device, tmp_path, capsys, fleet_dir):
    from streamml.cli.__main__ import main as cli_main
    from streamml.ops.serve import read_fleet_index
    capsys.readouterr()
    names, _, _ = read_fleet_index(fleet_dir)
    topic, out = "SENSOR_FLEET_FALLBACK", "preds-fleet-fallback"
    argv = ["serve", "synthetic://600", topic, out, fleet_dir, "--workdir", str(tmp_path), "--device",
            str(cuda_device), "--model", "dense-fleet", "--synthetic-partitions", "1", "--idle-timeout", "0.3",
            "--fallback-model", names[1]]
    assert cli_main(argv) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["model"] == "dense-fleet" and summary["events"] == 600 and summary["keys_dropped"] == 0


def test_native_constructor_names_the_limit(cuda_device):
    """``_C.DenseFleetServe`` itself refuses 32 features, a bad stride and an empty fleet, with the
    limit in the message, before it allocates anything."""
    from streamml.ops import load_c
    from streamml.ops.serve import dense_fleet_serve_images
    C = load_c()
    rng = np.random.default_rng(0)

    def build(widths, M=2, stride_pad=0):
        layers = [(i, o, "tanh", True) for i, o in zip(widths[:-1], widths[1:])]
        ws = [[(rng.uniform(-1, 1, (i, o)).astype(np.float32), np.zeros(o, np.float32)) for i, o, _, _ in layers]
              for _ in range(max(M, 1))]
        images, table = dense_fleet_serve_images(layers, ws)
        img_floats = int(table[-1][4] + (table[-1][1] + 31) // 32 * 32)
        images = np.concatenate([images, np.zeros((images.shape[0], stride_pad), np.float32)], axis=1)[:M]
        return C.DenseFleetServe(0, 256, np.ascontiguousarray(images), img_floats, [list(t) for t in table],
                                 widths[0], None, None, np.full(M, 5.0, np.float32), 0.5)

    with pytest.raises(Exception, match="1..31 features"):
        build([32, 40, 32])
    with pytest.raises(Exception, match="stride"):
        build([18, 33, 18], stride_pad=2)
    with pytest.raises(Exception, match="models"):
        build([18, 33, 18], M=0)
    srv = build([18, 33, 18], stride_pad=4)      # a padded stride is fine
    assert srv.n_models == 2 and srv.kernel == "fleet"
    srv.stop()
