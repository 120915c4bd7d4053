"""The wide per-event LSTM forecaster on several resident lanes (csrc/kernels/lstm_serve_wide.hip,
csrc/runtime/serve.cpp): key k is served by lane k % lanes, so every result must have the bits
the one-lane server gives, whatever runs side by side.  The one-lane server itself is tied to the
float64 reference that rounds at the kernel's own points (tests/helpers/lstm_serve_ref.py).

Shapes are the smallest that reach every path: look_back 6 (not a multiple of the projection's
8-step block), 18 features, LSTM(136, sequences) -> LSTM(40) -> Dense(18): 136 pads to 160 (the
streamed-U recurrence), 40 pads to 64 (the register-resident one), and the sequence output
makes layer 2 read the lane's projection scratch a second time within one event."""
import functools
import time

import numpy as np
import pytest
import torch

from streamml.models.lstm import LSTMPredictor

pytestmark = pytest.mark.gpu

T, D = 6, 18
STACK = [("lstm", 136, True, "tanh"), ("lstm", 40, False, "tanh"), ("dense", 18, False)]
THR = 0.05
NKEYS = 64


@functools.lru_cache(maxsize=None)
def _model(dev):
    return LSTMPredictor(look_back=T, features=D, stack=STACK, device=torch.device(dev), seed=13)


def _server(dev, lanes, nkeys=NKEYS, **kw):
    from streamml.ops.serve import LSTMScoringServer
    return LSTMScoringServer(_model(dev), nkeys=nkeys, threshold=THR, normalizer=None, lanes=lanes, **kw)


@functools.lru_cache(maxsize=None)
def _stream():
    """64 keys x 10 events, round-robin."""
    n = NKEYS * 10
    keys = np.arange(n, dtype=np.int64) % NKEYS
    rows = np.random.default_rng(21).uniform(-1, 1, size=(n, D)).astype(np.float32)
    rows.setflags(write=False)
    keys.setflags(write=False)
    return rows, keys


def _run(dev, lanes, rows, keys, nkeys=NKEYS, **kw):
    with _server(dev, lanes, nkeys=nkeys, **kw) as srv:
        assert srv.kernel == "wide" and srv.lanes == lanes
        out = srv.forecast(rows, keys)
        counts = srv.lane_events
    assert counts.dtype == np.int64 and counts.shape == (lanes,)
    assert np.array_equal(counts, np.bincount(np.asarray(keys) % lanes, minlength=lanes)), counts
    return out


@functools.lru_cache(maxsize=None)
def _one_lane(dev):
    """The one-lane server's answer to the shared stream: computed once, never written."""
    out = _run(dev, 1, *_stream())
    for a in out:
        a.setflags(write=False)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(np.uint32)


def _assert_same_bits(got, want):
    for g, w, what in zip(got, want, ("forecast", "score", "flag")):
        assert g.shape == w.shape, what
        assert np.array_equal(_bits(g), _bits(w)), (what, int(np.sum(_bits(g) != _bits(w))))


@pytest.mark.parametrize("lanes", [2, 3, 8])
def test_lanes_give_the_one_lane_bits_under_concurrency(cuda_device, lanes):
    dev = str(cuda_device)
    want = _one_lane(dev)
    pred, score, flag = want
    assert np.abs(pred).max() > 0 and np.isnan(score).any() and (flag != 2).any()   # a real stream
    _assert_same_bits(_run(dev, lanes, *_stream()), want)


def test_one_lane_server_against_the_rounded_reference(cuda_device):
    """Ties the bit-identity chain to an oracle that is not the code under test: every forecast
    within 1e-3 (norm-relative) of the float64 reference that rounds to bf16 at the kernel's
    own points -- the helper and the bound of tests/test_lstm_serve_wide_gpu.py."""
    from helpers.lstm_serve_ref import forward, relerr, stack_weights
    rows, keys = _stream()
    pred, score, flag = _one_lane(str(cuda_device))
    cpu = LSTMPredictor(look_back=T, features=D, stack=STACK, device="cpu", seed=13)   # same seed: same weights
    at, windows = [], []
    for i in range(len(keys)):
        j = i // NKEYS          # the key's j-th event (round-robin)
        if j + 1 >= T:
            at.append(i)
            windows.append(rows[[int(keys[i]) + NKEYS * (j - T + 1 + s) for s in range(T)]])
        else:
            assert flag[i] == 2 and np.isnan(score[i]) and not pred[i].any()
    refs = forward(cpu, np.stack(windows), True, stack_weights(cpu, True))
    worst = max(relerr(pred[i], r) for i, r in zip(at, refs))
    print("one-lane server vs rounded reference: worst %.2e over %d forecasts" % (worst, len(at)))
    assert len(at) == NKEYS * (10 - T + 1)
    assert worst < 1e-3, worst


@pytest.mark.parametrize("lanes,nkeys,n", [(8, 3, 30), (4, 1, 40), (3, 7, 70), (4, 6, 50)],
                         ids=["more-lanes-than-keys", "one-hot-key", "7keys-3lanes", "6keys-4lanes"])
def test_edge_sharding(cuda_device, lanes, nkeys, n):
    dev = str(cuda_device)
    rng = np.random.default_rng(100 + lanes + nkeys)
    rows = rng.uniform(-1, 1, size=(n, D)).astype(np.float32)
    keys = np.arange(n, dtype=np.int64) % nkeys if nkeys < 7 else rng.integers(0, nkeys, size=n)
    want = _run(dev, 1, rows, keys, nkeys=nkeys)
    assert (want[2] != 2).any()   # forecasts were made: order within a key matters
    _assert_same_bits(_run(dev, lanes, rows, keys, nkeys=nkeys), want)


def test_per_lane_back_pressure(cuda_device):
    """300 events that all land on lane 1 of 4, with 64 slots per lane: the call completes and
    nothing is reordered or overwritten."""
    dev = str(cuda_device)
    rng = np.random.default_rng(5)
    n = 300
    rows = rng.uniform(-1, 1, size=(n, D)).astype(np.float32)
    keys = (4 * rng.integers(0, 4, size=n) + 1).astype(np.int64)   # 1, 5, 9, 13
    want = _run(dev, 1, rows, keys, nkeys=16, slots=64)
    with _server(dev, 4, nkeys=16, slots=64) as srv:
        assert srv.slots == 64
        got = srv.forecast(rows, keys)
        assert srv.lane_events.tolist() == [0, n, 0, 0]
    _assert_same_bits(got, want)
    # and a mixed batch in which one lane overflows its ring while the others do not
    keys2 = np.where(np.arange(n) % 5 == 0, np.arange(n) % 16, keys).astype(np.int64)
    want = _run(dev, 1, rows, keys2, nkeys=16, slots=64)
    _assert_same_bits(_run(dev, 4, rows, keys2, nkeys=16, slots=64), want)


@pytest.mark.parametrize("lanes", [2, 4])
def test_back_pressure_returns_to_a_lane_after_a_long_run_elsewhere(cuda_device, lanes):
    """Lane 1 gets exactly a ring of events (64 slots) that the host does not gather yet; a run of
    several rings' length on lane 0 blocks the host long enough for lane 1 to finish them all.  The
    next lane-1 event finds the ring full: the host waits for the oldest event, takes the other 63
    without waiting, and publishes 64 more into the slots it has just freed.  A second long run on
    lane 0 lets the device overwrite those slots' results.  The lane-1 event after that must wait
    from the first event NOT yet gathered: a wait that starts below it looks for a gathered
    event's tag in a slot that carries a later one, and never finds it."""
    dev = str(cuda_device)
    rng = np.random.default_rng(31)
    hot = lambda n: lanes * rng.integers(0, 4, size=n) + 1            # lane 1
    other = lambda n: lanes * rng.integers(0, 4, size=n)              # lane 0
    keys = np.concatenate([hot(64), other(200), hot(64), other(200), hot(40), other(30), hot(122)])
    keys = keys.astype(np.int64)
    rows = rng.uniform(-1, 1, size=(len(keys), D)).astype(np.float32)
    nkeys = 4 * lanes
    want = _run(dev, 1, rows, keys, nkeys=nkeys, slots=64)
    with _server(dev, lanes, nkeys=nkeys, slots=64) as srv:
        got = srv.forecast(rows, keys)
        again = srv.forecast(rows, keys)          # rings that start mid-way, not at slot 0
        counts = srv.lane_events
    _assert_same_bits(got, want)
    assert counts[1] == 2 * 290 and counts[0] == 2 * 430 and counts.sum() == 2 * len(keys)
    assert (again[2] != 2).all() and np.isfinite(again[1]).all()


def test_lanes_leave_together(cuda_device):
    """A quiet lane stays resident while another lane is busy (the idle timer is the whole
    server's), and the whole launch leaves once, together, when all traffic stops."""
    dev = str(cuda_device)
    rng = np.random.default_rng(9)
    sent_rows, sent_keys = [], []

    def one(srv, key):
        row = rng.uniform(-1, 1, size=(1, D)).astype(np.float32)
        sent_rows.append(row)
        sent_keys.append(key)
        return srv.forecast(row, np.array([key]))

    got = []
    with _server(dev, 4, nkeys=16, idle_seconds=0.3) as srv:
        got.append(one(srv, 1))
        base = srv.launches
        t0 = time.perf_counter()
        i = 0
        while time.perf_counter() - t0 < 1.0:     # lane 1 only, for more than three idle timeouts
            got.append(one(srv, (1, 5, 9, 13)[i % 4]))
            i += 1
            time.sleep(0.02)
        assert srv.launches == base                # lane 1 was never idle
        got.append(one(srv, 2))                    # lane 2 had no event for 1 s > idle_seconds ...
        assert srv.launches == base                # ... and was still resident
        assert srv.lane_events.tolist() == [0, len(sent_keys) - 1, 1, 0]
        time.sleep(1.0)                            # no traffic at all: the launch leaves
        got.append(one(srv, 1))                    # a key with a full window: a real forecast
        assert srv.launches == base + 1            # one relaunch ...
        got.append(one(srv, 6))
        got.append(one(srv, 3))
        assert srv.launches == base + 1            # ... serves every lane
    rows, keys = np.concatenate(sent_rows), np.array(sent_keys, np.int64)
    want = _run(dev, 1, rows, keys, nkeys=16)
    _assert_same_bits([np.concatenate([g[j] for g in got]) for j in range(3)], want)
    assert want[2][-3] != 2 and np.abs(want[0][-3]).max() > 0   # the event that met the relaunch was forecast


def test_reset_and_close(cuda_device):
    dev = str(cuda_device)
    rows, keys = _stream()
    rows, keys = rows[:NKEYS * 8], keys[:NKEYS * 8]
    srv = _server(dev, 4, idle_seconds=5.0)
    try:
        first = srv.forecast(rows, keys)
        assert srv.lane_events.tolist() == [len(keys) // 4] * 4
        t0 = time.perf_counter()
        srv.reset()                  # the lanes leave on the stop flag, not at the idle timeout
        assert time.perf_counter() - t0 < 1.0
        assert srv.lane_events.tolist() == [0, 0, 0, 0]
        again = srv.forecast(rows, keys)
        assert srv.lane_events.tolist() == [len(keys) // 4] * 4
    finally:
        t0 = time.perf_counter()
        srv.close()
        assert time.perf_counter() - t0 < 1.0
    _assert_same_bits(again, first)
    fresh = _one_lane(dev)
    _assert_same_bits(again, [a[:len(keys)] for a in fresh])


def test_latency_us_reads_the_lane_that_ran_the_event(cuda_device):
    dev = str(cuda_device)
    rows, keys = _stream()
    n = 120
    with _server(dev, 4) as srv:
        host, total, comp = srv.latency_us(rows[:n], keys[:n], qps=0, device_breakdown=True)
        load = srv.last_device_load_us
        assert srv.lane_events.tolist() == [n // 4] * 4
    for a in (host, total, comp, load):
        assert a.shape == (n,) and np.all(np.isfinite(a))
    assert np.all(host > 0) and np.all(total > 0) and np.all(load > 0) and np.all(comp >= 0)
    assert np.all(load <= total) and np.all(load + comp <= total + 1e-6)
    assert np.all(total < host)        # a stale slot of another lane would carry another event's times


def _loop_records(dev, lanes, name):
    """200 events of 12 cars over two partitions through the low-latency loop; the result
    records' bytes per partition."""
    from streamml.data.avro import AvroCodec
    from streamml.data.cardata import FEATURES, INT_FEATURES
    from streamml.data.produce import encode_chunk
    from streamml.kafka import KafkaClient, fake_broker
    from streamml.kafka.scoreloop import LowLatencyScorer
    from streamml.ops.serve import LSTMScoringServer
    rng = np.random.default_rng(17)
    n, ncar = 200, 12
    raw = rng.uniform(0, 40, size=(n, 18)).astype(np.float32)
    for j, f in enumerate(FEATURES):   # the Avro schema's int fields carry whole numbers
        if f in INT_FEATURES:
            raw[:, j] = np.round(raw[:, j])
    cars = [f"vehicles/sensor/data/electric-vehicle-{int(c):05d}" for c in rng.integers(0, ncar, size=n)]
    part = np.array([int(c[-5:]) % 2 for c in cars])        # a car's events stay in one partition
    b = fake_broker(name)
    b.create_topic("S", 2)
    b.create_topic("R", 2)
    codec = AvroCodec("cardata-v1")
    cli = KafkaClient(f"fake://{name}")
    for p in (0, 1):
        idx = np.nonzero(part == p)[0]
        buf, offs = encode_chunk(codec, raw[idx].astype(np.float64), np.zeros(len(idx), np.uint8))
        cli.produce("S", p, [bytes(buf[offs[i]:offs[i + 1]]) for i in range(len(idx))],
                    keys=[cars[i].encode() for i in idx])
    with LSTMScoringServer(_model(dev), nkeys=16, threshold=THR, lanes=lanes) as srv:
        assert srv.kernel == "wide" and srv.lanes == lanes
        loop = LowLatencyScorer(f"fake://{name}", "S", "R", [0, 1], srv, starts=[0, 0], emit_recon=True,
                                max_wait_ms=5, max_batch=64)
        st = loop.run(idle_timeout_s=0.3)
        counts = srv.lane_events
    assert st["events"] == n and st["keys"] == len(set(cars))
    assert counts.sum() == n and (lanes == 1 or np.count_nonzero(counts) > 1)
    return [[bytes(r[2]) for r in b.read("R", p, 0)] for p in (0, 1)]


def test_low_latency_loop_records_are_identical(cuda_device):
    dev = str(cuda_device)
    one = _loop_records(dev, 1, "lstm-ll-lanes-1")
    four = _loop_records(dev, 4, "lstm-ll-lanes-4")
    assert sum(len(p) for p in one) == 200
    assert b"anomaly" in one[0][0] and b"reconstruction" in one[0][0]
    assert one == four


def test_native_constructor_names_each_lane_limit(cuda_device):
    from streamml.ops import load_c
    from streamml.ops.serve import lstm_layer_table
    C = load_c()
    dev = cuda_device.index or 0
    flat, table = lstm_layer_table(LSTMPredictor(look_back=T, features=D, stack=STACK, device="cpu"))
    args = (dev, 64, flat, [list(t) for t in table], D, T, 2, None, None, 5.0, 2.0)
    for lanes in (0, 33):
        with pytest.raises(ValueError, match=r"lanes must be 1\.\.32"):
            C.LSTMServe(*args, lanes)
    narrow = LSTMPredictor(look_back=T, features=D, stack=[("lstm", 32, False, "tanh"), ("dense", 18, False)],
                           device="cpu")
    flat, table = lstm_layer_table(narrow)
    with pytest.raises(ValueError, match="only the streamed-weight"):
        C.LSTMServe(dev, 64, flat, [list(t) for t in table], D, T, 2, None, None, 5.0, 2.0, 2)
    s = C.LSTMServe(dev, 64, flat, [list(t) for t in table], D, T, 2, None, None, 5.0, 2.0, 1)   # one lane: served
    try:
        assert s.lanes == 1 and s.kernel != "wide"
    finally:
        s.stop()
