"""The fleet scorer's host side without a device: the stacked weight images
(``ops.serve.dense_fleet_serve_images``) against the single-model packer, ``supports`` against the
host program over ``sml_dense_fleet_serve.h``, the ``fleet --layers`` directory reader, and the
low-latency loop's preset key table against ``_io.EchoScorer``."""
import json
import os
import subprocess

import numpy as np
import pytest

import streamml
from streamml import nn
from streamml.nn.layers import Dense, Dropout
from streamml.ops.serve import (DenseFleetScoringServer, dense_fleet_serve_images, dense_layer_table,
                                dense_serve_image, read_fleet_index)

PKG = os.path.dirname(os.path.abspath(streamml.__file__))


def _stack(widths, acts, features, seed, bias_less=False):
    if bias_less:
        layers = [Dense(40, "relu", use_bias=False, input_shape=(features,)), Dropout(0.3), Dense(features, "linear")]
    else:
        layers = [Dense(u, a, input_shape=(features,) if i == 0 else None)
                  for i, (u, a) in enumerate(zip(widths, acts))]
    m = nn.Sequential(layers, device="cpu", seed=seed)
    rng = np.random.default_rng(seed)   # Keras biases start at zero, which would hide a misplaced bias
    m.set_weights([w if w.ndim == 2 else rng.uniform(-0.5, 0.5, w.shape).astype(np.float32) for w in m.get_weights()])
    return m


STACKS = {
    "18-33-18": dict(widths=[33, 18], acts=["tanh", "relu"], features=18),
    "18-64-16-64-18": dict(widths=[64, 16, 64, 18], acts=["tanh", "relu", "tanh", "linear"], features=18),
    "bias_less": dict(widths=None, acts=None, features=18, bias_less=True),
    "31-40-31": dict(widths=[40, 31], acts=["tanh", "linear"], features=31),
}


@pytest.mark.parametrize("name", list(STACKS))
def test_images_equal_the_single_model_packer_row_for_row(name):
    models = [_stack(seed=s, **STACKS[name]) for s in (3, 4, 5, 6)]
    layers, _ = dense_layer_table(models[0])
    weight_lists = [dense_layer_table(m)[1] for m in models]
    images, table = dense_fleet_serve_images(layers, weight_lists)
    M, stride = images.shape
    assert M == 4 and images.dtype == np.float32 and stride % 4 == 0
    for i, w in enumerate(weight_lists):
        one, one_table = dense_serve_image(layers, w)
        assert 0 <= stride - one.size < 4
        assert [tuple(t) for t in table] == [tuple(t) for t in one_table]
        assert np.array_equal(images[i], np.concatenate([one, np.zeros(stride - one.size, np.float32)]))
    # the same rows from flat parameter vectors (what DenseFleet.flat holds), also with a padded stride
    flats = np.stack([np.concatenate([a.ravel() for pair in w for a in pair if a is not None]) for w in weight_lists])
    assert np.array_equal(dense_fleet_serve_images(layers, flats)[0], images)
    padded = np.concatenate([flats, np.full((M, 5), 7.0, np.float32)], axis=1)
    assert np.array_equal(dense_fleet_serve_images(layers, padded)[0], images)


def test_images_take_explicit_offsets():
    models = [_stack(seed=s, **STACKS["18-33-18"]) for s in (1, 2)]
    layers, _ = dense_layer_table(models[0])
    weight_lists = [dense_layer_table(m)[1] for m in models]
    want = dense_fleet_serve_images(layers, weight_lists)[0]
    # biases first, then the kernels, with a gap between them
    nb = [o for _, o, _, _ in layers]
    nw = [i * o for i, o, _, _ in layers]
    b_off = [0, nb[0]]
    w_off = [sum(nb) + 3, sum(nb) + 3 + nw[0]]
    flats = np.full((2, w_off[1] + nw[1]), np.nan, np.float32)
    for m, w in enumerate(weight_lists):
        for l, (W, b) in enumerate(w):
            flats[m, b_off[l]:b_off[l] + nb[l]] = b
            flats[m, w_off[l]:w_off[l] + nw[l]] = W.ravel()
    got = dense_fleet_serve_images(layers, flats, offsets=list(zip(w_off, b_off)))[0]
    assert np.array_equal(got, want)


# ---- supports and the host checker ---------------------------------------------------------------
def _tanh_stack(widths, seed=0):
    return nn.Sequential([Dense(u, "tanh", input_shape=(widths[0],) if i == 0 else None)
                          for i, u in enumerate(widths[1:])], device="cpu", seed=seed)


#          widths, n_models, what the refusal names ("" = served)
SHAPES = [
    ([18, 64, 16, 64, 18], 5, ""),
    ([31, 40, 31], 1, ""),
    ([18, 33, 18], (1 << 24) - 1, ""),
    ([32, 40, 32], 5, "1..31 features"),                 # word 31 is the model index
    ([18, 513, 18], 5, "1..512 units"),
    ([18] + [20] * 8 + [18], 5, "1..8 Dense layers"),    # nine layers
    ([18, 33, 18], 0, "1..16777215 models"),
    ([18, 33, 18], 1 << 24, "1..16777215 models"),
    ([18, 33, 17], 5, "one unit per feature"),
]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")   # the host compiler the package itself is built with
    exe = str(tmp_path_factory.mktemp("dense_fleet_serve_check") / "dense_fleet_serve_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc", "include"),
                    os.path.join(PKG, "csrc", "tests", "dense_fleet_serve_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=120)
    return exe


def test_supports_names_each_limit():
    for widths, n_models, names in SHAPES:
        ok, why = DenseFleetScoringServer.supports(_tanh_stack(widths), n_models)
        assert ok == (names == "") and names in why, (widths, n_models, why)
    a, b = _tanh_stack([18, 33, 18], seed=1), _tanh_stack([18, 34, 18], seed=2)
    ok, why = DenseFleetScoringServer.supports([a, a, b], 3)
    assert not ok and "model 2" in why and "layer 0" in why, why
    c = nn.Sequential([Dense(33, "relu", input_shape=(18,)), Dense(18, "tanh")], device="cpu", seed=3)
    ok, why = DenseFleetScoringServer.supports([a, c], 2)
    assert not ok and "model 1" in why and "layer 0" in why and "relu" in why, why
    assert DenseFleetScoringServer.supports([a, a], 2) == (True, "")
    with pytest.raises(ValueError, match="model 2 differs from model 0 in layer 0"):
        DenseFleetScoringServer([a, a, b], device="cpu")


def test_host_checker_agrees_with_supports(checker):
    text = "".join(f"{','.join(map(str, w))} {n}\n" for w, n, _ in SHAPES)
    r = subprocess.run([checker], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert len(got) == len(SHAPES)
    for (widths, n_models, names), (why_c, img_floats, stride) in zip(SHAPES, got):
        ok, why_py = DenseFleetScoringServer.supports(_tanh_stack(widths), n_models)
        assert ok == (why_c == ""), (widths, n_models, why_c, why_py)
        assert names in why_c
        assert why_py.startswith(why_c), (why_c, why_py)   # the same refusal; Python adds the offending number
        if ok:
            layers, weights = dense_layer_table(_tanh_stack(widths))
            images, _ = dense_fleet_serve_images(layers, [weights])
            assert images.shape[1] == int(stride) and dense_serve_image(layers, weights)[0].size == int(img_floats)
    # the stride's own rules: 18-33-18 packs into (20 * 64 + 64) + (36 * 32 + 32) = 2528 floats
    r = subprocess.run([checker], input="18,33,18 5 2530\n18,33,18 5 2524\n18,33,18 5 2528\n18,33,18 5 2532\n",
                       capture_output=True, text=True, timeout=60)
    rows = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert [x[1] for x in rows] == ["2528"] * 4
    why = [x[0] for x in rows]
    assert "stride" in why[0] and "stride" in why[1] and why[2] == "" and why[3] == "", r.stdout


def test_host_checker_constants(checker):
    out = subprocess.run([checker, "-c"], capture_output=True, text=True, timeout=60, check=True).stdout
    c = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    S = DenseFleetScoringServer
    assert (c["DSV_MAXW"], c["DSV_MAXLAYERS"], c["DSV_EB"], c["DSV_FLEET_MAXD"], c["DSV_FLEET_MAXMODELS"] - 1) == (
        S.MAX_WIDTH, S.MAX_LAYERS, S.MAX_PASS, S.MAX_FEATURES, S.MAX_MODELS)


# ---- the fleet --layers directory ------------------------------------------------------------------
def _write_dir(path, members, hidden=(16,), meta=True, widths_of=None):
    from streamml.cli.fleet import INDEX_META, build_index, dense_stack, model_name
    os.makedirs(path, exist_ok=True)
    used = set(INDEX_META)
    names = [model_name(members, i, used) for i in range(len(members))]
    for i, name in enumerate(names):
        h = hidden if widths_of is None else widths_of(i)
        dense_stack(list(h), seed=i, lr=1e-3, device="cpu").save(os.path.join(path, name + ".h5"))
    index = build_index(names, members, [0.1 * i for i in range(len(members))], hidden if meta else None, "fp32")
    with open(os.path.join(path, "index.json"), "w") as f:
        json.dump(index, f)
    return names


def test_load_dir_one_model_per_key(tmp_path):
    members = [[f"electric-vehicle-{i:05d}"] for i in range(4)]
    names = _write_dir(str(tmp_path / "fleet"), members)
    models, got_names, key_to_model = DenseFleetScoringServer.load_dir(str(tmp_path / "fleet"))
    assert got_names == names == [m[0] for m in members]
    assert key_to_model == {m[0]: i for i, m in enumerate(members)}
    assert len(models) == 4 and dense_layer_table(models[0])[0] == dense_layer_table(models[3])[0]
    assert set(got_names).isdisjoint({"layers", "engine", "precision"})
    # without a ROCm device the directory is read and checked, then the server itself refuses
    with pytest.raises(RuntimeError, match="ROCm device"):
        DenseFleetScoringServer.from_dir(str(tmp_path / "fleet"), device="cpu")


def test_load_dir_models_that_own_several_keys(tmp_path):
    members = [["car-a", "car-d", "car-e"], ["car-b"], ["car-c", "car-f"]]   # fleet --models 3
    names = _write_dir(str(tmp_path / "fleet"), members)
    assert names == ["model00000", "car-b", "model00002"]
    _, got_names, key_to_model = DenseFleetScoringServer.load_dir(str(tmp_path / "fleet"))
    assert got_names == names
    assert key_to_model == {"car-a": 0, "car-d": 0, "car-e": 0, "car-b": 1, "car-c": 2, "car-f": 2}
    assert read_fleet_index(str(tmp_path / "fleet"))[2] == key_to_model


def test_directory_refusals(tmp_path, capsys):
    from streamml.cli.__main__ import main as cli_main
    from streamml.cli.serve import _FleetDir
    members = [["car-a"], ["car-b"]]
    # an AEFleet directory: no `layers` in the index
    _write_dir(str(tmp_path / "plain"), members, meta=False)
    with pytest.raises(ValueError, match="no 'layers'"):
        DenseFleetScoringServer.load_dir(str(tmp_path / "plain"))
    with pytest.raises(SystemExit, match="no 'layers'"):
        _FleetDir(str(tmp_path / "plain"), "cpu")
    # members that differ: supports refuses
    _write_dir(str(tmp_path / "mixed"), members, widths_of=lambda i: (16,) if i == 0 else (20,))
    with pytest.raises(ValueError, match="model 1 differs from model 0 in layer 0"):
        DenseFleetScoringServer.load_dir(str(tmp_path / "mixed"))
    with pytest.raises(SystemExit, match="model 1 differs from model 0 in layer 0"):
        _FleetDir(str(tmp_path / "mixed"), "cpu")
    # a fallback the index does not name
    _write_dir(str(tmp_path / "good"), members)
    with pytest.raises(SystemExit, match="--fallback-model car-z: index.json names no such model"):
        _FleetDir(str(tmp_path / "good"), "cpu", fallback="car-z")
    # not a directory at all, through the command line
    with pytest.raises(SystemExit, match="not a directory"):
        cli_main(["serve", "synthetic://10", "T", "R", str(tmp_path / "nothing"), "--model", "dense-fleet",
                  "--device", "cpu", "--workdir", str(tmp_path)])
    capsys.readouterr()
    fd = object.__new__(_FleetDir)   # the key lookup of the chunked path
    fd.key_to_model, fd.fallback = {"car-a": 0, "car-b": 1}, -1
    assert fd.indices([b"car-b", "car-a", None, "car-x"]).tolist() == [1, 0, -1, -1]
    fd.fallback = 1
    assert fd.indices([b"car-b", "car-a", None, "car-x"]).tolist() == [1, 0, -1, 1]


# ---- the low-latency loop's preset key table -------------------------------------------------------
def _produce(name, n, keys):
    from streamml.data import stream as S
    from streamml.data.avro import AvroCodec
    from streamml.data.produce import encode_chunk
    from streamml.kafka import KafkaClient, fake_broker
    b = fake_broker(name)
    b.create_topic("S", 1)
    b.create_topic("R", 1)
    c = next(iter(S.synthetic(n, chunk=n, seed=2, failure_rate=0.1)))
    buf, offs = encode_chunk(AvroCodec("cardata-v1"), c.x, c.label)
    offs = np.asarray(offs)
    KafkaClient(f"fake://{name}").produce("S", 0, [bytes(buf[offs[i]:offs[i + 1]]) for i in range(n)], keys=keys)
    return b


def test_loop_uses_a_preset_key_table():
    from streamml.kafka.scoreloop import LowLatencyScorer
    from streamml.ops._ext import load_io
    cars = [f"car{(i * 5) % 7}" for i in range(70)]
    table = {f"car{j}": (3 * j + 1) % 5 for j in range(6)}     # car6 is unknown; ids are not first-come
    keys = [c.encode() for c in cars] + [None]
    # unknown keys are dropped and counted
    b = _produce("fleet-keytable-drop", 71, keys)
    loop = LowLatencyScorer("fake://fleet-keytable-drop", "S", "R", [0], load_io().EchoScorer(18, 1e9, nkeys=5),
                            starts=[0], max_wait_ms=5, key_table=table, unknown_key_id=-1)
    st = loop.run(idle_timeout_s=0.2)
    res = [json.loads(r[2]) for r in b.read("R", 0, 0)]
    assert st["events"] == 60 == len(res) and st["keys_dropped"] == 11, st   # ten of car6 and the null key
    assert all(d["score"] == table[d["car"]] for d in res)                   # EchoScorer: score = the id
    assert [d["offset"] for d in res] == [i for i, c in enumerate(cars) if c != "car6"]
    assert loop.positions() == [71]
    # or scored by the fallback id; bytes keys in the table work as well
    b = _produce("fleet-keytable-fallback", 71, keys)
    loop = LowLatencyScorer("fake://fleet-keytable-fallback", "S", "R", [0], load_io().EchoScorer(18, 1e9, nkeys=5),
                            starts=[0], max_wait_ms=5, key_table={k.encode(): v for k, v in table.items()},
                            unknown_key_id=4)
    st = loop.run(idle_timeout_s=0.2)
    res = [json.loads(r[2]) for r in b.read("R", 0, 0)]
    assert st["events"] == 70 == len(res) and st["keys_dropped"] == 1, st
    assert all(d["score"] == table.get(d["car"], 4) for d in res)
    # an id the scorer does not have is refused at construction
    with pytest.raises(Exception, match="nkeys"):
        LowLatencyScorer("fake://fleet-keytable-fallback", "S", "R", [0], load_io().EchoScorer(18, 1e9, nkeys=5),
                         starts=[0], key_table={"car0": 5})
    with pytest.raises(Exception, match="nkeys"):
        LowLatencyScorer("fake://fleet-keytable-fallback", "S", "R", [0], load_io().EchoScorer(18, 1e9, nkeys=5),
                         starts=[0], key_table=table, unknown_key_id=5)
    with pytest.raises(ValueError, match="key_table"):
        LowLatencyScorer("fake://fleet-keytable-fallback", "S", "R", [0], load_io().EchoScorer(18, 1e9, nkeys=5),
                         starts=[0], unknown_key_id=2)


def test_loop_without_a_table_keeps_first_come_ids():
    from streamml.kafka.scoreloop import LowLatencyScorer
    from streamml.ops._ext import load_io
    cars = [f"car{(i * 5) % 7}" for i in range(70)]
    b = _produce("fleet-keytable-none", 70, [c.encode() for c in cars])
    loop = LowLatencyScorer("fake://fleet-keytable-none", "S", "R", [0], load_io().EchoScorer(18, 1e9, nkeys=7),
                            starts=[0], max_wait_ms=5)
    st = loop.run(idle_timeout_s=0.2)
    res = [json.loads(r[2]) for r in b.read("R", 0, 0)]
    first = {}
    for c in cars:
        first.setdefault(c, len(first))
    assert st["events"] == 70 and st["keys"] == 7 and st["keys_dropped"] == 0
    assert all(d["score"] == first[d["car"]] for d in res)
