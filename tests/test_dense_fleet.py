"""CPU side of Dense fleets (ops/dense_fleet.py, ``cli fleet --layers``): limits, the checks on the
members and on the row table, the command line and ``index.json``."""
import numpy as np
import pytest
import torch


def _stack(widths=(18, 20, 18), acts=("tanh", "sigmoid"), seed=0, bias=True, loss="mse", beta_1=0.9, l1=0.0):
    from streamml import nn
    from streamml.nn.layers import L1L2, Dense
    from streamml.nn.model import Adam
    layers = [Dense(u, a, use_bias=bias, activity_regularizer=L1L2(l1, 0.0) if (l1 and i == 0) else None,
                    input_shape=(widths[0],) if i == 0 else None) for i, (u, a) in enumerate(zip(widths[1:], acts))]
    model = nn.Sequential(layers, device="cpu", seed=seed)
    model.compile(optimizer=Adam(beta_1=beta_1), loss=loss, metrics=["accuracy"], fused=False)
    return model


class _FakeDeviceFleet:
    """A DenseFleet without a device, for the checks of ``attach_ragged`` that come before any launch."""

    def __new__(cls, n_models=3):
        from streamml.ops import dense_persistent as dp
        from streamml.ops.dense_fleet import DenseFleet
        f = object.__new__(DenseFleet)
        f._template = _stack()
        f._n_models = n_models
        f._precision = "fp32"
        f.table = dp.table(f._template)
        f.device = torch.device("cpu")
        f._cursor = np.zeros(n_models, np.int64)
        return f


def test_supports_gives_the_trainers_reason_and_its_own():
    from streamml.ops import dense_persistent as dp
    from streamml.ops.dense_fleet import DenseFleet
    wide = _stack(widths=(18, 129, 18))
    ok, why = DenseFleet.supports(wide, 32, 8)
    assert not ok and why == dp.supports(wide, 32)[1] and "MAX_WIDTH" in why
    ok, why = DenseFleet.supports(_stack(), 129, 8)
    assert not ok and "MAX_BATCH" in why
    big = _stack(widths=(64, 128, 65), acts=("tanh", "relu"))
    assert DenseFleet.supports(big, 32, 4, precision="fp32", own_targets=True)[0] is False
    assert DenseFleet.supports(_stack(), 32, 0) == (False, "a fleet of 0 models: it needs at least one")
    assert DenseFleet.supports(_stack(), 32, -2)[0] is False
    assert DenseFleet.supports(_stack(), 32, 1) == (True, "")
    assert DenseFleet.supports(_stack(), 32, 1000, precision="bf16") == (True, "")
    assert DenseFleet.supports(_stack(widths=(18, 8, 3), acts=("tanh", "linear")), 32, 2, own_targets=True)[0]
    assert not DenseFleet.supports(_stack(widths=(18, 8, 3), acts=("tanh", "linear")), 32, 2)[0]


@pytest.mark.parametrize("other, what", [
    (dict(widths=(18, 24, 18)), "layer 0 units"),
    (dict(acts=("relu", "sigmoid")), "layer 0 activation"),
    (dict(acts=("tanh", "linear")), "layer 1 activation"),
    (dict(bias=False), "layer 0 use_bias"),
    (dict(l1=1e-3), "layer 0 activity regulariser"),
    (dict(loss="mae"), "loss"),
    (dict(beta_1=0.8), "beta_1"),
    (dict(widths=(18, 20, 20, 18), acts=("tanh", "tanh", "sigmoid")), "depth"),
    (dict(widths=(20, 20, 20)), "input shape"),
])
def test_structurally_different_members_are_named(other, what):
    from streamml.ops.dense_fleet import DenseFleet
    with pytest.raises(ValueError, match=f"model 2 differs from model 0 in {what}"):
        DenseFleet([_stack(seed=1), _stack(seed=2), _stack(seed=3, **other)], "cpu")


def test_construction_needs_a_rocm_device_and_members():
    from streamml.ops.dense_fleet import DenseFleet
    with pytest.raises(RuntimeError, match="ROCm device"):
        DenseFleet([_stack(seed=1), _stack(seed=2)], "cpu")
    with pytest.raises(ValueError, match="at least one model"):
        DenseFleet([], "cpu")
    with pytest.raises(ValueError, match="precision"):
        DenseFleet([_stack()], "cpu", precision="fp16")
    with pytest.raises(ValueError, match="schedule"):
        DenseFleet([_stack()], "cpu", schedule="random")


def test_bad_row_tables_are_rejected():
    f = _FakeDeviceFleet(3)
    x = torch.zeros(100, 18)
    with pytest.raises(ValueError, match="outside the flat array"):
        f.attach_ragged(x, 32, [[0, 40], [40, 40], [80, 21]])
    with pytest.raises(ValueError, match="outside the flat array"):
        f.attach_ragged(x, 32, [[-1, 40], [40, 40], [80, 20]])
    with pytest.raises(ValueError, match=r"models \[1\] have no rows"):
        f.attach_ragged(x, 32, [[0, 40], [40, 0], [80, 20]])
    with pytest.raises(ValueError, match=r"\[3, 2\]"):
        f.attach_ragged(x, 32, [[0, 40], [40, 40]])
    with pytest.raises(ValueError, match=r"\[3, 2\]"):
        f.attach_ragged(x, 32, [[0.0, 40.0], [40.0, 40.0], [80.0, 20.0]])
    with pytest.raises(ValueError, match=r"\[N, 18\]"):
        f.attach_ragged(torch.zeros(100, 17), 32, [[0, 40], [40, 40], [80, 20]])
    with pytest.raises(ValueError, match="MAX_BATCH"):
        f.attach_ragged(x, 129, [[0, 40], [40, 40], [80, 20]])
    with pytest.raises(ValueError, match="y must be"):
        f.attach_ragged(x, 32, [[0, 40], [40, 40], [80, 20]], y=torch.zeros(99, 18))
    with pytest.raises(ValueError, match=r"\[3, n, D\]"):
        f.attach_rows(torch.zeros(2, 10, 18), 32)
    f.attach_ragged(x, 32, [[0, 40], [40, 40], [80, 20]])       # rows that are no multiple of the batch
    assert list(f.epoch_steps()) == [2, 2, 1]


def test_descriptor_layout_is_the_kernels():
    from streamml.ops.dense_fleet import DESCRIPTOR
    assert DESCRIPTOR.itemsize == 32
    assert [DESCRIPTOR.fields[k][1] for k in ("first_row", "rows", "row0", "nsteps", "lr")] == [0, 8, 16, 24, 28]


def test_fleet_without_layers_parses_as_before():
    from streamml.cli.fleet import parse_args
    ns = vars(parse_args(["synthetic", "--models", "64", "--epochs", "2"]))
    assert ns.pop("layers") is None and ns.pop("precision") is None
    assert ns == dict(source="synthetic", models=64, epochs=2, batch=32, lr=1e-3, out="fleet_models", device="cuda:0",
                      seed=0, synthetic_rows=1 << 20, synthetic_devices=1000)
    ns = parse_args(["synthetic", "--layers", "64,16,64", "--precision", "bf16"])
    assert ns.layers == "64,16,64" and ns.precision == "bf16"
    with pytest.raises(SystemExit):
        parse_args(["synthetic", "--precision", "bf16"])


def test_index_json_keys():
    from streamml.cli.fleet import INDEX_META, build_index, model_name
    members = [["car/1"], ["a", "b"], ["engine"]]
    used = set(INDEX_META)
    names = [model_name(members, i, used) for i in range(3)]
    assert names == ["car_1", "model00001", "engine-2"]           # a key named like a meta entry cannot shadow it
    index = build_index(names, members, [0.5, 0.25, None], layers=[64, 16, 64], precision="bf16")
    assert set(index) == set(names) | {"layers", "engine", "precision"}
    assert index["layers"] == [64, 16, 64] and index["engine"] == "persistent" and index["precision"] == "bf16"
    assert index["car_1"] == {"file": "car_1.h5", "keys": ["car/1"], "loss": 0.5}
    assert index["model00001"]["keys"] == ["a", "b"]
    assert build_index(names, members, [0.5, 0.25, None], layers=[8])["precision"] == "fp32"
    assert set(build_index(names[:2], members, [0.5, 0.25])) == set(names[:2])


def test_cli_stack_is_the_cardata_layers_stack():
    from streamml.cli.fleet import dense_stack
    from streamml.ops import dense_persistent as dp
    m = dense_stack([64, 16, 64], seed=3, lr=2e-3, precision="bf16")
    assert [(r[0], r[1], r[2]) for r in dp.table(m)] == [(18, 64, dp.ACT["tanh"]), (64, 16, dp.ACT["relu"]),
                                                         (16, 64, dp.ACT["tanh"]), (64, 18, dp.ACT["relu"])]
    assert m.hp["lr"] == 2e-3 and m.minibatch_precision == "bf16" and m.loss == "mean_squared_error"
