"""Fleets of Dense stacks (ops.dense_fleet.DenseFleet, the fleet entries of dense_minibatch.hip and
dense_minibatch_bf16.hip, ``cli fleet --layers``).

The main oracle is the single-model path: a fleet member must equal, bit for bit, the same model
trained alone by ``dense_persistent.train_steps`` on its slice of the rows (that path is held to
float64 and bf16 oracles by tests/test_dense_minibatch_gpu.py and test_dense_minibatch_bf16_gpu.py).
One fp32 test checks a member against the float64 reference directly, with the tolerances of
tests/test_dense_minibatch_gpu.py: weights rtol 2e-4 / atol 2e-5, first moments rtol 2e-3 / atol 1e-6,
per-step loss 1e-4 relative, per-step ``correct`` exact.
"""
import json
import os

import numpy as np
import pytest
import torch

from helpers import dense_mb_cases as cases

PRECISIONS = ("fp32", "bf16")
W_TOL = dict(rtol=2e-4, atol=2e-5)      # tests/test_dense_minibatch_gpu.py
M_TOL = dict(rtol=2e-3, atol=1e-6)
LOSS_RTOL = 1e-4


def _stack(device, widths, acts, seed, lr=None, precision=None, bias=None):
    from streamml import nn
    from streamml.nn.layers import Dense
    from streamml.nn.model import Adam
    bias = bias or [True] * len(acts)
    layers = [Dense(u, a, use_bias=bias[i], input_shape=(widths[0],) if i == 0 else None)
              for i, (u, a) in enumerate(zip(widths[1:], acts))]
    model = nn.Sequential(layers, device=device, seed=seed)
    model.compile(optimizer="adam" if lr is None else Adam(learning_rate=lr), loss="mse", metrics=["accuracy"],
                  fused=False if str(device) == "cpu" else None, minibatch_precision=precision)
    return model


def _table(rows):
    rows = np.asarray(rows, np.int64)
    return np.stack([np.concatenate([[0], np.cumsum(rows)[:-1]]), rows], axis=1)


def _alone(model, x, y, batch, nsteps, precision, row0=0, order=None):
    from streamml.ops import dense_persistent as dp
    return dp.train_steps(model, x, y, batch, nsteps, row0=row0, order=order, precision=precision)


def _assert_member(fleet, i, alone, out_alone, out_fleet):
    n = alone.fp.n
    for buf in ("flat", "m", "v"):
        assert torch.equal(getattr(fleet, buf)[i, :n], getattr(alone.fp, buf)[:n]), (i, buf)
    assert torch.equal(fleet.iter[i:i + 1], alone.fp.iter), i
    k = out_alone.size(0)
    assert torch.equal(out_fleet[i, :k], out_alone), i
    assert not out_fleet[i, k:].any(), f"model {i}: rows of out past its last step are not zero"


def _ragged_fleet(device, precision, schedule="longest_first", stride_extra=0, widths=(18, 20, 18),
                  acts=("tanh", "sigmoid"), rows=(21, 37, 7, 40, 28), batch=7, lrs=(1e-3, 3e-3, 1e-3, 5e-4, 1e-3)):
    from streamml.ops.dense_fleet import DenseFleet
    models = [_stack(device, widths, acts, seed=20 + i) for i in range(len(rows))]
    stride = models[0].fp.n_pad + stride_extra if stride_extra else None
    fleet = DenseFleet(models, device, precision=precision, lr=list(lrs), stride=stride, schedule=schedule)
    x = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (int(sum(rows)), widths[0])).astype(np.float32))
    x = x.to(device)
    fleet.attach_ragged(x, batch, _table(rows))
    return fleet, x


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fleet_member_equals_the_model_trained_alone(cuda_device, precision):
    rows, batch, lrs = (21, 37, 7, 40, 28), 7, (1e-3, 3e-3, 1e-3, 5e-4, 1e-3)
    fleet, x = _ragged_fleet(cuda_device, precision, stride_extra=12)
    n = fleet.nflat
    assert fleet.stride > n
    for buf in (fleet.flat, fleet.m, fleet.v):
        buf[:, n:] = 7.5                                         # sentinels in the gap between two models
    fleet.train_epoch()
    torch.cuda.synchronize()
    assert fleet.launches == 1
    out = fleet.last_out
    assert tuple(out.shape) == (5, 6, 2)                          # 37 and 40 rows: six steps of 7
    t = _table(rows)
    for i in range(5):
        alone = _stack(cuda_device, (18, 20, 18), ("tanh", "sigmoid"), seed=20 + i, lr=lrs[i])
        o = _alone(alone, x[t[i, 0]:t[i, 0] + t[i, 1]], None, batch, -(-rows[i] // batch), precision)
        _assert_member(fleet, i, alone, o, out)
    for buf in (fleet.flat, fleet.m, fleet.v):
        assert bool((buf[:, n:] == 7.5).all()), "the kernel wrote between two models' parameters"
    ms = fleet.read_metrics()
    assert [m["rows"] for m in ms] == [float(r) for r in rows]
    o = out.double().cpu().numpy()
    w = np.array([7, 7, 7, 7, 7, 2.0])                            # model 1: 37 rows, the last step has two
    assert ms[1]["loss"] == pytest.approx(float((o[1, :, 0] * w).sum() / 37), rel=1e-12)
    assert ms[1]["accuracy"] == pytest.approx(float(o[1, :, 1].sum() / 37), rel=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_widths_that_need_padding(cuda_device, precision):
    """33 units: the fp32 plan pads them to 36, the bf16 plan to 48."""
    from streamml.ops.dense_fleet import DenseFleet
    name = "ragged_sigmoid_18-33-18"
    widths, acts, batch, _, _ = cases.CASES[name]
    ws, xc, _, _ = cases.arrays(name)
    models = [_stack(cuda_device, widths, acts, seed=30 + i) for i in range(3)]
    models[1].set_weights(ws)
    xs = np.random.default_rng(4).uniform(0, 1, (3, 96, 18)).astype(np.float32)
    xs[1] = xc[:96]
    x = torch.from_numpy(xs).to(cuda_device)
    fleet = DenseFleet(models, cuda_device, precision=precision, stride=models[0].fp.n_pad + 4)
    n = fleet.nflat
    for buf in (fleet.flat, fleet.m, fleet.v):
        buf[:, n:] = 7.5
    fleet.attach_rows(x, batch)
    assert list(fleet.epoch_steps()) == [3, 3, 3]
    fleet.train_epoch()
    for i in range(3):
        alone = _stack(cuda_device, widths, acts, seed=30 + i)
        if i == 1:
            alone.set_weights(ws)
        o = _alone(alone, x[i], None, batch, 3, precision)
        _assert_member(fleet, i, alone, o, fleet.last_out)
    for buf in (fleet.flat, fleet.m, fleet.v):
        assert bool((buf[:, n:] == 7.5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_more_workgroups_than_cus(cuda_device, precision):
    from streamml.ops.dense_fleet import DenseFleet
    cus = torch.cuda.get_device_properties(cuda_device).multi_processor_count
    M = cus + 3
    models = [_stack("cpu", (18, 18), ("tanh",), seed=100 + i) for i in range(M)]
    x = torch.from_numpy(np.random.default_rng(5).uniform(0, 1, (M, 64, 18)).astype(np.float32)).to(cuda_device)
    fleet = DenseFleet(models, cuda_device, precision=precision)
    fleet.attach_rows(x, 32)
    fleet.train_epoch()
    assert fleet.launches == 1
    assert torch.equal(fleet.iter, torch.full((M,), 2, dtype=torch.int64, device=cuda_device))
    for i in (0, cus - 1, cus, M - 1):
        alone = _stack(cuda_device, (18, 18), ("tanh",), seed=100 + i)
        o = _alone(alone, x[i], None, 32, 2, precision)
        _assert_member(fleet, i, alone, o, fleet.last_out)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_split_launches_and_schedule_independence(cuda_device, precision):
    """44 rows at batch 7 end in a step of two rows; 42 rows end with the sixth step."""
    rows = (44, 60, 42, 47, 90)
    one, _ = _ragged_fleet(cuda_device, precision, rows=rows)
    split, _ = _ragged_fleet(cuda_device, precision, rows=rows)
    index, _ = _ragged_fleet(cuda_device, precision, rows=rows, schedule="index")
    one.train_steps(7)
    index.train_steps(7)
    outs = []
    for k in (2, 2, 3):
        split.train_steps(k)
        outs.append(split.last_out)
    assert split.launches == 3 and one.launches == 1
    for other in (split, index):
        for buf in ("flat", "m", "v", "iter"):
            assert torch.equal(getattr(one, buf), getattr(other, buf)), buf
    assert torch.equal(one.last_out, index.last_out)
    assert torch.equal(one.last_out, torch.cat(outs, dim=1))
    assert one.iter.tolist() == [7, 7, 6, 7, 7]
    a, b = one.read_metrics(), split.read_metrics()
    assert [m["rows"] for m in a] == [m["rows"] for m in b] == [44.0, 49.0, 42.0, 47.0, 49.0]
    for ma, mb in zip(a, b):
        assert ma["loss"] == pytest.approx(mb["loss"], rel=1e-12) and ma["accuracy"] == mb["accuracy"]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["own_targets_18-8-3", "order_given"])
def test_own_targets_and_a_given_order(cuda_device, precision, name):
    """The case is member 1 of a three-model fleet; its neighbours have other weights and rows."""
    from streamml.ops.dense_fleet import DenseFleet
    widths, acts, batch, n, _ = cases.CASES[name]
    ws, xc, yc, oc = cases.arrays(name)
    steps, rows = 4, [96, 4 * batch, 50]
    rng = np.random.default_rng(6)
    models = [_stack(cuda_device, widths, acts, seed=40 + i) for i in range(3)]
    models[1].set_weights(ws)
    t = _table(rows)
    xs = rng.uniform(0, 1, (sum(rows), widths[0])).astype(np.float32)
    xs[t[1, 0]:t[1, 0] + rows[1]] = xc[:rows[1]]
    ys = None
    if yc is not None:
        ys = rng.uniform(0, 1, (sum(rows), widths[-1])).astype(np.float32)
        ys[t[1, 0]:t[1, 0] + rows[1]] = yc[:rows[1]]
    order = None
    if oc is not None:                                           # local permutations of each slice
        order = np.concatenate([rng.permutation(r) for r in rows]).astype(np.int32)
    x = torch.from_numpy(xs).to(cuda_device)
    y = None if ys is None else torch.from_numpy(ys).to(cuda_device)
    od = None if order is None else torch.from_numpy(order).to(cuda_device)
    fleet = DenseFleet(models, cuda_device, precision=precision)
    fleet.attach_ragged(x, batch, t, y=y)
    fleet.train_steps(steps, order=od)
    for i in range(3):
        alone = _stack(cuda_device, widths, acts, seed=40 + i)
        if i == 1:
            alone.set_weights(ws)
        sl = slice(int(t[i, 0]), int(t[i, 0] + t[i, 1]))
        o = _alone(alone, x[sl], None if y is None else y[sl], batch, min(steps, -(-rows[i] // batch)), precision,
                   order=None if od is None else od[sl].contiguous())
        _assert_member(fleet, i, alone, o, fleet.last_out)


@pytest.mark.gpu
def test_fleet_member_meets_the_float64_reference(cuda_device):
    from streamml.ops.dense_fleet import DenseFleet
    name = "18-64-16-64-18"
    widths, acts, batch, n, _ = cases.CASES[name]
    _, xc, _, _ = cases.arrays(name)
    ref, ref_out = cases.reference(name)
    models = [_stack(cuda_device, widths, acts, seed=51), cases.build_model(name, cuda_device),
              _stack(cuda_device, widths, acts, seed=52)]
    rows = [70, n, 33]
    t = _table(rows)
    xs = np.random.default_rng(7).uniform(0, 1, (sum(rows), 18)).astype(np.float32)
    xs[t[1, 0]:t[1, 0] + n] = xc
    fleet = DenseFleet(models, cuda_device)
    fleet.attach_ragged(torch.from_numpy(xs).to(cuda_device), batch, t)
    fleet.train_epoch()
    k = sum(a.size for a in ref.weights())
    flat, m = fleet.flat[1].double().cpu().numpy(), fleet.m[1].double().cpu().numpy()
    out = fleet.last_out[1].double().cpu().numpy()
    np.testing.assert_allclose(flat[:k], cases.flat_of(ref.weights()), **W_TOL)
    np.testing.assert_allclose(m[:k], cases.flat_of(ref.moments("m")), **M_TOL)
    assert out.shape == ref_out.shape
    np.testing.assert_allclose(out[:, 0], ref_out[:, 0], rtol=LOSS_RTOL)
    np.testing.assert_array_equal(out[:, 1], ref_out[:, 1])
    assert int(fleet.iter[1].item()) == ref.t


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_model_round_trip(cuda_device, precision, tmp_path):
    from streamml.nn import load_model
    from streamml.ops.dense_fleet import DenseFleet
    from streamml.ops.serve import DenseScoringServer
    widths, acts = (18, 24, 8, 24, 18), ("tanh", "relu", "tanh", "relu")
    models = [_stack(cuda_device, widths, acts, seed=60 + i) for i in range(3)]
    x = torch.from_numpy(np.random.default_rng(8).uniform(0, 1, (3, 96, 18)).astype(np.float32)).to(cuda_device)
    fleet = DenseFleet(models, cuda_device, precision=precision, lr=[1e-3, 2e-3, 1e-3])
    fleet.attach_rows(x, 32)
    fleet.train_epoch()
    mdl = fleet.model(1)
    assert mdl.hp["lr"] == pytest.approx(2e-3, rel=1e-6) and int(mdl.fp.iter.item()) == 3
    mdl.fit(x[1], batch_size=32, epochs=1, shuffle=False, verbose=0, engine="persistent")
    assert mdl.last_fit_engine == "persistent" and mdl.last_fit_precision == precision
    fleet.train_epoch()
    n = fleet.nflat
    for buf in ("flat", "m", "v"):
        assert torch.equal(getattr(fleet, buf)[1, :n], getattr(mdl.fp, buf)[:n]), buf
    assert int(mdl.fp.iter.item()) == int(fleet.iter[1].item()) == 6
    for a, b in zip(fleet.get_weights(1), mdl.get_weights()):
        np.testing.assert_array_equal(a, b)
    path = str(tmp_path / "member1.h5")
    mdl.save(path)
    back = load_model(path, device="cpu")
    for a, b in zip(back.get_weights(), mdl.get_weights()):
        np.testing.assert_array_equal(a, b)
    assert int(back.fp.iter.item()) == 6
    assert DenseScoringServer.supports(back) == (True, "")
    fleet.set_weights(0, mdl.get_weights())
    assert torch.equal(fleet.flat[0, :n], fleet.flat[1, :n])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_cli_trains_a_dense_fleet(cuda_device, precision, tmp_path):
    from streamml.cli import fleet as cli
    from streamml.nn import load_model
    from streamml.ops.serve import DenseScoringServer
    out = str(tmp_path / "models")
    argv = ["synthetic", "--layers", "16,8,16", "--synthetic-rows", "2048", "--synthetic-devices", "4", "--epochs", "1",
            "--batch", "32", "--out", out]
    if precision == "bf16":
        argv += ["--precision", "bf16"]
    assert cli.main(argv) == 0
    files = sorted(f for f in os.listdir(out) if f.endswith(".h5"))
    assert len(files) == 4
    with open(os.path.join(out, "index.json")) as f:
        index = json.load(f)
    assert index["engine"] == "persistent" and index["precision"] == precision and index["layers"] == [16, 8, 16]
    entries = {k: v for k, v in index.items() if k not in cli.INDEX_META}
    assert sorted(e["file"] for e in entries.values()) == files
    assert all(np.isfinite(e["loss"]) and e["loss"] > 0 for e in entries.values())
    back = load_model(os.path.join(out, files[0]), device="cpu")
    assert [w.shape for w in back.get_weights()] == [(18, 16), (16,), (16, 8), (8,), (8, 16), (16,), (16, 18), (18,)]
    assert DenseScoringServer.supports(back) == (True, "")
