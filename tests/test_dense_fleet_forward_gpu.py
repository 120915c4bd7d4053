"""Fused bulk forward of a fleet of Dense stacks (dense_forward_fleet.hip) against the float64 reference
of tests/helpers/dense_serve_ref.py and, bit for bit, against the single-model kernel; the per-model
sums of DenseFleet.evaluate; calibrate_thresholds against np.quantile and the fleet scorer."""
import functools

import numpy as np
import pytest
import torch

from helpers.dense_serve_ref import forward, relerr, score
from streamml import nn
from streamml.data.cardata import normalize_affine
from streamml.nn.layers import Dense
from streamml.nn.model import Adam
from streamml.ops.serve import dense_layer_table

pytestmark = pytest.mark.gpu

TOL = 1e-4      # what tests/test_dense_forward_gpu.py holds this arithmetic to
DEV = "cuda:0"

#         widths, activations, features, normaliser
STACKS = {
    "18-33-18": ([33, 18], ["tanh", "relu"], 18, None),
    "18-64-16-64-18": ([64, 16, 64, 18], ["tanh", "relu", "tanh", "linear"], 18, "cardata"),
    "30-128-32-128-30": ([128, 32, 128, 30], ["tanh", "relu", "tanh", "linear"], 30, None),
    "64-128-128-64": ([128, 128, 64], ["tanh", "relu", "linear"], 64, None),              # the one-buffer plan
}
ROWS = [1, 0, 17, 32, 33, 203]
ORDER, GAP = [5, 2, 0, 4, 3, 1], 7       # members in the order their slices lie in memory; a gap after the third


def member(name, seed, device=DEV):
    widths, acts, feat, _ = STACKS[name]
    m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None) for i, (u, a) in enumerate(zip(widths, acts))],
                      device=device, seed=seed)
    m.compile(optimizer=Adam(learning_rate=1e-3), loss="mean_squared_error", metrics=["accuracy"])
    rng = np.random.default_rng(seed)   # Keras biases start at zero, which would hide a misplaced bias
    m.set_weights([w if w.ndim == 2 else rng.uniform(-0.5, 0.5, w.shape).astype(np.float32) for w in m.get_weights()])
    return m


def reference(name, models, table, n, seed):
    """(raw rows, float64 xn, reconstructions and scores with NaN where no slice covers), computed once."""
    feat, norm = STACKS[name][2], STACKS[name][3]
    raw = np.random.default_rng(seed).uniform(0, 40 if norm else 1, (n, feat)).astype(np.float32)
    sc, sh = normalize_affine() if norm else (1.0, 0.0)
    xn = raw.astype(np.float64) * sc + sh
    y, s = np.full((n, feat), np.nan), np.full(n, np.nan)
    for mdl, (first, rows) in zip(models, table):
        layers, weights = dense_layer_table(mdl)
        y[first:first + rows] = forward(layers, weights, xn[first:first + rows])
    covered = ~np.isnan(y[:, 0])
    s[covered] = score(y[covered], xn[covered])
    return raw, xn, y, s


@functools.lru_cache(maxsize=None)
def ragged(name):
    from streamml.ops.dense_fleet import DenseFleet
    models = [member(name, 20 + i) for i in range(len(ROWS))]
    table, at = np.zeros((len(ROWS), 2), np.int64), 0
    for k, m in enumerate(ORDER):
        table[m] = (at, ROWS[m])
        at += ROWS[m] + (GAP if k == 2 else 0)
    return DenseFleet(models, DEV), models, table, reference(name, models, table, at, 5)


@pytest.mark.parametrize("name", list(STACKS))
def test_float64_reference_and_bit_identity(cuda_device, name):
    from streamml.ops import dense_forward as dfw
    fleet, models, table, (raw, _, y, ref) = ragged(name)
    norm = STACKS[name][3]
    x = torch.from_numpy(raw).to(cuda_device)
    thr = np.array([np.median(ref[f:f + r]) if r else 0.0 for f, r in table], np.float32)
    runs = [fleet.reconstruct_and_score(x, table, normalizer=norm, thresholds=thr, max_blocks=mb) for mb in (1, 3, 0)]
    r, s, f = (t.cpu().numpy() for t in runs[0])
    covered = ~np.isnan(ref)
    assert covered.sum() == sum(ROWS) and len(ref) == sum(ROWS) + GAP and fleet.last_forward_launches == 1
    assert np.isnan(r[~covered]).all() and np.isnan(s[~covered]).all() and not f[~covered].any()
    for r2, s2, f2 in runs[1:]:     # one workgroup through every image switch; boundaries inside models; a CU each
        assert torch.equal(r2.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(s2.view(torch.int32), runs[0][1].view(torch.int32)) and torch.equal(f2, runs[0][2])
    for i, (first, rows) in enumerate(table):
        if rows == 0:
            continue
        sl = slice(first, first + rows)
        e_r, e_s = relerr(r[sl], y[sl]), float(np.max(np.abs(s[sl] - ref[sl]) / ref[sl]))
        print(f"{name} member {i} ({rows} rows): reconstruction {e_r:.2e}, score {e_s:.2e}")
        assert e_r <= TOL and e_s <= TOL
        near = np.abs(ref[sl] - thr[i]) <= TOL * thr[i]
        assert np.array_equal(f[sl][~near], (ref[sl] > thr[i])[~near])
        r1, s1, _ = dfw.forward(fleet.model(i), x[sl], rec=True, score=True, normalizer=norm)
        assert torch.equal(r1.view(torch.int32), runs[0][0][sl].view(torch.int32))
        assert torch.equal(s1.view(torch.int32), runs[0][1][sl].view(torch.int32))


EVAL_ROWS = [200, 203, 197, 201, 199]
EVAL_SEED = 12      # rows and targets: the float64 close calls stay under 1 % of every member (checked on the CPU)


def eval_case(own_targets, device=DEV):
    """(models, table, raw rows, targets or None, float64 loss sums, correct rows, close calls per member)."""
    name = "18-33-18" if own_targets else "18-64-16-64-18"
    models = [member(name, 40 + i, device) for i in range(5)]
    table = np.stack([np.cumsum([0] + EVAL_ROWS[:-1]), EVAL_ROWS], axis=1).astype(np.int64)
    raw, xn, y, s = reference(name, models, table, sum(EVAL_ROWS), EVAL_SEED)
    tgt = np.random.default_rng(EVAL_SEED).uniform(0, 1, y.shape).astype(np.float32) if own_targets else None
    want = np.asarray(tgt, np.float64) if own_targets else xn
    loss, correct, close = [], [], []
    for first, rows in table:
        a, b = y[first:first + rows], want[first:first + rows]
        loss.append(score(a, b).sum())
        correct.append(int((a.argmax(1) == b.argmax(1)).sum()))
        tops = [np.sort(v, axis=1)[:, -2:] for v in (a, b)]
        close.append(int(np.any([(t[:, 1] - t[:, 0]) < 1e-4 * np.abs(t[:, 1]) for t in tops], axis=0).sum()))
    return name, models, table, raw, tgt, np.array(loss), np.array(correct), np.array(close)


@pytest.mark.parametrize("own_targets", [False, True])
def test_per_model_sums(cuda_device, own_targets):
    """Two workgroups: member 2 is split between them, and its two slots fold into one entry."""
    from streamml.ops.dense_fleet import DenseFleet
    name, models, table, raw, tgt, loss, correct, close = eval_case(own_targets)
    fleet = DenseFleet(models, DEV)
    got = fleet.evaluate(torch.from_numpy(raw).to(cuda_device), table,
                         y=torch.from_numpy(tgt).to(cuda_device) if own_targets else None,
                         normalizer=STACKS[name][3], max_blocks=2)
    assert (close <= 0.01 * table[:, 1]).all()   # for these seeds, checked on the CPU
    for i, g in enumerate(got):
        rows = int(table[i, 1])
        got_correct = round(g["accuracy"] * rows)    # the count behind the ratio
        print(f"own_targets={own_targets} member {i}: loss {g['loss']:.6g} / {loss[i] / rows:.6g}, "
              f"correct {got_correct} / {correct[i]}, close calls {close[i]}")
        assert g["rows"] == rows and abs(g["loss"] * rows - loss[i]) <= TOL * loss[i]
        assert abs(got_correct - correct[i]) <= close[i]


def test_calibrate_thresholds(cuda_device):
    name = "18-64-16-64-18"
    fleet, _, table, (raw, _, _, ref) = ragged(name)
    x = torch.from_numpy(raw).to(cuda_device)
    with pytest.raises(ValueError, match="model 1 has no rows"):
        fleet.calibrate_thresholds(0.9, x, table, normalizer="cardata")
    table1 = table.copy()
    table1[1] = (int(np.flatnonzero(np.isnan(ref))[0]), GAP)    # the member without rows takes the gap
    thr = fleet.calibrate_thresholds(0.9, x, table1, normalizer="cardata")
    s = fleet.score(x, table1, normalizer="cardata").cpu().numpy()
    want = np.array([np.quantile(s[f:f + r], 0.9, method="higher") for f, r in table1], np.float32)
    assert thr.dtype == np.float32 and np.array_equal(thr, want)
    flags = fleet.detect(x, table1, thresholds=thr, normalizer="cardata").cpu().numpy()
    server = fleet.server(thresholds=thr, normalizer="cardata")
    idx = np.concatenate([np.full(r, m) for m, (f, r) in enumerate(table1)])
    pos = np.concatenate([np.arange(f, f + r) for f, r in table1])
    _, sf = server.score(raw[pos], idx)
    far = np.abs(s[pos] - thr[idx]) > TOL * thr[idx]
    assert np.array_equal(sf[far], flags[pos][far]) and 0 < flags.sum() < len(pos)
