"""Fused bulk forward of Dense stacks (dense_forward.hip) against the float64 reference of
tests/helpers/dense_serve_ref.py: reconstructions, scores and flags; the same bits wherever a row lands;
loss and accuracy sums; and through nn.Model's predict / score / detect / evaluate."""
import functools

import numpy as np
import pytest
import torch

from helpers.dense_serve_ref import forward, relerr, score
from streamml import nn
from streamml.data.cardata import normalize_affine
from streamml.nn.layers import Dense, Dropout

pytestmark = pytest.mark.gpu

TOL = 1e-4      # what tests/test_dense_serve_gpu.py holds the fp32 per-event scorers to, same act_fwd
DEV = "cuda:0"

#         widths, activations, features
CASES = {
    "18-64-16-64-18": ([64, 16, 64, 18], ["tanh", "relu", "tanh", "linear"], 18),     # cardata normaliser
    "18-33-18": ([33, 18], ["tanh", "relu"], 18),                                     # ragged unit block; skipped k-slices
    "30-128-32-128-30": ([128, 32, 128, 30], ["tanh", "relu", "tanh", "linear"], 30),  # maximum width; 64 KiB image
    "eight_layers": ([24, 16, 12, 8, 12, 16, 24, 18], ["tanh"] * 7 + ["linear"], 18),  # maximum depth
    "7-7": ([7], ["linear"], 7),                                                      # a single partial block
    "no_bias_dropout": None,                                                          # bias-less layer; identity Dropout
    "sigmoid_head": ([20, 18], ["relu", "sigmoid"], 18),
}


@functools.lru_cache(maxsize=None)
def _model(name):
    if name == "no_bias_dropout":
        m = nn.Sequential([Dense(40, "relu", use_bias=False, input_shape=(18,)), Dropout(0.3), Dense(18, "linear")],
                          device=DEV, seed=13)
    elif name == "wide":
        m = nn.Sequential([Dense(256, "tanh", input_shape=(18,)), Dense(18, "linear")], device=DEV, seed=13)
    else:
        widths, acts, feat = CASES[name]
        m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                           for i, (u, a) in enumerate(zip(widths, acts))], device=DEV, seed=13)
    # Keras initialises biases to zero, which would hide a misplaced bias: draw them
    rng = np.random.default_rng(13)
    m.set_weights([w if w.ndim == 2 else rng.uniform(-0.5, 0.5, w.shape).astype(np.float32)
                   for w in m.get_weights()])
    return m


def _normalizer(features):
    """cardata's for 18 features, else a (scale, shift) pair."""
    if features == 18:
        sc, sh = normalize_affine()
        return "cardata", np.asarray(sc, np.float32), np.asarray(sh, np.float32)
    sc, sh = np.full(features, 1 / 40, np.float32), np.linspace(-0.7, -0.3, features).astype(np.float32)
    return (sc, sh), sc, sh


@functools.lru_cache(maxsize=None)
def _reference(name, n=389, seed=13):
    """(raw rows, normaliser argument, float64 xn, float64 reconstructions, float64 scores), computed once."""
    from streamml.ops.serve import dense_layer_table
    layers, weights = dense_layer_table(_model(name))
    raw = np.random.default_rng(seed).uniform(0, 40, (n, layers[0][0])).astype(np.float32)
    arg, sc, sh = _normalizer(layers[0][0])
    xn = raw.astype(np.float64) * sc + sh
    y = forward(layers, weights, xn)
    return raw, arg, xn, y, score(y, xn)


@pytest.mark.parametrize("n", [1, 203])
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_float64_reference(cuda_device, name, n):
    from streamml.ops import dense_forward as dfw
    raw, arg, _, y, ref = (a if isinstance(a, (str, tuple)) else a[:n] for a in _reference(name))
    thr = float(np.median(_reference(name)[4][:203]))   # both flag values occur among the 203 rows
    r, s, f = dfw.forward(_model(name), torch.from_numpy(raw).to(cuda_device), rec=True, score=True, threshold=thr,
                          normalizer=arg)
    r, s, f = r.cpu().numpy(), s.cpu().numpy(), f.cpu().numpy()
    assert np.all(np.linalg.norm(y, axis=1) > 0) and np.all(ref > 0)   # the relative errors below are defined
    e_r, e_s = relerr(r, y), float(np.max(np.abs(s - ref) / ref))
    print(f"{name} n={n}: reconstruction {e_r:.2e}, score {e_s:.2e}, flagged {int(f.sum())}/{n}")
    assert r.shape == y.shape and s.shape == (n,) and f.shape == (n,) and f.dtype == bool
    assert e_r <= TOL
    assert e_s <= TOL
    near = np.abs(ref - thr) <= TOL * thr
    assert np.array_equal(f[~near], (ref > thr)[~near])
    assert n == 1 or 0 < int((ref > thr).sum()) < n


@pytest.mark.parametrize("name", ["18-64-16-64-18", "30-128-32-128-30"])
def test_placement_does_not_change_bits(cuda_device, name):
    """389 rows (24 tiles and a tail of 5 rows) as a strided view whose other columns are NaN, on ONE
    workgroup that loops, against the same rows contiguous on the default grid: over-reads, unzeroed
    padding, the prefetch hand-over and the tail tile would all show."""
    from streamml.ops import dense_forward as dfw
    raw, arg, _, y, ref = _reference(name)
    D = raw.shape[1]
    big = torch.full((389, D + 5), float("nan"), device=cuda_device)
    big[:, :D] = torch.from_numpy(raw).to(cuda_device)
    m = _model(name)
    r1, s1, _ = dfw.forward(m, big[:, :D], rec=True, score=True, normalizer=arg, max_blocks=1)
    r0, s0, _ = dfw.forward(m, big[:, :D].contiguous(), rec=True, score=True, normalizer=arg)
    assert torch.isfinite(r1).all() and torch.isfinite(s1).all()
    assert torch.equal(r1.view(torch.int32), r0.view(torch.int32))
    assert torch.equal(s1.view(torch.int32), s0.view(torch.int32))
    assert relerr(r1.cpu().numpy(), y) <= TOL and float(np.max(np.abs(s1.cpu().numpy() - ref) / ref)) <= TOL


def _close_calls(*arrays):
    """Rows whose float64 top-two margin, in any of the arrays, is below 1e-4 of the maximum."""
    close = np.zeros(len(arrays[0]), bool)
    for a in arrays:
        top = np.sort(a, axis=1)[:, -2:]
        close |= (top[:, 1] - top[:, 0]) < 1e-4 * np.abs(top[:, 1])
    return int(close.sum())


@pytest.mark.parametrize("own_targets", [False, True])
def test_sums_mode(cuda_device, own_targets):
    """Loss and correct-row sums over 1000 rows on two workgroups, y = x (the normalised row) and own
    targets, against float64; the count may differ by the rows whose argmax is a close call."""
    from streamml.ops import dense_forward as dfw
    name = "eight_layers" if own_targets else "18-64-16-64-18"
    raw, arg, xn, y, _ = _reference(name, 1000, 7)
    tgt = np.random.default_rng(7).uniform(0, 1, y.shape).astype(np.float32) if own_targets else xn
    x = torch.from_numpy(raw).to(cuda_device)
    loss, correct = dfw.evaluate_sums(_model(name), x, torch.from_numpy(tgt).to(cuda_device) if own_targets else None,
                                      normalizer=arg, max_blocks=2)
    want_loss = float(score(y, tgt).sum())
    want_correct = int((y.argmax(1) == np.asarray(tgt, np.float64).argmax(1)).sum())
    slack = _close_calls(y, np.asarray(tgt, np.float64))
    print(f"own_targets={own_targets}: loss {loss:.6g} / {want_loss:.6g}, correct {correct:.0f} / {want_correct}, "
          f"close calls {slack}")
    assert slack <= 10   # 1 % of the rows, for these seeds
    assert abs(loss - want_loss) <= TOL * want_loss
    assert abs(correct - want_correct) <= slack and 0 < want_correct < 1000


def test_model_interface(cuda_device):
    """nn.Model's predict / score / detect / evaluate take the kernel and match the float64 reference; a
    256-wide stack stays on the layer loop under "auto" and names the width limit under "fused"; the
    extension's check and its Python mirror say the same."""
    from streamml.ops import dense_forward as dfw
    from streamml.ops import load_c
    name = "18-64-16-64-18"
    m = _model(name)
    raw, arg, xn, y, ref = _reference(name)
    thr = float(np.median(ref))
    s = m.score(raw, normalizer=arg)
    assert m.last_score_engine == "fused" and float(np.max(np.abs(s - ref) / ref)) <= TOL
    f = m.detect(raw, threshold=thr, normalizer=arg)
    near = np.abs(ref - thr) <= TOL * thr
    assert f.dtype == bool and np.array_equal(f[~near], (ref > thr)[~near])
    r2, s2 = m.reconstruct_and_score(raw, normalizer=arg, batch_size=100)   # four launches
    assert np.array_equal(s2, s) and relerr(r2, y) <= TOL
    # predict / evaluate read the rows as they are: feed them normalised
    xn32 = xn.astype(np.float32)
    from streamml.ops.serve import dense_layer_table
    y32 = forward(*dense_layer_table(m), xn32)
    assert relerr(m.predict(xn32), y32) <= TOL and m.last_predict_engine == "fused"
    loss, acc = m.evaluate(xn32)
    want = score(y32, xn32)
    assert m.last_evaluate_engine == "fused" and abs(loss - want.mean()) <= TOL * want.mean()
    assert abs(acc - np.mean(y32.argmax(1) == xn32.argmax(1))) <= _close_calls(y32, xn32.astype(np.float64)) / len(xn32)
    assert m.predict(xn32, engine="layers").shape == y32.shape and m.last_predict_engine == "layers"

    wide = _model("wide")
    wide.predict(xn32)
    assert wide.last_predict_engine == "layers"
    with pytest.raises(ValueError, match="256 units: the limit is 128"):
        wide.predict(xn32, engine="fused")
    with pytest.raises(ValueError, match="256 units: the limit is 128"):
        wide.score(raw, engine="fused")
    C = load_c()
    for widths, acts in (([18, 256, 18], ["tanh", "linear"]), ([18] + [20] * 9, ["relu"] * 9), ([18, 32, 5], ["relu"] * 2),
                         ([128] * 5, ["relu"] * 4), ([18, 64, 18], ["tanh", "linear"])):
        table = [[i, o, dfw.ACT[a], 0, 0] for i, o, a in zip(widths[:-1], widths[1:], acts)]
        assert C.dense_fwd_check(table, -1, True) == dfw.check_shape(widths, acts, True)
