"""Wide fused bulk forward of Dense stacks (dense_forward_wide.hip) against O: the float64 forward of
tests/helpers/dense_serve_ref.py with ``bf`` of tests/helpers/dense_mb_bf16_ref.py applied to both operands
of every contraction.  Reconstructions, scores and flags; the same bits wherever a row lands; loss and
accuracy sums; and through nn.Model's predict / score / detect / evaluate(engine="wide").

TOLERANCES.  Each is 2 x the largest worst-row spread that a CPU model of the device shows against O over
these very cases and seeds (203 rows each): xn in fp32, fp32 accumulation with the halves of k swapped,
+-2.4e-7 noise on tanh and sigmoid, every intermediate rounded to fp32 (``kind="V"`` of
dense_mb_bf16_ref), five noise seeds.  Measured on the CPU:

    case                 reconstruction   score
    18-512-512-512-18    1.78e-3          2.26e-4
    30-129-30            4.57e-4          1.09e-4
    32-500-33-144-32     1.44e-3          3.35e-4
    eight_layers         1.55e-3          8.98e-5
    7-7                  5.67e-8          1.64e-7
    no_bias_dropout      9.16e-8          1.05e-7
    200-64-200           4.23e-4          5.19e-5

One flipped bf16 rounding of a hidden activation moves a row that far; a dropped k-element or unit block of
a 512-wide contraction moves a row by about 4e-2, so TOL_R stays below 1e-2; the plain float64 forward lies
2.6e-3 .. 7.0e-3 from O.  The 256-wide stack of the interface test measures 3.16e-4 / 6.16e-5.  O's own scores lie within
TOL_S of the median threshold on at most 2 of the 203 rows of a case (the 5 % allowance is 10)."""
import functools

import numpy as np
import pytest
import torch

from helpers.dense_mb_bf16_ref import bf
from helpers.dense_serve_ref import forward, relerr, score
from streamml import nn
from streamml.data.cardata import normalize_affine
from streamml.nn.layers import Dense, Dropout

pytestmark = pytest.mark.gpu

TOL_R = 2 * 1.785e-3  # worst-row ||r - r_O|| / ||r_O||
TOL_S = 2 * 3.348e-4  # worst-row |s - s_O| / s_O
assert TOL_R < 1e-2
DEV = "cuda:0"

#         widths, activations, features
CASES = {
    "18-512-512-512-18": ([512, 512, 512, 18], ["tanh", "relu", "tanh", "linear"], 18),   # maximum width
    "30-129-30": ([129, 30], ["tanh", "linear"], 30),                                    # first ragged block past 128
    "32-500-33-144-32": ([500, 33, 144, 32], ["tanh", "sigmoid", "relu", "linear"], 32),   # ragged k; narrow between wide
    "eight_layers": ([136, 16, 200, 8, 144, 24, 272, 18], ["tanh"] * 7 + ["linear"], 18),  # maximum depth
    "7-7": ([7], ["linear"], 7),                                                          # a single partial block
    "no_bias_dropout": None,                                                              # bias-less layer; identity Dropout
    "200-64-200": ([64, 200], ["tanh", "linear"], 200),                                   # wide input
}


@functools.lru_cache(maxsize=None)
def _model(name, device=DEV):
    if name == "no_bias_dropout":
        m = nn.Sequential([Dense(160, "relu", use_bias=False, input_shape=(18,)), Dropout(0.3), Dense(18, "linear")],
                          device=device, seed=13)
    elif name == "256":
        m = nn.Sequential([Dense(256, "tanh", input_shape=(18,)), Dense(18, "linear")], device=device, seed=13)
    else:
        widths, acts, feat = CASES[name]
        m = nn.Sequential([Dense(u, a, input_shape=(feat,) if i == 0 else None)
                           for i, (u, a) in enumerate(zip(widths, acts))], device=device, seed=13)
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


def oracle(layers, weights, xn):
    """O: float64, both operands of every contraction rounded to bf16, nothing else rounded."""
    h = np.asarray(xn, np.float64)
    for lyr, (W, b) in zip(layers, weights):
        h = forward([lyr], [(bf(W), b)], bf(h))
    return h


@functools.lru_cache(maxsize=None)
def _reference(name, n=389, seed=13, device=DEV):
    """(raw rows, normaliser argument, float64 xn, O's reconstructions, O's scores), computed once."""
    from streamml.ops.serve import dense_layer_table
    layers, weights = dense_layer_table(_model(name, device))
    raw = np.random.default_rng(seed).uniform(0, 40, (n, layers[0][0])).astype(np.float32)
    arg, sc, sh = _normalizer(layers[0][0])
    xn = raw.astype(np.float64) * sc + sh
    y = oracle(layers, weights, xn)
    return raw, arg, xn, y, score(y, xn)


def _score_err(s, ref):
    return float(np.max(np.abs(s - ref) / ref))


@pytest.mark.parametrize("n", [1, 203])
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_bf16_oracle(cuda_device, name, n):
    from streamml.ops import dense_forward_wide as dfww
    raw, arg, _, y, ref = (a if isinstance(a, (str, tuple)) else a[:n] for a in _reference(name))
    thr = float(np.median(_reference(name)[4][:203]))   # both flag values occur among the 203 rows
    r, s, f = dfww.forward(_model(name), torch.from_numpy(raw).to(cuda_device), rec=True, score=True, threshold=thr,
                           normalizer=arg)
    assert r.dtype == torch.float32 and s.dtype == torch.float32 and f.dtype == torch.bool
    r, s, f = r.cpu().numpy(), s.cpu().numpy(), f.cpu().numpy()
    assert np.all(np.linalg.norm(y, axis=1) > 0) and np.all(ref > 0)   # the relative errors below are defined
    e_r, e_s = relerr(r, y), _score_err(s, ref)
    near = np.abs(ref - thr) <= TOL_S * thr
    print(f"{name} n={n}: reconstruction {e_r:.2e}, score {e_s:.2e}, flagged {int(f.sum())}/{n}, near {int(near.sum())}")
    assert r.shape == y.shape and s.shape == (n,) and f.shape == (n,)
    assert e_r <= TOL_R
    assert e_s <= TOL_S
    assert near.sum() <= 0.05 * 203
    assert np.array_equal(f[~near], (ref > thr)[~near])
    assert n == 1 or 0 < int((ref > thr).sum()) < n


@pytest.mark.parametrize("name", ["18-512-512-512-18", "32-500-33-144-32"])
def test_placement_does_not_change_bits(cuda_device, name):
    """389 rows (full tiles and a ragged tail for 64- and for 128-row tiles) as a strided view whose other
    columns are NaN, on ONE workgroup that loops over 128-row tiles, against the same rows contiguous on
    the default grid of 64-row tiles: over-reads, stale LDS padding and the tail tile would all show."""
    from streamml.ops import dense_forward_wide as dfww
    raw, arg, _, y, ref = _reference(name)
    D = raw.shape[1]
    big = torch.full((389, D + 5), float("nan"), device=cuda_device)
    big[:, :D] = torch.from_numpy(raw).to(cuda_device)
    m = _model(name)
    r1, s1, _ = dfww.forward(m, big[:, :D], rec=True, score=True, normalizer=arg, max_blocks=1, tile=128)
    r0, s0, _ = dfww.forward(m, big[:, :D].contiguous(), rec=True, score=True, normalizer=arg, tile=64)
    r2, s2, _ = dfww.forward(m, big[:, :D], rec=True, score=True, normalizer=arg, max_blocks=1)
    assert torch.isfinite(r1).all() and torch.isfinite(s1).all()
    for r, s in ((r0, s0), (r2, s2)):
        assert torch.equal(r1.view(torch.int32), r.view(torch.int32))
        assert torch.equal(s1.view(torch.int32), s.view(torch.int32))
    assert relerr(r1.cpu().numpy(), y) <= TOL_R and _score_err(s1.cpu().numpy(), ref) <= TOL_S


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
    targets, against float64 sums of O; the count may differ by the rows whose argmax is a close call."""
    from streamml.ops import dense_forward_wide as dfww
    name = "eight_layers" if own_targets else "18-512-512-512-18"
    raw, arg, xn, y, _ = _reference(name, 1000, 7)
    tgt = np.random.default_rng(7).uniform(0, 1, y.shape).astype(np.float32) if own_targets else xn
    x = torch.from_numpy(raw).to(cuda_device)
    loss, correct = dfww.evaluate_sums(_model(name), x, torch.from_numpy(tgt).to(cuda_device) if own_targets else None,
                                       normalizer=arg, max_blocks=2)
    want_loss = float(score(y, tgt).sum())
    want_correct = int((y.argmax(1) == np.asarray(tgt, np.float64).argmax(1)).sum())
    slack = _close_calls(y, np.asarray(tgt, np.float64))
    print(f"own_targets={own_targets}: loss {loss:.6g} / {want_loss:.6g}, correct {correct:.0f} / {want_correct}, "
          f"close calls {slack}")
    assert slack <= 10   # 1 % of the rows, for these seeds
    assert abs(loss - want_loss) <= TOL_S * want_loss
    assert abs(correct - want_correct) <= slack


def test_model_interface(cuda_device):
    """nn.Model's predict / score / detect / evaluate(engine="wide") take the kernel on a 256-wide stack and
    match O; "auto" stays on the layer loop and "fused" names its width limit; a CPU model and float64
    rows are refused with the reason; the extension's check and its Python mirror say the same."""
    from streamml.ops import dense_forward_wide as dfww
    from streamml.ops import load_c
    from streamml.ops.serve import dense_layer_table
    m = _model("256")
    raw, arg, xn, y, ref = _reference("256")
    thr = float(np.median(ref))
    s = m.score(raw, normalizer=arg, engine="wide")
    assert m.last_score_engine == "wide" and _score_err(s, ref) <= TOL_S
    f = m.detect(raw, threshold=thr, normalizer=arg, engine="wide")
    near = np.abs(ref - thr) <= TOL_S * thr
    assert f.dtype == bool and near.sum() <= 0.05 * len(ref) and np.array_equal(f[~near], (ref > thr)[~near])
    r2, s2 = m.reconstruct_and_score(raw, normalizer=arg, batch_size=100, engine="wide")   # four launches
    assert np.array_equal(s2, s) and relerr(r2, y) <= TOL_R
    # predict / evaluate read the rows as they are: feed them normalised
    xn32 = xn.astype(np.float32)
    y32 = oracle(*dense_layer_table(m), xn32)
    assert relerr(m.predict(xn32, engine="wide"), y32) <= TOL_R and m.last_predict_engine == "wide"
    loss, acc = m.evaluate(xn32, engine="wide")
    want = score(y32, xn32)
    assert m.last_evaluate_engine == "wide" and abs(loss - want.mean()) <= TOL_S * want.mean()
    assert abs(acc - np.mean(y32.argmax(1) == xn32.argmax(1))) <= _close_calls(y32, xn32.astype(np.float64)) / len(xn32)

    m.predict(xn32)
    assert m.last_predict_engine == "layers"
    with pytest.raises(ValueError, match="256 units: the limit is 128"):
        m.predict(xn32, engine="fused")
    with pytest.raises(ValueError, match="rows of dtype float64"):
        m.predict(xn, engine="wide")
    with pytest.raises(ValueError, match="not on a ROCm device"):
        _model("256", "cpu").score(raw, engine="wide")
    C = load_c()
    for widths, acts in (([18, 512, 512, 512, 18], ["tanh", "relu", "tanh", "linear"]), ([18] + [20] * 9, ["relu"] * 9),
                         ([18, 32, 5], ["relu"] * 2), ([18, 513, 18], ["relu"] * 2), ([513, 18], ["tanh"])):
        table = [[i, o, dfww.ACT[a], 0, 0] for i, o, a in zip(widths[:-1], widths[1:], acts)]
        assert C.dense_fwdw_check(table, -1, True) == dfww.check_shape(widths, acts, True)
