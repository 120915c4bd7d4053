"""The softmax + sparse-categorical-cross-entropy head of the wide Dense kernels
(csrc/include/sml_dense_head.h in dense_batch_wide.hip and dense_forward_wide.hip; ``fit`` / ``predict`` /
``evaluate(engine="wide")`` of a classifier).

The reference ``_ref`` is a numpy float64 evaluation of the SAME rounded model ("O": bf16-rounded weights
and layer inputs, fp64 contraction, log_softmax, dz rounded to bf16 before the weight gradient).  "V" is an
fp32 evaluation of that model (fp32 accumulation in another k order, fp32 softmax, the helper's noise on
tanh), "exact" the unrounded one.  Each case of CASES is the smallest shape at which one mechanism can go
wrong: one unit block with seven neutral waves and a last tile of one row; ragged spans, a layer without
bias and an l1 penalty; two blocks (the odd-block zero-fill next to the head); nine blocks (layer<2>);
layer<4>; and logits beyond +-100, where exp overflows fp32 unless the maximum is subtracted.

BOUNDS, measured on the CPU (``_measure`` below, V seeds 0, 1, 2; largest of the three):

    case          |g_V - g_O| / |g_O|   gap exact to O   loss rel V to O   max |p_V - p_O|
    w33_c2_b65    6.155e-8              -                3.456e-9          7.823e-8
    c10_g3_s2     1.331e-5              -                1.039e-6          9.250e-5
    c17_b129      4.689e-8              -                3.537e-9          3.497e-8
    c130_b200     8.349e-5              4.341e-3         1.763e-7          2.339e-6
    w512_b129     2.194e-4              4.959e-2         3.149e-7          6.110e-7
    c10_scaled    5.823e-5              -                2.152e-8          3.340e-5

TOL_G, LOSS_RTOL and TOL_P are twice the largest entry of their columns; TOL_G stays below half the
smaller gap of the two cases wider than 128, so it tells the bf16 step from an fp32 one:

    TOL_G = 2 x 2.194e-4 = 4.39e-4  <=  4.341e-3 / 2 = 2.17e-3;  LOSS_RTOL = 2 x 1.039e-6;  TOL_P = 2 x 9.250e-5

The last case's logits span -438.7 .. 477.9.

``correct`` must match exactly.  That is a fair demand: the seeds of CASES were chosen so that in the
reference no row's two largest logits are closer than 1e-3 * max|z| (``_measure`` asserts it), far above
what fp32 accumulation moves a logit by.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import dense_mb_bf16_ref as ref
from helpers.dense_mb_ref import act_fwd, act_grad

TOL_G = 2.0 * 2.194e-4
LOSS_RTOL = 2.0 * 1.039e-6
TOL_P = 2.0 * 9.250e-5
CASES = {
    "w33_c2_b65": dict(widths=(18, 33, 2), acts=("tanh",), batch=65, seed=0),
    "c10_g3_s2": dict(widths=(19, 40, 10), acts=("tanh",), batch=200, groups=3, splits=2, bias=(False, True),
                      l1=(1e-3, 0.0), seed=0),
    "c17_b129": dict(widths=(30, 64, 17), acts=("relu",), batch=129, seed=1),
    "c130_b200": dict(widths=(18, 144, 130), acts=("tanh",), batch=200, seed=2),
    "w512_b129": dict(widths=(30, 512, 32, 512), acts=("tanh", "relu"), batch=129, seed=3),
    "c10_scaled": dict(widths=(19, 40, 10), acts=("tanh",), batch=64, scale=400.0, seed=0),
}


def _spec(case):
    return ref.Spec(case["widths"], case["acts"] + ("linear",), case.get("bias"), case.get("l1"))


@functools.lru_cache(maxsize=None)
def _arrays(name, rows=None):
    """(weights in FlatParams order, x, labels) of a case: Glorot kernels (the last one times ``scale``),
    small biases, uniform rows, uniform labels with every class present where the rows allow."""
    case = CASES[name]
    widths, spec = case["widths"], _spec(case)
    rng = np.random.default_rng([41, case["seed"], len(name), widths[1]])
    ws = []
    for l, (fin, fout) in enumerate(zip(widths[:-1], widths[1:])):
        lim = np.sqrt(6.0 / (fin + fout)) * (case.get("scale", 1.0) if l == spec.nl - 1 else 1.0)
        ws.append(rng.uniform(-lim, lim, size=(fin, fout)).astype(np.float32))
        if spec.bias[l]:
            ws.append(rng.uniform(-0.1, 0.1, size=(fout,)).astype(np.float32))
    n, C = rows or case["batch"], widths[-1]
    x = rng.uniform(0, 1, size=(n, widths[0])).astype(np.float32)
    labels = rng.integers(0, C, size=n)
    if n >= C:
        labels[rng.permutation(n)[:C]] = np.arange(C)
    return ws, x, labels.astype(np.int64)


def _ref(name, kind="O", seed=0, rows=None):
    """(loss incl. penalties, correct rows, gradients in the order of the weights, probabilities, logits)
    of one step over the case's rows."""
    spec = _spec(CASES[name])
    ws, x, labels = _arrays(name, rows)
    V = kind == "V"
    rb = (lambda a: np.asarray(a, np.float64)) if kind == "exact" else ref.bf
    mm = ref._mm32_halves if V else ref._mm64
    ft = np.float32 if V else np.float64
    r32 = lambda a: np.asarray(a, ft).astype(np.float64)
    rng = np.random.default_rng([seed, 77])
    ws = [np.asarray(w, np.float64) for w in ws]
    Ws, bs = [], []
    for l in range(spec.nl):
        Ws.append(ws.pop(0))
        bs.append(ws.pop(0) if spec.bias[l] else None)
    B, hs = x.shape[0], [np.asarray(x, np.float64)]
    for l in range(spec.nl):
        z = mm(rb(hs[-1]), rb(Ws[l]))
        z = r32(z + bs[l]) if bs[l] is not None else z
        h = act_fwd(spec.acts[l], z)
        if V and spec.acts[l] == "tanh":
            h = h + rng.uniform(-ref.NOISE, ref.NOISE, size=h.shape)
        hs.append(r32(h))
    z = hs[-1].astype(ft)
    zs = z - z.max(-1, keepdims=True)
    lsm = zs - np.log(np.exp(zs).sum(-1, keepdims=True, dtype=ft))
    p = np.exp(lsm).astype(np.float64)
    loss = float(-lsm[np.arange(B), labels].astype(np.float64).mean())
    for l in range(spec.nl):
        loss += (spec.l1[l] * np.abs(hs[l + 1]).sum() + spec.l2[l] * (hs[l + 1] ** 2).sum()) / B
    correct = int((z.argmax(-1) == labels).sum())
    g = p.copy()
    g[np.arange(B), labels] -= 1.0
    g, gl = r32(g / B), []
    for l in range(spec.nl - 1, -1, -1):
        h = hs[l + 1]
        if l < spec.nl - 1:
            g = r32(g + (spec.l1[l] * np.sign(h) + 2.0 * spec.l2[l] * h) / B)
        dz = r32(g * act_grad(spec.acts[l], h))
        gl = [mm(rb(hs[l]).T, rb(dz))] + ([r32(dz.sum(0))] if spec.bias[l] else []) + gl
        g = mm(rb(dz), rb(Ws[l]).T)
    return loss, correct, gl, p, hs[-1]


_oracle = functools.lru_cache(maxsize=None)(lambda name, rows=None: _ref(name, "O", rows=rows))


def _measure():
    """Prints the docstring's table; asserts the condition on the logits that makes ``correct`` exact."""
    for name in CASES:
        lo, _, go, po, z = _oracle(name)
        top = np.sort(z, -1)[:, -2:]
        assert (top[:, 1] - top[:, 0]).min() > 1e-3 * np.abs(z).max(), (name, (top[:, 1] - top[:, 0]).min(), np.abs(z).max())
        v = [_ref(name, "V", s) for s in range(3)]
        gap = ref.relerr(_ref(name, "exact")[2], go) if max(CASES[name]["widths"]) > 128 else float("nan")
        print(f"{name:14s}{max(ref.relerr(r[2], go) for r in v):.3e}   {gap:.3e}   {max(abs(r[0] - lo) / lo for r in v):.3e}"
              f"   {max(np.abs(r[3] - po).max() for r in v):.3e}   span {z.min():.1f}..{z.max():.1f}")


def _model(name, device):
    from streamml import nn
    from streamml.nn.layers import L1L2, Dense
    spec = _spec(CASES[name])
    layers = []
    for l in range(spec.nl):
        reg = L1L2(spec.l1[l], spec.l2[l]) if (spec.l1[l] or spec.l2[l]) else None
        layers.append(Dense(spec.widths[l + 1], "softmax" if l == spec.nl - 1 else spec.acts[l], use_bias=spec.bias[l],
                            activity_regularizer=reg, input_shape=(spec.widths[0],) if l == 0 else None))
    model = nn.Sequential(layers, device=device, seed=1)
    model.compile(loss="sparse_categorical_crossentropy", metrics=["accuracy"])
    model.set_weights(_arrays(name)[0])
    return model


def _dev(a, device):
    return torch.from_numpy(a).to(device)


def _state(model):
    return [getattr(model.fp, buf).clone() for buf in ("flat", "m", "v", "iter")]


def _bits_equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(_state(a), _state(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_step_matches_the_reference_and_repeats_its_bits(cuda_device, name):
    from streamml.ops import dense_batch_wide as dbw
    case, spec = CASES[name], _spec(CASES[name])
    ws, x, labels = _arrays(name)
    model = _model(name, cuda_device)
    kw = dict(groups=case.get("groups"), splits=case.get("splits"))
    g, loss, correct = dbw.grad_step(model, _dev(x, cuda_device), _dev(labels, cuda_device), **kw)
    g2, loss2, _ = dbw.grad_step(model, _dev(x, cuda_device), _dev(labels[:, None], cuda_device).int(), **kw)
    assert torch.equal(g, g2) and loss == loss2
    lo, co, go, _, _ = _oracle(name)
    n, g = spec.nparams(), g.double().cpu().numpy()
    eo = ref.relerr([g[:n]], go)
    print(f"{name}: |g-gO|/|gO| {eo:.3e}  loss {loss:.6f} rel {abs(loss - lo) / lo:.3e}  correct {correct}/{co}")
    assert np.isfinite(loss) and eo <= TOL_G, (name, eo)
    if max(case["widths"]) > 128:
        assert 4.0 * eo <= ref.relerr([g[:n]], _ref(name, "exact")[2]), name
    assert abs(loss - lo) <= LOSS_RTOL * abs(lo), (name, loss, lo)
    assert correct == co and not g[n:].any()


@pytest.mark.gpu
def test_three_steps_are_three_single_steps(cuda_device):
    from streamml.ops import dense_batch_wide as dbw
    name, B = "c10_g3_s2", 200
    _, x, labels = _arrays(name, 500)
    x, labels = _dev(x, cuda_device), _dev(labels, cuda_device)
    order = torch.randperm(500, generator=torch.Generator().manual_seed(3)).int().to(cuda_device)
    a, b = _model(name, cuda_device), _model(name, cuda_device)
    oa = dbw.train_steps(a, x, labels, B, 3, order=order, groups=3, splits=2)   # the last step is 100 rows
    for s in range(3):
        assert torch.equal(dbw.train_steps(b, x, labels, B, 1, row0=s * B, order=order, groups=3, splits=2)[0], oa[s])
    assert int(a.fp.iter.item()) == 3 and _bits_equal(a, b) and bool((oa[:, 0] > 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w33_c2_b65", "c130_b200", "w512_b129", "c10_scaled"])
def test_predict_and_evaluate_match_the_reference(cuda_device, name):
    from streamml.ops import dense_batch_wide as dbw
    from streamml.ops import dense_forward_wide as dfww
    _, x, labels = _arrays(name)
    lo, co, _, po, _ = _oracle(name)
    model, C = _model(name, cuda_device), CASES[name]["widths"][-1]
    p = model.predict(x, engine="wide")
    assert model.last_predict_engine == "wide" and p.shape == po.shape
    print(f"{name}: max |p - pO| {np.abs(p - po).max():.3e}  max |sum - 1| {np.abs(p.sum(-1, dtype=np.float64) - 1).max():.3e}")
    assert np.abs(p - po).max() <= TOL_P
    assert np.abs(p.sum(-1, dtype=np.float64) - 1.0).max() <= 4 * np.finfo(np.float32).eps * C
    xd = _dev(x, cuda_device)
    for kw in (dict(tile=64), dict(tile=128), dict(max_blocks=1)):
        assert torch.equal(dfww.forward(model, xd, head=True, **kw)[0].cpu(), torch.from_numpy(p)), kw
    loss, acc = model.evaluate(x, labels, engine="wide")
    assert model.last_evaluate_engine == "wide"
    assert abs(loss - lo) <= LOSS_RTOL * abs(lo) and acc == co / len(x), (loss, lo, acc, co)
    assert abs(loss - dbw.grad_step(model, xd, _dev(labels, cuda_device))[1]) <= LOSS_RTOL * abs(lo)
    with pytest.raises(ValueError, match="scores need a reconstruction, not a softmax head"):
        dfww.forward(model, xd, score=True, head=True)


@pytest.mark.gpu
def test_fit_wide_of_a_classifier_is_train_steps_with_the_layer_loops_batches(cuda_device):
    from streamml import nn
    from streamml.nn.layers import Dense
    from streamml.ops import dense_batch_wide as dbw
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, size=(512, 18)).astype(np.float32)
    y = (x[:, 0] > x[:, 1]).astype(np.int64)   # separable
    models = []
    for _ in range(2):
        m = nn.Sequential([Dense(64, "tanh", input_shape=(18,)), Dense(2, "softmax")], device=cuda_device, seed=1)
        m.compile(loss="sparse_categorical_crossentropy", metrics=["accuracy"])
        models.append(m)
    a, b = models
    hist = a.fit(x, y, batch_size=128, epochs=1, verbose=0, seed=7, shuffle=True, engine="wide")
    assert a.last_fit_engine == "wide" and int(a.fp.iter.item()) == 4
    order = torch.from_numpy(np.random.default_rng([7, 0, 0]).permutation(512).astype(np.int32)).to(cuda_device)
    out = dbw.train_steps(b, _dev(x, cuda_device), _dev(y, cuda_device), 128, 4, 0, order)
    assert _bits_equal(a, b)
    assert abs(hist.history["loss"][0] - float(out[:, 0].double().mean())) < 1e-6
    with pytest.raises(ValueError, match="labels span"):
        a.fit(x, y + 1, batch_size=128, epochs=1, verbose=0, engine="wide")
