"""The fused MNIST-classifier train step (mlp_step.hip) against a float64 numpy oracle.

Tolerance rule: the layer path (``engine="layers"``) runs from the same seed in the same test; both are
fp32 chains that differ only in order, so the fused step may show at most 4x the layer path's max-norm
relative error against the oracle, plus a floor of 1e-7 (about one fp32 rounding of the largest
element)."""
import numpy as np
import pytest
import torch

from streamml.models.mlp import MLPClassifier
from streamml.ops import mlp_step

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-7)


def _data(n, features, classes, u8, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, features), dtype=np.uint8) if u8 else rng.uniform(0, 1, (n, features)).astype(np.float32)
    return x, rng.integers(0, classes, n).astype(np.int64)


def _model(dev, features, hidden, classes, rate):
    return MLPClassifier(hidden=hidden, classes=classes, input_shape=(features,), dropout=rate, device=dev, seed=3)


def _oracle(model, x, y, batches):
    """float64 Keras steps over the index batches from the model's present state, with the kernels'
    own Dropout multipliers: (flat, m, v, [(loss sum, correct)] per step)."""
    from streamml.ops import load_c
    W1, b1, W2, b2 = [a.astype(np.float64) for a in model.fp.get()]
    p = [W1, b1, W2, b2]
    m, v = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    xf = x.astype(np.float64) / 255.0 if x.dtype == np.uint8 else x.astype(np.float64)
    keep = np.float32(1.0 - model.dropout)
    pairs = []
    for s, idx in enumerate(batches):
        xb, yb, B = xf[idx], y[idx], len(idx)
        h = np.maximum(xb @ p[0] + p[1], 0.0)
        if model.dropout > 0:
            h = h * load_c().mlp_dropout_mask(model.fp.flat, B, model.hidden, float(keep), model._seed, s).cpu().numpy()
        z = h @ p[2] + p[3]
        e = np.exp(z - z.max(1, keepdims=True))
        pr = e / e.sum(1, keepdims=True)
        pairs.append((-np.log(pr[np.arange(B), yb]).sum(), float((z.argmax(1) == yb).sum())))
        dz = pr.copy()
        dz[np.arange(B), yb] -= 1.0
        dz /= B
        dh = (dz @ p[2].T) * (h > 0) * float(np.float32(1.0) / keep)
        g = [xb.T @ dh, dh.sum(0), h.T @ dz, dz.sum(0)]
        t = s + 1
        lr_t = HP["lr"] * np.sqrt(1 - HP["b2"] ** t) / (1 - HP["b1"] ** t)
        for i in range(4):
            m[i] = HP["b1"] * m[i] + (1 - HP["b1"]) * g[i]
            v[i] = HP["b2"] * v[i] + (1 - HP["b2"]) * g[i] * g[i]
            p[i] = p[i] - lr_t * m[i] / (np.sqrt(v[i]) + HP["eps"])
    return tuple(np.concatenate([a.ravel() for a in t]) for t in (p, m, v)) + (pairs,)


def _err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _state(model):
    n = model.fp.n
    return [t[:n].cpu().numpy() for t in (model.fp.flat, model.fp.m, model.fp.v)] + [model._acc.cpu().numpy()]


@pytest.mark.parametrize("batch,features,hidden,classes,u8,rate", [
    (1, 784, 128, 10, True, 0.0),
    (32, 784, 512, 10, True, 0.2),
    (17, 37, 70, 3, False, 0.0),
    (5, 100, 65, 2, False, 0.5),
], ids=["b1_mnist128", "b32_mnist512_dropout", "b17_in37_h70_c3", "b5_in100_h65_c2_dropout"])
def test_three_steps_against_float64(cuda_device, batch, features, hidden, classes, u8, rate):
    n = 3 * batch
    x, y = _data(n, features, classes, u8, seed=batch)
    order = np.random.default_rng(5).permutation(n)       # what fit(seed=5) draws
    ref = _model(cuda_device, features, hidden, classes, rate)
    *want, pairs = _oracle(ref, x, y, [order[s * batch:(s + 1) * batch] for s in range(3)])
    want.append(np.sum(np.asarray(pairs), axis=0))
    errs = {}
    for engine in ("layers", "fused"):
        model = _model(cuda_device, features, hidden, classes, rate)
        model.fit(x, y, epochs=1, batch_size=batch, seed=5, verbose=0, engine=engine)
        assert model.last_fit_engine == engine and int(model.fp.iter.item()) == 3 and model._step == 3
        errs[engine] = [_err(g, w) for g, w in zip(_state(model), want)]
    print("max-norm relative error of flat, m, v, (loss, correct):", errs)
    for name, lay, fus in zip(("flat", "m", "v", "(loss, correct)"), errs["layers"], errs["fused"]):
        assert fus <= 4.0 * lay + 1e-7, (name, lay, fus)


def test_bits_do_not_depend_on_the_split(cuda_device):
    batch, features, hidden, classes = 19, 100, 130, 10
    x, y = _data(3 * batch, features, classes, True, seed=11)
    xd, yd = torch.as_tensor(x).to(cuda_device), torch.as_tensor(y).to(cuda_device)
    order = torch.randperm(3 * batch, generator=torch.Generator().manual_seed(2)).to(cuda_device)
    states = []
    for groups in (1, 3, 0):
        model = _model(cuda_device, features, hidden, classes, 0.2)
        mlp_step.train_steps(model, xd, yd, order, batch, 3, groups=groups)
        states.append([model.fp.flat.clone(), model.fp.m.clone(), model.fp.v.clone()])
    assert not torch.equal(states[0][0], _model(cuda_device, features, hidden, classes, 0.2).fp.flat)
    for other in states[1:]:
        for a, b in zip(states[0], other):
            assert torch.equal(a, b)


def test_through_fit(cuda_device):
    """200 rows at batch 32 (a short last batch of 8), 2 epochs: the history of engine="fused" against the
    oracle's, by the tolerance rule over engine="layers"; auto picks the fused step; the two checks agree."""
    from streamml.ops import load_c
    n, batch, features, hidden, classes, rate = 200, 32, 784, 128, 10, 0.2
    x, y = _data(n, features, classes, True, seed=7)
    rng = np.random.default_rng(9)
    batches = [o[s:s + batch] for o in (rng.permutation(n), rng.permutation(n)) for s in range(0, n, batch)]
    pairs = np.asarray(_oracle(_model(cuda_device, features, hidden, classes, rate), x, y, batches)[3])
    want = pairs.reshape(2, -1, 2).sum(1) / n             # [epoch][loss, accuracy]
    errs = {}
    for engine in ("layers", "fused", "auto"):
        model = _model(cuda_device, features, hidden, classes, rate)
        hist = model.fit(x, y, epochs=2, batch_size=batch, seed=9, verbose=0, engine=engine).history
        assert model.last_fit_engine == ("layers" if engine == "layers" else "fused")
        assert int(model.fp.iter.item()) == 14 and model._step == 14
        errs[engine] = [_err(hist[k], want[:, i]) for i, k in enumerate(("loss", "accuracy"))]
    print("max-norm relative error of the epochs' loss, accuracy:", errs)
    for engine in ("fused", "auto"):
        for lay, fus in zip(errs["layers"], errs[engine]):
            assert fus <= 4.0 * lay + 1e-7, (engine, lay, fus)
    for args in ((32, 784, 512, 10, 0.2, 1), (1, 1, 1, 2, 0.0, 1), (33, 784, 128, 10, 0.0, 1), (32, 1025, 128, 10, 0.0, 1),
                 (32, 784, 513, 10, 0.0, 1), (32, 784, 128, 65, 0.0, 1), (32, 784, 128, 10, 1.0, 1), (32, 784, 128, 10, 0.0, 2)):
        assert load_c().mlp_step_check(*args) == mlp_step.check(*args)
