"""The large-batch Dense train step (csrc/kernels/dense_batch.hip, ``ops.dense_batch``,
``fit(engine="throughput")``).

* ``grad_step`` against the float64 oracle of the bf16 step (helpers/dense_mb_bf16_ref, kind "O") at
  the four shapes of CASES: a last chunk of one row, five chunks over three groups with every option of
  a layer, more groups asked than chunks, and the default grid.  The bound on ||g - g_O|| / ||g_O|| is
  the helper's TOL_G = 8.71e-4, because the helper's device model "V" stays inside its SPREAD_MAX =
  4.355e-4 at these shapes.  Measured on the CPU with ``_arrays`` below, V seeds 0, 1, 2:

      case            spread V to O (largest of 3)   gap exact to O
      ae_b129         5.32e-5                        8.06e-3
      odd_b160_g3     1.23e-5                        2.66e-3
      wide_b129_g8    7.45e-5                        1.52e-2
      ae_b1000        2.27e-5                        4.57e-3

  The loss is held to 1e-4 relative (V differs from O by at most 3.0e-5 in the helper's record),
  ``correct`` exactly.
* ``groups=1`` is the persistent bf16 trainer's arithmetic in its order: bit-identical state and pairs.
* a split over several groups is static: two runs give the same bits.
* ``fit(engine="throughput")`` is ``train_steps`` with the layer loop's permutations.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import dense_mb_bf16_ref as ref

LOSS_RTOL = 1e-4
AE = dict(widths=(18, 64, 16, 64, 18), acts=("tanh", "relu", "tanh", "relu"))
CASES = {
    "ae_b129": dict(AE, batch=129, groups=None),
    "odd_b160_g3": dict(widths=(19, 33, 17, 5), acts=("sigmoid", "tanh", "linear"), batch=160, groups=3, own=True,
                        bias=(True, False, True), l1=(1e-3, 0.0, 0.0), l2=(0.0, 1e-3, 0.0)),
    "wide_b129_g8": dict(widths=(30, 128, 32, 128, 30), acts=("tanh", "relu", "tanh", "relu"), batch=129, groups=8),
    "ae_b1000": dict(AE, batch=1000, groups=None),
}


def _spec(case):
    return ref.Spec(case["widths"], case["acts"], case.get("bias"), case.get("l1"), case.get("l2"))


@functools.lru_cache(maxsize=None)
def _arrays(name, rows=None):
    """(weights in FlatParams order, x, y or None) of a case, fp32: Glorot kernels, small biases,
    uniform rows."""
    case = CASES[name]
    widths, spec = case["widths"], _spec(case)
    rng = np.random.default_rng([21, len(name), widths[1]])
    ws = []
    for l, (fin, fout) in enumerate(zip(widths[:-1], widths[1:])):
        lim = np.sqrt(6.0 / (fin + fout))
        ws.append(rng.uniform(-lim, lim, size=(fin, fout)).astype(np.float32))
        if spec.bias[l]:
            ws.append(rng.uniform(-0.1, 0.1, size=(fout,)).astype(np.float32))
    n = rows or case["batch"]
    x = rng.uniform(0, 1, size=(n, widths[0])).astype(np.float32)
    y = rng.uniform(0, 1, size=(n, widths[-1])).astype(np.float32) if case.get("own") else None
    return ws, x, y


def _model(name, device):
    from streamml import nn
    from streamml.nn.layers import L1L2, Dense
    case = CASES[name]
    spec = _spec(case)
    layers = []
    for l in range(spec.nl):
        reg = L1L2(spec.l1[l], spec.l2[l]) if (spec.l1[l] or spec.l2[l]) else None
        layers.append(Dense(spec.widths[l + 1], spec.acts[l], use_bias=spec.bias[l], activity_regularizer=reg,
                            input_shape=(spec.widths[0],) if l == 0 else None))
    model = nn.Sequential(layers, device=device, seed=1)
    model.compile(loss="mse", metrics=["accuracy"])
    model.set_weights(_arrays(name)[0])
    return model


def _dev(a, device):
    return None if a is None else torch.from_numpy(a).to(device)


def _bits_equal(a, b):
    return all(torch.equal(getattr(a.fp, buf), getattr(b.fp, buf)) for buf in ("flat", "m", "v", "iter"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gradient_loss_and_accuracy_match_the_oracle(cuda_device, name):
    from streamml.ops import dense_batch as db
    case, spec = CASES[name], _spec(CASES[name])
    ws, x, y = _arrays(name)
    model = _model(name, cuda_device)
    before = model.fp.flat.clone()
    g, loss, correct = db.grad_step(model, _dev(x, cuda_device), _dev(y, cuda_device), groups=case["groups"])
    lo, co, go = ref.grads(spec, ws, x, y, kind="O")
    ge = ref.grads(spec, ws, x, y, kind="exact")[2]
    g = g.double().cpu().numpy()
    n = spec.nparams()
    eo, ee = ref.relerr([g[:n]], go), ref.relerr([g[:n]], ge)
    print(f"{name}: |g-gO|/|gO| {eo:.3e}  |g-gexact|/|gexact| {ee:.3e}  loss rel {abs(loss - lo) / lo:.3e}  "
          f"correct {correct}/{co}")
    assert eo <= ref.TOL_G, (name, eo)
    assert abs(loss - lo) <= LOSS_RTOL * abs(lo), (name, loss, lo)
    assert correct == co, (name, correct, co)
    assert not g[n:].any() and torch.equal(model.fp.flat, before) and int(model.fp.iter.item()) == 0


@pytest.mark.gpu
def test_one_group_is_the_persistent_bf16_trainer_bit_for_bit(cuda_device):
    from streamml.ops import dense_batch as db
    from streamml.ops import dense_persistent as dp
    x = _dev(_arrays("ae_b129", 300)[1], cuda_device)
    a, b = _model("ae_b129", cuda_device), _model("ae_b129", cuda_device)
    oa = db.train_steps(a, x, None, 100, 3, groups=1)
    ob = dp.train_steps(b, x, None, 100, 3, precision="bf16")
    assert int(a.fp.iter.item()) == 3 and _bits_equal(a, b) and torch.equal(oa, ob)


@pytest.mark.gpu
def test_same_split_twice_gives_the_same_bits(cuda_device):
    from streamml.ops import dense_batch as db
    _, x, y = _arrays("odd_b160_g3", 400)
    x, y = _dev(x, cuda_device), _dev(y, cuda_device)
    order = torch.randperm(400, generator=torch.Generator().manual_seed(3)).int().to(cuda_device)
    a, b = _model("odd_b160_g3", cuda_device), _model("odd_b160_g3", cuda_device)
    oa = db.train_steps(a, x, y, 160, 3, order=order, groups=3)      # the last step is 80 rows: three chunks
    ob = db.train_steps(b, x, y, 160, 3, order=order, groups=3)
    assert int(a.fp.iter.item()) == 3 and _bits_equal(a, b) and torch.equal(oa, ob)
    assert bool((oa[:, 0] > 0).all())


@pytest.mark.gpu
def test_fit_throughput_is_train_steps_with_the_layer_loops_batches(cuda_device):
    from streamml.ops import dense_batch as db
    x = _arrays("ae_b129", 600)[1]
    a, b = _model("ae_b129", cuda_device), _model("ae_b129", cuda_device)
    hist = a.fit(x, batch_size=256, epochs=2, verbose=0, seed=7, engine="throughput")
    assert a.last_fit_engine == "throughput" and a.last_fit_precision == "bf16"
    assert int(a.fp.iter.item()) == 6
    for epoch in range(2):
        order = torch.from_numpy(np.random.default_rng([7, 0, epoch]).permutation(600).astype(np.int32))
        db.train_steps(b, _dev(x, cuda_device), None, 256, 3, 0, order.to(cuda_device))
    assert _bits_equal(a, b)
    assert hist.history["loss"][1] < hist.history["loss"][0]
