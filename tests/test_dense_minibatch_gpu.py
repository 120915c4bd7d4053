"""Persistent small-batch Dense trainer (csrc/kernels/dense_minibatch.hip, ops.dense_persistent,
``nn.Model.fit(engine=)``) against a float64 numpy run of the same Keras steps
(tests/helpers/dense_mb_ref.py).

Tolerances are those tests/test_ae_minibatch_gpu.py holds the fp32 AE trainer to: weights rtol 2e-4
/ atol 2e-5, first moments rtol 2e-3 / atol 1e-6, per-step loss 1e-4 relative, per-step ``correct``
exact.

Every case has ordinary weights (Glorot kernels, biases in +-0.2) and trains at the default learning
rate; helpers/dense_mb_cases.py says how each row gets its margin.

Seeds.  A case's seed (helpers/dense_mb_cases.SEEDS) is acceptable only if, on the CPU,
(a) the fp32 ``nn.Model`` run of the case stays within HALF those tolerances of the float64 run
(no relu sign flip in the case), and (b) in the float64 run every row's top two outputs differ by
more than 1e-3 and so do its top two targets (``correct`` is well posed).
``test_case_seed_is_acceptable`` asserts both for every case, and that the predicted class depends
on the row: at least three distinct classes over the case and within one step (two where the model
has three outputs or the batch one row).  Seeds as checked on the CPU: see SEEDS.
"""
import numpy as np
import pytest
import torch

from helpers import dense_mb_cases as cases

W_TOL = dict(rtol=2e-4, atol=2e-5)
M_TOL = dict(rtol=2e-3, atol=1e-6)
LOSS_RTOL = 1e-4
NAMES = list(cases.CASES)


def _half(tol):
    return {k: v / 2 for k, v in tol.items()}


def _check_against_reference(name, flat, m, out, it, tol_scale=1.0):
    ref, ref_out = cases.reference(name)
    wt = W_TOL if tol_scale == 1.0 else _half(W_TOL)
    mt = M_TOL if tol_scale == 1.0 else _half(M_TOL)
    n = sum(a.size for a in ref.weights())
    np.testing.assert_allclose(flat[:n], cases.flat_of(ref.weights()), **wt)
    np.testing.assert_allclose(m[:n], cases.flat_of(ref.moments("m")), **mt)
    assert out.shape == ref_out.shape
    np.testing.assert_allclose(out[:, 0], ref_out[:, 0], rtol=LOSS_RTOL * tol_scale)
    np.testing.assert_array_equal(out[:, 1], ref_out[:, 1])
    assert it == ref.t


@pytest.mark.parametrize("name", NAMES)
def test_case_seed_is_acceptable(name):
    """CPU only: the two conditions of the module docstring for the case's seed."""
    _, _, batch, n, _ = cases.CASES[name]
    ws, x, y, order = cases.arrays(name)
    ref, _ = cases.reference(name)
    assert ref.min_top2_gap > 1e-3, f"top-two gap {ref.min_top2_gap:.2e}: pick another seed"
    few = 2 if cases.CASES[name][0][-1] <= 3 else 3
    assert len(ref.pred_classes) >= few, f"predicted classes {sorted(ref.pred_classes)}: the output ignores the row"
    assert ref.max_classes_in_step >= min(few, batch), ref.max_classes_in_step
    model = cases.build_model(name, "cpu")
    out = []
    for s in range(cases.steps_of(name)):
        idx = np.arange(s * batch, min((s + 1) * batch, n))
        if order is not None:
            idx = order[idx]
        model._acc.zero_()
        loss = model.train_on_batch(x[idx], x[idx] if y is None else y[idx])
        out.append((float(loss.detach()), float(model._acc[1])))
    _check_against_reference(name, model.fp.flat.double().numpy(), model.fp.m.double().numpy(), np.asarray(out),
                             int(model.fp.iter.item()), tol_scale=0.5)


def _gpu_run(name, device, launches=1):
    from streamml.ops import dense_persistent as dp
    _, _, batch, _, _ = cases.CASES[name]
    _, x, y, order = cases.arrays(name)
    model = cases.build_model(name, device)
    xd = torch.from_numpy(x).to(device)
    yd = None if y is None else torch.from_numpy(y).to(device)
    od = None if order is None else torch.from_numpy(order).to(device)
    steps = cases.steps_of(name)
    outs, s0 = [], 0
    for i in range(launches):
        k = steps // launches if i < launches - 1 else steps - s0
        outs.append(dp.train_steps(model, xd, yd, batch, k, row0=s0 * batch, order=od))
        s0 += k
    torch.cuda.synchronize()
    return model, torch.cat(outs).double().cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_steps_match_float64(cuda_device, name):
    model, out = _gpu_run(name, cuda_device)
    fp = model.fp
    _check_against_reference(name, fp.flat.double().cpu().numpy(), fp.m.double().cpu().numpy(), out,
                             int(fp.iter.item()))
    # second moments: no tolerance of their own is set; they enter the weights, which are checked


@pytest.mark.gpu
def test_same_fit_twice_and_split_launches_give_the_same_bits(cuda_device):
    name = "30-128-32-128-30_b100"
    a, out_a = _gpu_run(name, cuda_device)
    b, out_b = _gpu_run(name, cuda_device)
    c, out_c = _gpu_run(name, cuda_device, launches=3)
    for other, out in ((b, out_b), (c, out_c)):
        for buf in ("flat", "m", "v"):
            assert torch.equal(getattr(a.fp, buf), getattr(other.fp, buf)), buf
        assert np.array_equal(out_a, out)
        assert int(other.fp.iter.item()) == cases.steps_of(name)


@pytest.mark.gpu
def test_partial_and_ordered_cases_split_bit_identically(cuda_device):
    for name in ("partial_last_step", "order_given", "own_targets_18-8-3"):
        a, out_a = _gpu_run(name, cuda_device)
        c, out_c = _gpu_run(name, cuda_device, launches=3)
        for buf in ("flat", "m", "v"):
            assert torch.equal(getattr(a.fp, buf), getattr(c.fp, buf)), (name, buf)
        assert np.array_equal(out_a, out_c)


def _data(n=320, d=18, seed=5):
    return np.random.default_rng(seed).uniform(0, 1, size=(n, d)).astype(np.float32)


def _stack(device, widths=(64, 16, 64, 18), acts=("tanh", "sigmoid", "tanh", "linear"), fused=None, seed=3):
    from streamml import nn
    from streamml.nn.layers import Dense
    layers = [Dense(u, a, input_shape=(18,) if i == 0 else None) for i, (u, a) in enumerate(zip(widths, acts))]
    model = nn.Sequential(layers, device=device, seed=seed)
    model.compile(loss="mse", metrics=["accuracy"], fused=fused)
    return model


@pytest.mark.gpu
def test_fit_takes_the_persistent_engine(cuda_device):
    model = _stack(cuda_device)
    it0 = int(model.fp.iter.item())
    hist = model.fit(_data(), batch_size=32, epochs=2, verbose=0)
    assert model.last_fit_engine == "persistent"
    assert int(model.fp.iter.item()) == it0 + 20
    assert len(hist.history["loss"]) == 2 and hist.history["loss"][1] < hist.history["loss"][0]
    assert 0.0 <= hist.history["accuracy"][0] <= 1.0


@pytest.mark.gpu
def test_engine_layers_and_fused_false_keep_the_layer_loop(cuda_device):
    model = _stack(cuda_device)
    model.fit(_data(64), batch_size=32, epochs=1, verbose=0, engine="layers")
    assert model.last_fit_engine == "layers"
    model = _stack(cuda_device, fused=False)
    model.fit(_data(64), batch_size=32, epochs=1, verbose=0)
    assert model.last_fit_engine == "layers"


@pytest.mark.gpu
def test_engine_layers_on_the_recognised_autoencoder_runs_the_layer_loop(cuda_device):
    model = _stack(cuda_device, widths=(14, 7, 7, 18), acts=("tanh", "relu", "tanh", "relu"))
    assert model.fused
    w0 = model.get_weights()
    model.fit(_data(64), batch_size=32, epochs=1, verbose=0, engine="layers")
    assert model.last_fit_engine == "layers" and int(model.fp.iter.item()) == 2
    w1 = model.get_weights()                          # read through the fused backend
    assert any(not np.array_equal(a, b) for a, b in zip(w0, w1))
    for a, b in zip(w1, model.fp.get()):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="fused kernel"):
        model.fit(_data(64), batch_size=32, epochs=1, verbose=0, engine="persistent")
    model.fit(_data(64), batch_size=32, epochs=1, verbose=0)
    assert model.last_fit_engine == "fused"
    assert model._fused.backend.get_optimizer_state()[0] > 2      # the layer loop's two steps came along


@pytest.mark.gpu
def test_engine_persistent_on_an_unsupported_model_names_the_limit(cuda_device):
    model = _stack(cuda_device, widths=(129, 18), acts=("tanh", "linear"))
    with pytest.raises(ValueError, match="MAX_WIDTH"):
        model.fit(_data(64), batch_size=32, epochs=1, verbose=0, engine="persistent")
    model = _stack(cuda_device)
    with pytest.raises(ValueError, match="MAX_BATCH"):
        model.fit(_data(300), batch_size=129, epochs=1, verbose=0, engine="persistent")
    model.fit(_data(300), batch_size=129, epochs=1, verbose=0)     # auto falls back
    assert model.last_fit_engine == "layers"


@pytest.mark.gpu
def test_shuffled_fit_matches_the_cpu_model(cuda_device):
    x = _data(300)                                   # 300 = 9 * 32 + 12: a partial last step per epoch
    gpu, cpu = _stack(cuda_device), _stack("cpu")
    cpu.set_weights(gpu.get_weights())
    hg = gpu.fit(x, batch_size=32, epochs=2, verbose=0, seed=7)
    hc = cpu.fit(x, batch_size=32, epochs=2, verbose=0, seed=7)
    assert gpu.last_fit_engine == "persistent" and cpu.last_fit_engine == "layers"
    np.testing.assert_allclose(gpu.fp.flat.cpu().numpy(), cpu.fp.flat.numpy(), **W_TOL)
    np.testing.assert_allclose(gpu.fp.m.cpu().numpy(), cpu.fp.m.numpy(), **M_TOL)
    np.testing.assert_allclose(hg.history["loss"], hc.history["loss"], rtol=LOSS_RTOL)
    # 300 rows per epoch: both count rows, so accuracies differ by whole rows (k / 300) or not at all; a
    # row within fp32 rounding of a tie may fall either way, which the exact per-step checks above exclude
    # by construction and this random data does not -- allow one such row per epoch
    np.testing.assert_allclose(hg.history["accuracy"], hc.history["accuracy"], atol=1.01 / 300)
    assert int(gpu.fp.iter.item()) == int(cpu.fp.iter.item()) == 20


@pytest.mark.gpu
def test_stream_fit_equals_the_array_fit_bit_for_bit(cuda_device):
    from streamml.data.stream import from_arrays
    x = _data(500)
    a, b = _stack(cuda_device), _stack(cuda_device)
    b.STREAM_SEGMENT_ROWS = 96                       # three batches per launch: 10 steps = 4 segments
    a.fit(x[:320], batch_size=32, epochs=1, verbose=0, shuffle=False)
    hb = b.fit(from_arrays(x, chunk=70), batch_size=32, epochs=1, verbose=0, steps_per_epoch=10)
    assert a.last_fit_engine == b.last_fit_engine == "persistent"
    assert len(hb.history["loss"]) == 1
    for buf in ("flat", "m", "v", "iter"):
        assert torch.equal(getattr(a.fp, buf), getattr(b.fp, buf)), buf


@pytest.mark.gpu
def test_python_supports_agrees_with_the_cpp_check(cuda_device):
    from streamml.ops import dense_persistent as dp
    from streamml.ops._ext import load_c
    C = load_c()
    assert (C.DMB_MAXLAYERS, C.DMB_MAXW, C.DMB_MAXBATCH, C.DMB_MAXPARAMS, C.DMB_LDS_BYTES) == \
        (dp.MAX_LAYERS, dp.MAX_WIDTH, dp.MAX_BATCH, dp.MAX_PARAMS, dp.LDS_BYTES)
    for widths, batch, own in cases.SHAPES:
        off, table = 0, []
        for fin, fout in zip(widths[:-1], widths[1:]):
            table.append([fin, fout, 2, 1, 0.0, 0.0, off, off + fin * fout])
            off += fin * fout + fout
        assert C.dense_mb_check(table, batch, off, own) == dp.check_shape(list(widths), batch, own), (widths, batch)
