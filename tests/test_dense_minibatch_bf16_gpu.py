"""The bf16-MFMA persistent Dense trainer (csrc/kernels/dense_minibatch_bf16.hip,
``ops.dense_persistent.train_steps(precision="bf16")``, ``compile(minibatch_precision="bf16")``).

A free-running comparison with a float64 oracle over 24 steps is ill-conditioned (one flipped bf16
rounding or relu gate compounds through Adam), so:

* the multi-step behaviour is pinned by bit-identity: one launch == one launch per step == a
  second run (test 1), which makes the per-step checks statements about the real trajectory;
* at the checked steps {0, 1, 11, last} the oracle (helpers/dense_mb_bf16_ref, ``O``) runs ONE step
  from the kernel's own state: the gradient recovered from the first moments,
  g = (m_after - b1 m_before) / (1 - b1), is held to ``TOL_G`` norm-wise over the whole flat
  gradient, the loss to 1e-3 relative (the bound tests/test_ae_minibatch_gpu.py holds the other
  bf16 trainer to), ``correct`` exactly;
* Adam is held to the per-step bounds of tests/test_reduce_adam_gpu.py (helpers/adam_ref): the
  parameter update from the kernel's own m_after / v_after to ``bp``, and v_after to ``bv`` plus
  what the recovered gradient's own error (the m equation's rounding, bm / (1 - b1)) moves
  (1 - b2) g^2 by;
* on the four wide cases the kernel must be at least four times nearer to ``O`` than to the
  unrounded float64 step, and the fp32 kernel the other way round.

TOL_G is derived in helpers/dense_mb_bf16_ref (2 x the oracle pair's own spread);
``test_tol_g_is_the_measured_one`` recomputes it on the CPU.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import dense_mb_bf16_cases as cases
from helpers import dense_mb_bf16_ref as ref
from helpers import dense_mb_cases as base
from helpers.adam_ref import KERAS_HP, U, adam_c, adam_step64

NAMES = cases.NAMES
LOSS_RTOL = 1e-3
B1, B2 = float(np.float32(KERAS_HP["b1"])), float(np.float32(KERAS_HP["b2"]))


# ------------------------------------------------------------------ CPU: the tolerance
def test_tol_g_is_the_measured_one():
    """Recomputes the oracle pair's spread and the bf16 / exact gap and asserts the pinned
    constants (2 % leeway for another libm's tanh), and the issue's condition on TOL_G."""
    out = ref.measure()
    worst = max(out, key=lambda k: out[k][0])
    spread = out[worst][0]
    print(f"spread max {spread:.4e} ({worst}); gaps " + ", ".join(f"{k} {out[k][1]:.3e}" for k in ref.WIDE))
    assert abs(spread - ref.SPREAD_MAX) <= 0.02 * ref.SPREAD_MAX, (worst, spread)
    assert ref.TOL_G == 2.0 * ref.SPREAD_MAX
    for k in ref.WIDE:
        assert abs(out[k][1] - ref.GAP_MEDIANS[k]) <= 0.02 * ref.GAP_MEDIANS[k], (k, out[k][1])
    assert ref.TOL_G <= 0.5 * min(out[k][1] for k in ref.WIDE)
    assert max(v[2] for v in out.values()) < LOSS_RTOL / 10      # the loss bound is ten reference spreads wide
    assert not any(v[3] for v in out.values())                   # ``correct`` never differs


def test_extra_case_is_well_posed():
    _, x, _, _ = cases.arrays("64-128-64_b32")
    assert x.shape == (32 * 24, 64) and cases.steps_of("64-128-64_b32") == 24
    s = np.sort(x, axis=-1)
    assert (s[:, -1] - s[:, -2]).min() > 1e-3


# ------------------------------------------------------------------ GPU runs, shared
def _snap(fp):
    return tuple(getattr(fp, b).detach().cpu().numpy().copy() for b in ("flat", "m", "v", "iter"))


@functools.lru_cache(maxsize=None)
def _run(name, precision="bf16", per_step=False, rep=0, device="cuda:0"):
    """The case on the device (computed once per argument tuple; ``rep`` asks for another run).
    per_step: one launch per step with snapshots around the checked steps.  Returns (final (flat, m,
    v, iter), out [nsteps, 2], {step: (before, after)})."""
    from streamml.ops import dense_persistent as dp
    _, _, batch, _, _ = cases.case(name)
    _, x, y, order = cases.arrays(name)
    model = cases.build_model(name, device)
    xd = torch.from_numpy(x).to(device)
    yd = None if y is None else torch.from_numpy(y).to(device)
    od = None if order is None else torch.from_numpy(order).to(device)
    steps = cases.steps_of(name)
    snaps, outs = {}, []
    if per_step:
        chk = ref.checked_steps(steps)
        for s in range(steps):
            before = _snap(model.fp) if s in chk else None
            outs.append(dp.train_steps(model, xd, yd, batch, 1, row0=s * batch, order=od, precision=precision))
            if s in chk:
                torch.cuda.synchronize()
                snaps[s] = (before, _snap(model.fp))
    else:
        outs.append(dp.train_steps(model, xd, yd, batch, steps, order=od, precision=precision))
    torch.cuda.synchronize()
    return _snap(model.fp), torch.cat(outs).double().cpu().numpy(), snaps


def _same(a, b, what):
    for x, y, buf in zip(a[0], b[0], ("flat", "m", "v", "iter")):
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x,
                              y.view(np.int32) if y.dtype == np.float32 else y), (what, buf)
    assert np.array_equal(a[1], b[1]), (what, "out")


@functools.lru_cache(maxsize=None)
def _step_errors(name, precision):
    """Per checked step, from the kernel's own state: (||g - g_O|| / ||g_O||, ||g - g_exact|| /
    ||g_exact||, relative loss error against O, correct, O's correct)."""
    spec = cases.spec(name)
    n = spec.nparams()
    _, x, y, order = cases.arrays(name)
    _, out, snaps = _run(name, precision, True)
    rows = dict((s, (xb, yb)) for s, xb, yb in ref.batches(x, y, order, cases.batch_of(name)))
    res = {}
    for s, (before, after) in sorted(snaps.items()):
        g = (after[1][:n].astype(np.float64) - B1 * before[1][:n].astype(np.float64)) / (1.0 - B1)
        ws = spec.split(before[0])
        lo, co, go = ref.grads(spec, ws, *rows[s], kind="O")
        ge = ref.grads(spec, ws, *rows[s], kind="exact")[2]
        go, ge = ref.flat_of(go), ref.flat_of(ge)
        res[s] = (np.linalg.norm(g - go) / np.linalg.norm(go), np.linalg.norm(g - ge) / np.linalg.norm(ge),
                  abs(out[s, 0] - lo) / abs(lo), out[s, 1], co)
    return res


# ------------------------------------------------------------------ 1. split invariance, reproducibility
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_launch_equals_one_launch_per_step(cuda_device, name):
    a, b = _run(name), _run(name, per_step=True)
    _same(a, b, name)
    assert int(a[0][3].item()) == cases.steps_of(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["30-128-32-128-30_b100", "order_given"])
def test_same_run_twice_gives_the_same_bits(cuda_device, name):
    _same(_run(name), _run(name, rep=1), name)


# ------------------------------------------------------------------ 2, 3. per-step gradient, loss, accuracy
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_step_gradient_loss_and_accuracy_match_the_oracle(cuda_device, name):
    errs = _step_errors(name, "bf16")
    assert sorted(errs) == ref.checked_steps(cases.steps_of(name))
    for s, (eo, ee, el, c, co) in errs.items():
        print(f"{name} step {s}: |g-gO|/|gO| {eo:.3e}  |g-gexact|/|gexact| {ee:.3e}  loss rel {el:.3e}  "
              f"correct {c:.0f}/{co}")
    for s, (eo, ee, el, c, co) in errs.items():
        assert eo <= ref.TOL_G, (name, s, eo)
        assert el <= LOSS_RTOL, (name, s, el)
        assert c == co, (name, s, c, co)


# ------------------------------------------------------------------ 4. Adam
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_adam_step_is_the_shared_update(cuda_device, name):
    n = cases.spec(name).nparams()
    hp = KERAS_HP
    _, _, snaps = _run(name, "bf16", True)
    for s, (before, after) in sorted(snaps.items()):
        p0, m0, v0 = (before[k][:n].astype(np.float64) for k in range(3))
        p1, m1, v1 = (after[k][:n].astype(np.float64) for k in range(3))
        t = int(before[3].item()) + 1
        assert int(after[3].item()) == t
        g = (m1 - B1 * m0) / (1.0 - B1)
        r = adam_step64(g, m0, v0, p0, t, hp["lr"], hp["b1"], hp["b2"], hp["eps"], 1.0)
        dg = r.bm / (1.0 - B1)                       # the recovered gradient's own error
        assert np.all(np.abs(v1 - r.v) <= r.bv + (1.0 - B2) * (2.0 * np.abs(g) * dg + dg * dg)), (name, s)
        # the parameter from the kernel's own moments: adam_step64's bp with this update
        upd = r.lr_t * m1 / (np.sqrt(v1) + float(np.float32(hp["eps"])))
        bound = U * np.abs(p0 - upd) + adam_c(float(np.float32(t)), B1, B2) * np.abs(upd)
        assert np.all(np.abs(p1 - (p0 - upd)) <= bound), (name, s)


# ------------------------------------------------------------------ 5. the bf16 path ran, and is this bf16
@pytest.mark.gpu
def test_bf16_kernel_is_nearer_the_bf16_oracle_and_fp32_kernel_the_exact_step(cuda_device):
    for name in ref.WIDE:
        eb = np.array([v[:2] for v in _step_errors(name, "bf16").values()])
        ef = np.array([v[:2] for v in _step_errors(name, "fp32").values()])
        mo, me = np.median(eb[:, 0]), np.median(eb[:, 1])
        fo, fe = np.median(ef[:, 0]), np.median(ef[:, 1])
        print(f"{name}: bf16 kernel to O {mo:.3e} to exact {me:.3e}; fp32 kernel to O {fo:.3e} to exact {fe:.3e}")
        assert mo <= me / 4, (name, mo, me)
        assert fe <= fo / 4, (name, fe, fo)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ref.WIDE)
def test_bf16_and_fp32_fits_differ_in_bits_and_agree_to_3e_2(cuda_device, name):
    spec = cases.spec(name)
    a, b = _run(name, "bf16")[0], _run(name, "fp32")[0]
    n = spec.nparams()
    assert not np.array_equal(a[0][:n], b[0][:n])
    for wa, wb, shape in zip(spec.split(a[0]), spec.split(b[0]), spec.shapes()):
        d = np.linalg.norm(wa - wb) / np.linalg.norm(wb)
        print(f"{name} {shape}: {d:.3e}")
        assert d <= 3e-2, (name, shape, d)


# ------------------------------------------------------------------ 6. limits
@pytest.mark.gpu
def test_python_bf16_limits_agree_with_the_cpp_check(cuda_device):
    from streamml.ops import dense_persistent as dp
    from streamml.ops._ext import load_c
    C = load_c()
    assert C.DMB_MAXPARAMS_BF16 == dp.MAX_PARAMS_BF16
    shapes = list(base.SHAPES) + [([64, 128, 64], 32, False), ([65, 113, 65], 32, False), ([18, 129, 18], 32, False),
                                  ([18] + [20] * 8 + [18], 32, False), ([18, 33, 18], 0, False),
                                  ([18, 33, 18], 129, False), ([30, 128, 32, 128, 30], 128, True)]
    answers = []
    for widths, batch, own in shapes:
        off, table = 0, []
        for fin, fout in zip(widths[:-1], widths[1:]):
            table.append([fin, fout, 2, 1, 0.0, 0.0, off, off + fin * fout])
            off += fin * fout + fout
        py = dp.check_shape(list(widths), batch, own, precision="bf16")
        assert C.dense_mb_check(table, batch, off, own, precision=1) == py, (widths, batch)
        assert C.dense_mb_check(table, batch, off, own) == dp.check_shape(list(widths), batch, own), (widths, batch)
        answers.append(py)
    assert any("MAX_PARAMS_BF16" in a for a in answers) and sum(a == "" for a in answers) >= 8


@pytest.mark.gpu
def test_train_steps_names_the_bf16_limit(cuda_device):
    from streamml.ops import dense_persistent as dp
    model = _stack(cuda_device, (113, 65), ("tanh", "linear"), features=65)
    x = torch.rand((64, 65), device=cuda_device)
    with pytest.raises(ValueError, match="MAX_PARAMS_BF16"):
        dp.train_steps(model, x, None, 32, 2, precision="bf16")
    dp.train_steps(model, x, None, 32, 2)            # the fp32 kernel takes it


# ------------------------------------------------------------------ 7. fit
def _data(n=320, d=18, seed=5):
    return np.random.default_rng(seed).uniform(0, 1, size=(n, d)).astype(np.float32)


def _stack(device, widths=(64, 16, 64, 18), acts=("tanh", "relu", "tanh", "relu"), features=18, seed=3, **compile_kw):
    from streamml import nn
    from streamml.nn.layers import Dense
    layers = [Dense(u, a, input_shape=(features,) if i == 0 else None) for i, (u, a) in enumerate(zip(widths, acts))]
    model = nn.Sequential(layers, device=device, seed=seed)
    model.compile(loss="mse", metrics=["accuracy"], **compile_kw)
    return model


def _bits_equal(a, b):
    return all(torch.equal(getattr(a.fp, buf), getattr(b.fp, buf)) for buf in ("flat", "m", "v", "iter"))


@pytest.mark.gpu
def test_shuffled_fit_equals_train_steps_with_the_same_permutation(cuda_device):
    from streamml.ops import dense_persistent as dp
    x = _data(300)
    a = _stack(cuda_device, minibatch_precision="bf16")
    b = _stack(cuda_device)
    a.fit(x, batch_size=32, epochs=1, verbose=0, seed=7)
    assert a.last_fit_engine == "persistent" and a.last_fit_precision == "bf16"
    order = torch.from_numpy(np.random.default_rng([7, 0, 0]).permutation(300).astype(np.int32)).to(cuda_device)
    dp.train_steps(b, torch.from_numpy(x).to(cuda_device), None, 32, 10, 0, order, precision="bf16")
    assert _bits_equal(a, b)
    c = _stack(cuda_device)
    c.fit(x, batch_size=32, epochs=1, verbose=0, seed=7)
    assert c.last_fit_precision == "fp32" and not torch.equal(a.fp.flat, c.fp.flat)


@pytest.mark.gpu
def test_stream_fit_equals_the_array_fit_bit_for_bit(cuda_device):
    from streamml.data.stream import from_arrays
    x = _data(500)
    a, b = _stack(cuda_device, minibatch_precision="bf16"), _stack(cuda_device, minibatch_precision="bf16")
    b.STREAM_SEGMENT_ROWS = 96                       # three batches per launch: 10 steps = 4 segments
    a.fit(x[:320], batch_size=32, epochs=1, verbose=0, shuffle=False)
    b.fit(from_arrays(x, chunk=70), batch_size=32, epochs=1, verbose=0, steps_per_epoch=10)
    assert a.last_fit_precision == b.last_fit_precision == "bf16"
    assert _bits_equal(a, b)


@pytest.mark.gpu
def test_layer_engine_ignores_the_option(cuda_device):
    x = _data(64)
    a, b = _stack(cuda_device, minibatch_precision="bf16"), _stack(cuda_device)
    a.fit(x, batch_size=32, epochs=1, verbose=0, engine="layers")
    b.fit(x, batch_size=32, epochs=1, verbose=0, engine="layers")
    assert a.last_fit_engine == "layers" and a.last_fit_precision is None
    assert _bits_equal(a, b)


@pytest.mark.gpu
def test_stack_outside_the_bf16_limits_trains_on_the_fp32_kernel(cuda_device):
    x = _data(64, d=65)
    kw = dict(widths=(113, 65), acts=("tanh", "linear"), features=65)
    a, b = _stack(cuda_device, minibatch_precision="bf16", **kw), _stack(cuda_device, **kw)
    a.fit(x, batch_size=32, epochs=1, verbose=0)
    b.fit(x, batch_size=32, epochs=1, verbose=0)
    assert a.last_fit_engine == "persistent" and a.last_fit_precision == "fp32"
    assert _bits_equal(a, b)


@pytest.mark.gpu
def test_recognised_autoencoder_receives_the_option(cuda_device):
    x = _data(320)
    out = {}
    for prec in ("bf16", "fp32"):
        model = _stack(cuda_device, widths=(14, 7, 7, 18), minibatch_precision=prec)
        assert model.fused and model._fused.minibatch_precision == prec
        model.fit(x, batch_size=32, epochs=1, verbose=0, shuffle=False)
        assert model.last_fit_engine == "fused" and model.last_fit_precision is None
        out[prec] = [w.copy() for w in model.get_weights()]
    assert any(not np.array_equal(a, b) for a, b in zip(out["bf16"], out["fp32"]))
