"""The float64 Adam oracle of tests/helpers/adam_ref.py and its rounding bounds, without a device.

* A plain numpy-float32 evaluation of csrc/include/sml_adam.h meets the bounds the device kernels
  are held to in tests/test_reduce_adam_gpu.py, so the bounds can be met.  Largest observed ratios
  err / bound over both streams below: m 0.43, v 0.50, p 0.99 (the p bound's u |p| term is the
  final subtraction's half ulp, reached whenever p sits just above a power of two).
* The two host oracles the other GPU tests lean on -- the CPU branch of ops.adam.FlatAdam.step and
  models.reference.KerasAdam -- are held to adam_step64 on the same stream.  Both compute lr_t and
  1 - b in Python floats from the hyper-parameters as given, so they are compared with the oracle
  at unrounded hyper-parameters (``hyper64``); their torch float32 arithmetic then has at most
  three roundings per term of m (the scalar's cast, the product, the sum), four of v and five of
  the update, inside the same bounds.  gscale is a power of two: scaling the gradient is exact.
"""
import numpy as np
import pytest
import torch

from helpers.adam_ref import ADAM_STEPS, KERAS_HP, GradStream, adam_step32, adam_step64

from streamml.models.reference import KerasAdam
from streamml.ops.adam import FlatAdam, FlatParams


def _ratios(got, ref):
    """largest err / bound of m, v, p; where a bound is zero the value must be exact"""
    out = []
    for a, b, bd in zip(got, (ref.m, ref.v, ref.p), (ref.bm, ref.bv, ref.bp)):
        err = np.abs(np.asarray(a, np.float64) - b)
        assert np.all(err[bd == 0] == 0)
        out.append(float((err[bd > 0] / bd[bd > 0]).max()))
    return out


def _check(name, step, S, gscale, hyper64):
    """``step(g, t) -> (m0, v0, p0, m1, v1, p1)``: the state before and after one step at count t"""
    st = GradStream(S, seed=5)
    worst = [0.0, 0.0, 0.0]
    for t in ADAM_STEPS:
        g = st.next()
        m0, v0, p0, m1, v1, p1 = step(g, t)
        ref = adam_step64(g, m0, v0, p0, t, gscale=gscale, hyper64=hyper64, **KERAS_HP)
        r = _ratios((m1, v1, p1), ref)
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= 1.0, (name, t, r)
        # a slot whose gradient is always zero: m = v = 0 and the parameter must not move at all
        assert not m1[st.zero].any() and not v1[st.zero].any()
        assert np.array_equal(p1[st.zero].view(np.int32), p0[st.zero].view(np.int32))
        assert not np.array_equal(p1[~st.zero], p0[~st.zero])
    print("%s S=%d gscale=%g: max err/bound m %.3f v %.3f p %.3f" % (name, S, gscale, *worst))


def _p_init(S):
    return np.random.default_rng(1).standard_normal(S).astype(np.float32)


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 512])
@pytest.mark.parametrize("S", [1540, 8])
def test_numpy_float32_adam_meets_the_bounds(S, gscale):
    state = [np.zeros(S, np.float32), np.zeros(S, np.float32), _p_init(S)]

    def step(g, t):
        before = list(state)
        state[:] = adam_step32(g, *before, t, gscale=gscale, **KERAS_HP)
        return (*before, *state)

    _check("numpy-f32", step, S, gscale, hyper64=False)


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 512])
@pytest.mark.parametrize("S", [1540, 8])
def test_flat_adam_cpu_branch_matches_adam_step64(S, gscale):
    fp = FlatParams([(S,)], "cpu", init=[_p_init(S)])
    opt = FlatAdam(fp, lr=KERAS_HP["lr"], beta_1=KERAS_HP["b1"], beta_2=KERAS_HP["b2"], epsilon=KERAS_HP["eps"])
    assert not opt.on_gpu

    def step(g, t):
        before = [x.numpy().copy() for x in (fp.m, fp.v, fp.flat)]
        fp.grad.copy_(torch.from_numpy(g))
        fp.iter.fill_(t)
        opt.step(grad_scale=gscale, counted=True)
        assert int(fp.iter.item()) == t
        return (*before, *(x.numpy().copy() for x in (fp.m, fp.v, fp.flat)))

    _check("FlatAdam-cpu", step, S, gscale, hyper64=True)


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 512])
@pytest.mark.parametrize("S", [1540, 8])
def test_keras_adam_matches_adam_step64(S, gscale):
    p = torch.from_numpy(_p_init(S))
    opt = KerasAdam([p], lr=KERAS_HP["lr"], beta_1=KERAS_HP["b1"], beta_2=KERAS_HP["b2"], epsilon=KERAS_HP["eps"])

    def step(g, t):
        before = [x.numpy().copy() for x in (opt.m[0], opt.v[0], p)]
        opt.iterations = t - 1
        opt.apply([torch.from_numpy(g) * gscale])   # KerasAdam takes the scaled gradient (exact: 2^-9)
        assert opt.iterations == t
        return (*before, *(x.numpy().copy() for x in (opt.m[0], opt.v[0], p)))

    _check("KerasAdam", step, S, gscale, hyper64=True)


def test_adam_step64_catches_the_bug_classes_of_interest():
    """The oracle's bounds separate sml_adam.h from its near misses by orders of magnitude: epsilon
    inside the root, a shifted or missing bias correction, m and v swapped, gscale applied twice or
    not at all -- each evaluated in float64 (no rounding of its own) on the stream's 40th step."""
    S, gscale, t = 1540, 1.0 / 512, 40
    st = GradStream(S, seed=5)
    m, v, p = np.zeros(S, np.float32), np.zeros(S, np.float32), _p_init(S)
    for k in range(1, t):
        m, v, p = adam_step32(st.next(), m, v, p, k, gscale=gscale, **KERAS_HP)
    g = st.next()
    ref = adam_step64(g, m, v, p, t, gscale=gscale, **KERAS_HP)
    hp = {k: float(np.float32(x)) for k, x in KERAS_HP.items()}
    lr, b1, b2, eps = hp["lr"], hp["b1"], hp["b2"], hp["eps"]
    m64, v64, p64, g64 = (a.astype(np.float64) for a in (m, v, p, g))

    def variant(gs=gscale, tt=t, bias=True, eps_in=False, swap=False):
        gr = g64 * gs
        lr_t = lr * np.sqrt(1 - b2 ** tt) / (1 - b1 ** tt) if bias else lr
        m1 = b1 * m64 + (1 - b1) * gr
        v1 = b2 * v64 + (1 - b2) * gr * gr
        if swap:
            m1, v1 = b1 * v64 + (1 - b1) * gr, b2 * m64 + (1 - b2) * gr * gr
        den = np.sqrt(np.abs(v1) + eps) if eps_in else np.sqrt(np.abs(v1)) + eps
        return m1, v1, p64 - lr_t * m1 / den

    assert max(_ratios(variant(), ref)) < 1e-6   # the formula itself
    for kw in (dict(eps_in=True), dict(tt=t - 1), dict(tt=t + 1), dict(bias=False), dict(swap=True),
               dict(gs=gscale * gscale), dict(gs=1.0)):
        assert max(_ratios(variant(**kw), ref)) > 100.0, kw
