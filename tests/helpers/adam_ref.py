"""Oracles for the slab reductions and the device Adam (tests/test_reduce_adam_gpu.py,
tests/test_adam_reference.py).

* ``int_slabs``: slabs of small integers whose column sums are exact in fp32 in ANY order, so a
  reduction kernel is held to an int64 sum bit for bit.
* ``float_slabs`` / ``sum_bound``: slabs over six decades and the standard recursive-summation
  bound for the one float case per kernel.
* ``adam_step64``: one Keras/TF ResourceApplyAdam step in float64 with componentwise rounding
  bounds for an fp32 implementation that follows csrc/include/sml_adam.h.
* ``GradStream``: the gradient stream of the per-step Adam checks; its values carry 20-bit
  significands and are presented as slabs g/2, g/4, g/4, so the slab sum of every kernel is exact
  in any order and the Adam bounds need no summation allowance.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24   # fp32 unit roundoff

RA_WRITE_GRAD, RA_ADAM, RA_METRICS, RA_ADVANCE = 1, 2, 4, 8

KERAS_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-7)


def int_slabs(G: int, S: int, seed: int):
    """float32 [G, S] of random integers in [-8, 8], every slab different, and the int64 column
    sums.  For G <= 2^20 every partial sum is an integer below 2^24: exact in fp32 in any order."""
    assert 1 <= G <= 1 << 20
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(G, S), dtype=np.int64)
    k = min(S, 8)   # distinct on a prefix is distinct
    assert 17 ** k >= 4 * G, "too few columns for G different slabs"
    for _ in range(64):
        _, first = np.unique(x[:, :k], axis=0, return_index=True)
        if len(first) == G:
            break
        dup = np.setdiff1d(np.arange(G), first)
        x[dup] = rng.integers(-8, 9, size=(len(dup), S), dtype=np.int64)
    else:
        raise AssertionError("could not make every slab different")
    return x.astype(np.float32), x.sum(axis=0)


def float_slabs(G: int, S: int, seed: int):
    """float32 [G, S] of randn * 10^uniform(-3, 3), the float64 column sums and sum_g |x_g|."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((G, S)) * 10.0 ** rng.uniform(-3, 3, (G, S))).astype(np.float32)
    x64 = x.astype(np.float64)
    return x, x64.sum(axis=0), np.abs(x64).sum(axis=0)


def sum_bound(L: int, abs_sum):
    """|fl(sum) - sum| <= (L + 1) u sum|x| when no value passes through more than L additions
    (gamma_L = L u / (1 - L u) <= (L + 1) u for the L used here, L u < 1e-4)."""
    return (L + 1) * U * np.asarray(abs_sum, np.float64)


def adam_c(t: float, b1: float, b2: float) -> float:
    """Relative allowance on the update lr_t m / (sqrt(v) + eps): its own four roundings and lr_t's
    four (8 u), plus two powf each off by up to 2 ulp, amplified by the cancellation in 1 - b^t
    (d log sqrt(1 - b2^t) = b2^t / (2 (1 - b2^t)) per relative unit of b2^t, d log (1 - b1^t) =
    b1^t / (1 - b1^t))."""
    p1, p2 = np.power(b1, t), np.power(b2, t)
    return U * (8.0 + 2.0 * (p2 / (2.0 * (1.0 - p2)) + p1 / (1.0 - p1)))


def adam_step64(g, m, v, p, t, lr, b1, b2, eps, gscale, hyper64: bool = False):
    """Keras/TF ResourceApplyAdam in float64: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
    p -= lr_t m / (sqrt(v) + eps) (epsilon OUTSIDE the root), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t),
    with g scaled by gscale first.

    Evaluated on the float32-rounded hyper-parameters and on float32(t), as the kernels see them
    (the binding casts to float, the kernel computes (float)iter[0]).  ``hyper64`` keeps the
    hyper-parameters and t as given: the host oracles (FlatAdam's CPU branch, KerasAdam) compute
    lr_t and 1 - b in Python floats.

    Returns m, v, p, the update and the componentwise bounds bm, bv, bp (module docstring of
    tests/test_reduce_adam_gpu.py derives them)."""
    f = (lambda x: float(x)) if hyper64 else (lambda x: float(np.float32(x)))
    lr, b1, b2, eps, gscale, t = f(lr), f(b1), f(b2), f(eps), f(gscale), f(t)
    g, m, v, p = (np.asarray(a, np.float64) for a in (g, m, v, p))
    gr = g * gscale
    lr_t = lr * np.sqrt(1.0 - np.power(b2, t)) / (1.0 - np.power(b1, t))
    m1 = b1 * m + (1.0 - b1) * gr
    v1 = b2 * v + (1.0 - b2) * gr * gr
    upd = lr_t * m1 / (np.sqrt(v1) + eps)
    p1 = p - upd
    bm = 4.0 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * gr))
    bv = 4.0 * U * v1
    bp = U * np.abs(p1) + adam_c(t, b1, b2) * np.abs(upd)
    return SimpleNamespace(m=m1, v=v1, p=p1, update=upd, bm=bm, bv=bv, bp=bp, lr_t=lr_t)


def adam_step32(g, m, v, p, t, lr, b1, b2, eps, gscale):
    """sml_adam.h in plain numpy float32 (one rounding per operation, no contraction)."""
    f = np.float32
    lr, b1, b2, eps, gscale, t = f(lr), f(b1), f(b2), f(eps), f(gscale), f(t)
    one = f(1.0)
    g, m, v, p = (np.asarray(a, np.float32) for a in (g, m, v, p))
    lr_t = lr * np.sqrt(one - np.power(b2, t)) / (one - np.power(b1, t))
    gr = g * gscale
    m1 = b1 * m + (one - b1) * gr
    v1 = b2 * v + ((one - b2) * gr) * gr
    p1 = p - (lr_t * m1) / (np.sqrt(v1) + eps)
    assert m1.dtype == v1.dtype == p1.dtype == np.float32
    return m1, v1, p1


# the step counts of the per-step checks: 40 consecutive steps, then three jumps; the last does not
# fit a float ((float)(2^24 + 3) == 2^24 + 4)
ADAM_STEPS = list(range(1, 41)) + [1000, 100000, (1 << 24) + 3]


class GradStream:
    """Per-slot base magnitudes 10^uniform(-6, 2), every 17th slot an exact zero; each step
    multiplies by 1 + 0.5 uniform(-1, 1) and flips the sign of a tenth of the slots.  Values are
    cut to 20-bit significands so ``slabs`` (g/2, g/4, g/4 in a per-slot rotation) sums back to g
    exactly in fp32 whatever the order: partial sums g/4 .. g need at most 22 bits."""

    def __init__(self, S: int, seed: int):
        self.rng = np.random.default_rng(seed)
        self.S = S
        self.base = 10.0 ** self.rng.uniform(-6, 2, S)
        self.base[::17] = 0.0
        self.zero = self.base == 0.0

    def next(self) -> np.ndarray:
        g = self.base * (1.0 + 0.5 * self.rng.uniform(-1, 1, self.S))
        g = np.where(self.rng.random(self.S) < 0.1, -g, g).astype(np.float32)
        g[self.zero] = 0.0   # +0: a flipped zero would be -0, and the kernels' sums give +0
        return (g.view(np.int32) & np.int32(~0xF)).view(np.float32)

    def slabs(self, g: np.ndarray, G: int = 3, rows=(0, 1, 2)) -> np.ndarray:
        """[G, S] float32 slabs that sum to g exactly: the three parts in slab rows ``rows``, zero
        slabs elsewhere."""
        parts = np.stack([g * np.float32(0.5), g * np.float32(0.25), g * np.float32(0.25)])
        rot = np.arange(self.S) % 3
        out = np.zeros((G, self.S), np.float32)
        for k, r in enumerate(rows):
            out[r] = parts[(k + rot) % 3, np.arange(self.S)]
        assert np.array_equal(out.astype(np.float64).sum(axis=0), g.astype(np.float64))
        return out
