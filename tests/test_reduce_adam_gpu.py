"""The slab reductions and the device Adam every training path ends in, against oracles of their
own (tests/helpers/adam_ref.py) instead of against each other:

* reduce_adam_kernel, slab_adam_kernel (csrc/kernels/ae_fused.hip),
* slab_sum_kernel (every level, the MAP scatter included), slab_sum1_kernel and
  slab_sum2_kernel<ADAM> (csrc/kernels/dense.hip),
* the shared update of csrc/include/sml_adam.h.

Reductions are EXACT: slabs of integers in [-8, 8] sum without rounding in fp32 in any order, so
the device result must equal the int64 sum bit for bit; sentinel tails behind every output and NaN
slabs behind the last one catch a write or a read out of range.  One float case per kernel holds
the sum to (L + 1) u sum|x|, L the longest chain of additions counted from the kernel's code.

Adam is checked one step at a time: the float64 oracle gets the device's own state from before
the step, so the bound is a per-step rounding bound (u = 2^-24), not a drifting trajectory:

    |dm| <= 4u (|b1 m0| + |(1 - b1) g gscale|)       product, product, fma: < 4 roundings per term
    |dv| <= 4u v64                                   gr, (1 - b2) gr, * gr, fma
    |dp| <= u |p64| + c(t) |update|                  the subtraction's half ulp + adam_ref.adam_c

The gradients of the Adam checks carry 20-bit significands and arrive as slabs g/2, g/4, g/4 (plus
zero slabs), so every kernel's slab sum is exact whatever its order and the bounds above are used
as they stand, with no summation allowance.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers.adam_ref import (ADAM_STEPS, KERAS_HP, RA_ADAM, RA_ADVANCE, RA_METRICS, RA_WRITE_GRAD, GradStream,
                              adam_step64, float_slabs, int_slabs, sum_bound)

pytestmark = pytest.mark.gpu

PAD = 64          # sentinel elements behind every output
NAN_ROWS = 3      # NaN slabs behind the last slab of every partials buffer
HP = (KERAS_HP["lr"], KERAS_HP["b1"], KERAS_HP["b2"], KERAS_HP["eps"])


@pytest.fixture(scope="module")
def C(cuda_device):
    from streamml.ops._ext import load_c
    return load_c()


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)   # a copy: never aliases the host array


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.dtype == want.dtype, (got.dtype, want.dtype, what)
    np.testing.assert_array_equal(got, want, err_msg=str(what))


def _sentinel(n, k=0):
    return (-1000.5 - 3.0 * np.arange(n) - 7.0 * k).astype(np.float32)


def _with_nan_rows(x):
    return np.concatenate([x, np.full((NAN_ROWS, x.shape[1]), np.nan, np.float32)])


def _columns(S):   # slab_adam_columns
    return (S // 4 + 63) // 64


# ----------------------------------------------------------------------------------------------
# reduce_adam without Adam: sums, metrics, cursor, and nothing else
# ----------------------------------------------------------------------------------------------
def _reduce_exact(C, dev, G, S, seed, wide=False):
    """All nparam x flag combinations (no RA_ADAM) of one (G, S), two calls each."""
    x, sums = int_slabs(G, S, seed)
    part = _dev(_with_nan_rows(x), dev)
    want_grad = sums.astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    gy = (G + 31) // 32
    for ni, nparam in enumerate((S, S - 4, S - 6)):
        if nparam < 0:   # S = 4: no parameter count below zero
            continue
        met_n = S - nparam
        tail = sums[nparam:]
        grad0 = _dev(_sentinel(S + PAD), dev)
        met0 = np.concatenate([rng.integers(-4, 5, met_n).astype(np.float32), _sentinel(PAD, 1)])
        pmv0 = [rng.standard_normal(nparam + PAD).astype(np.float32) for _ in range(3)]
        # the ring cursor: one case wraps exactly to 0 on the first call
        start, cstep, ring = ((64, 32, 96), (90, 32, 100), (5, 1, 7))[ni]
        for flags in range(16):
            if flags & RA_ADAM:
                continue
            grad = grad0.clone()
            met = _dev(met0, dev)
            params, m, v = (_dev(a, dev) for a in pmv0)
            it = torch.full((1,), 5, dtype=torch.int64, device=dev)
            cur = torch.tensor([start, -12345], dtype=torch.int64, device=dev)
            scratch = counters = None
            if wide:
                scratch = _dev(_sentinel(gy * S + PAD, 2), dev)
                counters = torch.zeros(_columns(S) + 8, dtype=torch.int32, device=dev)
                counters[_columns(S):] = 4242
            for call in (1, 2):
                what = dict(G=G, S=S, nparam=nparam, flags=flags, call=call)
                grad.copy_(grad0)   # the second call has to write the sums again
                C.reduce_adam(part, G, S, nparam, grad, params, m, v, it, *HP, 0.5, met, flags, cur, cstep, ring,
                              scratch, counters)
                if flags & RA_WRITE_GRAD:
                    _same_bits(grad[:S], want_grad, ("grad_out", what))
                    _same_bits(grad[S:], _sentinel(S + PAD)[S:], ("grad_out tail", what))
                else:
                    _same_bits(grad, grad0, ("grad_out untouched", what))
                if flags & RA_METRICS:   # accumulates: preset + call * tail sums
                    _same_bits(met[:met_n], (met0[:met_n].astype(np.int64) + call * tail).astype(np.float32),
                               ("metrics", what))
                    _same_bits(met[met_n:], met0[met_n:], ("metrics tail", what))
                else:
                    _same_bits(met, met0, ("metrics untouched", what))
                for name, t, a in zip(("params", "m", "v"), (params, m, v), pmv0):
                    _same_bits(t, a, (name + " untouched", what))
                want_cur = (start + call * cstep) % ring if flags & RA_ADVANCE else start
                assert cur.tolist() == [want_cur, -12345], what
                assert it.item() == 5, what
                if wide:
                    _same_bits(scratch[gy * S:], _sentinel(gy * S + PAD, 2)[gy * S:], ("scratch tail", what))
                    # re-armed for the next call (the two-launch path never touches them)
                    assert counters.tolist() == [0] * _columns(S) + [4242] * 8, what


# G: the lane-group stride of 16 and the eight-deep load batch (128 starts the loop's second
# trip); S: one quad, a partial block, exactly one block, a block plus one quad, the AE's NSLOT
@pytest.mark.parametrize("S", [4, 60, 64, 68, 1540])
@pytest.mark.parametrize("G", [1, 2, 15, 16, 17, 64, 127, 128, 129, 300])
def test_reduce_adam_narrow_exact(C, cuda_device, G, S):
    _reduce_exact(C, cuda_device, G, S, seed=1000 * G + S)


# 64 still takes the narrow path; 4097 gives 129 chunk sums: the second trip of both 128-wide loops
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("G", [64, 65, 96, 97, 2048, 4097])
def test_reduce_adam_wide_exact(C, cuda_device, monkeypatch, G, fused):
    monkeypatch.setenv("SML_AE_FUSED_REDUCE", fused)
    _reduce_exact(C, cuda_device, G, 1540, seed=7 * G, wide=True)


# ----------------------------------------------------------------------------------------------
# slab_sum2
# ----------------------------------------------------------------------------------------------
SS2_G = [1, 16, 17, 63, 64, 65, 113, 4096]   # the 64-stride main loop, its g + 48 < G edge, the tail
SS2_S = [4, 68, 1028]


def _ss2_pairs():
    """G0 and G1 drawn independently; every value appears on either side."""
    rng = np.random.default_rng(2)
    return ([(g, int(rng.choice(SS2_G))) for g in SS2_G] + [(int(rng.choice(SS2_G)), g) for g in SS2_G])


_slab_cache = {}


def _int_slabs_dev(G, S, dev):
    key = (G, S, str(dev))
    if key not in _slab_cache:
        x, sums = int_slabs(G, S, seed=31 * G + S)
        _slab_cache[key] = (_dev(x, dev), sums)
    return _slab_cache[key]


def _maps(S0, S1, extra, seed):
    """Two disjoint injective maps into n = S0 + S1 + extra slots, about a tenth of the entries
    dropped (-1); rest = exactly the slots neither map covers."""
    rng = np.random.default_rng(seed)
    n = S0 + S1 + extra
    perm = rng.permutation(n).astype(np.int32)
    maps = [perm[:S0].copy(), perm[S0:S0 + S1].copy()]
    for mp in maps:
        drop = rng.random(len(mp)) < 0.1
        if len(mp) >= 8:
            drop[rng.integers(len(mp))] = True
        mp[drop] = -1
    covered = np.concatenate([mp[mp >= 0] for mp in maps])
    assert len(set(covered.tolist())) == len(covered)
    rest = np.setdiff1d(np.arange(n, dtype=np.int32), covered).astype(np.int32)
    assert len(rest) + len(covered) == n
    return n, maps[0], maps[1], rest


def _adam_ratios(got, ref, what):
    out = []
    for name, a, b, bd in zip("mvp", got, (ref.m, ref.v, ref.p), (ref.bm, ref.bv, ref.bp)):
        err = np.abs(np.asarray(a, np.float64) - b)
        assert np.all(err[bd == 0] == 0), (name, what)
        r = float((err[bd > 0] / bd[bd > 0]).max()) if (bd > 0).any() else 0.0
        assert r <= 1.0, (name, r, what)
        out.append(r)
    return out


@pytest.mark.parametrize("G0,G1", _ss2_pairs())
def test_slab_sum2_exact(C, cuda_device, G0, G1):
    dev = cuda_device
    for S0 in SS2_S:
        for S1 in SS2_S:
            what = dict(G0=G0, S0=S0, G1=G1, S1=S1)
            p0, sums0 = _int_slabs_dev(G0, S0, dev)
            p1, sums1 = _int_slabs_dev(G1, S1, dev)
            n, map0, map1, rest = _maps(S0, S1, extra=37, seed=G0 + 3 * G1 + 5 * S0 + 7 * S1)
            rng = np.random.default_rng(n)
            grad0 = rng.integers(-99, 100, n).astype(np.float32) + np.float32(0.5)   # no sum is a half
            want = grad0.copy()
            want[map0[map0 >= 0]] = sums0[map0 >= 0]
            want[map1[map1 >= 0]] = sums1[map1 >= 0]
            m0 = rng.standard_normal(n).astype(np.float32)
            v0 = rng.random(n).astype(np.float32)
            pr0 = rng.standard_normal(n).astype(np.float32)
            d_map0, d_map1, d_rest = _dev(map0, dev), _dev(map1, dev), _dev(rest, dev)
            it = torch.full((1,), 3, dtype=torch.int64, device=dev)
            # without params: sums scattered, nothing else written
            grad, m, v = _dev(grad0, dev), _dev(m0, dev), _dev(v0, dev)
            C.slab_sum2(p0, d_map0, p1, d_map1, grad, None, m, v, it, *HP, 1.0, d_rest)
            _same_bits(grad, want, ("grad", what))
            _same_bits(m, m0, ("m untouched", what))
            _same_bits(v, v0, ("v untouched", what))
            # with Adam: the same gradient, and every slot -- mapped or rest -- updated exactly once
            grad, params = _dev(grad0, dev), _dev(pr0, dev)
            C.slab_sum2(p0, d_map0, p1, d_map1, grad, params, m, v, it, *HP, 1.0 / 512, d_rest)
            _same_bits(grad, want, ("grad with Adam", what))
            ref = adam_step64(want, m0, v0, pr0, 3, *HP, 1.0 / 512)
            _adam_ratios([t.cpu().numpy() for t in (m, v, params)], ref, what)
            assert it.item() == 3


# ----------------------------------------------------------------------------------------------
# dense_wgrad through every reduction level
# ----------------------------------------------------------------------------------------------
WG_K, WG_N = 18, 16


def _kwaves():
    from streamml._build import CSRC
    with open(os.path.join(CSRC, "kernels", "dense.hip")) as f:
        return int(re.search(r"constexpr int kWaves = (\d+);", f.read()).group(1))


def _wgrad_grid(M, max_blocks, kw):   # dense.hip grid_for
    return max(1, min((((M + 15) // 16) + kw - 1) // kw, max_blocks))


@pytest.fixture(scope="module")
def wgrad_data(cuda_device):
    """x, dy of integers in [-2, 2] (exact in bf16; products and sums exact below 2^24) at the two
    row counts, with the exact slab [KP x NP of dW | NP of db] each must reduce to."""
    kw = _kwaves()
    rows = {"small": 16 * kw * 17 - 5, "big": 16 * kw * 4096 + 1}
    rng = np.random.default_rng(12)
    out = {"kw": kw}
    for name, M in rows.items():
        x = rng.integers(-2, 3, (M, WG_K))
        dy = rng.integers(-2, 3, (M, WG_N))
        dW = np.rint(x.T.astype(np.float64) @ dy.astype(np.float64)).astype(np.int64)   # < 2^53: exact
        assert np.abs(dW).max() < 1 << 24 and 4 * M < 1 << 24
        KP, NP = 32, 16
        slab = np.zeros(KP * NP + NP, np.int64)
        slab[:KP * NP].reshape(KP, NP)[:WG_K, :WG_N] = dW
        slab[KP * NP:KP * NP + WG_N] = dy.sum(axis=0)
        out[name] = (_dev(x.astype(np.float32), cuda_device), _dev(dy.astype(np.float32), cuda_device), dW,
                     dy.sum(axis=0), slab)
    return out


# G = 1 and 17: slab_sum1_kernel; 4096: its last one-pass size; 4097 -> 129 -> 5 -> 1: three levels
# of slab_sum_kernel, the last one scattering through the map
@pytest.mark.parametrize("rows,max_blocks,G", [("small", 1, 1), ("small", 1024, 17), ("big", 4096, 4096),
                                               ("big", 4097, 4097)])
def test_dense_wgrad_exact_through_the_reduction_levels(C, cuda_device, wgrad_data, rows, max_blocks, G):
    x, dy, dW, db, slab = wgrad_data[rows]
    assert _wgrad_grid(x.shape[0], max_blocks, wgrad_data["kw"]) == G
    assert C.dense_wgrad_slab(WG_K, WG_N) == len(slab)
    gW, gb = C.dense_wgrad(x, dy, 0, True, max_blocks)
    _same_bits(gW.contiguous(), dW.astype(np.float32), "dW")
    _same_bits(gb.contiguous(), db.astype(np.float32), "db")
    # the slab permuted into a flat gradient, a tenth of its entries dropped
    S = len(slab)
    rng = np.random.default_rng(G)
    mp = rng.permutation(S).astype(np.int32)
    mp[rng.random(S) < 0.1] = -1
    grad0 = np.concatenate([rng.integers(-99, 100, S).astype(np.float32) + np.float32(0.5), _sentinel(PAD)])
    want = grad0.copy()
    want[mp[mp >= 0]] = slab[mp >= 0]
    grad = _dev(grad0, cuda_device)
    C.dense_wgrad(x, dy, 0, True, max_blocks, grad, _dev(mp, cuda_device))
    _same_bits(grad, want, "mapped grad: scattered sums, dropped targets and the tail as preset")


# ----------------------------------------------------------------------------------------------
# one float case per kernel: the only place summation order matters
# ----------------------------------------------------------------------------------------------
def _float_reduce(C, dev, G, S, L, scratch=False):
    x, s64, sabs = float_slabs(G, S, seed=G)
    grad = _dev(_sentinel(S + PAD), dev)
    gy = (G + 31) // 32
    sc = torch.empty(gy * S, device=dev) if scratch else None
    cn = torch.zeros(_columns(S), dtype=torch.int32, device=dev) if scratch else None
    C.reduce_adam(_dev(_with_nan_rows(x), dev), G, S, S, grad, None, None, None, None, *HP, 1.0, None, RA_WRITE_GRAD,
                  None, 0, 0, sc, cn)
    err = np.abs(grad[:S].cpu().numpy().astype(np.float64) - s64)
    ratio = float((err / sum_bound(L, sabs)).max())
    print("float sum G=%d S=%d L=%d: max err/bound %.3f" % (G, S, L, ratio))
    assert ratio <= 1.0


def test_reduce_adam_kernel_float_sum(C, cuda_device):
    # reduce_adam_kernel: a thread adds its ceil(G / 16) slabs one after another (the eight-deep
    # batches are added in order), then group 0 adds the other 15 groups' sums: ceil(G / 16) + 15
    G = 300
    _float_reduce(C, cuda_device, G, 1540, L=math.ceil(G / 16) + 15)


@pytest.mark.parametrize("fused", ["0", "1"])
def test_wide_reduce_float_sum(C, cuda_device, monkeypatch, fused):
    # slab_sum_kernel level (and slab_adam_kernel's copy of it): 8 slabs per thread, then 3 adds
    # over the 4 groups = 11; then reduce_adam_kernel's chain (slab_adam_kernel's final pass has
    # the same order) over the gy = ceil(G / 32) chunk sums: ceil(gy / 16) + 15
    monkeypatch.setenv("SML_AE_FUSED_REDUCE", fused)
    G = 4097
    gy = (G + 31) // 32
    _float_reduce(C, cuda_device, G, 1540, L=11 + math.ceil(gy / 16) + 15, scratch=True)


def test_slab_sum2_kernel_float_sum(C, cuda_device):
    # slab_sum1_body: four accumulators per thread, each taking every 64th slab: ceil(G / 64) adds,
    # 2 more to combine them, then 15 over the groups
    dev = cuda_device
    (G0, S0), (G1, S1) = (113, 68), (4096, 1028)
    n, map0, map1, rest = _maps(S0, S1, extra=37, seed=3)
    x0, s0, a0 = float_slabs(G0, S0, seed=1)
    x1, s1, a1 = float_slabs(G1, S1, seed=2)
    grad0 = _sentinel(n)
    grad = _dev(grad0, dev)
    C.slab_sum2(_dev(x0, dev), _dev(map0, dev), _dev(x1, dev), _dev(map1, dev), grad)
    got = grad.cpu().numpy()
    want = grad0.astype(np.float64)
    bound = np.zeros(n)
    for mp, s, a, G in ((map0, s0, a0, G0), (map1, s1, a1, G1)):
        want[mp[mp >= 0]] = s[mp >= 0]
        bound[mp[mp >= 0]] = sum_bound(math.ceil(G / 64) + 2 + 15, a)[mp >= 0]
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err[bound == 0] == 0)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print("float sum slab_sum2: max err/bound %.3f" % ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("rows,max_blocks,G", [("small", 1024, 17), ("big", 4097, 4097)])
def test_dense_wgrad_float_sum(C, cuda_device, wgrad_data, rows, max_blocks, G):
    # slab_sum1_kernel (G = 17) and three levels of slab_sum_kernel (G = 4097) behind wgrad_kernel.
    # x, dy are bf16 values, so every product is exact in fp32 and the error is summation alone:
    # a wave's accumulator takes one 16-row MFMA per tile (at most 16 additions each) over its
    # ceil(tiles / (G WR)) tiles, the block's WR = kWaves row phases add up in WR - 1 steps, then
    # the slab reduction: ceil(17 / 64) + 17 one-pass, 3 x 11 over the three levels.  db: 4 adds per
    # tile, 2 across the lanes, the same phases and slab levels: a shorter chain.
    kw = wgrad_data["kw"]
    M = wgrad_data[rows][0].shape[0]
    rng = np.random.default_rng(G + 1)
    x = _dev((rng.standard_normal((M, WG_K)) * 10.0 ** rng.uniform(-2, 2, (M, WG_K))).astype(np.float32),
             cuda_device).bfloat16()
    dy = _dev((rng.standard_normal((M, WG_N)) * 10.0 ** rng.uniform(-2, 2, (M, WG_N))).astype(np.float32),
              cuda_device).bfloat16()
    assert _wgrad_grid(M, max_blocks, kw) == G
    gW, gb = C.dense_wgrad(x, dy, 0, True, max_blocks)
    x64, dy64 = x.double().cpu().numpy(), dy.double().cpu().numpy()
    tiles = math.ceil(math.ceil(M / 16) / (G * kw))
    L = 16 * tiles + (kw - 1) + (math.ceil(G / 64) + 17 if G <= 4096 else 33)
    for name, got, want, sabs in (("dW", gW, x64.T @ dy64, np.abs(x64).T @ np.abs(dy64)),
                                  ("db", gb, dy64.sum(axis=0), np.abs(dy64).sum(axis=0))):
        err = np.abs(got.double().cpu().numpy() - want)
        ratio = float((err / sum_bound(L, sabs)).max())
        print("float sum dense_wgrad G=%d %s L=%d: max err/bound %.3f" % (G, name, L, ratio))
        assert ratio <= 1.0, name


# ----------------------------------------------------------------------------------------------
# Adam, one step at a time
# ----------------------------------------------------------------------------------------------
class _ReduceAdam:
    """reduce_adam with RA_ADAM | RA_WRITE_GRAD: g as G slabs (NaN slabs behind them), S = nparam."""

    def __init__(self, C, dev, S, G, rows, wide):
        self.C, self.dev, self.S, self.G, self.rows, self.wide = C, dev, S, G, rows, wide
        self.n = S
        rng = np.random.default_rng(S + G)
        self.tails = [_sentinel(PAD, k) for k in range(4)]
        self.m, self.v = (_dev(np.concatenate([np.zeros(S, np.float32), self.tails[k]]), dev) for k in (0, 1))
        self.p = _dev(np.concatenate([rng.standard_normal(S).astype(np.float32), self.tails[2]]), dev)
        self.grad = _dev(_sentinel(S + PAD, 3), dev)
        gy = (G + 31) // 32
        self.scratch = torch.empty(gy * S, device=dev) if wide else None
        self.counters = torch.zeros(_columns(S), dtype=torch.int32, device=dev) if wide else None

    def state(self):
        return [t[:self.S].cpu().numpy().copy() for t in (self.m, self.v, self.p)]

    def launch(self, st, g, it, gscale):
        slabs = g[None] if self.G == 1 else st.slabs(g, self.G, self.rows)
        self.grad.copy_(_dev(_sentinel(self.S + PAD, 3), self.dev))
        self.C.reduce_adam(_dev(_with_nan_rows(slabs), self.dev), self.G, self.S, self.S, self.grad, self.p, self.m,
                           self.v, it, *HP, gscale, None, RA_ADAM | RA_WRITE_GRAD, None, 0, 0, self.scratch,
                           self.counters)
        _same_bits(self.grad[:self.S], g, "grad_out is the exact slab sum")
        for k, t in enumerate((self.m, self.v, self.p, self.grad)):
            _same_bits(t[self.S:], _sentinel(PAD, k) if k < 3 else _sentinel(self.S + PAD, 3)[self.S:], "tail %d" % k)
        if self.wide:
            assert not self.counters.any()


class _SlabSum2Adam:
    """slab_sum2 with Adam over n slots: two slab sets scattered through maps with dropped entries
    (their slab columns are NaN), the rest list updating every other slot from grad as it stands."""

    def __init__(self, C, dev, n):
        self.C, self.dev, self.n = C, dev, n
        self.S0, self.S1 = 1028, 68
        n2, self.map0, self.map1, self.rest = _maps(self.S0, self.S1, extra=n - 1028 - 68, seed=8)
        assert n2 == n
        self.d = [_dev(a, dev) for a in (self.map0, self.map1, self.rest)]
        self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.p = _dev(np.random.default_rng(n).standard_normal(n).astype(np.float32), dev)

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.m, self.v, self.p)]

    def launch(self, st, g, it, gscale):
        parts = st.slabs(g, 3)   # [3, n] by target slot
        sets = []
        for mp in (self.map0, self.map1):
            s = np.full((3, len(mp)), np.nan, np.float32)
            s[:, mp >= 0] = parts[:, mp[mp >= 0]]
            sets.append(_dev(s, self.dev))
        grad0 = _sentinel(self.n)
        grad0[self.rest] = g[self.rest]   # written by an earlier launch
        grad = _dev(grad0, self.dev)
        self.C.slab_sum2(sets[0], self.d[0], sets[1], self.d[1], grad, self.p, self.m, self.v, it, *HP, gscale,
                         self.d[2])
        _same_bits(grad, g, "every slot's gradient: the exact slab sum, or as it stood")


def _adam_steps(name, kern, gscale, seed=5):
    """40 consecutive steps from m = v = 0, then t = 1000, 100000 and 2^24 + 3, each step held to
    adam_step64 on the device's own state from before it.  Largest err / bound seen on an MI355X
    over every kernel and gscale below: m 0.447, v 0.443, p 0.998 (the p bound's u |p| term is the
    subtraction's half ulp, reached whenever p sits just above a power of two; a plain numpy
    float32 evaluation reaches 0.99 too, tests/test_adam_reference.py)."""
    dev = kern.dev
    st = GradStream(kern.n, seed)
    it = torch.zeros(1, dtype=torch.int64, device=dev)
    worst = [0.0, 0.0, 0.0]
    for t in ADAM_STEPS:
        g = st.next()
        m0, v0, p0 = kern.state()
        it.fill_(t)   # the kernels read the step count and never advance it
        kern.launch(st, g, it, gscale)
        assert it.item() == t
        m1, v1, p1 = kern.state()
        ref = adam_step64(g, m0, v0, p0, t, *HP, gscale)
        r = _adam_ratios((m1, v1, p1), ref, (name, t))
        worst = [max(a, b) for a, b in zip(worst, r)]
        # gradient always zero: m = v = 0 and the parameter does not move at all
        assert not m1[st.zero].any() and not v1[st.zero].any(), (name, t)
        _same_bits(p1[st.zero], p0[st.zero], (name, t, "zero-gradient slots"))
        assert not np.array_equal(p1[~st.zero], p0[~st.zero])
    print("%s gscale=%g: max err/bound m %.3f v %.3f p %.3f" % (name, gscale, *worst))
    return worst


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 512])
@pytest.mark.parametrize("S,G", [(1540, 1), (8, 1), (1540, 3), (8, 3)])
def test_adam_steps_reduce_adam_narrow(C, cuda_device, S, G, gscale):
    """G = 1 is FlatAdam's call; G = 3 makes the slab sum part of the step."""
    _adam_steps("reduce_adam S=%d G=%d" % (S, G), _ReduceAdam(C, cuda_device, S, G, (0, 1, 2), wide=False), gscale)


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 512])
@pytest.mark.parametrize("fused", ["0", "1"])
def test_adam_steps_reduce_adam_wide(C, cuda_device, monkeypatch, fused, gscale):
    """G = 97: four chunk sums; the three non-zero slabs sit in chunks 0, 1 and 3."""
    monkeypatch.setenv("SML_AE_FUSED_REDUCE", fused)
    _adam_steps("reduce_adam wide fused=%s" % fused, _ReduceAdam(C, cuda_device, 1540, 97, (0, 50, 96), wide=True),
                gscale)


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 512])
def test_adam_steps_slab_sum2(C, cuda_device, gscale):
    """Mapped slots and rest slots alike: every slot gets exactly one update per step."""
    _adam_steps("slab_sum2", _SlabSum2Adam(C, cuda_device, 1540), gscale)
