"""The lane-ordered compact ring and the trimmed packed-pair loop (``csrc/kernels/ae_fused.hip``).

The compact packed ring stores a row's 14 live features in the order the train loop's lanes read
them (features 16, 1, 17, 3, 6, 7, ..., 15: ``pack_tiles_argmax(..., lane_order=True)``), so every
live input is read straight into its operand slot; the loop itself lost selects, conversions and
its vector loop control.  None of that may change a bit of any result: every comparison below is
``assert_array_equal``.

``tests/golden/ae_loop_diet_parent.npz`` holds the gradient images, metric sums and final
parameters of the 18-column ring run and of the raw-row (``step``) run, recorded on an MI355X from
the build before this change by ``record_parent_golden`` below (same seeds, same calls).
"""
import os

import numpy as np
import pytest
import torch

from streamml.data.cardata import normalize_affine
from streamml.models.reference import ae_forward_torch, init_dense_weights
from streamml.ops._ext import load_c
from streamml.ops.ae import NPARAM, AESpec, FusedAE

pytestmark = pytest.mark.gpu

DEAD = [0, 2, 4, 5]
LIVE_MASK = sum(1 << f for f in range(18) if f not in DEAD)
LANE_ORDER = [16, 1, 17, 3] + list(range(6, 16))
FULL_TILE, COMPACT_TILE = 64 * 18 + 16, 64 * 14 + 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ae_loop_diet_parent.npz")
GOLDEN_SHAPES = [(30, 16), (64 * 5, 16)]


def _weights(spec, seed=0):
    w = init_dense_weights(spec.layer_sizes, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for i in range(1, 8, 2):
        w[i] = rng.uniform(-0.2, 0.2, size=w[i].shape).astype(np.float32)
    return w


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, size=(n, 18)) * 40).astype(np.float32)


def _norm_t(dev):
    return tuple(torch.tensor(a, dtype=torch.float32, device=dev) for a in normalize_affine())


def _split(packed, tile, cols):
    """Packed ring bytes -> (rows [n, cols] float32, argmax bytes [n])."""
    tiles = packed.cpu().numpy().reshape(-1, tile)
    rows = tiles[:, :64 * cols].copy().view(np.float32).reshape(-1, cols)
    return rows, tiles[:, 64 * cols:].reshape(-1)


def _lane(C, x, sc, sh, *a, **kw):
    return C.pack_tiles_argmax(x, 18, sc, sh, *a, live_mask=LIVE_MASK, lane_order=True, **kw)


def test_lane_ordered_pack_is_those_columns_of_the_full_pack(cuda_device):
    C = load_c()
    sc, sh = _norm_t(cuda_device)
    x = torch.from_numpy(_raw(64, 3)).to(cuda_device)
    full = C.pack_tiles_argmax(x, 18, sc, sh)
    lane = _lane(C, x, sc, sh)
    assert full.numel() == 4 * FULL_TILE and lane.numel() == 4 * COMPACT_TILE
    frows, farg = _split(full, FULL_TILE, 18)
    lrows, larg = _split(lane, COMPACT_TILE, 14)
    np.testing.assert_array_equal(lrows.view(np.uint32), frows[:, LANE_ORDER].copy().view(np.uint32))
    np.testing.assert_array_equal(larg, farg)


def test_lane_ordered_pack_index_perm_out_and_contiguous_forms_agree(cuda_device):
    C = load_c()
    sc, sh = _norm_t(cuda_device)
    x = torch.from_numpy(_raw(4096 + 37, 11)).to(cuda_device)
    idx = C.perm_indices(x, x.size(0), 777, 0, 4096)
    a = _lane(C, x, sc, sh, idx, None)
    b = _lane(C, x, sc, sh, None, None, perm_key=777, perm_n=x.size(0), n_rows=4096)
    assert a.numel() == 256 * COMPACT_TILE
    assert torch.equal(a, b)
    c = _lane(C, x[idx].contiguous(), sc, sh)
    assert torch.equal(a, c)
    out = torch.zeros(256 * COMPACT_TILE + 64, dtype=torch.uint8, device=cuda_device)
    _lane(C, x[idx].contiguous(), sc, sh, None, out)
    assert torch.equal(out[:a.numel()], a) and int(out[a.numel():].sum()) == 0
    rows, _ = _split(a, COMPACT_TILE, 14)
    frows, _ = _split(C.pack_tiles_argmax(x, 18, sc, sh, idx, None), FULL_TILE, 18)
    np.testing.assert_array_equal(rows.view(np.uint32), frows[:, LANE_ORDER].copy().view(np.uint32))


def test_lane_ordered_pack_nan_in_a_dead_column_changes_nothing(cuda_device):
    C = load_c()
    sc, sh = _norm_t(cuda_device)
    raw = _raw(64, 5)
    clean = _lane(C, torch.from_numpy(raw).to(cuda_device), sc, sh)
    raw[::3, 0] = np.nan
    raw[1::5, 4] = np.inf
    raw[2::7, 5] = -np.inf
    raw[7, 2] = np.nan
    dirty = _lane(C, torch.from_numpy(raw).to(cuda_device), sc, sh)
    assert torch.equal(dirty, clean)
    assert np.isfinite(_split(dirty, COMPACT_TILE, 14)[0]).all()


def test_lane_order_is_refused_for_other_layouts(cuda_device):
    C = load_c()
    sc, sh = _norm_t(cuda_device)
    x = torch.from_numpy(_raw(64, 9)).to(cuda_device)
    with pytest.raises(RuntimeError):
        C.pack_tiles_argmax(x, 18, sc, sh, lane_order=True)                           # 18-column layout
    with pytest.raises(RuntimeError):
        C.pack_tiles_argmax(x, 18, sc, sh, live_mask=LIVE_MASK | 1, lane_order=True)   # another live set


def _ring_steps(monkeypatch, dev, compact, w, raw, B, blocks):
    """Three step_ring calls: (gradient images incl. the four metric sums, final parameters)."""
    monkeypatch.setenv("SML_AE_COMPACT", "1" if compact else "0")
    scale, shift = normalize_affine()
    f = FusedAE(AESpec(), w, dev, max_blocks=blocks, scale=scale, shift=shift)
    f.attach_ring(raw, B)
    assert f.ring_xpack.numel() == raw.size(0) // 16 * (COMPACT_TILE if compact else FULL_TILE)
    assert f.ring_live == (LIVE_MASK if compact else 0)
    imgs = []
    for _ in range(3):
        f.step_ring(allreduce=lambda g: imgs.append(g.detach().cpu().numpy().copy()))
    torch.cuda.synchronize()
    return np.stack(imgs), f.params.detach().cpu().numpy()


def _direct_steps(dev, w, raw, B, blocks):
    """Three raw-row step calls (batches 0, 1, 0 of raw)."""
    scale, shift = normalize_affine()
    f = FusedAE(AESpec(), w, dev, max_blocks=blocks, scale=scale, shift=shift)
    imgs = []
    for i in (0, 1, 0):
        f.step(raw[i * B:(i + 1) * B], allreduce=lambda g: imgs.append(g.detach().cpu().numpy().copy()))
    torch.cuda.synchronize()
    return np.stack(imgs), f.params.detach().cpu().numpy()


def _case(ntiles):
    B = 16 * ntiles
    return _weights(AESpec(), seed=7), _raw(2 * B, 17), B


@pytest.mark.parametrize("ntiles,blocks", [(2, 16), (30, 16), (64 * 4, 16), (64 * 5, 16), (2 * 4096 + 6, 48)])
def test_lane_ordered_ring_is_bit_identical_to_18_column_ring(cuda_device, monkeypatch, ntiles, blocks):
    """Waves with zero, one, an even and an odd number of pairs (the unrolled loop's early exit and
    the empty wave); the ring is two batches, so the third step wraps."""
    w, raw, B = _case(ntiles)
    raw = torch.from_numpy(raw).to(cuda_device)
    old, old_p = _ring_steps(monkeypatch, cuda_device, False, w, raw, B, blocks)
    new, new_p = _ring_steps(monkeypatch, cuda_device, True, w, raw, B, blocks)
    assert (old[:, NPARAM + 3] == B).all()
    np.testing.assert_array_equal(new[:, NPARAM:], old[:, NPARAM:])     # the four metric sums
    np.testing.assert_array_equal(new.view(np.uint32), old.view(np.uint32))
    np.testing.assert_array_equal(new_p.view(np.uint32), old_p.view(np.uint32))


@pytest.mark.parametrize("ntiles,blocks", GOLDEN_SHAPES)
def test_18_column_ring_matches_parent_build(cuda_device, monkeypatch, ntiles, blocks):
    gold = np.load(GOLDEN)
    w, raw, B = _case(ntiles)
    imgs, params = _ring_steps(monkeypatch, cuda_device, False, w, torch.from_numpy(raw).to(cuda_device), B, blocks)
    np.testing.assert_array_equal(imgs.view(np.uint32), gold[f"ring18_{ntiles}_imgs"].view(np.uint32))
    np.testing.assert_array_equal(params.view(np.uint32), gold[f"ring18_{ntiles}_params"].view(np.uint32))


@pytest.mark.parametrize("ntiles,blocks", GOLDEN_SHAPES)
def test_raw_row_step_matches_parent_build(cuda_device, monkeypatch, ntiles, blocks):
    monkeypatch.delenv("SML_AE_COMPACT", raising=False)
    gold = np.load(GOLDEN)
    w, raw, B = _case(ntiles)
    imgs, params = _direct_steps(cuda_device, w, torch.from_numpy(raw).to(cuda_device), B, blocks)
    np.testing.assert_array_equal(imgs.view(np.uint32), gold[f"direct_{ntiles}_imgs"].view(np.uint32))
    np.testing.assert_array_equal(params.view(np.uint32), gold[f"direct_{ntiles}_params"].view(np.uint32))


def record_parent_golden(dev, path):
    """Run on the build the fixture is to pin (not a test): writes GOLDEN's arrays to ``path``."""
    class _Env:   # the two calls of monkeypatch that _ring_steps uses
        @staticmethod
        def setenv(k, v):
            os.environ[k] = v

    out = {}
    for ntiles, blocks in GOLDEN_SHAPES:
        w, raw, B = _case(ntiles)
        rawt = torch.from_numpy(raw).to(dev)
        out[f"ring18_{ntiles}_imgs"], out[f"ring18_{ntiles}_params"] = _ring_steps(_Env, dev, False, w, rawt, B, blocks)
        os.environ.pop("SML_AE_COMPACT", None)
        out[f"direct_{ntiles}_imgs"], out[f"direct_{ntiles}_params"] = _direct_steps(dev, w, rawt, B, blocks)
    np.savez_compressed(path, **out)


def test_lane_ordered_accuracy_ties_match_18_column(cuda_device, monkeypatch):
    """A clear input winner per row, rows whose live values are all negative (a dead column's 0
    wins, the lowest of them) and, through a negative output bias, rows whose outputs are all 0
    after the relu (the argmax of y is the lowest ORIGINAL index): the correct count on the
    lane-ordered ring equals the 18-column ring's exactly."""
    spec = AESpec()
    w = _weights(spec, seed=21)
    w[7] = (-0.3 * np.abs(w[6]).sum(0)).astype(np.float32)
    scale, shift = normalize_affine()
    n = 16 * 64
    rng = np.random.default_rng(31)
    xn = rng.uniform(-1.5, 1.0, size=(n, 18)).astype(np.float32)
    xn[:, [1, 8]] = -1.4
    k = rng.integers(0, 18, n)
    xn[np.arange(n), k] = 1.3 + rng.uniform(0, 0.5, n).astype(np.float32)   # clear winner per row
    neg = np.isin(k, DEAD)                                                   # the winner was a dead column:
    xn[neg] = -np.abs(xn[neg]) - 0.1                                         # every live value negative
    live = np.asarray(scale) != 0
    raw = np.where(live, (xn - np.asarray(shift)) / np.where(live, scale, 1), 0).astype(np.float32)
    xin = (raw * scale + shift).astype(np.float32)
    assert neg.sum() > 50 and (np.argmax(xin[neg], 1) == 0).all()
    y, _ = ae_forward_torch(torch.from_numpy(xin), [torch.from_numpy(a) for a in w], spec.activations)
    allzero = y.numpy().max(1) == 0
    assert allzero.sum() > 50 and (~allzero).sum() > 50
    rawt = torch.from_numpy(raw).to(cuda_device)
    got = {}
    for compact in (False, True):
        monkeypatch.setenv("SML_AE_COMPACT", "1" if compact else "0")
        f = FusedAE(spec, w, cuda_device, max_blocks=16, scale=scale, shift=shift)
        f.attach_ring(rawt, n)
        assert f.ring_xpack.numel() == n // 16 * (COMPACT_TILE if compact else FULL_TILE)
        imgs = []
        f.step_ring(allreduce=lambda g: imgs.append(g.detach().cpu().numpy().copy()))
        torch.cuda.synchronize()
        got[compact] = imgs[0][NPARAM:]
    print("correct", got[False][2], got[True][2], "of", n)
    assert got[True][3] == got[False][3] == n
    assert 0 < got[False][2] < n
    assert got[True][2] == got[False][2]
