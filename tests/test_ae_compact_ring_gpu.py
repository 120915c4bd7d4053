"""The compact packed training ring: the four features the reference's normalize_fn zeroes
(cardata indices 0, 2, 4, 5) are left out of the tile-packed ring, and the packed-pair kernel
reads its 18-column operands from 14 floats per row (``csrc/kernels/ae_fused.hip`` CM variants,
``pack_tiles_argmax`` with a live mask).  ``SML_AE_COMPACT=0`` keeps the 18-column ring: the A/B the tests below run."""
import numpy as np
import pytest
import torch

from streamml.data.cardata import normalize_affine
from streamml.models.reference import ae_forward_torch, ae_loss_torch, init_dense_weights
from streamml.ops._ext import load_c
from streamml.ops.ae import NPARAM, AESpec, FusedAE, unpack_image

pytestmark = pytest.mark.gpu

DEAD = [0, 2, 4, 5]
LIVE = [f for f in range(18) if f not in DEAD]
LIVE_MASK = sum(1 << f for f in LIVE)
FULL_TILE, COMPACT_TILE = 64 * 18 + 16, 64 * 14 + 16


def _weights(spec, seed=0):
    w = init_dense_weights(spec.layer_sizes, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for i in range(1, 8, 2):
        w[i] = rng.uniform(-0.2, 0.2, size=w[i].shape).astype(np.float32)
    return w


def _relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)


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


def test_compact_pack_is_the_live_columns_of_the_full_pack(cuda_device):
    C = load_c()
    sc, sh = _norm_t(cuda_device)
    x = torch.from_numpy(_raw(64, 3)).to(cuda_device)
    full = C.pack_tiles_argmax(x, 18, sc, sh)
    comp = C.pack_tiles_argmax(x, 18, sc, sh, live_mask=LIVE_MASK)
    assert full.numel() == 4 * FULL_TILE and comp.numel() == 4 * COMPACT_TILE
    frows, farg = _split(full, FULL_TILE, 18)
    crows, carg = _split(comp, COMPACT_TILE, 14)
    np.testing.assert_array_equal(crows.view(np.uint32), frows[:, LIVE].copy().view(np.uint32))
    np.testing.assert_array_equal(carg, farg)


def test_compact_pack_index_perm_and_contiguous_forms_agree(cuda_device):
    C = load_c()
    sc, sh = _norm_t(cuda_device)
    x = torch.from_numpy(_raw(4096 + 37, 11)).to(cuda_device)
    idx = C.perm_indices(x, x.size(0), 777, 0, 4096)
    a = C.pack_tiles_argmax(x, 18, sc, sh, idx, None, live_mask=LIVE_MASK)
    b = C.pack_tiles_argmax(x, 18, sc, sh, None, None, perm_key=777, perm_n=x.size(0), n_rows=4096,
                            live_mask=LIVE_MASK)
    assert a.numel() == 256 * COMPACT_TILE
    assert torch.equal(a, b)
    c = C.pack_tiles_argmax(x[idx].contiguous(), 18, sc, sh, live_mask=LIVE_MASK)
    assert torch.equal(a, c)
    out = torch.zeros(256 * COMPACT_TILE + 64, dtype=torch.uint8, device=cuda_device)
    C.pack_tiles_argmax(x[idx].contiguous(), 18, sc, sh, None, out, live_mask=LIVE_MASK)
    assert torch.equal(out[:a.numel()], a) and int(out[a.numel():].sum()) == 0


def test_compact_pack_nan_in_a_dead_column_stays_out(cuda_device):
    """Dead columns are the constant 0, not raw * 0 + 0: the rows and the argmax stay finite / exact."""
    C = load_c()
    sc, sh = _norm_t(cuda_device)
    raw = _raw(64, 5)
    clean = C.pack_tiles_argmax(torch.from_numpy(raw).to(cuda_device), 18, sc, sh, live_mask=LIVE_MASK)
    raw[::3, 0] = np.nan
    raw[1::5, 4] = np.inf
    raw[2::7, 5] = -np.inf
    raw[7, 2] = np.nan
    comp = C.pack_tiles_argmax(torch.from_numpy(raw).to(cuda_device), 18, sc, sh, live_mask=LIVE_MASK)
    rows, arg = _split(comp, COMPACT_TILE, 14)
    assert np.isfinite(rows).all()
    assert torch.equal(comp, clean)
    scale, shift = normalize_affine()
    xn = np.nan_to_num(raw, posinf=0.0, neginf=0.0) * scale.astype(np.float32) + shift.astype(np.float32)
    xn[:, DEAD] = 0
    np.testing.assert_array_equal(arg, np.argmax(xn, axis=1))


def _three_steps(monkeypatch, cuda_device, compact, w, raw, B, blocks):
    monkeypatch.setenv("SML_AE_COMPACT", "1" if compact else "0")
    scale, shift = normalize_affine()
    f = FusedAE(AESpec(), w, cuda_device, max_blocks=blocks, scale=scale, shift=shift)
    f.attach_ring(raw, B)
    assert f.ring_xpack.numel() == raw.size(0) // 16 * (COMPACT_TILE if compact else FULL_TILE)
    imgs = []
    for _ in range(3):
        f.step_ring(allreduce=lambda g: imgs.append(g.detach().cpu().numpy().copy()))
    torch.cuda.synchronize()
    return imgs, f.params.detach().cpu().numpy()


@pytest.mark.parametrize("ntiles,blocks", [(2, 16), (30, 16), (64 * 4, 16), (64 * 5, 16), (2 * 4096 + 6, 48)])
def test_compact_ring_matches_18_column_ring(cuda_device, monkeypatch, ntiles, blocks):
    """Same grid, same pairs per wave in the same order (zero, one, even and odd pair counts; the
    ring is two batches, so the third step wraps).  The compact loop feeds the same operands to
    the same instructions (measured: every figure below is 0), and is held to the bounds that
    test_tile_pair_loop_matches_one_tile_loop sets for a K-order change."""
    spec = AESpec()
    w = _weights(spec, seed=7)
    B = 16 * ntiles
    raw = torch.from_numpy(_raw(2 * B, 17)).to(cuda_device)
    old, old_p = _three_steps(monkeypatch, cuda_device, False, w, raw, B, blocks)
    new, new_p = _three_steps(monkeypatch, cuda_device, True, w, raw, B, blocks)
    print("step-0 grad relerr", _relerr(new[0][:NPARAM], old[0][:NPARAM]),
          "later", [_relerr(b[:NPARAM], a[:NPARAM]) for a, b in zip(old[1:], new[1:])],
          "params", _relerr(new_p, old_p), "metrics", old[0][NPARAM:], new[0][NPARAM:])
    assert _relerr(new[0][:NPARAM], old[0][:NPARAM]) < 1e-6
    for a, b in zip(old, new):
        np.testing.assert_allclose(b[NPARAM:NPARAM + 2], a[NPARAM:NPARAM + 2], rtol=1e-6)   # loss, |h1| sums
        assert abs(b[NPARAM + 2] - a[NPARAM + 2]) <= max(2, 1e-3 * B)                     # argmax near-ties
        assert b[NPARAM + 3] == a[NPARAM + 3] == B
    for a, b in zip(old[1:], new[1:]):
        assert _relerr(b[:NPARAM], a[:NPARAM]) < 1e-4
    assert _relerr(new_p, old_p) < 1e-4


def test_compact_gradient_placement_vs_autograd(cuda_device, monkeypatch):
    """One step's gradient through the compact ring against torch autograd.  The dead inputs'
    W1 rows and the dead outputs' W4 columns are non-zero random: the dead inputs' dW1 rows are
    exact zeros, the dead outputs' dW4 columns and db4 entries do get their gradients.  A wrong
    fold or slot permutation is off by orders of magnitude, not by the bf16 noise bounded here."""
    monkeypatch.delenv("SML_AE_COMPACT", raising=False)
    spec = AESpec()
    w = _weights(spec, seed=13)
    assert all(np.abs(w[0][f]).min() > 0 for f in DEAD) and all(np.abs(w[6][:, f]).min() > 0 for f in DEAD)
    scale, shift = normalize_affine()
    B = 16 * 64
    raw = _raw(B, 23)
    f = FusedAE(spec, w, cuda_device, max_blocks=16, scale=scale, shift=shift)
    f.attach_ring(torch.from_numpy(raw).to(cuda_device), B)
    assert f.ring_xpack.numel() == B // 16 * COMPACT_TILE
    imgs = []
    f.step_ring(allreduce=lambda g: imgs.append(g.detach().cpu().numpy().copy()))
    torch.cuda.synchronize()
    g_fused = unpack_image(imgs[0][:NPARAM] / B, spec)
    xin = torch.from_numpy((raw * scale + shift).astype(np.float32))
    wt = [torch.tensor(a, dtype=torch.float32, requires_grad=True) for a in w]
    loss, _, _ = ae_loss_torch(xin, wt, spec.activations, spec.activity_l1)
    g_ref = [g.numpy() for g in torch.autograd.grad(loss, wt)]
    for i, (gf, gr) in enumerate(zip(g_fused, g_ref)):
        print("tensor", i, "relerr", _relerr(gf, gr))
        assert gf.shape == gr.shape and _relerr(gf, gr) < 3e-2
    assert not g_fused[0][DEAD].any() and not g_ref[0][DEAD].any()
    assert np.abs(g_ref[6][:, DEAD]).max() > 0 and np.abs(g_ref[7][DEAD]).max() > 0
    assert _relerr(g_fused[6][:, DEAD], g_ref[6][:, DEAD]) < 3e-2
    assert _relerr(g_fused[7][DEAD], g_ref[7][DEAD]) < 3e-2
    for d in DEAD:   # each dead output on its own: a swap among them would pass the joint norm
        assert _relerr(g_fused[6][:, d], g_ref[6][:, d]) < 3e-2
    assert imgs[0][NPARAM + 3] == B


def test_compact_accuracy_ties_match_18_column(cuda_device, monkeypatch):
    """A clear input winner per row, rows whose live values are all negative (a dead column's 0
    wins, the lowest of them) and, through a negative output bias, rows whose outputs are all 0
    after the relu (the argmax of y is the lowest ORIGINAL index): the correct count of the
    compact step equals the 18-column step's exactly."""
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


@pytest.mark.parametrize("norm", ["all_live", "none"])
def test_other_normalisers_keep_the_18_column_ring(cuda_device, monkeypatch, norm):
    monkeypatch.delenv("SML_AE_COMPACT", raising=False)
    spec = AESpec()
    w = _weights(spec, seed=3)
    B = 16 * 8
    raw = torch.from_numpy(_raw(2 * B, 41)).to(cuda_device)
    kw = {} if norm == "none" else {"scale": np.full(18, 0.05), "shift": np.full(18, -1.0)}
    f = FusedAE(spec, w, cuda_device, max_blocks=16, **kw)
    f.attach_ring(raw, B)
    assert f.ring_xpack.numel() == 2 * B // 16 * FULL_TILE and f.ring_live == 0
    before = f.params.clone()
    for _ in range(2):
        f.step_ring()
    torch.cuda.synchronize()
    assert torch.isfinite(f.params).all() and not torch.equal(f.params, before)
    assert f.read_metrics()["rows"] == 2 * B


def test_compact_buffer_is_refused_by_18_column_variants(cuda_device, monkeypatch):
    C = load_c()
    spec = AESpec()
    scale, shift = normalize_affine()
    B = 16 * 8
    raw = torch.from_numpy(_raw(2 * B, 43)).to(cuda_device)
    f = FusedAE(spec, _weights(spec, seed=3), cuda_device, max_blocks=16, scale=scale, shift=shift)
    f.attach_ring(raw, B)
    assert f.ring_live == LIVE_MASK and f.ring_xpack.numel() == 2 * B // 16 * COMPACT_TILE

    def launch(live):
        return C.ae_train_partials(f.ring, f.scale, f.shift, f.params, f.partials, None, spec.dims, spec.act_codes,
                                   float(spec.activity_l1), True, f.max_blocks, B, f.cursor, f.ring_xpack,
                                   xpack_live=live)

    with pytest.raises(RuntimeError):   # declared as the 18-column layout: the size does not fit
        launch(0)
    monkeypatch.setenv("SML_AE_ILP", "1")   # the one-tile loop reads 18-column tiles only
    with pytest.raises(RuntimeError):
        launch(LIVE_MASK)
    monkeypatch.delenv("SML_AE_ILP")
    assert launch(LIVE_MASK) > 0
    torch.cuda.synchronize()
