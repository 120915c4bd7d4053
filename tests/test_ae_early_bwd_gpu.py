"""Early backward LDS writes in the packed-pair train loop (``XP 4``, ``csrc/kernels/ae_fused.hip``).

``XP 4`` brings five of the seven backward weight-gradient operands (``dz4b[0..1]``, ``dz4bu``,
``dz3b``, ``dz2b``) to the rows-on-K layout through per-wave LDS slots 7..11, written as soon as
each is packed and read back transposed before the gradient MFMAs, instead of one MFMA against the
identity plus two ``v_cvt_pk_bf16_f32`` each (``XP 3``).  The transposed copy is the same bf16 bits
either way and every MFMA that feeds a result keeps its shape, operands, K positions and order, so
``XP 4`` is held to ``XP 3`` bit for bit: every comparison below is ``assert_array_equal`` on
``uint32``.  ``XP 3`` is the kernel of the build before this change, itself tied to that build's
recorded outputs through ``tests/test_ae_lane_ring_gpu.py``.

``SML_AE_PAIR_XP`` is read at every launch, so both run in one process;
``ae_train_last_variant()`` says which instance each run really launched.
"""
import numpy as np
import pytest
import torch

from streamml.data.cardata import normalize_affine
from streamml.models.reference import init_dense_weights
from streamml.ops._ext import load_c
from streamml.ops.ae import NPARAM, AESpec, FusedAE

pytestmark = pytest.mark.gpu

# the 4-wave compact-ring instances: (XP, TS, LDS bytes per workgroup)
XP3 = (3, 10, 35328)
XP4 = (4, 12, 39424)


def _weights(spec, seed=0):   # as tests/test_ae_lane_ring_gpu.py
    w = init_dense_weights(spec.layer_sizes, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for i in range(1, 8, 2):
        w[i] = rng.uniform(-0.2, 0.2, size=w[i].shape).astype(np.float32)
    return w


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, size=(n, 18)) * 40).astype(np.float32)


def _case(ntiles):
    B = 16 * ntiles
    return _weights(AESpec(), seed=7), _raw(2 * B, 17), B


def _ring_steps(monkeypatch, dev, xp, w, raw, B, blocks):
    """Three step_ring calls on the compact ring at 4 waves per SIMD with SML_AE_PAIR_XP=xp:
    (gradient images incl. the four metric sums, parameters, adam m, adam v, launched variants)."""
    monkeypatch.setenv("SML_AE_COMPACT", "1")
    monkeypatch.setenv("SML_AE_PAIR_OCC", "4")
    monkeypatch.setenv("SML_AE_PAIR_XP", str(xp))
    C = load_c()
    scale, shift = normalize_affine()
    f = FusedAE(AESpec(), w, dev, max_blocks=blocks, scale=scale, shift=shift)
    f.attach_ring(raw, B)
    imgs, variants = [], []
    for _ in range(3):
        f.step_ring(allreduce=lambda g: imgs.append(g.detach().cpu().numpy().copy()))
        variants.append(tuple(C.ae_train_last_variant()))
    torch.cuda.synchronize()
    state = [t.detach().cpu().numpy().copy() for t in (f.params, f.m, f.v)]
    return np.stack(imgs), state, variants


@pytest.mark.parametrize("ntiles,blocks", [(2, 16), (30, 16), (64 * 4, 16), (64 * 5, 16), (2 * 4096 + 6, 48)])
def test_early_backward_writes_are_bit_identical_to_mfma_identity(cuda_device, monkeypatch, ntiles, blocks):
    """Waves with zero, one, an even and an odd number of pairs: the odd count takes the unrolled
    loop's early exit, the even one reuses the slots across consecutive trips; the ring is two
    batches, so the third step wraps."""
    w, raw, B = _case(ntiles)
    raw = torch.from_numpy(raw).to(cuda_device)
    old, old_s, old_v = _ring_steps(monkeypatch, cuda_device, 3, w, raw, B, blocks)
    new, new_s, new_v = _ring_steps(monkeypatch, cuda_device, 4, w, raw, B, blocks)
    print("launched", old_v, new_v)
    assert old_v == [XP3] * 3   # a comparison of XP 3 with itself would prove nothing
    assert new_v == [XP4] * 3
    assert (old[:, NPARAM + 3] == B).all()
    np.testing.assert_array_equal(new.view(np.uint32), old.view(np.uint32))   # gradients + metric sums
    for a, b in zip(new_s, old_s):                                             # params, adam m, adam v
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(new_s[1]).max() > 0   # the steps did train: adam m is not the zeros it started as


def test_xp4_means_xp3_where_no_xp4_instance_exists(cuda_device, monkeypatch):
    """The 18-column ring has no XP 4 instance (it would lose a workgroup per CU): the switch falls
    back to the XP 3 kernel there, which is not one of the two noted instances."""
    w, raw, B = _case(30)
    raw = torch.from_numpy(raw).to(cuda_device)
    monkeypatch.setenv("SML_AE_PAIR_OCC", "4")
    C = load_c()
    scale, shift = normalize_affine()
    got = {}
    for xp in (3, 4):
        monkeypatch.setenv("SML_AE_COMPACT", "0")
        monkeypatch.setenv("SML_AE_PAIR_XP", str(xp))
        f = FusedAE(AESpec(), w, cuda_device, max_blocks=16, scale=scale, shift=shift)
        f.attach_ring(raw, B)
        imgs = []
        f.step_ring(allreduce=lambda g: imgs.append(g.detach().cpu().numpy().copy()))
        assert tuple(C.ae_train_last_variant())[:2] == (-1, -1)
        torch.cuda.synchronize()
        got[xp] = imgs[0]
    np.testing.assert_array_equal(got[4].view(np.uint32), got[3].view(np.uint32))
