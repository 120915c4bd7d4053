"""Lane masks by masked transposed reads in the packed-pair train loop (``XP 5``, ``csrc/kernels/ae_fused.hip``).

``XP 4`` builds the lane-masked copies of three weight-gradient operands (``xur``, ``h3r``, ``dz2r``)
with twelve ``v_cndmask`` per trip.  ``XP 5`` reads each of them twice through two loop-invariant
lane addresses (``tr_rd_off_half``, ``csrc/include/sml_common.h``) whose masked source lanes point
at cells of zeros (and, for the ``xub`` slot, at the bf16 1.0 of the bias feature), and takes the
pad lane out of the L1 sum with a multiply by 0 / 1 instead of a select.  The operands are the same
bf16 bits, the masked products stay exact zeros and no MFMA changes shape, K positions or order, so
``XP 5`` is held to ``XP 4`` bit for bit: every comparison below is ``assert_array_equal`` on the
raw words.  ``XP 4`` is itself tied to the recorded outputs of an older build through
``tests/test_ae_early_bwd_gpu.py`` and ``tests/test_ae_lane_ring_gpu.py``.

``SML_AE_PAIR_XP`` is read at every launch, so both run in one process;
``ae_train_last_variant()`` says which instance each run really launched.  The 18-column ring and
the raw-row ``step`` have no ``XP 5`` instance (the switch means ``XP 3`` there, as ``XP 4`` does).
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
XP4 = (4, 12, 39424)
XP5 = (5, 12, 40480)   # + the lane-mask cells: two 512-B slot strides and 32 B


def _weights(spec, seed=0):   # as tests/test_ae_lane_ring_gpu.py
    w = init_dense_weights(spec.layer_sizes, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for i in range(1, 8, 2):
        w[i] = rng.uniform(-0.2, 0.2, size=w[i].shape).astype(np.float32)
    return w


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, size=(n, 18)) * 40).astype(np.float32)


def _ring_steps(monkeypatch, dev, xp, compact, w, raw, B, blocks):
    """Three step_ring calls at 4 waves per SIMD with SML_AE_PAIR_XP=xp: (gradient images incl. the
    four metric sums, [params, adam m, adam v, step counter, ring cursor], launched variants)."""
    monkeypatch.setenv("SML_AE_COMPACT", compact)
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
    state = [t.detach().cpu().numpy().copy() for t in (f.params, f.m, f.v, f.iter, f.cursor)]
    return np.stack(imgs), state, variants


def _assert_same_bits(new, new_s, old, old_s):
    np.testing.assert_array_equal(new.view(np.uint32), old.view(np.uint32))   # gradients + metric sums
    for a, b in zip(new_s[:3], old_s[:3]):                                     # params, adam m, adam v
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(new_s[3], old_s[3])                          # step counter
    np.testing.assert_array_equal(new_s[4], old_s[4])                          # ring cursor


@pytest.mark.parametrize("ntiles,blocks", [(2, 16), (30, 16), (64 * 4, 16), (64 * 5, 16), (2 * 4096 + 6, 48)])
def test_masked_reads_are_bit_identical_to_selects(cuda_device, monkeypatch, ntiles, blocks):
    """Waves with zero, one, an even and an odd number of pairs: the odd count takes the unrolled
    loop's early exit, the even one reuses the slots across consecutive trips; the ring is two
    batches, so the third step wraps."""
    B = 16 * ntiles
    w = _weights(AESpec(), seed=7)
    raw = torch.from_numpy(_raw(2 * B, 17)).to(cuda_device)
    old, old_s, old_v = _ring_steps(monkeypatch, cuda_device, 4, "1", w, raw, B, blocks)
    new, new_s, new_v = _ring_steps(monkeypatch, cuda_device, 5, "1", w, raw, B, blocks)
    print("launched", old_v, new_v)
    assert old_v == [XP4] * 3   # a comparison of XP 4 with itself would prove nothing
    assert new_v == [XP5] * 3
    assert (old[:, NPARAM + 3] == B).all()
    _assert_same_bits(new, new_s, old, old_s)
    assert int(new_s[3][0]) == 3 and np.abs(new_s[1]).max() > 0   # the steps did train
    assert np.isfinite(new[:, NPARAM + 1]).all() and (new[:, NPARAM + 1] > 0).all()   # the L1 sums


def test_xp5_means_xp3_where_no_xp5_instance_exists(cuda_device, monkeypatch):
    """The 18-column ring has no XP 4 / XP 5 instance: the switch falls back to the XP 3 kernel
    there, which is not one of the noted instances, and computes what XP 4 does."""
    B = 16 * 30
    w = _weights(AESpec(), seed=7)
    raw = torch.from_numpy(_raw(2 * B, 17)).to(cuda_device)
    old, old_s, old_v = _ring_steps(monkeypatch, cuda_device, 4, "0", w, raw, B, 16)
    new, new_s, new_v = _ring_steps(monkeypatch, cuda_device, 5, "0", w, raw, B, 16)
    assert [v[:2] for v in old_v + new_v] == [(-1, -1)] * 6
    _assert_same_bits(new, new_s, old, old_s)
