// sml-build: no-slp
// Fused dense-autoencoder kernels for gfx950 (MI355X).
//
// Model family: Input(D) -> Dense(n1, a1) -> Dense(n2, a2) -> Dense(n3, a3) -> Dense(D, a4)
// (reference: AUTOENCODER-TensorFlow-IO-Kafka/cardata-v3.py:187-194, D=18, 14/7/7,
//  tanh/relu/tanh/relu, L1 activity regulariser 1e-7 on layer 1; the creditcard
//  notebook uses D=30).  Loss = MSE (+ l1*sum|h1| / B), metric = categorical
// accuracy of the reconstruction -- the op census decoded from the reference's TF
// profile trace (MatMul/BiasAdd/Tanh/Relu/SquaredDifference/
// ActivityRegularizer/ArgMax...).
//
// Design (MI355X-first, not a port of the 11-GEMM TF graph):
//  * one wave owns 16-row tiles; every layer is one or two 16x16x16 bf16 MFMAs in
//    feature-major orientation so activations flow layer->layer in registers;
//  * weights (as MFMA A fragments) stay in VGPRs for the whole launch;
//  * biases ride in the padded parameter image as the row of a constant-1 input
//    slot, so bias gradients fall out of the weight-gradient MFMA for free;
//  * weight gradients are MFMA contractions over rows (K = 16 rows per tile),
//    accumulated in registers across all tiles the wave visits; a per-workgroup
//    fp32 slab is written once per launch (deterministic, no float atomics);
//  * a second small kernel reduces the slabs and applies Adam (Keras semantics:
//    bias-corrected lr_t, epsilon 1e-7) elementwise on the padded image.
//  * the reference model's default loop (SML_AE_ILP=3, train_pair_packed) takes two
//    contiguous tiles per iteration and packs them into ONE fragment wherever a layer is
//    narrower than 16: the 7-wide layers 2-3 (+ bias slots), inputs 16-17 + the bias input
//    of layer 1 and outputs 16-17 of layer 4.  The weights become block-diagonal / masked
//    copies built once per launch, so every layer is still one MFMA, and the packed
//    accumulators are folded into the image when the slab is written (packed_fold_src).
//    The loop is issue-bound: this cut VALU 27 %, LDS 31 %, SALU 40 % per row against
//    the one-tile loop (SML_AE_ILP=1), 37 -> 47 G rows/s (profiles/r02/ilp).
//  * the cardata normaliser zeroes four of the 18 features, so its packed ring stores the 14
//    live ones (compact ring, CM variants of the packed-pair loop): 57 instead of 73 B per
//    row from HBM and through LDS.  The compute is the 18-column loop's, operand for operand,
//    so the results are bit-identical to it (profiles/r07/compact_ring).  A compact row holds
//    its features in the order the loop's lanes read them (16, 1, 17, 3, 6, 7, ..., 15), so
//    every live input lands in its operand slot with no select (profiles/r08/loop_diet).
//
// Padded parameter image (fp32, 1536 floats), row-major [in][out]:
//   L1 [32][16] @0    (bias = row 31)     requires D  <= 31, n1 <= 15
//   L2 [16][16] @512  (bias = row 15)     requires n1 <= 15, n2 <= 15
//   L3 [16][16] @768  (bias = row 15)     requires n2 <= 15, n3 <= 15
//   L4 [16][32] @1024 (bias = row 15)     requires n3 <= 15
// Slab = 1536 gradient sums + 4 metric sums {sum sq err, sum |h1|, correct, rows}.
#include <cstdlib>

#include "sml_common.h"
#include "sml_adam.h"
#include "sml_ae_variants.h"

using namespace sml;

namespace {

constexpr int WAVES = 4;  // waves per workgroup
constexpr int OFF1 = 0, OFF2 = 512, OFF3 = 768, OFF4 = 1024;
constexpr int NPARAM = 1536;
constexpr int NSLOT = 1540;
// LDS-DMA input ring (PF > 0 variants): per wave ring_bytes<OCC>() after the slab area.
// A 16-row tile of contiguous rows is 64*D bytes (D = 18: 1152 B), moved by two
// global_load_lds_dwordx4 (64 lanes x 16 B + (4D - 64) lanes x 16 B).
constexpr int SLAB_BYTES = WAVES * NSLOT * 4;  // 24640, a multiple of 16

struct AEArgs {
  const float* x;        // [n, ld] raw or normalised rows
  int64_t n;
  int64_t ld;
  const float* scale;    // [D] per-column affine (fused normalize_fn), may be null
  const float* shift;
  const float* params;   // padded image
  float* partials;       // [grid][NSLOT]
  int64_t* iter;         // incremented by block 0 when non-null
  const int64_t* cursor; // device ring cursor: rows start at x + cursor[0]*ld (null = 0)
  // tile-packed ring (XM 1): per 16-row tile the 64*D bytes of NORMALISED rows, then the
  // 16 bytes of argmax(normalised x), both computed once at ingest (pack_tiles_argmax:
  // normalize_fn, cardata-v3.py:78-168, applied where the event enters, like K8) -- one 64*D + 16 byte
  // block, so the tile's two DMAs carry the argmax too.  x is data, not a model output, so
  // its half of the accuracy metric (tf.argmax(x) == tf.argmax(y)) need not be recomputed
  // every time a row is trained on.
  const uint8_t* xpack;
  int D, n1, n2, n3;
  int a1, a2, a3, a4;
  float l1;
  int want_acc;
};

// Activation codes are compile-time when PACK >= 0 (a1 | a2<<2 | a3<<4 | a4<<6),
// runtime otherwise.  The reference model (tanh, relu, tanh, relu) is PACK 0x66.
// (PACK_REF, PACK_DYN: sml_ae_variants.h)
static_assert(PACK_REF == (ACT_TANH | (ACT_RELU << 2) | (ACT_TANH << 4) | (ACT_RELU << 6)), "the reference pack");

template <int PACK>
__device__ __forceinline__ int act_of(const AEArgs& a, int i) {
  if constexpr (PACK >= 0) {
    return (PACK >> (2 * i)) & 3;
  } else {
    return i == 0 ? a.a1 : i == 1 ? a.a2 : i == 2 ? a.a3 : a.a4;
  }
}

struct Frags {  // register-resident operands for one launch
  bf16x4 w1t[2], w2t, w3t, w4t[2];  // forward A operands  (W^T)
  bf16x4 w4[2], w3, w2;             // backward A operands (W)
  f32x4 b1, b2, b3, b4[2];          // biases in C layout
};

__device__ __forceinline__ short bfbits(float v) { return __builtin_bit_cast(short, (__bf16)v); }

template <int PACK>
constexpr bool zero_preserving() {
  if (PACK < 0) return false;
  for (int i = 0; i < 4; ++i)
    if (((PACK >> (2 * i)) & 3) == ACT_SIGMOID) return false;
  return true;
}

// Branch-free guarded parameter load: the address is clamped to a valid element and
// the value selected afterwards (a `cond ? P[i] : 0` makes hipcc branch around every
// load and wait vmcnt(0) for each one -- ~50 serial L2 round trips per wave).
__device__ __forceinline__ float ldsel(const float* P, bool cond, int idx) {
  const float v = P[cond ? idx : 0];
  return cond ? v : 0.f;
}

// FOLD: biases enter the forward MFMAs through the constant-1 input slot
// (row 31 of L1, row 15 of L2..L4) instead of an fp32 accumulator init.
// PRE: layers 1 and 3 are tanh; their forward weights (and folded biases) are stored
// pre-multiplied by 2*log2(e), so the MFMA already yields the exp2 argument of
// tanh(z) = 1 - 2 / (2^(2 log2(e) z) + 1) (one v_mul per activation saved).
constexpr float kTanhExp2 = 2.8853900817779268f;

// INJ (with FOLD + PRE, layer 2 relu / linear): the constant-1 bias slot 15 of each hidden
// layer is produced by the forward MFMA itself instead of a v_add after the activation:
// the fragment entry [in = bias slot][out = 15] is set to a value whose activation is
// exactly 1 -- 256 for the prescaled tanh layers (exp2(256) = inf, so 1 - 2 / (inf + 1)
// = 1), 1.0 for layer 2.  Fragments only: the parameter image keeps 0 there, and its
// gradient is 0 (dz at an output of exactly 1 is (1 - 1*1) * ... = 0 for tanh; layer 2's
// backward never reads its bias row).  Needs n1, n2, n3 <= 15 (as FOLD does).
template <bool FOLD, bool PRE = false, bool INJ = false>
__device__ __forceinline__ void load_frags(const AEArgs& a, int c, int g, Frags& F, bool bwd) {
  const float* P = a.params;
  const float k1 = PRE ? kTanhExp2 : 1.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * g + j;
    // forward: A[m = out = c][k = in]
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int in = 16 * s + k;
      const bool row_ok = in < a.D || (FOLD && in == 31);
      F.w1t[s][j] = bfbits(k1 * ldsel(P, row_ok && c < a.n1, OFF1 + in * 16 + c));
    }
    const bool k15 = FOLD && k == 15;
    F.w2t[j] = bfbits(ldsel(P, (k < a.n1 || k15) && c < a.n2, OFF2 + k * 16 + c));
    F.w3t[j] = bfbits(k1 * ldsel(P, (k < a.n2 || k15) && c < a.n3, OFF3 + k * 16 + c));
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int out = 16 * t + c;
      F.w4t[t][j] = bfbits(ldsel(P, (k < a.n3 || k15) && out < a.D, OFF4 + k * 32 + out));
    }
    if (bwd) {
      // backward: A[m = in = c][k = out]; bias rows never propagate gradients
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int out = 16 * s + k;
        // the MSE gradient's 2/D rides in the backward W4 operand (dz4 is left unscaled;
        // the W4 weight-gradient slab is scaled once at the end of the launch)
        F.w4[s][j] = bfbits((2.0f / (float)a.D) * ldsel(P, c < a.n3 && out < a.D, OFF4 + c * 32 + out));
      }
      F.w3[j] = bfbits(ldsel(P, c < a.n2 && k < a.n3, OFF3 + c * 16 + k));
      F.w2[j] = bfbits(ldsel(P, c < a.n1 && k < a.n2, OFF2 + c * 16 + k));
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = 4 * g + i;
    F.b1[i] = ldsel(P, !FOLD && f < a.n1, OFF1 + 31 * 16 + f);
    F.b2[i] = ldsel(P, !FOLD && f < a.n2, OFF2 + 15 * 16 + f);
    F.b3[i] = ldsel(P, !FOLD && f < a.n3, OFF3 + 15 * 16 + f);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ft = 16 * t + f;
      F.b4[t][i] = ldsel(P, !FOLD && ft < a.D, OFF4 + 15 * 32 + ft);
    }
  }
  if constexpr (INJ) {
    if (c == 15 && g == 3) {   // A[m = out 15][k = in 4g + 3 = bias slot]
      F.w1t[1][3] = bfbits(256.0f);
      F.w2t[3] = bfbits(1.0f);
      F.w3t[3] = bfbits(256.0f);
    }
  }
}

// fused normalize_fn (cardata-v3.py:78-168) as a per-feature affine: feature f of the
// raw row -> x * scale[f] + shift[f]; features >= D get scale 0 (and so read as 0)
__device__ __forceinline__ float norm_scale(const AEArgs& a, int f) {
  if (f >= a.D) return 0.f;
  return a.scale ? a.scale[f] : 1.0f;
}
__device__ __forceinline__ float norm_shift(const AEArgs& a, int f) {
  return (f < a.D && a.scale) ? a.shift[f] : 0.f;
}

// register copy of the normaliser in the B layout (lane (c, g): features 16s + 4g + j)
__device__ __forceinline__ void norm_regs(const AEArgs& a, int g, f32x4 sc[2], f32x4 sh[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sc[s][j] = norm_scale(a, 16 * s + 4 * g + j);
      sh[s][j] = norm_shift(a, 16 * s + 4 * g + j);
    }
}

// The train kernel keeps the normaliser in LDS (NORM_BYTES: scale[32] then shift[32])
// and re-reads it per tile with four 16-byte ds_reads instead of pinning 16 VGPRs.
constexpr int NORM_BYTES = 256;
__device__ __forceinline__ void norm_lds(const char* norm, int g, f32x4 sc[2], f32x4 sh[2]) {
  typedef __attribute__((address_space(3))) const f32x4 lds_f4;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    sc[s] = *(lds_f4*)(norm + (16 * s + 4 * g) * 4);
    sh[s] = *(lds_f4*)(norm + 128 + (16 * s + 4 * g) * 4);
  }
}

// Raw tile fetch in the B-operand layout: lane (c, g) holds features 16s + 4g + j
// of row r.  Branch-free: column indices are clamped into the row and the
// out-of-range features are zeroed by the caller's loop-invariant mask (the
// normaliser's scale/shift are 0 there), so no load sits behind a divergent
// branch.  Rows r >= n are clamped to row n-1 (only the ragged tail has them).
// VEC: 8-byte loads of feature pairs (row stride and D even, 8-byte aligned base).
template <bool VEC>
__device__ __forceinline__ void fetch_x(const AEArgs& a, int64_t r, int g, f32x4 xr[2]) {
  const int64_t rr = r < a.n ? r : a.n - 1;
  const float* row = a.x + rr * a.ld;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if constexpr (VEC) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int f = min(16 * s + 4 * g + 2 * p, a.D - 2);
        const float2 v = *reinterpret_cast<const float2*>(row + f);
        xr[s][2 * p] = v.x;
        xr[s][2 * p + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) xr[s][j] = row[min(16 * s + 4 * g + j, a.D - 1)];
    }
  }
}

// Asynchronous global -> LDS copy of 16 B per lane (LDS destination = M0 + 16*lane).
// Issued from inline asm on purpose: the compiler cannot tell that the ring a wave
// reads is disjoint from the DMA target, and would drain the whole pipeline with a
// vmcnt(0) in front of every LDS read in the loop (the transposes included).  The
// ring's ordering is explicit instead: a counted `s_waitcnt vmcnt(N)` per tile.
// m0 is otherwise unused by this kernel (gfx9+ LDS instructions do not read it).
// Address = wave-uniform base (SGPR pair) + per-lane 32-bit offset; LDS destination =
// M0 + 16*lane.  Both uniform operands must already be wave-uniform values.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is deliberately clobbered (see above)
__device__ __forceinline__ void glds16(const void* gbase, unsigned voff, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_addr), "v"(voff), "s"(gbase)
               : "memory", "m0");
}
#pragma clang diagnostic pop

// One tile from a wave's LDS ring slot in the B-operand layout (cf. fetch_x):
// lane (c, g) reads features 16s + 4g + 2p.. of row c with 8-byte ds_reads;
// columns past D are clamped into the row (their scale is 0).
__device__ __forceinline__ void ring_x(const AEArgs& a, const char* slot, int c, int g, f32x4 xr[2]) {
  typedef __attribute__((address_space(3))) const f32x2_t lds_f2;
  const char* row = slot + c * 4 * a.D;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int f = min(16 * s + 4 * g + 2 * p, a.D - 2);
      const f32x2_t v = *(lds_f2*)(row + 4 * f);
      xr[s][2 * p] = v[0];
      xr[s][2 * p + 1] = v[1];
    }
}

// activation + padding: real features f < n get act(z); the bias slot (15) gets 1.
__device__ __forceinline__ f32x4 activate_pad(int act, f32x4 z, int n, int g) {
  f32x4 h;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = 4 * g + i;
    h[i] = f < n ? act_fwd(act, z[i]) : (f == 15 ? 1.0f : 0.0f);
  }
  return h;
}

template <int PACK>
__device__ __forceinline__ void forward_tile(const AEArgs& a, const Frags& F, int g, const f32x4 xf[2],
                                             bf16x4& xb0, bf16x4& xb1, f32x4& h1, f32x4& h2, f32x4& h3,
                                             bf16x4& h1b, bf16x4& h2b, bf16x4& h3b, f32x4 y[2]) {
  f32x4 x1 = xf[1];
  if (g == 3) x1[3] = 1.0f;  // feature 31 = constant-1 bias slot of layer 1
  xb0 = pack4(xf[0]);
  xb1 = pack4(x1);
  f32x4 z1 = mfma16(F.w1t[0], xb0, F.b1);
  z1 = mfma16(F.w1t[1], xb1, z1);
  h1 = activate_pad(act_of<PACK>(a, 0), z1, a.n1, g);
  h1b = pack4(h1);
  f32x4 z2 = mfma16(F.w2t, h1b, F.b2);
  h2 = activate_pad(act_of<PACK>(a, 1), z2, a.n2, g);
  h2b = pack4(h2);
  f32x4 z3 = mfma16(F.w3t, h2b, F.b3);
  h3 = activate_pad(act_of<PACK>(a, 2), z3, a.n3, g);
  h3b = pack4(h3);
  const int a4 = act_of<PACK>(a, 3);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    f32x4 z4 = mfma16(F.w4t[t], h3b, F.b4[t]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = 16 * t + 4 * g + i;
      y[t][i] = f < a.D ? act_fwd(a4, z4[i]) : 0.f;
    }
  }
}

__device__ __forceinline__ void argmax_combine(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// Branch-free argmax over the 8 features a lane holds + its 3 partner lanes
// (row r = lane & 15 is spread over lane groups g = 0..3).  Ties -> lowest index
// (tf.argmax).  Features >= D are masked to -inf (lane-uniform compares, hoisted).
// max of three floats in one v_max3_f32.  Inline asm on purpose: fmaxf() makes the
// compiler canonicalise operands it cannot prove canonical (the MFMA/med3 outputs)
// with an extra v_max each; the data here is finite, so plain IEEE max3 is exact.
__device__ __forceinline__ float max3f(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Branch-free argmax over the 8 features a lane holds + its 3 partner lanes
// (row r = lane & 15 is spread over lane groups g = 0..3).  Ties -> lowest index
// (tf.argmax).  Features >= D are masked to -inf; LOW_REAL (D >= 16, all ring
// variants) skips the mask on the first 16 features, which are then always real.
// Feature 16 + 4g + i of the upper half is real for some lane iff 16 + i < D; with a
// compile-time D (DC > 0) the halves i >= DC - 16 are dropped from every loop.
template <int DC>
__device__ __forceinline__ constexpr bool live_hi(int i) { return DC == 0 || 16 + i < DC; }

// Reductions over the 4 lanes of a row (l, l^16, l^32, l^48) with the gfx950 row
// swaps: permlane16_swap(a, b) of two copies leaves {rows 0,0,2,2} in one result and
// {rows 1,1,3,3} in the other, so their max is the xor-16 butterfly with no select;
// permlane32_swap does the same across halves.
__device__ __forceinline__ float bfly_max(float m) {
  const unsigned u = __float_as_uint(m);
  const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  m = max3f(__uint_as_float(r16[0]), __uint_as_float(r16[1]), __uint_as_float(r16[1]));   // no canonicalising v_max
  const unsigned v = __float_as_uint(m);
  const auto r32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return max3f(__uint_as_float(r32[0]), __uint_as_float(r32[1]), __uint_as_float(r32[1]));
}
__device__ __forceinline__ int bfly_min(int x) {
  const auto r16 = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
  x = min((int)r16[0], (int)r16[1]);
  const auto r32 = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
  return min((int)r32[0], (int)r32[1]);
}

template <bool LOW_REAL, int DC = 0>
__device__ __forceinline__ int row_argmax_fast(const f32x4 v[2], int D, int g) {
  float vv[8];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      vv[4 * t + i] = (t == 1 && !live_hi<DC>(i))                          ? -INFINITY
                      : ((t == 0 && LOW_REAL) || (16 * t + 4 * g + i) < D) ? v[t][i]
                                                                            : -INFINITY;
  float m = max3f(max3f(vv[0], vv[1], vv[2]), vv[3], live_hi<DC>(0) ? vv[4] : vv[3]);
  if (live_hi<DC>(1) || live_hi<DC>(2)) m = max3f(m, live_hi<DC>(1) ? vv[5] : m, live_hi<DC>(2) ? vv[6] : m);
  if (live_hi<DC>(3)) m = max3f(m, vv[7], m);
  m = bfly_max(m);
  int idx = 64;
#pragma unroll
  for (int q = 7; q >= 0; --q) {
    if (q >= 4 && !live_hi<DC>(q - 4)) continue;
    const int f = 16 * (q >> 2) + 4 * g + (q & 3);
    idx = (vv[q] == m) ? f : idx;
  }
  return bfly_min(idx);
}

// Argmax of a row of NON-NEGATIVE values (a relu output) as one integer max: each live
// feature f becomes the key (bits(v) & 0x7fffffc0) | (63 - f) -- a non-negative float's
// bits order like the float (the sign bit is cleared, so a -0 from med3 counts as 0),
// and the low 6 bits break ties toward the lowest index (tf.argmax).  Only compile-time
// padding is masked (key 0): the callers' padded features f >= D hold exactly 0 (zero
// weights, relu(0)), so their keys 63 - f lose to every real feature's -- a real 0 has the
// lower index, anything larger has value bits >= 0x40 -- and need no per-lane mask (a
// lane-dependent select around the asm key became four divergent branches).  Exact except when the two largest values agree in
// all but the last 6 of 23 mantissa bits (relative gap < 2^-17, far below the bf16
// noise of the values), where the lower index wins.  ~16 VALU instead of ~35.
__device__ __forceinline__ unsigned umax3(unsigned a, unsigned b, unsigned c) {
  unsigned r;
  asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// (bits & 0x7fffffc0) | lo in ONE v_bfi_b32 (hipcc otherwise emits an and + sub pair)
__device__ __forceinline__ unsigned bfi_key(unsigned bits, unsigned lo) {
  unsigned r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(0x7fffffc0u), "v"(bits), "v"(lo));   // mask from an SGPR
  return r;
}
template <int DC>
__device__ __forceinline__ unsigned nonneg_key_max(const f32x4 v[2], int D, int g) {   // the lane's 8 features
  unsigned k[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int t = q >> 2, i = q & 3;
    const int f = 16 * t + 4 * g + i;
    const bool live = t == 0 || live_hi<DC>(i);
    (void)D;
    k[q] = live ? bfi_key(__float_as_uint(v[t][i]), (unsigned)(63 - f)) : 0u;
  }
  unsigned m = umax3(umax3(k[0], k[1], k[2]), k[3], live_hi<DC>(0) ? k[4] : k[3]);
  if (live_hi<DC>(1) || live_hi<DC>(2)) m = umax3(m, live_hi<DC>(1) ? k[5] : m, live_hi<DC>(2) ? k[6] : m);
  if (live_hi<DC>(3)) m = umax3(m, k[7], m);
  return m;
}
template <int DC>
__device__ __forceinline__ int row_argmax_nonneg(const f32x4 v[2], int D, int g) {
  unsigned m = nonneg_key_max<DC>(v, D, g);
  const auto r16 = __builtin_amdgcn_permlane16_swap(m, m, false, false);
  m = umax3(r16[0], r16[1], r16[1]);
  const auto r32 = __builtin_amdgcn_permlane32_swap(m, m, false, false);
  m = umax3(r32[0], r32[1], r32[1]);
  return 63 - (int)(m & 63u);
}
// Two tiles' row argmaxes with ONE butterfly: permlane16_swap(m0, m1) moves tile 1's even
// rows next to tile 0's odd rows, so after its max rows 0 / 2 hold tile 0's pairwise maxima
// and rows 1 / 3 tile 1's; the permlane32 step then completes both.  Lane group g gets the
// argmax of row c of tile (g & 1).
template <int DC>
__device__ __forceinline__ int row_argmax_nonneg_pair(const f32x4 v0[2], const f32x4 v1[2], int D, int g) {
  const unsigned m0 = nonneg_key_max<DC>(v0, D, g), m1 = nonneg_key_max<DC>(v1, D, g);
  const auto r16 = __builtin_amdgcn_permlane16_swap(m0, m1, false, false);
  unsigned m = r16[0] > r16[1] ? r16[0] : r16[1];
  const auto r32 = __builtin_amdgcn_permlane32_swap(m, m, false, false);
  m = umax3(r32[0], r32[1], r32[1]);
  return 63 - (int)(m & 63u);
}
// The same for the packed-pair output layout: outputs 0..15 of tile u in lo[u] (lane (c, g)
// features 4g..4g+3 of row c), outputs 16 / 17 of both tiles in ONE register `up` (lane group
// g holds output 16 + (g & 1) of tile g >> 1).  D = 18.
__device__ __forceinline__ int row_argmax_up_pair(const f32x4 lo0, const f32x4 lo1, float up, int g) {
  unsigned k0[4], k1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    k0[i] = bfi_key(__float_as_uint(lo0[i]), (unsigned)(63 - 4 * g - i));
    k1[i] = bfi_key(__float_as_uint(lo1[i]), (unsigned)(63 - 4 * g - i));
  }
  const unsigned ku = bfi_key(__float_as_uint(up), (unsigned)(63 - 16 - (g & 1)));
  const unsigned own0 = g < 2 ? ~0u : 0u;   // which tile's row this lane's `up` belongs to
  const unsigned m0 = umax3(umax3(k0[0], k0[1], k0[2]), k0[3], ku & own0);
  const unsigned m1 = umax3(umax3(k1[0], k1[1], k1[2]), k1[3], ku & ~own0);
  const auto r16 = __builtin_amdgcn_permlane16_swap(m0, m1, false, false);
  unsigned m = r16[0] > r16[1] ? r16[0] : r16[1];
  const auto r32 = __builtin_amdgcn_permlane32_swap(m, m, false, false);
  m = umax3(r32[0], r32[1], r32[1]);
  return 63 - (int)(m & 63u);
}

// The same argmax for values of ANY sign (normalised inputs, argmax(x) of the accuracy
// metric): the float bits become a signed-int-ordered key (a negative value's magnitude bits
// flipped: v_ashrrev + v_xor + v_bfi), then (key & ~63) | (63 - f) as above -- ties and gaps
// below 2^-17 relative go to the lowest index.  Four VALU per feature, one butterfly per pair.
__device__ __forceinline__ int imax3(int a, int b, int c) {
  int r;
  asm("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ int signed_key(float v, unsigned lo) {
  const unsigned u = __float_as_uint(v);
  const unsigned sx = u ^ (unsigned)((int)u >> 31);   // every bit flipped when negative
  unsigned t, k;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(t) : "s"(0x7fffffffu), "v"(sx), "v"(u));   // keep the sign bit
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(k) : "s"(0xffffffc0u), "v"(t), "v"(lo));
  return (int)k;
}
__device__ __forceinline__ int row_argmax_up_pair_signed(const f32x4 lo0, const f32x4 lo1, float up, int g) {
  int k0[4], k1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    k0[i] = signed_key(lo0[i], (unsigned)(63 - 4 * g - i));
    k1[i] = signed_key(lo1[i], (unsigned)(63 - 4 * g - i));
  }
  const int ku = signed_key(up, (unsigned)(63 - 16 - (g & 1)));
  const bool own0 = g < 2;   // which tile's row this lane's `up` belongs to
  const int m0 = imax3(imax3(k0[0], k0[1], k0[2]), k0[3], own0 ? ku : (-2147483647 - 1));
  const int m1 = imax3(imax3(k1[0], k1[1], k1[2]), k1[3], own0 ? (-2147483647 - 1) : ku);
  const auto r16 = __builtin_amdgcn_permlane16_swap((unsigned)m0, (unsigned)m1, false, false);
  int m = max((int)r16[0], (int)r16[1]);
  const auto r32 = __builtin_amdgcn_permlane32_swap((unsigned)m, (unsigned)m, false, false);
  m = imax3((int)r32[0], (int)r32[1], (int)r32[1]);
  return 63 - (m & 63);
}

// One 16-row tile: forward, loss, metrics, backward, weight-gradient MFMAs.
// FAST (zero-preserving activations): no per-feature masks -- padded features
// stay exactly 0 because their weights are 0 and act(0) = 0; only the bias slot
// is set.  TAIL: rows beyond n are masked (only the last tile of a launch).
// tanh of an argument already multiplied by 2*log2(e) (see load_frags<., true>)
__device__ __forceinline__ float tanh_exp2(float z2) {
  return fmaf(-2.0f, rcp_fast(__builtin_amdgcn_exp2f(z2) + 1.0f), 1.0f);
}

template <int PACK>
constexpr bool prescaled_tanh() {
  return PACK >= 0 && ((PACK & 3) == ACT_TANH) && (((PACK >> 4) & 3) == ACT_TANH) && zero_preserving<PACK>();
}

// bias slots made by the forward MFMAs (load_frags<., ., true>)
template <int PACK>
constexpr bool inject_bias_slots() {
  return prescaled_tanh<PACK>() && (((PACK >> 2) & 3) == ACT_RELU || ((PACK >> 2) & 3) == ACT_LINEAR);
}

template <int PACK, bool FAST, bool TAIL, bool LOW_REAL = false, int DC = 0, bool XA = false>
__device__ __forceinline__ void train_tile(const AEArgs& a, const Frags& F, char* scr, int c, int g, int lane,
                                           bool valid, const f32x4 xf[2], float pad1,
                                           f32x4 acc1[2], f32x4& acc2, f32x4& acc3, f32x4 acc4[2], float& sq,
                                           float& ab, float& corr, float& rows, int ix_pre = -1) {
  const int a1 = act_of<PACK>(a, 0), a2 = act_of<PACK>(a, 1), a3 = act_of<PACK>(a, 2), a4 = act_of<PACK>(a, 3);
  constexpr bool PRE = FAST && prescaled_tanh<PACK>();
  constexpr bool INJ = FAST && inject_bias_slots<PACK>();
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bool pad_lane = (g == 3);
  const bool vm = !TAIL || valid;

  bf16x4 xb0, xb1, h1b, h2b, h3b;
  f32x4 h1, h2, h3, y[2];
  if constexpr (FAST) {
    // padded features are exactly 0 (zero weights, act(0) = 0); feature 15 of
    // each hidden layer / 31 of the input is the constant-1 bias slot: +pad1.
    f32x4 x1 = xf[1];
    x1[3] += pad1;
    xb0 = pack4(xf[0]);
    xb1 = pack4(x1);
    // the 32 input features (18 real + bias slot) in ONE 16x16x32 MFMA
    const f32x4 z1 = mfma32(F.w1t[0], F.w1t[1], xb0, xb1, zero4);
#pragma unroll
    for (int i = 0; i < 4; ++i) h1[i] = PRE ? tanh_exp2(z1[i]) : act_fwd(a1, z1[i]);
    if constexpr (!INJ) h1[3] += pad1;
    h1b = pack4(h1);
    const f32x4 z2 = mfma16(F.w2t, h1b, zero4);
#pragma unroll
    for (int i = 0; i < 4; ++i) h2[i] = act_fwd(a2, z2[i]);
    if constexpr (!INJ) h2[3] += pad1;
    h2b = pack4(h2);
    const f32x4 z3 = mfma16(F.w3t, h2b, zero4);
#pragma unroll
    for (int i = 0; i < 4; ++i) h3[i] = PRE ? tanh_exp2(z3[i]) : act_fwd(a3, z3[i]);
    if constexpr (!INJ) h3[3] += pad1;
    h3b = pack4(h3);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const f32x4 z4 = mfma16(F.w4t[t], h3b, zero4);
#pragma unroll
      for (int i = 0; i < 4; ++i) y[t][i] = (t == 0 || live_hi<DC>(i)) ? act_fwd(a4, z4[i]) : 0.f;
    }
  } else {
    forward_tile<PACK>(a, F, g, xf, xb0, xb1, h1, h2, h3, h1b, h2b, h3b, y);
  }

  // MSE loss + dL/dz4 (sum-scaled; the 1/B factor is applied in the Adam kernel)
  f32x4 dz4[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (t == 1 && !live_hi<DC>(i)) {  // compile-time padding (no real feature on any lane)
        dz4[t][i] = 0.f;
        continue;
      }
      float e = y[t][i] - xf[t][i];
      if constexpr (!FAST) e = (16 * t + 4 * g + i) < a.D ? e : 0.f;
      if constexpr (TAIL) e = vm ? e : 0.f;
      sq = fmaf(e, e, sq);
      dz4[t][i] = act_grad(a4, y[t][i], e);   // x 2/D folded into F.w4 / the acc4 slab
    }
  if (a.want_acc) {
    // relu output layer (the reference model): integer-key argmax of the non-negative y
    int iy;
    if constexpr (PACK >= 0 && ((PACK >> 6) & 3) == ACT_RELU && LOW_REAL)
      iy = row_argmax_nonneg<DC>(y, a.D, g);
    else
      iy = row_argmax_fast<LOW_REAL, DC>(y, a.D, g);
    const int ix = XA ? ix_pre : row_argmax_fast<LOW_REAL, DC>(xf, a.D, g);
    corr += (g == 0 && vm && iy == ix) ? 1.f : 0.f;
  }
  rows += (g == 0 && vm) ? 1.f : 0.f;

  // backward through the layers (feature-major, in registers)
  const bf16x4 dz4b0 = pack4(dz4[0]), dz4b1 = pack4(dz4[1]);
  const f32x4 dh3 = mfma32(F.w4[0], F.w4[1], dz4b0, dz4b1, zero4);   // K = 32 outputs in one MFMA
  f32x4 dz3, dz2, dz1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dz3[i] = act_grad(a3, h3[i], dh3[i]);
    if constexpr (!FAST) dz3[i] = (4 * g + i) < a.n3 ? dz3[i] : 0.f;
  }
  const bf16x4 dz3b = pack4(dz3);
  const f32x4 dh2 = mfma16(F.w3, dz3b, zero4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dz2[i] = act_grad(a2, h2[i], dh2[i]);
    if constexpr (!FAST) dz2[i] = (4 * g + i) < a.n2 ? dz2[i] : 0.f;
  }
  const bf16x4 dz2b = pack4(dz2);
  const f32x4 dh1 = mfma16(F.w2, dz2b, zero4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float hv = h1[i];
    const bool real = FAST ? !(i == 3 && pad_lane) : ((4 * g + i) < a.n1);
    const bool use = real && vm;
    ab += use ? fabsf(hv) : 0.f;
    // Keras L1 activity regulariser gradient: l1 * sign(h1) (sign(0) = 0)
    float d;
    if constexpr (PRE && !TAIL) {
      // one v_med3: clamp(h, -l1, l1) = l1 * sign(h) for |h| >= l1 (and 0 at h = 0); it
      // differs only for 0 < |h1| < l1 = 1e-7, by less than l1.  The bias slot (h = 1)
      // needs no mask: the tanh derivative 1 - h*h is exactly 0 there.
      d = act_grad(a1, hv, dh1[i] + __builtin_amdgcn_fmed3f(hv, -a.l1, a.l1));
    } else {
      const float sgn = (use && hv != 0.f) ? __builtin_copysignf(1.0f, hv) : 0.f;
      d = act_grad(a1, hv, fmaf(a.l1, sgn, dh1[i]));
    }
    if constexpr (!FAST) d = real ? d : 0.f;
    dz1[i] = d;
  }
  const bf16x4 dz1b = pack4(dz1);

  // weight gradients: contraction over the 16 rows of the tile (operands
  // re-laid out rows-on-K through LDS transposed reads; 512 B per slot)
  const bf16x4 xr0 = lds_transpose(xb0, scr + 0 * 512, c, g);
  const bf16x4 xr1 = lds_transpose(xb1, scr + 1 * 512, c, g);
  const bf16x4 dz1r = lds_transpose(dz1b, scr + 2 * 512, c, g);
  const bf16x4 h1r = lds_transpose(h1b, scr + 3 * 512, c, g);
  const bf16x4 dz2r = lds_transpose(dz2b, scr + 4 * 512, c, g);
  const bf16x4 h2r = lds_transpose(h2b, scr + 5 * 512, c, g);
  const bf16x4 dz3r = lds_transpose(dz3b, scr + 6 * 512, c, g);
  const bf16x4 h3r = lds_transpose(h3b, scr + 7 * 512, c, g);
  const bf16x4 dz4r0 = lds_transpose(dz4b0, scr + 8 * 512, c, g);
  const bf16x4 dz4r1 = lds_transpose(dz4b1, scr + 9 * 512, c, g);
  acc1[0] = mfma16(xr0, dz1r, acc1[0]);
  acc1[1] = mfma16(xr1, dz1r, acc1[1]);
  acc2 = mfma16(h1r, dz2r, acc2);
  acc3 = mfma16(h2r, dz3r, acc3);
  acc4[0] = mfma16(h3r, dz4r0, acc4[0]);
  acc4[1] = mfma16(h3r, dz4r1, acc4[1]);
}

// U (1 or 2) whole tiles of one wave in ONE interleaved instruction stream (ILP variant of
// train_tile for the headline configuration: zero-preserving, prescaled tanh, bias slots
// from the MFMAs, ingest-time argmax of x, compile-time D).  Every stage is written as a
// loop over the U tiles, so the two tiles' dependent MFMA -> activation -> MFMA chains
// are independent instruction sequences the scheduler can pair: while one tile waits on
// an MFMA result the other's VALU issues (profiles/r02: 43 % of wave cycles were issue
// stalls on the one-tile chain at 4 waves / SIMD).  The weight-gradient contraction of
// the pair is one v_mfma_f32_16x16x32_bf16 per weight block (K = 2 x 16 rows) instead of
// two 16x16x16s.  U = 1 pads the second K half with zeros, so every accumulator is only
// ever fed by 16x16x32 MFMAs (a 16x16x16 taking a 16x16x32 result as SrcC miscomputed on
// this toolchain, see the LSTM notes in profiles/r02).  The tiles share the wave's
// transpose scratch: LDS ops of one wave execute in order, so tile 1's write of a slot
// cannot overtake tile 0's transposed read of it.
template <int PACK, int DC, int U>
__device__ __forceinline__ void train_tiles_ilp(const AEArgs& a, const Frags& F, char* scr, int c, int g,
                                                const f32x4 (&xf)[U][2], const int (&ix)[U], float pad1,
                                                f32x4 acc1[2], f32x4& acc2, f32x4& acc3, f32x4 acc4[2], float& sq,
                                                float& ab, float& corr, float& rows) {
  static_assert(zero_preserving<PACK>() && inject_bias_slots<PACK>() && DC > 16, "headline configuration only");
  static_assert(U == 1 || U == 2, "one or two tiles");
  const int a2 = act_of<PACK>(a, 1), a3 = act_of<PACK>(a, 2), a4 = act_of<PACK>(a, 3);
  const int a1 = act_of<PACK>(a, 0);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bf16x4 zb = {0, 0, 0, 0};
  const bool pad_lane = (g == 3);

  bf16x4 xb0[U], xb1[U], h1b[U], h2b[U], h3b[U];
  f32x4 h1[U], h2[U], h3[U], y[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    f32x4 x1 = xf[u][1];
    x1[3] += pad1;
    xb0[u] = pack4(xf[u][0]);
    xb1[u] = pack4(x1);
  }
  f32x4 z[U];
#pragma unroll
  for (int u = 0; u < U; ++u) z[u] = mfma32(F.w1t[0], F.w1t[1], xb0[u], xb1[u], zero4);
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) h1[u][i] = tanh_exp2(z[u][i]);
    h1b[u] = pack4(h1[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) z[u] = mfma16(F.w2t, h1b[u], zero4);
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) h2[u][i] = act_fwd(a2, z[u][i]);
    h2b[u] = pack4(h2[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) z[u] = mfma16(F.w3t, h2b[u], zero4);
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) h3[u][i] = tanh_exp2(z[u][i]);
    h3b[u] = pack4(h3[u]);
  }
  f32x4 z4[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < 2; ++t) z4[u][t] = mfma16(F.w4t[t], h3b[u], zero4);
  f32x4 dz4[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (t == 1 && !live_hi<DC>(i)) {
          y[u][t][i] = 0.f;
          dz4[u][t][i] = 0.f;
          continue;
        }
        y[u][t][i] = act_fwd(a4, z4[u][t][i]);
        const float e = y[u][t][i] - xf[u][t][i];
        sq = fmaf(e, e, sq);
        dz4[u][t][i] = act_grad(a4, y[u][t][i], e);   // x 2/D folded into F.w4 / the acc4 slab
      }
  if (a.want_acc) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int iy;
      if constexpr (((PACK >> 6) & 3) == ACT_RELU)
        iy = row_argmax_nonneg<DC>(y[u], a.D, g);
      else
        iy = row_argmax_fast<true, DC>(y[u], a.D, g);
      corr += (g == 0 && iy == ix[u]) ? 1.f : 0.f;
    }
  }
  rows += (g == 0) ? (float)U : 0.f;

  bf16x4 dz4b0[U], dz4b1[U], dz3b[U], dz2b[U], dz1b[U];
  f32x4 d[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    dz4b0[u] = pack4(dz4[u][0]);
    dz4b1[u] = pack4(dz4[u][1]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) d[u] = mfma32(F.w4[0], F.w4[1], dz4b0[u], dz4b1[u], zero4);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    f32x4 dz3;
#pragma unroll
    for (int i = 0; i < 4; ++i) dz3[i] = act_grad(a3, h3[u][i], d[u][i]);
    dz3b[u] = pack4(dz3);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) d[u] = mfma16(F.w3, dz3b[u], zero4);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    f32x4 dz2;
#pragma unroll
    for (int i = 0; i < 4; ++i) dz2[i] = act_grad(a2, h2[u][i], d[u][i]);
    dz2b[u] = pack4(dz2);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) d[u] = mfma16(F.w2, dz2b[u], zero4);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    f32x4 dz1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float hv = h1[u][i];
      ab += (i == 3 && pad_lane) ? 0.f : fabsf(hv);
      // Keras L1 activity regulariser gradient as one v_med3 (see train_tile)
      dz1[i] = act_grad(a1, hv, d[u][i] + __builtin_amdgcn_fmed3f(hv, -a.l1, a.l1));
    }
    dz1b[u] = pack4(dz1);
  }

  // weight gradients: rows-on-K operands through the LDS transpose, both tiles per MFMA
  bf16x4 xr0[2], xr1[2], dz1r[2], h1r[2], dz2r[2], h2r[2], dz3r[2], h3r[2], dz4r0[2], dz4r1[2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    xr0[u] = lds_transpose(xb0[u], scr + 0 * 512, c, g);
    xr1[u] = lds_transpose(xb1[u], scr + 1 * 512, c, g);
    dz1r[u] = lds_transpose(dz1b[u], scr + 2 * 512, c, g);
    h1r[u] = lds_transpose(h1b[u], scr + 3 * 512, c, g);
    dz2r[u] = lds_transpose(dz2b[u], scr + 4 * 512, c, g);
    h2r[u] = lds_transpose(h2b[u], scr + 5 * 512, c, g);
    dz3r[u] = lds_transpose(dz3b[u], scr + 6 * 512, c, g);
    h3r[u] = lds_transpose(h3b[u], scr + 7 * 512, c, g);
    dz4r0[u] = lds_transpose(dz4b0[u], scr + 8 * 512, c, g);
    dz4r1[u] = lds_transpose(dz4b1[u], scr + 9 * 512, c, g);
  }
  if constexpr (U == 1) {
    xr0[1] = xr1[1] = dz1r[1] = h1r[1] = dz2r[1] = h2r[1] = dz3r[1] = h3r[1] = dz4r0[1] = dz4r1[1] = zb;
  }
  acc1[0] = mfma32(xr0[0], xr0[1], dz1r[0], dz1r[1], acc1[0]);
  acc1[1] = mfma32(xr1[0], xr1[1], dz1r[0], dz1r[1], acc1[1]);
  acc2 = mfma32(h1r[0], h1r[1], dz2r[0], dz2r[1], acc2);
  acc3 = mfma32(h2r[0], h2r[1], dz3r[0], dz3r[1], acc3);
  acc4[0] = mfma32(h3r[0], h3r[1], dz4r0[0], dz4r0[1], acc4[0]);
  acc4[1] = mfma32(h3r[0], h3r[1], dz4r1[0], dz4r1[1], acc4[1]);
}

// ---------------------------------------------------------------------------------------
// Packed tile pairs (ILP 3).  Layers 2 and 3 of the reference model are 7 wide (+ the bias
// slot = 8), so in the 16-feature fragment of one tile half the lanes' elementwise work is
// padding.  Two tiles share ONE fragment there: packed feature p < 8 is feature p of tile 0,
// p >= 8 feature p - 8 of tile 1 (packed 7 / 15 = the tiles' constant-1 bias slots, image
// row 15).  The weights become block-diagonal (or one block beside zeros) so every layer
// is still one MFMA; the relu / tanh / derivative work of layers 2-3 and four of the ten
// LDS transposes are done once per PAIR.  Layer 1 and the output layer stay per tile.
//   forward  L2: z2p = [W2^T 0; 0 W2^T] . [h1_0; h1_1]          (one 16x16x32)
//            L3: z3p = blockdiag(W3^T, W3^T) . h2p              (one 16x16x16)
//            L4: z4_u = [W4^T 0] / [0 W4^T] . h3p              (per tile, per 16-output half)
//   backward dh3p = [W4 0; 0 W4] . [dz4_0; dz4_1]              (two chained 16x16x32)
//            dh2p = blockdiag(W3, W3) . dz3p;  dh1_u = [W2 0] / [0 W2] . dz2p
//   weight gradients: dW2 / dW4 contract one tile against a lane-masked copy of the packed
//   operand (the other tile's half zeroed); dW3 is the diagonal blocks of ONE contraction.
//   The accumulators hold both tiles' halves side by side and are folded into the parameter
//   image once per launch (packed_fold_src).  Needs n2, n3 <= 7.
//
// Compact ring (CM, pack_tiles_argmax with a live mask and lane_order): the reference's
// normalize_fn assigns the constant 0 to features 0, 2, 4 and 5 (cardata NORMALIZE_RANGES None),
// so the packed ring stores only the 14 live ones, in LANE order (compact float k: feature 16, 1,
// 17, 3, 6, 7, ..., 15).  The loop keeps the 18-column operand layout -- lane (c, g) holds inputs
// 4g..4g+3 of row c, inputs 16 / 17 come as UP -- and reads them as four consecutive floats of
// the row from ONE lane offset (cm_off: byte 0, 8, 24, 40), every live input already in its slot:
//   g = 0: inputs (0, 1, 2, 3)   <- k0..k3 = (*16, 1, *17, 3)     g = 2: inputs 8..11  <- k6..k9
//   g = 1: inputs (4, 5, 6, 7)   <- k2..k5 = (*17, *3, 6, 7)      g = 3: inputs 12..15 <- k10..k13
// and UP from k0 / k2.  A dead slot `*` holds whatever float of the same row came along
// (always landed, always finite -- nothing outside the row is read): its layer-1
// weight row is zeroed in the fragment (the 18-column loop multiplies a zero input by the
// weight, this one a finite input by zero: both products are 0), its dW1 row is written as the
// exact 0 it is (packed_fold_src), and the loss selects 0 as its target.  Everything else is
// the same instruction on the same operands, so the results are the 18-column loop's.
__host__ __device__ constexpr bool cm_dead(int f) { return f == 0 || f == 2 || f == 4 || f == 5; }
// byte offset, from the row's first compact float, of the lane's four floats: {0, 8, 24, 40} for
// g = 0..3.  Branch-free on purpose: a nested ?: over g became exec-masked branches inside the loop.
__device__ __forceinline__ int cm_off(int g) { return max(16 * g - 8, 0); }
// the lane's inputs 4g..4g+3 of one compact row (dead slots: finite don't-cares): the four
// consecutive floats at `lane_row` = the row's first float + cm_off(g), no select
typedef __attribute__((address_space(3))) const char lds_cc;
__device__ __forceinline__ f32x4 ring_row4(lds_cc* lane_row) {   // one ds_read2_b64
  typedef __attribute__((address_space(3))) const f32x2_t lds_f2;
  const f32x2_t a = *(lds_f2*)lane_row, b = *(lds_f2*)(lane_row + 8);
  return f32x4{a[0], a[1], b[0], b[1]};
}
__device__ __forceinline__ f32x4 cm_row_x(const char* lane_row) { return ring_row4((lds_cc*)lane_row); }

template <int V>
struct RingSlot {   // a ring slot as a compile-time value (the unrolled pair loop)
  static constexpr int value = V;
};

struct FragsP {
  bf16x4 w1t;         // L1 forward from inputs 0..15 (prescaled)
  bf16x4 w1u[2];      // L1 forward [tile] from the UP inputs 16 / 17 and the constant-1 bias input
  bf16x4 w2t[2];      // L2 forward, K halves = tile 0 / tile 1 inputs
  bf16x4 w3t;         // L3 forward, block-diagonal (prescaled, packed bias slots injected)
  bf16x4 w4t[2];      // L4 forward, outputs 0..15 [tile]
  bf16x4 w4u;         // L4 forward, outputs 16, 17 of both tiles into one register (see UP below)
  bf16x4 w4b[2];      // L4 backward from outputs 0..15 [tile] (x 2/D)
  bf16x4 w4bu;        // L4 backward from the packed outputs 16, 17 (x 2/D)
  bf16x4 w3b;         // L3 backward, block-diagonal
  bf16x4 w2b[2];      // L2 backward [tile]
  // the 16x16x32 A operands, concatenated once per launch: tile 1's layer 1 takes its K halves
  // in the order [UP | inputs 0..15] so the shared UP B operand can sit between the tiles' own
  s16x8 w1a[2], w2a, w4ba, w4bua;
  // one layer-1 A operand for BOTH tiles: [inputs 0..15 | UP of both tiles + bias]; the tile is picked
  // by lane-masking the UP B operand instead (MA variants: 4 fewer persistent registers)
  s16x8 w1s;
};

__device__ __forceinline__ int img_row_of_packed(int i) { return i == 7 ? 15 : i; }   // i = packed % 8

template <bool CM = false>
__device__ __forceinline__ void load_frags_packed(const AEArgs& a, int c, int g, FragsP& F) {
  const float* P = a.params;
  const float k1 = kTanhExp2;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * g + j;
    // CM: the dead inputs' slots hold don't-care floats, so their weight rows are 0 here
    F.w1t[j] = bfbits(k1 * ldsel(P, k < a.D && c < a.n1 && !(CM && cm_dead(k)), OFF1 + k * 16 + c));
    // L1 from UP: B row k = 4q (j = 0) is input 16 + (q & 1) of tile q >> 1, k = 1 (g = 0, j = 1)
    // the constant 1 of the bias; bias slot 15's output is injected there (tanh_exp2(256) = 1)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int in = 16 + (g & 1);
      float v = 0.f;
      if (j == 0 && (g >> 1) == u) v = k1 * ldsel(P, in < a.D && c < a.n1, OFF1 + in * 16 + c);
      if (j == 1 && g == 0) v = c == 15 ? 256.0f : k1 * ldsel(P, c < a.n1, OFF1 + 31 * 16 + c);
      F.w1u[u][j] = bfbits(v);
    }
    // L2 forward: A[m = packed out c][k = in (of tile h)]
    const int o2 = c & 7;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool ok = (c >> 3) == h && o2 < a.n2 && (k < a.n1 || k == 15);
      float v = ldsel(P, ok, OFF2 + k * 16 + o2);
      if ((c >> 3) == h && o2 == 7 && k == 15) v = 1.0f;   // packed bias slot: relu(1) = 1
      F.w2t[h][j] = bfbits(v);
    }
    // L3 forward: A[m = packed out c][k = packed in k], same tile only
    {
      const int o = c & 7, i = k & 7;
      const bool same = (c >> 3) == (k >> 3);
      float v = k1 * ldsel(P, same && o < a.n3 && (i < a.n2 || i == 7), OFF3 + img_row_of_packed(i) * 16 + o);
      if (same && o == 7 && i == 7) v = 256.0f;   // tanh_exp2(256) = 1 exactly
      F.w3t[j] = bfbits(v);
    }
    // L4 forward, outputs 0..15: A[m = out c][k = packed in of tile u]
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = k & 7;
      const bool ok = (k >> 3) == u && c < a.D && (i < a.n3 || i == 7);
      F.w4t[u][j] = bfbits(ldsel(P, ok, OFF4 + img_row_of_packed(i) * 32 + c));
    }
    // L4 forward, outputs 16 / 17: A[m = 4q (UP slot q: tile q >> 1, output 16 + (q & 1))][k = packed in]
    {
      const int q = c >> 2, i = k & 7, out = 16 + (q & 1);
      const bool ok = (c & 3) == 0 && (k >> 3) == (q >> 1) && out < a.D && (i < a.n3 || i == 7);
      F.w4u[j] = bfbits(ldsel(P, ok, OFF4 + img_row_of_packed(i) * 32 + out));
    }
    // L4 backward from outputs 0..15: A[m = packed in c (tile u)][k = out k]; bias rows carry no gradient
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = c & 7;
      const bool ok = (c >> 3) == u && i < a.n3 && k < a.D;
      F.w4b[u][j] = bfbits((2.0f / (float)a.D) * ldsel(P, ok, OFF4 + i * 32 + k));
    }
    // L4 backward from UP: A[m = packed in c][k = 4q + j], only j = 0 and q's tile = c's tile
    {
      const int i = c & 7, q = g, out = 16 + (q & 1);
      const bool ok = j == 0 && (q >> 1) == (c >> 3) && i < a.n3 && out < a.D;
      F.w4bu[j] = bfbits((2.0f / (float)a.D) * ldsel(P, ok, OFF4 + i * 32 + out));
    }
    // L3 backward: A[m = packed in c][k = packed out k], same tile
    {
      const int i = c & 7, o = k & 7;
      const bool ok = (c >> 3) == (k >> 3) && i < a.n2 && o < a.n3;
      F.w3b[j] = bfbits(ldsel(P, ok, OFF3 + i * 16 + o));
    }
    // L2 backward: A[m = in c][k = packed out of tile u]
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = k & 7;
      const bool ok = (k >> 3) == u && c < a.n1 && o < a.n2;
      F.w2b[u][j] = bfbits(ldsel(P, ok, OFF2 + c * 16 + o));
    }
  }
  const bf16x4 zb = {0, 0, 0, 0};
  F.w1a[0] = cat8(F.w1t, F.w1u[0]);
  F.w1a[1] = cat8(F.w1u[1], F.w1t);
  bf16x4 w1ub;   // w1u[0] and w1u[1] have disjoint supports (lane groups g < 2 / g >= 2, + the bias)
#pragma unroll
  for (int j = 0; j < 4; ++j) w1ub[j] = (g >> 1) == 0 ? F.w1u[0][j] : F.w1u[1][j];
  F.w1s = cat8(F.w1t, w1ub);
  F.w2a = cat8(F.w2t[0], F.w2t[1]);
  F.w4ba = cat8(F.w4b[0], F.w4b[1]);
  // the second K half meets an all-zero B half (d3's UP MFMA), so it can be any finite fragment:
  // w3b's registers serve as that half instead of two more persistent zero registers
  F.w4bua = cat8(F.w4bu, F.w3b);
  (void)zb;
}

// Image slot s -> the packed-accumulator slab slots whose sum it is (-1: none, gradient 0).
// CM: the dead inputs' layer-1 rows accumulated don't-care inputs; their gradient is exactly 0.
template <bool CM = false>
__device__ __forceinline__ void packed_fold_src(int s, int& s1, int& s2) {
  s1 = s;
  s2 = -1;
  if (CM && s < OFF1 + 16 * 16 && cm_dead((s - OFF1) >> 4)) {
    s1 = -1;
    return;
  }
  if (s >= OFF1 + 16 * 16 && s < OFF2) {   // layer-1 rows 16..31: UP rows 16 + m of the slab
    const int in = (s - OFF1) >> 4, out = (s - OFF1) & 15;
    if (in == 16 || in == 17) {
      s1 = OFF1 + (16 + 4 * (in - 16)) * 16 + out;        // tile 0: m = 4q
      s2 = OFF1 + (16 + 8 + 4 * (in - 16)) * 16 + out;    // tile 1: m = 8 + 4q
    } else if (in == 31) {
      s1 = OFF1 + (16 + 1) * 16 + out;                     // the bias input, m = 1 (both tiles)
    } else {
      s1 = -1;
    }
    return;
  }
  if (s < OFF2 || s >= NPARAM) return;   // layer-1 rows 0..15 and the metric sums are not packed
  if (s < OFF3) {
    const int in = (s - OFF2) >> 4, out = (s - OFF2) & 15;
    if (out < 7) s2 = s + 8;
    else s1 = -1;
    return;
  }
  const bool l3 = s < OFF4;
  const int base = l3 ? OFF3 : OFF4, w = l3 ? 16 : 32;
  const int in = (s - base) / w, out = (s - base) % w;
  const int pin = in < 7 ? in : (in == 15 ? 7 : -1);
  if (pin < 0 || (l3 && out >= 7)) {
    s1 = -1;
    return;
  }
  if (!l3 && out >= 16) {   // outputs 16 / 17 live in the UP columns 4q: tile 0 q = 0, 1; tile 1 q = 2, 3
    if (out >= 18) {
      s1 = -1;
      return;
    }
    s1 = base + pin * w + 16 + 4 * (out - 16);
    s2 = base + (pin + 8) * w + 16 + 8 + 4 * (out - 16);
    return;
  }
  s1 = base + pin * w + out;
  s2 = base + (pin + 8) * w + out + (l3 ? 8 : 0);
}

// The two halves of lds_transpose, for operands whose transposed copy is only needed at the end
// of the step: write it to its own slot as soon as it exists (its registers die there), read the
// transposed copy back right before the weight-gradient MFMA (EW variants).
__device__ __forceinline__ void tr_write(bf16x4 v, char* slot, int c, int g) {
  *(lds_bf16x4*)(slot + tr_wr_off(c, g)) = v;   // the swizzled layout of lds_transpose
}
__device__ __forceinline__ bf16x4 tr_read(char* slot, int c, int g) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(slot + tr_rd_off(c, g)));
}
// the same read at a lane address the caller keeps (tr_rd_off_half: the lane-masked reads)
__device__ __forceinline__ bf16x4 tr_read_at(lds_cc* lane_addr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)lane_addr);
}
// Lane-masked reads (XP 5): the masked slots MASK_SLOT0 .. MASK_SLOT0 + 2 hold xub, h3b, dz2b.  Their
// cells (tr_mask_cell_word), shared by the workgroup's waves, sit past the rings; the xub slot's
// constant is the bias feature c == 1 that the second half of dW1's UP operand keeps.
constexpr int MASK_SLOT0 = 9, MASK_CELL_BYTES = TR_MASK_CELL_BYTES;

// NP packed pairs of whole tiles in ONE interleaved instruction stream (NP = 1 or 2).  Every
// stage is a loop over the NP pairs, so with NP = 2 the two pairs' dependent MFMA -> activation
// -> MFMA chains are independent instruction sequences the compiler interleaves: one pair's
// VALU issues while the other's MFMA result is in flight (the chain has ~13 dependent stages;
// one pair per wave leaves most of a trip waiting on them, profiles/r06/SUMMARY.md §1).  The
// pairs share the weight fragments and the gradient accumulators; each has TS transpose slots.
// XP: how the weight-gradient operands reach the rows-on-K layout.  0: LDS transposes at the end
// of the step; 1: the forward ones written to LDS as soon as they exist (EW), the tile halves of
// dW2 / dW4 in one accumulator each (MA); 2: no LDS at all -- each operand is the A operand of one
// 16x16x16 MFMA against the identity (C = A . I is the operand in the rows-on-K C layout, exact in
// fp32, repacked to bf16 bit-exactly), plus MA; 3: EW for the 7 forward operands (LDS slots 0..6),
// the MFMA identity for the 7 backward ones, plus MA; 4 (TS 12): XP 3, and the five backward
// operands that exist before the end of the chain -- dz4b[0..1], dz4bu (packed before d3), dz3b
// (before d2), dz2b (before d1) -- are written to slots 7..11 as soon as they are packed and read
// back transposed with the forward ones, the rest of the backward chain hiding the round trip;
// only dz1b[0..1], produced last, keep the MFMA identity (5 MFMA and 10 cvt_pk fewer per pair, the
// same bf16 bits); 5: XP 4 with the lane masks of the MA operands in the read addresses -- xur, h3r
// and dz2r are each read once through rd_lo and once through rd_hi (tr_rd_off_half: the masked
// source lanes read cells of zeros) instead of twelve selects per pair, and the pad lane leaves the
// L1 sum by a multiply; the same bf16 bits again (profiles/r17/mask_reads/SUMMARY.md).
// The LDS-transpose loop spends half its issue
// stalls waiting to issue LDS instructions (SQ_WAIT_INST_LDS, profiles/r06/SUMMARY.md §1).
// RX (tile-packed ring only): the fp32 inputs the loss needs (y - x) are read again from the pair's
// ring slot at the output layer instead of being held in 9 registers across the whole forward
// chain (`xrow[p]` / `xupa[p]`: the LDS addresses this lane read its four inputs of the pair's first
// tile and its UP input from; the slot is only re-filled after the next iteration's DMA issue).
// The ring's rows are the normalised ones, bit-identical to the first read.
// CM (compact ring): xf's dead-input slots are don't-cares (see cm_row_x); the RX re-read takes
// the compact offsets and the loss masks the dead slots' targets to 0.
// WA: the variant is only ever launched with want_acc (the tile-packed ring variants, XM 1), so the
// metric block is unconditional: no branch, and the argmax of y fills the backward chain's MFMA waits.
// RC: count the rows here (false: the caller sets them from its trip count after the loop).
template <int PACK, int DC, int TS = 10, int NP = 1, int XP = 0, bool RX = false, bool CM = false,
          bool WA = false, bool RC = true>
__device__ __forceinline__ void train_pair_packed(const AEArgs& a, const FragsP& F, char* scr, int c, int g,
                                                  const f32x4 (&xf)[NP][2][2], const float (&xup)[NP],
                                                  const int (&ix)[NP][2], f32x4 acc1[2], f32x4& acc2, f32x4& acc3,
                                                  f32x4 acc4[2], f32x4& acc2b, f32x4& acc4b, float& sq, float& ab,
                                                  float& corr, float& rows, lds_cc* const* xrow = nullptr,
                                                  lds_cc* const* xupa = nullptr, lds_cc* rd_lo = nullptr,
                                                  lds_cc* rd_hi = nullptr) {
  // xup: the UP-layout copy of inputs 16 / 17 (lane group g: input 16 + (g & 1) of tile g >> 1)
  static_assert(PACK == PACK_REF && DC == 18, "reference model, D = 18 (outputs 16, 17 packed as UP)");
  static_assert(NP == 1 || NP == 2, "one or two pairs per iteration");
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bf16x4 zb = {0, 0, 0, 0};
  const bool pad_lane = (g == 3);
  const bool lo = c < 8;   // lanes holding tile 0's half of a packed operand (as n or m = c)
  const float pad_m = pad_lane ? 0.f : 1.f;
  constexpr bool EW = XP == 1 || XP >= 3, MA = XP >= 1, TRM = XP == 2;
  constexpr bool EB = XP >= 4;   // the early backward writes (slots 7..11)
  constexpr bool MR = XP == 5;   // lane masks by masked transposed reads, pad lane by a multiply
  // transpose slots.  MR renumbers them so that the three lane-masked operands (xub, h3b, dz2b) are
  // adjacent: their zero cells (tr_mask_cell_word) then span two slot strides and 32 bytes.
  constexpr int S_XU = MR ? 9 : 2, S_H1 = MR ? 2 : 3, S_H2 = MR ? 4 : 5, S_H3 = MR ? 10 : 6, S_DZ4 = MR ? 5 : 7,
                S_DZ4U = MR ? 7 : 9, S_DZ3 = MR ? 8 : 10, S_DZ2 = 11;
  static_assert(!MR || (NP == 1 && S_XU == MASK_SLOT0 && S_H3 == MASK_SLOT0 + 1 && S_DZ2 == MASK_SLOT0 + 2),
                "masked reads: one pair per wave, the masked slots where the kernel put their cells");
  // identity B operand (lane (n = c, g) holds k = 4g..4g+3): 1 where k == n
  bf16x4 ident;
#pragma unroll
  for (int j = 0; j < 4; ++j) ident[j] = bfbits(4 * g + j == c ? 1.0f : 0.0f);
  auto mfma_tr = [&](bf16x4 v) -> bf16x4 { return pack4(mfma16(v, ident, zero4)); };

  bf16x4 xb0[NP][2], h1b[NP][2], xub[NP];
  f32x4 h1[NP][2], y[NP][2], z1[NP][2], l1s[NP][2];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int u = 0; u < 2; ++u) xb0[p][u] = pack4(xf[p][u][0]);
    // inputs 16 / 17 of both tiles (UP) and the constant-1 bias input (k = 1, lane group 0) in
    // one B operand; layer 1 is one 16x16x32 per tile: [inputs 0..15 | UP + bias]
    xub[p] = pack4(f32x4{xup[p], g == 0 ? 1.0f : 0.0f, 0.f, 0.f});
    if constexpr (EW) {   // slots 0..6 of the pair: the forward operands of the weight gradients
      tr_write(xb0[p][0], scr + (p * TS + 0) * 512, c, g);
      tr_write(xb0[p][1], scr + (p * TS + 1) * 512, c, g);
      tr_write(xub[p], scr + (p * TS + S_XU) * 512, c, g);
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if constexpr (MA) {   // the shared A operand; tile u's UP lanes (g >> 1 == u) + the bias lane
      // (xup of tile u's lanes | the bias one) without converting again: the low word of xub is
      // (bf16(xup), bf16 one-or-zero), so xu0 is xub with lane groups 2 / 3 zeroed, and xu1 is xub in
      // lane groups 2 / 3 (whose bias half is 0) and the lane-invariant (0, one-or-zero) elsewhere --
      // the fp32 bits of 1.0 / 0.0 are that packed word.  The same bf16 bits as two more pack4s.
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
      const unsigned xw = __builtin_bit_cast(u32x2, xub[p])[0];
      const unsigned bias_w = __float_as_uint(g == 0 ? 1.0f : 0.0f);
      const bf16x4 xu0 = __builtin_bit_cast(bf16x4, u32x2{g < 2 ? xw : 0u, 0u});
      const bf16x4 xu1 = __builtin_bit_cast(bf16x4, u32x2{g >= 2 ? xw : bias_w, 0u});
      z1[p][0] = mfma32a(F.w1s, xb0[p][0], xu0, zero4);
      z1[p][1] = mfma32a(F.w1s, xb0[p][1], xu1, zero4);
    } else {
      z1[p][0] = mfma32a(F.w1a[0], xb0[p][0], xub[p], zero4);
      z1[p][1] = mfma32a(F.w1a[1], xub[p], xb0[p][1], zero4);
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) h1[p][u][i] = tanh_exp2(z1[p][u][i]);
      h1b[p][u] = pack4(h1[p][u]);
      if constexpr (EW) tr_write(h1b[p][u], scr + (p * TS + S_H1 + u) * 512, c, g);
    }
  // Keras L1 activity-regulariser gradient l1 * sign(h1) as one v_med3 (see train_tile), computed
  // off the critical path and fed to the dh1 MFMA as its accumulator input (EW: right before it,
  // so its registers are not live across the whole step)
  auto l1_sign = [&] {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) l1s[p][u][i] = __builtin_amdgcn_fmed3f(h1[p][u][i], -a.l1, a.l1);
  };
  if constexpr (!MA) l1_sign();
  f32x4 z2[NP], h2[NP], h3[NP], z3[NP];
  bf16x4 h2b[NP], h3b[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) z2[p] = mfma32a(F.w2a, h1b[p][0], h1b[p][1], zero4);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int i = 0; i < 4; ++i) h2[p][i] = relu_fast(z2[p][i]);
    h2b[p] = pack4(h2[p]);
    if constexpr (EW) tr_write(h2b[p], scr + (p * TS + S_H2) * 512, c, g);
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) z3[p] = mfma16(F.w3t, h2b[p], zero4);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int i = 0; i < 4; ++i) h3[p][i] = tanh_exp2(z3[p][i]);
    h3b[p] = pack4(h3[p]);
    if constexpr (EW) tr_write(h3b[p], scr + (p * TS + S_H3) * 512, c, g);
  }
  // output layer: outputs 0..15 per tile, outputs 16 / 17 of BOTH tiles in one register (UP:
  // lane group g = output 16 + (g & 1) of tile g >> 1; w4u's rows m = 4q, so only C entry 0 is used)
  f32x4 dz4[NP][2], z4[NP][2], z4u[NP];
  float dz4up[NP], yup[NP];
  f32x4 xl[NP][2];   // the loss's x: xf, or (RX) a second read of the ring slot
  float xul[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if constexpr (RX) {
      typedef __attribute__((address_space(3))) const float lds_f;
      constexpr int DR = CM ? 14 : 18, SLOTB = 64 * DR + 16;
#pragma unroll
      for (int u = 0; u < 2; ++u) xl[p][u] = ring_row4(xrow[p] + u * SLOTB);
      xul[p] = *(lds_f*)xupa[p];
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) xl[p][u] = xf[p][u][0];
      xul[p] = xup[p];
    }
  }
  // CM: the dead slots' targets are 0.  e = fma(-x, m, y) with the lane-invariant mask m (1 live,
  // 0 dead; slot 3 is always live) instead of a select per target: m = 1 is y - x with its one
  // rounding, m = 0 leaves y (x is finite, and where y is a zero of either sign the loss and the
  // relu derivative below do not see the sign of e).
  const float cm_m[3] = {g < 2 ? 0.f : 1.f, g == 1 ? 0.f : 1.f, g == 0 ? 0.f : 1.f};
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int u = 0; u < 2; ++u) z4[p][u] = mfma16(F.w4t[u], h3b[p], zero4);
    z4u[p] = mfma16(F.w4u, h3b[p], zero4);
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        y[p][u][i] = relu_fast(z4[p][u][i]);
        float e = (CM && i < 3) ? fmaf(-xl[p][u][i], cm_m[i], y[p][u][i]) : y[p][u][i] - xl[p][u][i];
        sq = fmaf(e, e, sq);
        dz4[p][u][i] = y[p][u][i] > 0.f ? e : 0.f;   // relu'; x 2/D folded into F.w4b / the acc4 slab
      }
    yup[p] = relu_fast(z4u[p][0]);
    float eup = yup[p] - xul[p];
    sq = fmaf(eup, eup, sq);
    dz4up[p] = yup[p] > 0.f ? eup : 0.f;
  }
  if (WA || a.want_acc) {   // lane group 0 counts row c of tile 0, group 1 row c of tile 1
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int iy = row_argmax_up_pair(y[p][0], y[p][1], yup[p], g);
      const int sel = -(g & 1);   // bit-select: a ?: on the pair becomes a scratch array indexed by g
      const int ixs = (ix[p][0] & ~sel) | (ix[p][1] & sel);
      corr += (g < 2 && iy == ixs) ? 1.f : 0.f;
    }
  }
  if constexpr (RC) rows += (g == 0) ? 2.f * NP : 0.f;

  bf16x4 dz4b[NP][2], dz1b[NP][2], dz4bu[NP], dz3b[NP], dz2b[NP];
  f32x4 d3[NP], d2[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int u = 0; u < 2; ++u) dz4b[p][u] = pack4(dz4[p][u]);
    dz4bu[p] = pack4(f32x4{dz4up[p], 0.f, 0.f, 0.f});
    if constexpr (EB) {
      tr_write(dz4b[p][0], scr + (p * TS + S_DZ4) * 512, c, g);
      tr_write(dz4b[p][1], scr + (p * TS + S_DZ4 + 1) * 512, c, g);
      tr_write(dz4bu[p], scr + (p * TS + S_DZ4U) * 512, c, g);
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    d3[p] = mfma32a(F.w4ba, dz4b[p][0], dz4b[p][1], zero4);   // K halves: tile 0 / tile 1 outputs 0..15
    d3[p] = mfma32a(F.w4bua, dz4bu[p], zb, d3[p]);             // + outputs 16 / 17 (one shape per chain)
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    f32x4 dz3;
#pragma unroll
    for (int i = 0; i < 4; ++i) dz3[i] = d3[p][i] * fmaf(-h3[p][i], h3[p][i], 1.0f);   // 0 at the bias slots (h = 1)
    dz3b[p] = pack4(dz3);
    if constexpr (EB) tr_write(dz3b[p], scr + (p * TS + S_DZ3) * 512, c, g);
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) d2[p] = mfma16(F.w3b, dz3b[p], zero4);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    f32x4 dz2;
#pragma unroll
    for (int i = 0; i < 4; ++i) dz2[i] = h2[p][i] > 0.f ? d2[p][i] : 0.f;
    dz2b[p] = pack4(dz2);
    if constexpr (EB) tr_write(dz2b[p], scr + (p * TS + S_DZ2) * 512, c, g);
  }
  f32x4 d1[NP][2];
  if constexpr (MA) l1_sign();
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int u = 0; u < 2; ++u) d1[p][u] = mfma16(F.w2b[u], dz2b[p], l1s[p][u]);   // dh1 + l1 * sign(h1)
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      f32x4 dz1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hv = h1[p][u][i];
        // MR: the pad lane's slot 3 leaves the L1 sum by a multiply with the lane-invariant 0 / 1
        // (|h| * 1 and ab + 0 are exact: the same bits as the select, one VALU less)
        if (MR && i == 3)
          ab = fmaf(fabsf(hv), pad_m, ab);
        else
          ab += (i == 3 && pad_lane) ? 0.f : fabsf(hv);
        dz1[i] = d1[p][u][i] * fmaf(-hv, hv, 1.0f);
      }
      dz1b[p][u] = pack4(dz1);
    }

  // weight gradients (rows on K through the LDS transpose).  Pair p owns slots [p*TS, p*TS + TS);
  // TS < 10: slots k and k + TS share 512 B of scratch -- a wave's LDS operations execute in order,
  // so a later write cannot overtake an earlier transposed read of the same slot
  // EW: slots 0..6 hold the forward operands written early, 7..9 take the backward ones in turn
  // (XP 1); XP 4 (TS 12): 7..11 hold dz4b[0..1], dz4bu, dz3b, dz2b, written early too.  Slot reuse
  // across trips is safe for the same in-order reason: the next trip's write of a slot follows
  // this trip's read of it in the wave's LDS stream.
  static_assert(TS >= 1 && TS <= 12 && (!EW || TS == (EB ? 12 : 10)), "transpose slots");
  (void)mfma_tr;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    char* sp = scr + p * TS * 512;
    bf16x4 xr0[2], dz1r[2], h1r[2], dz4r[2], xur, dz4ru, dz2r, h2r, dz3r, h3r;
    bf16x4 xur_m[2], dz2r_m[2], h3r_m[2];   // MR: the [c < 8 | c >= 8] lane-masked copies, as read
    if constexpr (MR) {
      // the order of XP 4; each masked operand once through rd_lo (result lanes c >= 8 are zeros)
      // and once through rd_hi (c < 8 zeros; the xub slot's cell keeps the bias feature c == 1)
      h3r = tr_read(sp + S_H3 * 512, c, g);
      h3r_m[0] = tr_read_at(rd_lo + S_H3 * 512);
      h3r_m[1] = tr_read_at(rd_hi + S_H3 * 512);
      dz4r[0] = tr_read(sp + S_DZ4 * 512, c, g);
      dz4r[1] = tr_read(sp + (S_DZ4 + 1) * 512, c, g);
      dz4ru = tr_read(sp + S_DZ4U * 512, c, g);
      h2r = tr_read(sp + S_H2 * 512, c, g);
      dz3r = tr_read(sp + S_DZ3 * 512, c, g);
      h1r[0] = tr_read(sp + S_H1 * 512, c, g);
      h1r[1] = tr_read(sp + (S_H1 + 1) * 512, c, g);
      dz2r_m[0] = tr_read_at(rd_lo + S_DZ2 * 512);
      dz2r_m[1] = tr_read_at(rd_hi + S_DZ2 * 512);
      xr0[0] = tr_read(sp + 0 * 512, c, g);
      xr0[1] = tr_read(sp + 1 * 512, c, g);
      xur_m[0] = tr_read_at(rd_lo + S_XU * 512);
      xur_m[1] = tr_read_at(rd_hi + S_XU * 512);
      dz1r[0] = mfma_tr(dz1b[p][0]);
      dz1r[1] = mfma_tr(dz1b[p][1]);
    } else if constexpr (EB) {
      // LDS reads return in order (behind the RX re-read of the ring slot), so the operands of
      // the gradient MFMAs that can go first are asked for first: dW4, dW3, dW2 need nothing
      // else; dW1's partners dz1r come off the matrix pipe last, so xr0 / xur are read last.
      h3r = tr_read(sp + 6 * 512, c, g);
      dz4r[0] = tr_read(sp + 7 * 512, c, g);
      dz4r[1] = tr_read(sp + 8 * 512, c, g);
      dz4ru = tr_read(sp + 9 * 512, c, g);
      h2r = tr_read(sp + 5 * 512, c, g);
      dz3r = tr_read(sp + 10 * 512, c, g);
      h1r[0] = tr_read(sp + 3 * 512, c, g);
      h1r[1] = tr_read(sp + 4 * 512, c, g);
      dz2r = tr_read(sp + 11 * 512, c, g);
      xr0[0] = tr_read(sp + 0 * 512, c, g);
      xr0[1] = tr_read(sp + 1 * 512, c, g);
      xur = tr_read(sp + 2 * 512, c, g);
      dz1r[0] = mfma_tr(dz1b[p][0]);
      dz1r[1] = mfma_tr(dz1b[p][1]);
    } else if constexpr (TRM) {
      xr0[0] = mfma_tr(xb0[p][0]);
      xr0[1] = mfma_tr(xb0[p][1]);
      xur = mfma_tr(xub[p]);
      h1r[0] = mfma_tr(h1b[p][0]);
      h1r[1] = mfma_tr(h1b[p][1]);
      h2r = mfma_tr(h2b[p]);
      h3r = mfma_tr(h3b[p]);
      dz4r[0] = mfma_tr(dz4b[p][0]);
      dz4r[1] = mfma_tr(dz4b[p][1]);
      dz4ru = mfma_tr(dz4bu[p]);
      dz3r = mfma_tr(dz3b[p]);
      dz2r = mfma_tr(dz2b[p]);
      dz1r[0] = mfma_tr(dz1b[p][0]);
      dz1r[1] = mfma_tr(dz1b[p][1]);
    } else if constexpr (EW) {
      xr0[0] = tr_read(sp + 0 * 512, c, g);
      xr0[1] = tr_read(sp + 1 * 512, c, g);
      xur = tr_read(sp + 2 * 512, c, g);
      h1r[0] = tr_read(sp + 3 * 512, c, g);
      h1r[1] = tr_read(sp + 4 * 512, c, g);
      h2r = tr_read(sp + 5 * 512, c, g);
      h3r = tr_read(sp + 6 * 512, c, g);
      if constexpr (XP == 3) {   // the backward operands by MFMA against the identity
        dz4r[0] = mfma_tr(dz4b[p][0]);
        dz4r[1] = mfma_tr(dz4b[p][1]);
        dz4ru = mfma_tr(dz4bu[p]);
        dz3r = mfma_tr(dz3b[p]);
        dz2r = mfma_tr(dz2b[p]);
        dz1r[0] = mfma_tr(dz1b[p][0]);
        dz1r[1] = mfma_tr(dz1b[p][1]);
      } else {
        dz4r[0] = lds_transpose(dz4b[p][0], sp + 7 * 512, c, g);
        dz4r[1] = lds_transpose(dz4b[p][1], sp + 8 * 512, c, g);
        dz4ru = lds_transpose(dz4bu[p], sp + 9 * 512, c, g);
        dz3r = lds_transpose(dz3b[p], sp + 7 * 512, c, g);
        dz2r = lds_transpose(dz2b[p], sp + 8 * 512, c, g);
        dz1r[0] = lds_transpose(dz1b[p][0], sp + 9 * 512, c, g);
        dz1r[1] = lds_transpose(dz1b[p][1], sp + 7 * 512, c, g);
      }
    } else {
      xur = lds_transpose(xub[p], sp + (1 % TS) * 512, c, g);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        xr0[u] = lds_transpose(xb0[p][u], sp + (0 % TS) * 512, c, g);
        dz1r[u] = lds_transpose(dz1b[p][u], sp + (2 % TS) * 512, c, g);
        h1r[u] = lds_transpose(h1b[p][u], sp + (3 % TS) * 512, c, g);
        dz4r[u] = lds_transpose(dz4b[p][u], sp + (8 % TS) * 512, c, g);
      }
      dz4ru = lds_transpose(dz4bu[p], sp + (9 % TS) * 512, c, g);
      dz2r = lds_transpose(dz2b[p], sp + (4 % TS) * 512, c, g);
      h2r = lds_transpose(h2b[p], sp + (5 % TS) * 512, c, g);
      dz3r = lds_transpose(dz3b[p], sp + (6 % TS) * 512, c, g);
      h3r = lds_transpose(h3b[p], sp + (7 % TS) * 512, c, g);
    }
    acc1[0] = mfma32(xr0[0], xr0[1], dz1r[0], dz1r[1], acc1[0]);
    // rows 16 + m: m = 0 / 4 tile 0's inputs 16 / 17, m = 8 / 12 tile 1's, m = 1 the bias (both)
    if constexpr (MR)
      acc1[1] = mfma32(xur_m[0], xur_m[1], dz1r[0], dz1r[1], acc1[1]);
    else
      acc1[1] = mfma32(lo ? xur : zb, (!lo || c == 1) ? xur : zb, dz1r[0], dz1r[1], acc1[1]);
    // dW2 / dW4 (outputs 0..15): each tile against the whole packed operand, in an accumulator
    // of its own (only its half -- n < 8 / m < 8 for tile 0 -- is kept when the slab is written):
    // two 16x16x16 instead of a 16x16x32 on lane-masked copies (no per-pair selects)
    if constexpr (MR) {   // MA with the masks already in the operands
      acc2 = mfma32(h1r[0], h1r[1], dz2r_m[0], dz2r_m[1], acc2);
      acc3 = mfma16(h2r, dz3r, acc3);
      acc4[0] = mfma32(h3r_m[0], h3r_m[1], dz4r[0], dz4r[1], acc4[0]);
    } else if constexpr (MA) {
      // 8 fewer accumulator registers: each tile's contraction against its own half of the packed
      // operand (the other half lane-masked to 0) in ONE 16x16x32 -- dW2 columns n < 8 / n >= 8
      // (lane c) from tile 0 / 1, dW4 rows m < 8 / m >= 8 (lane c of the A operand) likewise; the
      // masked products are exact zeros, acc2b / acc4b stay 0 and the slab fold keeps acc2 / acc4[0]
      acc2 = mfma32(h1r[0], h1r[1], lo ? dz2r : zb, lo ? zb : dz2r, acc2);
      acc3 = mfma16(h2r, dz3r, acc3);
      acc4[0] = mfma32(lo ? h3r : zb, lo ? zb : h3r, dz4r[0], dz4r[1], acc4[0]);
    } else {
      acc2 = mfma16(h1r[0], dz2r, acc2);
      acc2b = mfma16(h1r[1], dz2r, acc2b);
      acc3 = mfma16(h2r, dz3r, acc3);   // diagonal blocks; acc3's chain is 16x16x16 only in this variant
      acc4[0] = mfma16(h3r, dz4r[0], acc4[0]);
      acc4b = mfma16(h3r, dz4r[1], acc4b);
    }
    // outputs 16 / 17: UP columns 4q pair with their own tile's rows m by construction (the
    // other tile's blocks are never folded), so h3r needs no mask; acc4[1]'s chain is 16x16x16
    acc4[1] = mfma16(h3r, dz4ru, acc4[1]);
  }
}

// 3 waves/SIMD: caps the allocation at 168 VGPRs (no spills); 171 would drop to 2.
// PF > 0: the input rows stream through a per-wave LDS ring PF tiles deep, filled
// by LDS-DMA (no VGPRs held for the prefetch, PF-1 tiles in flight per wave);
// requires contiguous rows (ld == D), 17 <= D <= 31 and D even.  PF = 0: one tile
// of register prefetch (any ld / D).
// OCC = waves per SIMD the variant is built for: 3 (168-VGPR budget, 6 KB ring per
// wave) or 4 (128-VGPR budget, 3968-B ring per wave so four workgroups fit in LDS).
// ILP 2 (tile pairs, 3 waves/SIMD): 7008 B = six 1168-B packed tiles per wave; with the
// slab area and the normaliser 52928 B per workgroup, three workgroups per CU.
// Packed pairs (ILP 3) at OCC >= 4: two pair slots (4 x 1168 B) per wave.
template <int OCC, int ILP = 1>
constexpr int ring_bytes() { return ILP == 3 ? (OCC >= 4 ? 4672 : 7008) : OCC >= 4 ? 3968 : (ILP >= 2 ? 7008 : 6144); }
// packed pairs: PF tiles of 64 * 18 + 16 B (sized by the ring depth, not the occupancy);
// compact ring (CM): 64 * 14 + 16 = 912 B per tile
template <int OCC, int ILP, int PF, int CM = 0>
constexpr int ring_bytes_pf() { return ILP == 3 ? PF * (CM ? 912 : 1168) : ring_bytes<OCC, ILP>(); }
static_assert(ring_bytes<4>() == kRing1Tile4w && ring_bytes<3>() == kRing1Tile3w, "the launcher's ring depths");

// LDS layout.  Default: [slab area = per-wave transpose scratch (10 x 512 B) | normaliser | rings].
// Packed pairs (ILP 3): [TS x 512 B transpose scratch per wave | normaliser | rings], and the
// per-wave gradient slabs written after the loop ALIAS that whole area (the rings are retired
// with vmcnt(0) and a workgroup barrier first) -- so the loop's LDS is not charged for the slab:
// OCC 4 (two pair slots, TS 10) is 39 424 B = four workgroups per CU on the 18-column ring and 35 328 B
// on the compact one.  XP 4 (TS 12, the early backward writes) is built for the compact ring only:
// 39 424 B there; the 18-column and the raw-row 4-wave instances are at 39 424 B with TS 10 already
// and would drop to three workgroups per CU, so they keep XP 3.
// MC: bytes of lane-mask cells past the rings (XP 5: 40 480 B, inside the 40 960 B that four
// workgroups per CU allow).
template <int PF, int OCC, int ILP, int TS, int NPW = 1, int CM = 0, int MC = 0>
struct AELds {
  static constexpr int SCR = (ILP == 3 ? NPW * TS : 10) * 512;      // per wave (0: MFMA transposes)
  static constexpr int NORM_OFF = ILP == 3 ? WAVES * SCR : SLAB_BYTES;
  static constexpr int RING_OFF = NORM_OFF + NORM_BYTES;
  static constexpr int RING = ring_bytes_pf<OCC, ILP, PF, CM>();
  static constexpr int CELLS_OFF = RING_OFF + (PF > 0 ? WAVES * RING : 0);
  static constexpr int END = CELLS_OFF + MC;
  static constexpr int BYTES = END > SLAB_BYTES ? END : SLAB_BYTES;
};

// NPW (packed pairs only): pairs trained per loop iteration in one interleaved stream.
// XP (packed pairs only): the weight-gradient operand path of train_pair_packed.
// CM (packed pairs on the tile-packed ring only): the compact ring of the 14 live cardata
// features: 912-B tile slots, a pair = two DMAs of 1024 + 800 B.
// V: the instance's eleven values as a named type (the variants of sml_ae_variants.h).
template <class V>
__global__ __launch_bounds__(WAVES * 64, V::OCC) void ae_train_kernel(AEArgs a) {
  constexpr int PACK = V::PACK, PF = V::PF, OCC = V::OCC, DC = V::DC, XM = V::XM, ILP = V::ILP, TS = V::TS,
                NPW = V::NPW, XP = V::XP, CM = V::CM;
  constexpr bool VEC = V::VEC;
  constexpr bool FAST = zero_preserving<PACK>();
  constexpr bool CMP = CM != 0;
  static_assert(!CMP || (ILP == 3 && XM == 1 && DC == 18), "compact ring: packed pairs, tile-packed ring, D = 18");
  constexpr int DR = CMP ? 14 : DC;   // floats per ring row (0: a.D)
  constexpr bool MR = XP == 5;   // lane masks by masked transposed reads (train_pair_packed)
  static_assert(!MR || (ILP == 3 && XM == 1 && NPW == 1 && PF == 4 && TS == 12), "XP 5: the unrolled two-slot pair loop");
  using L = AELds<PF, OCC, ILP, (XP == 2 ? 0 : TS), NPW, CM, MR ? MASK_CELL_BYTES : 0>;
  static_assert(L::BYTES <= 40960 || OCC < 4, "four workgroups per CU");
  static_assert(NPW == 1 || ILP == 3, "several pairs per iteration: packed pairs only");
  constexpr int RING = L::RING;
  static_assert(WAVES * (ILP == 3 && NPW == 1 ? TS : 10) * 512 <= SLAB_BYTES,
                "transpose scratch must fit in the slab buffer");
  static_assert(ILP == 3 || TS == 10, "shared transpose slots: packed pairs only");
  static_assert(PF == 0 || CMP || PF * 64 * 17 <= RING, "ring slots must fit the smallest ring tile");
  // XM: x-argmax mode. 0 in-kernel argmax; 1 tile-packed ring (rows + ingest-time argmax
  // bytes per tile, pack_tiles_argmax)
  static_assert(XM == 0 || XM == 1, "x-argmax mode");
  constexpr bool XA = XM == 1;
  static_assert(XM != 1 || (DC > 0 && PF > 0 && PF * (64 * DR + 16) <= RING), "XA: compile-time D, ring slots + argmax");
  // one LDS array: per-wave transpose scratch during the tile loop, per-wave
  // gradient slabs afterwards | the normaliser | (PF > 0) the per-wave input rings
  __shared__ __attribute__((aligned(16))) float smem[L::BYTES / 4];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  char* scr = reinterpret_cast<char*>(smem) + wid * L::SCR;
  const char* norm = reinterpret_cast<const char*>(smem) + L::NORM_OFF;
  if (a.cursor) {  // streaming ring consumer (uniform scalar load)
    a.x += a.cursor[0] * a.ld;
    if (XM == 1) a.xpack += (a.cursor[0] >> 4) * (int64_t)(64 * (CMP ? DR : a.D) + 16);
  }

  if (a.iter && blockIdx.x == 0 && threadIdx.x == 0) a.iter[0] += 1;
  if (threadIdx.x < 64) {
    const int f = threadIdx.x & 31;
    smem[L::NORM_OFF / 4 + threadIdx.x] = threadIdx.x < 32 ? norm_scale(a, f) : norm_shift(a, f);
  }

  Frags F;
  FragsP FP;   // ILP 3 (packed pairs) only
  if constexpr (ILP == 3)
    load_frags_packed<CMP>(a, c, g, FP);
  else
    load_frags<FAST, FAST && prescaled_tanh<PACK>(), FAST && inject_bias_slots<PACK>()>(a, c, g, F, true);
  const float pad1 = (g == 3) ? 1.0f : 0.0f;
  if constexpr (MR) {   // the lane-mask cells: zeros, and bf16 1.0 at feature 1 of the xub slot's first cell
    for (int i = threadIdx.x; i < MASK_CELL_BYTES / 4; i += WAVES * 64)
      smem[L::CELLS_OFF / 4 + i] = __uint_as_float(tr_mask_cell_word(i));
  }
  __syncthreads();  // normaliser visible (before any LDS-DMA is in flight)

  f32x4 acc1[2], acc2, acc3, acc4[2], acc2b, acc4b;   // acc2b / acc4b: packed pairs' tile-1 halves
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  acc1[0] = acc1[1] = acc2 = acc3 = acc4[0] = acc4[1] = acc2b = acc4b = zero4;
  float sq = 0.f, ab = 0.f, corr = 0.f, rows = 0.f;

  const int64_t nfull = a.n >> 4;
  const int64_t stride = (int64_t)gridDim.x * WAVES;
  const int64_t first = (int64_t)blockIdx.x * WAVES + wid;
  if constexpr (PF > 0) {
    // LDS-DMA ring: tile first + k*stride lives in slot k % PF.  Every issue is
    // exactly two VMEM instructions (tiles past the end are clamped to the last
    // full tile, never skipped), so "tile k landed" is vmcnt(2 * (PF - 1)).
    const int slotb = 64 * (DR > 0 ? DR : a.D) + (XM == 1 ? 16 : 0);   // compile-time with DC: immediate offsets
    constexpr int NV = 2;  // VMEM instructions per tile issue
    const int nl2 = (slotb - 1024) >> 4;  // lanes of the second 16-B-per-lane DMA (>= 4)
    const int uwid = __builtin_amdgcn_readfirstlane(wid);  // keep the ring bookkeeping scalar
    const int ring_off = L::RING_OFF + uwid * RING;
    const unsigned ring_lds =
        (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + ring_off;
    const char* ring = reinterpret_cast<const char*>(smem) + ring_off;
    const int64_t ufirst = (int64_t)blockIdx.x * WAVES + uwid;
    const unsigned voff = lane * 16;
    // Retire the prologue's parameter loads with a compiler-visible wait: the
    // waitcnt pass cannot see the asm DMA counts, and a load still pending at the
    // loop entry would otherwise put a vmcnt(0) (a full ring drain) in every iteration.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
    if (nfull > 0) {
      auto issue = [&](int64_t tt, int slot) {
        tt = tt < nfull ? tt : nfull - 1;
        const char* src = XM == 1 ? reinterpret_cast<const char*>(a.xpack) + tt * slotb
                                  : reinterpret_cast<const char*>(a.x + tt * 16 * a.ld);
        const unsigned dst = ring_lds + slot * slotb;
        glds16(src, voff, dst);
        if (lane < nl2) glds16(src + 1024, voff, dst + 1024);
      };
      // Tile order of this wave: the tiles are interleaved over the waves;
      // increasing, so t >= nfull ends the wave.  (A lambda on purpose: with `+ stride` written
      // out at its three uses, four of the one-tile ring instances are scheduled differently.)
      auto next_tile = [&](int64_t t) -> int64_t { return t + stride; };
      const int64_t t0 = ufirst;
      if constexpr (ILP >= 2) {
        // ILP 2: tile pairs (t, t + stride), two issues per iteration, the pair's two tiles
        // landed = vmcnt(NV * (PF - 2)); a last unpaired tile runs alone (U = 1).  ILP 3:
        // contiguous tile pairs (below).
        static_assert((XM == 1 || ILP == 3) && PF >= 3, "tile pairs: tile-packed ring (or raw rows, packed pairs)");
        auto ring_tile = [&](int slot, f32x4 xf[2], int& ix) {
          typedef __attribute__((address_space(3))) const unsigned char lds_u8;
          if constexpr (XM == 1) ix = (int)*(lds_u8*)(ring + slot * slotb + (slotb - 16) + c);
          if constexpr (CMP) {   // the same inputs 0..15 from the compact row
            xf[0] = cm_row_x(ring + slot * slotb + c * 4 * DR + cm_off(g));
            xf[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            return;
          }
          if constexpr (ILP == 3) {   // inputs 0..15 only (16 / 17 come as UP, ring_up)
            typedef __attribute__((address_space(3))) const f32x2_t lds_f2;
            const char* row = ring + slot * slotb + c * 4 * a.D + 16 * g;
            const f32x2_t v0 = *(lds_f2*)row, v1 = *(lds_f2*)(row + 8);
            xf[0] = f32x4{v0[0], v0[1], v1[0], v1[1]};
            xf[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            return;
          }
          ring_x(a, ring + slot * slotb, c, g, xf);
#pragma unroll
          for (int j = 0; j < 4; ++j) xf[1][j] = (live_hi<DC>(j) && 16 + 4 * g + j < DC) ? xf[1][j] : 0.f;
        };
        // packed pairs' UP copy of inputs 16 / 17: lane group g reads input 16 + (g & 1) of row c
        // of the tile in `slot` (the caller passes tile g >> 1's slot)
        // tile 1 of a pair sits in the next slot (pairs start on even slots, PF even), so one
        // loop-invariant lane offset covers both tiles
        static_assert(ILP != 3 || PF % 2 == 0, "pairs start on even ring slots");
        const int row_off = c * 4 * DR + (CMP ? cm_off(g) : 16 * g);   // the lane's inputs 4g..4g+3 (packed pairs)
        const int up_off = c * 4 * DR + (CMP ? 8 * (g & 1) : 4 * (DR - 2 + (g & 1))) + (g >= 2 ? slotb : 0);   // CM: compact floats 0 / 2
        auto ring_up = [&](int slot) -> float {   // slot: the pair's first tile
          typedef __attribute__((address_space(3))) const float lds_f;
          return *(lds_f*)(ring + slot * slotb + up_off);
        };
        if constexpr (ILP == 3) {
          // Packed pairs take CONTIGUOUS tiles (2p, 2p + 1): one pair is one 2 x 1168-B block of
          // the tile-packed ring, moved by three LDS-DMAs (64 + 64 + 18 lanes x 16 B) instead of
          // two per tile; pairs are interleaved over the waves.  The launcher guarantees an even
          // tile count (no half pair).  Ring: PF / 2 pair slots, one pair in flight per slot.
          // Compact ring: a pair is 2 x 912 B, two DMAs (64 + 50 lanes x 16 B).
          constexpr int PS = PF / 2, NVP = CMP ? 2 : 3;
          const int pairb = 2 * slotb;
          const int nl3 = (pairb - (CMP ? 1024 : 2048)) >> 4;   // lanes of the last DMA
          const int64_t npairs = nfull >> 1;
          auto issue_pair_at = [&](int64_t pi, int ps) {   // pi < npairs
            // XM 1: the tile-packed ring; XM 0: the raw rows themselves (ld == D: a pair of
            // whole tiles is 32 contiguous rows = pairb bytes)
            const char* src = (XM == 1 ? reinterpret_cast<const char*>(a.xpack) : reinterpret_cast<const char*>(a.x)) +
                              pi * pairb;
            const unsigned dst = ring_lds + ps * pairb;
            glds16(src, voff, dst);
            if constexpr (CMP) {
              if (lane < nl3) glds16(src + 1024, voff, dst + 1024);
            } else {
              glds16(src + 1024, voff, dst + 1024);
              if (lane < nl3) glds16(src + 2048, voff, dst + 2048);
            }
          };
          auto issue_pair = [&](int64_t pi, int ps) {
            issue_pair_at(pi < npairs ? pi : npairs - 1, ps);   // prefetch past the end re-reads the last pair
          };
          (void)issue_pair;
          // NPW pairs per iteration (pi, pi + stride, ...): the ring holds PS = PF / 2 pair slots, PS - NPW
          // of them in flight while the NPW oldest are trained on.
          static_assert(PS > NPW, "ring: at least one pair in flight");
          auto load_pair = [&](int slot, f32x4 (&xf)[2][2], float& xup, int (&ix)[2]) {
            ring_tile(2 * slot, xf[0], ix[0]);
            ring_tile(2 * slot + 1, xf[1], ix[1]);
            xup = ring_up(2 * slot);
            if constexpr (XM == 0) {
              // raw rows (the direct step: rows trained once): normalize_fn on the lane's inputs
              // 4g..4g+3 of both tiles and its UP input 16 + (g & 1), then argmax(x) of both
              // tiles' rows with one butterfly -- what pack_tiles_argmax does at ingest for XM 1
              typedef __attribute__((address_space(3))) const f32x4 lds_f4;
              typedef __attribute__((address_space(3))) const float lds_f;
              const f32x4 nsc = *(lds_f4*)(norm + 16 * g), nsh = *(lds_f4*)(norm + 128 + 16 * g);
              const int fu = 4 * (16 + (g & 1));
              const float usc = *(lds_f*)(norm + fu), ush = *(lds_f*)(norm + 128 + fu);
#pragma unroll
              for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) xf[u][0][j] = fmaf(xf[u][0][j], nsc[j], nsh[j]);
              xup = fmaf(xup, usc, ush);
              ix[0] = ix[1] = a.want_acc ? row_argmax_up_pair_signed(xf[0][0], xf[1][0], xup, g) : -1;
            }
          };
          (void)load_pair;
          // (the 3-wave builds' three-slot ring and the raw-row variants spill with it and keep the
          // rolled loop below)
          if constexpr (NPW == 1 && XM == 1 && PS == 2) {
            // One pair per trip, two pair slots: the loop control is wave-uniform and 32-bit (the launcher bounds the
            // pair count), so it stays on the scalar unit -- the trip count once, the prefetch index
            // clamped by a scalar min -- and the loop is unrolled by the ring depth, so trip j reads
            // pair slot j % PS and fills slot (j - 1) % PS as compile-time LDS offsets.  Same pairs in
            // the same order per wave, same DMA and vmcnt counts as the rolled loop.
            const unsigned np32 = (unsigned)npairs, st32 = (unsigned)stride, uf32 = (unsigned)ufirst;
            const unsigned ntrip = __builtin_amdgcn_readfirstlane(uf32 < np32 ? (np32 - 1u - uf32) / st32 + 1u : 0u);
            unsigned pq = uf32;   // next pair to prefetch
            auto issue_next = [&](int ps) {
              issue_pair_at(pq < np32 ? pq : np32 - 1u, ps);   // past the end: re-read the last pair
              pq += st32;
            };
#pragma unroll
            for (int k = 0; k < PS - 1; ++k) issue_next(k);
            // the lane's three ring addresses, each ONE register for the whole loop (opaque to the
            // compiler, so every slot is base + immediate and no per-slot copy of them is kept)
            lds_cc* rowb = (lds_cc*)(ring + row_off);
            lds_cc* upb = (lds_cc*)(ring + up_off);
            lds_cc* axb = (lds_cc*)(ring + (slotb - 16) + c);   // XM 1: the tile's argmax byte of row c
            asm volatile("" : "+v"(rowb), "+v"(upb));
            asm volatile("" : "+v"(axb));
            // MR: the lane's two masked transposed-read addresses (tr_rd_off_half), one register each
            lds_cc* rd_lo = nullptr;
            lds_cc* rd_hi = nullptr;
            if constexpr (MR) {
              const int cells = L::CELLS_OFF - MASK_SLOT0 * 512 - wid * L::SCR;   // from this wave's slot
              rd_lo = (lds_cc*)scr + tr_rd_off_half(c, g, 0, cells);
              rd_hi = (lds_cc*)scr + tr_rd_off_half(c, g, 1, cells);
              asm volatile("" : "+v"(rd_lo), "+v"(rd_hi));
            }
            auto trip = [&](auto slot) {
              constexpr int rs = decltype(slot)::value, ws = (rs + PS - 1) % PS;
              issue_next(ws);
              asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NVP * (PS - 1)) : "memory");
              typedef __attribute__((address_space(3))) const unsigned char lds_u8;
              typedef __attribute__((address_space(3))) const float lds_f;
              f32x4 xf[1][2][2];
              float xup[1];
              int ix[1][2];
              lds_cc* const xr[1] = {rowb + 2 * rs * slotb};
              lds_cc* const xu[1] = {upb + 2 * rs * slotb};
#pragma unroll
              for (int u = 0; u < 2; ++u) {
                xf[0][u][0] = ring_row4(xr[0] + u * slotb);
                xf[0][u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                ix[0][u] = (int)*(lds_u8*)(axb + (2 * rs + u) * slotb);
              }
              xup[0] = *(lds_f*)xu[0];
              constexpr bool RX = OCC >= 4;
              train_pair_packed<PACK, DC, TS, 1, XP, RX, CMP, true, false>(
                  a, FP, scr, c, g, xf, xup, ix, acc1, acc2, acc3, acc4, acc2b, acc4b, sq, ab, corr, rows, xr, xu, rd_lo,
                  rd_hi);
            };
            // one copy of each slot's trip: the wave leaves the unrolled body after its last trip
            for (unsigned k = ntrip; k > 0; k -= PS) {
              trip(RingSlot<0>{});
              if (k == 1) break;
              trip(RingSlot<1>{});
            }
            // two rows of row-counting lane group 0 per trip: an exact small integer, as the
            // per-trip adds were
            rows += (g == 0) ? 2.f * (float)ntrip : 0.f;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may land after the ring is retired
          } else {
          int64_t pp = ufirst;
#pragma unroll
          for (int k = 0; k < PS - NPW; ++k) {
            issue_pair(pp, k);
            pp += stride;
          }
          int rs = 0, ws = PS - NPW;
          int64_t pi = ufirst;
          for (; pi + (NPW - 1) * stride < npairs; pi += NPW * stride) {
#pragma unroll
            for (int k = 0; k < NPW; ++k) {
              issue_pair(pp, ws);
              pp += stride;
              ws = ws + 1 == PS ? 0 : ws + 1;
            }
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NVP * (PS - NPW)) : "memory");
            f32x4 xf[NPW][2][2];
            float xup[NPW];
            int ix[NPW][2];
            lds_cc* xr[NPW];
            lds_cc* xu[NPW];
#pragma unroll
            for (int k = 0; k < NPW; ++k) {
              load_pair(rs, xf[k], xup[k], ix[k]);
              xr[k] = (lds_cc*)(ring + 2 * rs * slotb + row_off);
              xu[k] = (lds_cc*)(ring + 2 * rs * slotb + up_off);
              rs = rs + 1 == PS ? 0 : rs + 1;
            }
            constexpr bool RX = XM == 1 && OCC >= 4;
            train_pair_packed<PACK, DC, TS, NPW, XP, RX, CMP, XM == 1>(a, FP, scr, c, g, xf, xup, ix, acc1, acc2,
                                                                       acc3, acc4, acc2b, acc4b, sq, ab, corr,
                                                                       rows, xr, xu);
          }
          if (NPW == 2 && pi < npairs) {   // a last lone pair: the oldest of the PS - NPW in flight
            static_assert(NPW == 1 || PS - NPW - 1 >= 0, "ring depth");
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NVP * (PS - NPW - 1)) : "memory");
            f32x4 xf[1][2][2];
            float xup[1];
            int ix[1][2];
            load_pair(rs, xf[0], xup[0], ix[0]);
            train_pair_packed<PACK, DC, TS, 1, XP, false, CMP, XM == 1>(a, FP, scr, c, g, xf, xup, ix, acc1, acc2,
                                                                        acc3, acc4, acc2b, acc4b, sq, ab, corr,
                                                                        rows);
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may land after the ring is retired
          }
        } else {
        int64_t tp = t0;
#pragma unroll
        for (int k = 0; k < PF - 2; ++k) {
          issue(tp, k);
          tp += stride;
        }
        int rd = 0, wr = PF - 2;
        int64_t t = t0;
        for (; t + stride < nfull; t += 2 * stride) {
          issue(tp, wr);
          issue(tp + stride, wr + 1 == PF ? 0 : wr + 1);
          tp += 2 * stride;
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NV * (PF - 2)) : "memory");
          f32x4 xf[2][2];
          int ix[2];
          ring_tile(rd, xf[0], ix[0]);
          ring_tile(rd + 1 == PF ? 0 : rd + 1, xf[1], ix[1]);
          rd = rd + 2 >= PF ? rd + 2 - PF : rd + 2;
          wr = wr + 2 >= PF ? wr + 2 - PF : wr + 2;
          train_tiles_ilp<PACK, DC, 2>(a, F, scr, c, g, xf, ix, pad1, acc1, acc2, acc3, acc4, sq, ab, corr, rows);
        }
        if (t < nfull) {   // already issued: the oldest of the PF - 2 tiles in flight
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NV * (PF - 3)) : "memory");
          f32x4 xf[1][2];
          int ix[1];
          ring_tile(rd, xf[0], ix[0]);
          train_tiles_ilp<PACK, DC, 1>(a, F, scr, c, g, xf, ix, pad1, acc1, acc2, acc3, acc4, sq, ab, corr, rows);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may land after the ring is retired
        }
      } else {
      int64_t tp = t0;   // tile of the next DMA issue (PF - 1 ahead of t)
#pragma unroll
      for (int k = 0; k < PF - 1; ++k) {
        issue(tp, k);
        tp = next_tile(tp);
      }
      int rd = 0, wr = PF - 1;
      for (int64_t t = t0; t < nfull; t = next_tile(t)) {
        issue(tp, wr);
        tp = next_tile(tp);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NV * (PF - 1)) : "memory");
        f32x4 xf[2], sc[2], sh[2];
        ring_x(a, ring + rd * slotb, c, g, xf);
        if constexpr (XM != 1) norm_lds(norm, g, sc, sh);
        int ix = -1;
        if constexpr (XM == 1) {
          typedef __attribute__((address_space(3))) const unsigned char lds_u8;
          ix = (int)*(lds_u8*)(ring + rd * slotb + 64 * a.D + c);
        }
        rd = rd + 1 == PF ? 0 : rd + 1;
        wr = wr + 1 == PF ? 0 : wr + 1;
        if constexpr (XM == 1) {
          // packed rows are already normalised at ingest: only the features past D
          // (clamped duplicates from ring_x) are zeroed
#pragma unroll
          for (int j = 0; j < 4; ++j) xf[1][j] = (live_hi<DC>(j) && 16 + 4 * g + j < DC) ? xf[1][j] : 0.f;
        } else {
#pragma unroll
          for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              xf[s][j] = (s == 0 || live_hi<DC>(j)) ? fmaf(xf[s][j], sc[s][j], sh[s][j]) : 0.f;
        }
        train_tile<PACK, FAST, false, true, DC, XA>(a, F, scr, c, g, lane, true, xf, pad1, acc1, acc2, acc3, acc4,
                                                    sq, ab, corr, rows, ix);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may land after the ring is retired
      }
    }
  } else {
    f32x4 xnext[2];
    if (first < nfull) fetch_x<VEC>(a, first * 16 + c, g, xnext);
    for (int64_t t = first; t < nfull; t += stride) {
      f32x4 xf[2], sc[2], sh[2];
      norm_lds(norm, g, sc, sh);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[s][j] = fmaf(xnext[s][j], sc[s][j], sh[s][j]);
      if (t + stride < nfull) fetch_x<VEC>(a, (t + stride) * 16 + c, g, xnext);  // prefetch
      train_tile<PACK, FAST, false>(a, F, scr, c, g, lane, true, xf, pad1, acc1, acc2, acc3, acc4, sq, ab, corr,
                                    rows);
    }
  }
  // ragged last tile: handled by the wave that would own tile index nfull (never with packed
  // pairs: that variant runs on whole tiles only)
  if (ILP != 3 && (a.n & 15) && first == nfull % stride) {
    const int64_t r = nfull * 16 + c;
    const bool valid = r < a.n;
    f32x4 xf[2], sc[2], sh[2];
    fetch_x<VEC>(a, r, g, xf);
    norm_lds(norm, g, sc, sh);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) xf[s][j] = valid ? fmaf(xf[s][j], sc[s][j], sh[s][j]) : 0.f;
    train_tile<PACK, FAST, true>(a, F, scr, c, g, lane, valid, xf, pad1, acc1, acc2, acc3, acc4, sq, ab, corr, rows);
  }

  // per-wave slab in LDS (every slot written exactly once per wave)
  __syncthreads();  // all waves done with their transpose scratch
  float* my = smem + wid * NSLOT;
  // MR: the slab indices are derived again from the lane id here (opaque to the compiler), so that
  // they are not carried in registers across the pair loop, which has none to spare
  int ce = c, ge = g;
  if constexpr (MR) {
    int le = threadIdx.x & 63;
    asm volatile("" : "+v"(le));
    ce = le & 15;
    ge = le >> 4;
  }
  if constexpr (ILP == 3) {   // tile 1's halves: dW2 columns n >= 8, dW4 rows m >= 8 (lane groups 2, 3)
    if constexpr (XP == 0) {   // XP >= 1 (MA) holds both halves in acc2 / acc4[0]
      acc2 = ce < 8 ? acc2 : acc2b;
      acc4[0] = ge < 2 ? acc4[0] : acc4b;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = 4 * ge + i;
    my[OFF1 + m * 16 + ce] = acc1[0][i];
    my[OFF1 + (16 + m) * 16 + ce] = acc1[1][i];
    my[OFF2 + m * 16 + ce] = acc2[i];
    my[OFF3 + m * 16 + ce] = acc3[i];
    my[OFF4 + m * 32 + ce] = acc4[0][i] * (2.0f / (float)a.D);
    my[OFF4 + m * 32 + 16 + ce] = acc4[1][i] * (2.0f / (float)a.D);
  }
  sq = wave_sum(sq);
  ab = wave_sum(ab);
  corr = wave_sum(corr);
  rows = wave_sum(rows);
  if (lane == 0) {
    my[NPARAM + 0] = sq;
    my[NPARAM + 1] = ab;
    my[NPARAM + 2] = corr;
    my[NPARAM + 3] = rows;
  }
  __syncthreads();
  float* out = a.partials + (int64_t)blockIdx.x * NSLOT;
  for (int s = threadIdx.x; s < NSLOT; s += WAVES * 64) {
    if constexpr (ILP == 3) {   // packed accumulators -> parameter-image slots
      int s1, s2;
      packed_fold_src<CMP>(s, s1, s2);
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (s1 >= 0) v += smem[w * NSLOT + s1];
        if (s2 >= 0) v += smem[w * NSLOT + s2];
      }
      out[s] = v;
    } else {
      float v = smem[s];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) v += smem[w * NSLOT + s];
      out[s] = v;
    }
  }
}

struct FwdArgs {
  const float* x;
  int64_t n;
  int64_t ld;
  const float* scale;
  const float* shift;
  const float* params;
  float* recon;          // [n, D] or null
  float* score;          // [n] per-row MSE or null
  uint8_t* flag;         // [n] score > threshold or null
  float threshold;
  int D, n1, n2, n3;
  int a1, a2, a3, a4;
  float* metrics;        // [4] += (sum sq err, sum |h1|, correct argmax, rows), or null (evaluate)
};

template <int PACK, bool VEC>
__global__ __launch_bounds__(WAVES * 64) void ae_forward_kernel(FwdArgs fa) {
  AEArgs a{};
  a.x = fa.x; a.n = fa.n; a.ld = fa.ld; a.scale = fa.scale; a.shift = fa.shift; a.params = fa.params;
  a.D = fa.D; a.n1 = fa.n1; a.n2 = fa.n2; a.n3 = fa.n3;
  a.a1 = fa.a1; a.a2 = fa.a2; a.a3 = fa.a3; a.a4 = fa.a4;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  // the reference model takes the train kernel's FAST forward: biases folded into the MFMAs,
  // hidden bias slots injected, prescaled tanh (padded features stay exactly 0)
  constexpr bool FASTF = inject_bias_slots<PACK>();
  Frags F;
  load_frags<FASTF, FASTF, FASTF>(a, c, g, F, false);
  const float pad1 = (g == 3) ? 1.0f : 0.0f;
  f32x4 nsc[2], nsh[2];
  norm_regs(a, g, nsc, nsh);
  const int64_t ntiles = (a.n + 15) >> 4;
  const int64_t stride = (int64_t)gridDim.x * WAVES;
  const float inv_d = 1.0f / (float)a.D;
  float m_sq = 0.f, m_ab = 0.f, m_corr = 0.f, m_rows = 0.f;
  for (int64_t t = (int64_t)blockIdx.x * WAVES + wid; t < ntiles; t += stride) {
    const int64_t r = t * 16 + c;
    const bool valid = r < a.n;
    f32x4 xf[2];
    fetch_x<VEC>(a, r, g, xf);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) xf[s][j] = fmaf(xf[s][j], nsc[s][j], nsh[s][j]);
    bf16x4 xb0, xb1, h1b, h2b, h3b;
    f32x4 h1, h2, h3, y[2];
    if constexpr (FASTF) {
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      f32x4 x1 = xf[1];
      x1[3] += pad1;   // input 31: the constant-1 bias slot (features >= D read 0: scale / shift 0)
      xb0 = pack4(xf[0]);
      xb1 = pack4(x1);
      const f32x4 z1 = mfma32(F.w1t[0], F.w1t[1], xb0, xb1, zero4);
#pragma unroll
      for (int i = 0; i < 4; ++i) h1[i] = tanh_exp2(z1[i]);
      h1b = pack4(h1);
      const f32x4 z2 = mfma16(F.w2t, h1b, zero4);
#pragma unroll
      for (int i = 0; i < 4; ++i) h2[i] = act_fwd(act_of<PACK>(a, 1), z2[i]);
      h2b = pack4(h2);
      const f32x4 z3 = mfma16(F.w3t, h2b, zero4);
#pragma unroll
      for (int i = 0; i < 4; ++i) h3[i] = tanh_exp2(z3[i]);
      h3b = pack4(h3);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x4 z4 = mfma16(F.w4t[t], h3b, zero4);
#pragma unroll
        for (int i = 0; i < 4; ++i) y[t][i] = act_fwd(act_of<PACK>(a, 3), z4[i]);   // 0 past D
      }
    } else {
      forward_tile<PACK>(a, F, g, xf, xb0, xb1, h1, h2, h3, h1b, h2b, h3b, y);
    }
    float se = 0.f;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = 16 * tt + 4 * g + i;
        if (f < a.D) {
          const float e = y[tt][i] - xf[tt][i];
          se = fmaf(e, e, se);
          if (valid && fa.recon) fa.recon[r * a.D + f] = y[tt][i];
        }
      }
    se += __shfl_xor(se, 16, 64);
    se += __shfl_xor(se, 32, 64);
    if (g == 0 && valid) {
      const float sc = se * inv_d;
      if (fa.score) fa.score[r] = sc;
      if (fa.flag) fa.flag[r] = sc > fa.threshold ? 1 : 0;
    }
    if (fa.metrics) {   // Keras evaluate(): the train step's loss terms + accuracy, no backward
      m_sq += (g == 0 && valid) ? se : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) m_ab += (valid && 4 * g + i < a.n1) ? fabsf(h1[i]) : 0.f;
      const int iy = row_argmax_fast<false>(y, a.D, g), ix = row_argmax_fast<false>(xf, a.D, g);
      m_corr += (g == 0 && valid && iy == ix) ? 1.f : 0.f;
      m_rows += (g == 0 && valid) ? 1.f : 0.f;
    }
  }
  if (fa.metrics) {   // one float atomic per wave and metric (evaluation only: order-insensitive sums)
    const float vals[4] = {wave_sum(m_sq), wave_sum(m_ab), wave_sum(m_corr), wave_sum(m_rows)};
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 4; ++k) atomicAdd(fa.metrics + k, vals[k]);
  }
}

}  // namespace

// ----------------------------------------------------------------------------
// Slab reduction + Adam (Keras/TF ResourceApplyAdam semantics).
// ----------------------------------------------------------------------------
namespace {
struct AdamHP {
  float lr, beta1, beta2, eps;
};

enum : int { RA_WRITE_GRAD = 1, RA_ADAM = 2, RA_METRICS = 4, RA_ADVANCE = 8 };

struct CursorAdv {
  int64_t* cursor;   // ring cursor advanced by `step` rows modulo `ring` after the update
  int64_t step;
  int64_t ring;
};

// One Adam update (sml_adam.h: roundings pinned, shared with dense.hip's fused slab-sum update)
__device__ __forceinline__ void adam_update(float tot, float m0, float v0, float p0, float lr_t, const AdamHP& hp,
                                            float gscale, float& mm, float& vv, float& pn) {
  sml::adam_update(tot, m0, v0, p0, lr_t, hp.beta1, hp.beta2, hp.eps, gscale, mm, vv, pn);
}

__device__ __forceinline__ void adam_one(float tot, int slot, int nparam, float* grad_out, float* params, float* m,
                                         float* v, float lr_t, const AdamHP& hp, float gscale, float* metrics_acc,
                                         int flags) {
  if (flags & RA_WRITE_GRAD) grad_out[slot] = tot;
  if (slot < nparam) {
    if (flags & RA_ADAM) {
      float mm, vv, pn;
      adam_update(tot, m[slot], v[slot], params[slot], lr_t, hp, gscale, mm, vv, pn);
      m[slot] = mm;
      v[slot] = vv;
      params[slot] = pn;
    }
  } else if ((flags & RA_METRICS) && metrics_acc) {
    metrics_acc[slot - nparam] += tot;
  }
}

// Block = 16 groups x 16 float4 slot-quads.  Each thread sums its quad over
// G / 16 slabs with 8 independent 16-byte loads in flight, then the 16 groups
// combine in LDS in a fixed order (deterministic).
__global__ __launch_bounds__(256) void reduce_adam_kernel(const float* __restrict__ partials, int G, int S,
                                                          int nparam, float* grad_out, float* params, float* m,
                                                          float* v, const int64_t* iter, AdamHP hp, float gscale,
                                                          float* metrics_acc, int flags, CursorAdv adv) {
  __shared__ f32x4 red[16][16];
  if ((flags & RA_ADVANCE) && adv.cursor && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t nx = adv.cursor[0] + adv.step;
    adv.cursor[0] = nx >= adv.ring ? nx - adv.ring : nx;
  }
  const int q = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int slot0 = (blockIdx.x * 16 + q) * 4;
  // the Adam operands (moments, parameters, step count) are loaded BEFORE the slab sum, so their
  // latency overlaps the partial loads' instead of following it (one HBM round trip less per step)
  float pm[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f}, pp[4] = {0.f, 0.f, 0.f, 0.f};
  float lr_t = 0.f;
  if ((flags & RA_ADAM) && grp == 0 && slot0 < S) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (slot0 + e < nparam) {
        pm[e] = m[slot0 + e];
        pv[e] = v[slot0 + e];
        pp[e] = params[slot0 + e];
      }
    const float t = (float)iter[0];
    lr_t = sml::adam_lr_t(hp.lr, hp.beta1, hp.beta2, t);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (slot0 < S) {
    for (int gi = grp; gi < G; gi += 16 * 8) {
      f32x4 vals[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = gi + 16 * u;
        vals[u] = idx < G ? *reinterpret_cast<const f32x4*>(partials + (int64_t)idx * S + slot0)
                          : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += vals[u];
    }
  }
  red[grp][q] = acc;
  __syncthreads();
  if (grp != 0 || slot0 >= S) return;
  f32x4 tot = red[0][q];
#pragma unroll
  for (int k = 1; k < 16; ++k) tot += red[k][q];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int slot = slot0 + e;
    if (flags & RA_WRITE_GRAD) grad_out[slot] = tot[e];
    if (slot < nparam) {
      if (flags & RA_ADAM) {   // adam_one's arithmetic on the prefetched operands
        float mm, vv, pn;
        adam_update(tot[e], pm[e], pv[e], pp[e], lr_t, hp, gscale, mm, vv, pn);
        m[slot] = mm;
        v[slot] = vv;
        params[slot] = pn;
      }
    } else if ((flags & RA_METRICS) && metrics_acc) {
      metrics_acc[slot - nparam] += tot[e];
    }
  }
}

// The wide-grid step's two reduction launches (slab_sum_kernel level: G -> gy = G / 32 chunk sums,
// then reduce_adam_kernel over the gy sums) in ONE launch.  Grid (S / 256 column blocks, gy chunks):
// every workgroup writes its chunk's sums exactly as the level kernel does, then counts itself in
// its column's counter; the column's last workgroup (release / acquire fences at agent scope: the
// sums come from every XCD's L2) sums the gy chunk sums in reduce_adam_kernel's order -- 16 virtual
// groups k summing chunks k, k + 16, ... then group 0 + ... + group 15 -- and applies Adam.  So the
// result is bit-identical to the two launches whichever workgroup ends last; only who does the
// final sum depends on timing.  The last workgroup re-arms its counter (stream order separates steps).
// Opt-in (SML_AE_FUSED_REDUCE=1): measured 80 us against the two launches' 5.9 + 5.9 us -- each
// workgroup's release fence is a buffer_wbl2 of its XCD's L2, full of the train kernel's slabs.
__global__ __launch_bounds__(256) void slab_adam_kernel(const float* __restrict__ partials, int G, int S, int nparam,
                                                        float* scratch, unsigned* counters, float* grad_out,
                                                        float* params, float* m, float* v, const int64_t* iter,
                                                        AdamHP hp, float gscale, float* metrics_acc, int flags,
                                                        CursorAdv adv) {
  constexpr int CH = 32;   // == dense.hip kSlabChunk (the level kernel's chunk)
  __shared__ f32x4 red[16][64];
  __shared__ int last;
  const int q = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int quad = blockIdx.x * 64 + q;
  const bool on = quad * 4 < S;
  const int gy = gridDim.y;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    f32x4 vals[CH / 4];
    const int g0 = blockIdx.y * CH;
#pragma unroll
    for (int u = 0; u < CH / 4; ++u) {
      const int gi = g0 + grp + 4 * u;
      vals[u] = gi < G ? *reinterpret_cast<const f32x4*>(partials + (int64_t)gi * S + quad * 4)
                       : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < CH / 4; ++u) acc += vals[u];
  }
  red[grp][q] = acc;
  __syncthreads();
  if (grp == 0 && on)
    *reinterpret_cast<f32x4*>(scratch + (int64_t)blockIdx.y * S + quad * 4) = red[0][q] + red[1][q] + red[2][q] + red[3][q];
  __threadfence();   // release: the chunk sums reach the device-coherent level before the count
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(counters + blockIdx.x, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
           (unsigned)gy - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();   // acquire: no stale line of another workgroup's chunk sums
  // virtual groups k = 4 grp + j of reduce_adam_kernel, all 32 loads of a batch in flight at once
  f32x4 a2[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int base = 0; base < gy; base += 16 * 8) {
    f32x4 vals[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = base + 4 * grp + j + 16 * u;
        vals[j][u] = (on && idx < gy) ? *reinterpret_cast<const f32x4*>(scratch + (int64_t)idx * S + quad * 4)
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int u = 0; u < 8; ++u) a2[j] += vals[j][u];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[4 * grp + j][q] = a2[j];
  __syncthreads();
  if (threadIdx.x == 0) counters[blockIdx.x] = 0u;
  if ((flags & RA_ADVANCE) && adv.cursor && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t nx = adv.cursor[0] + adv.step;
    adv.cursor[0] = nx >= adv.ring ? nx - adv.ring : nx;
  }
  if (grp != 0 || !on) return;
  f32x4 tot = red[0][q];
#pragma unroll
  for (int k = 1; k < 16; ++k) tot += red[k][q];
  float lr_t = 0.f;
  if (flags & RA_ADAM) {
    const float t = (float)iter[0];
    lr_t = sml::adam_lr_t(hp.lr, hp.beta1, hp.beta2, t);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    adam_one(tot[e], quad * 4 + e, nparam, grad_out, params, m, v, lr_t, hp, gscale, metrics_acc, flags);
}
}  // namespace

// ----------------------------------------------------------------------------
// host launchers (called from the torch binding)
// ----------------------------------------------------------------------------
namespace sml {

// Every SML_AE_* variable ae_train_launch looks at.  The first three are read once per process;
// the others at every launch (one getenv each per ~1 ms step), so a test can A/B them in one process.
// SML_AE_RING=0 selects the register-prefetch variant (A/B comparisons).
// SML_AE_ROUNDS: residency rounds of the pair variants' grid;
// default 3: 47.05 vs 46.86 (2), 46.17 (1), 46.86 (4) G rows/s (profiles/r02/ilp/rounds)
// SML_AE_DIRECT_OCC=3: the 3-wave build of the direct step (A/B).  Default the 4-wave one (128 VGPRs,
// 39 424 B LDS): 45.9 vs 45.3 G fresh rows/s on one box (profiles/r06/serve/fresh_direct_occ*.json)
// SML_AE_OCC=3|4 picks the waves-per-SIMD variant of the ring kernel.  Default 4:
// 128 VGPRs, 4 workgroups/CU; on MI355X 27.1 vs 25.7 G rows/s at B = 8M
// (profiles/r01_v4/sweep_occ*.log).
// SML_AE_ILP=1|2 picks the one-tile or the tile-pair (train_tiles_ilp, 3 waves/SIMD) loop of
// the headline variant (reference model, D = 18, tile-packed ring).
// Default 3 (packed pairs: 40.4 vs 36.9 G rows/s for the one-tile loop, profiles/r02/ilp);
// the pair variants always run at 3 waves/SIMD, SML_AE_OCC only picks the one-tile variants'.
// SML_AE_DIRECT_PAIRS=0: raw-row steps on the one-tile loop (in-kernel normalise + argmax)
// instead of the packed-pair loop (A/B)
// SML_AE_PAIR_OCC=2|3|4: waves per SIMD (2: two packed pairs per loop iteration) of the packed-pair kernel on the tile-packed ring
// Default 4: 4 waves per SIMD, forward operands through early LDS writes and backward
// ones through the MFMA identity (XP 3) -- 51.6-53.4 vs 48.6-49.5 G rows/s for the round-5 loop
// (3, XP 0) on the same boxes (profiles/r06/SUMMARY.md §1).
// SML_AE_PAIR_XP=0|1|2|3|4|5: the packed-pair weight-gradient operand path (train_pair_packed's XP);
// at SML_AE_PAIR_OCC=4, 0 means 1 (the 4-wave build needs the early writes' registers).  4 (the
// early backward writes, TS 12) and 5 (4 with the lane masks in the read addresses) are built for
// the compact ring at 4 waves only and mean 3 everywhere else.  XP 4 over XP 3: 56.78-57.60 vs
// 55.62-55.67 G rows/s in alternating runs (profiles/r10/early_bwd/SUMMARY.md).  Default 5:
// 54.98-55.28 vs 54.38-54.56 G rows/s for XP 4 (the parent build) in alternating runs, and 57.00-57.28
// vs 56.24-56.53 on another box, bit-identical results; 14 VALU fewer and 4 LDS reads more per trip,
// SQ_WAIT_INST_LDS rises from 232 to 300 cycles per trip and the wave still spends 88 cycles fewer
// in a trip (profiles/r17/mask_reads/SUMMARY.md).
static AETrainKnobs ae_train_knobs() {
  // the variable's first character where it is one of lo..hi, as a number; dflt otherwise
  auto digit = [](const char* name, char lo, char hi, int dflt) {
    const char* e = getenv(name);
    return (e && e[0] >= lo && e[0] <= hi) ? e[0] - '0' : dflt;
  };
  static const AETrainKnobs once = [&] {
    AETrainKnobs k{};
    k.ring = digit("SML_AE_RING", '0', '0', 1) != 0;
    const char* e = getenv("SML_AE_ROUNDS");
    const int r = e ? std::atoi(e) : 3;
    k.rounds = r >= 1 && r <= 8 ? r : 3;
    k.direct_occ = digit("SML_AE_DIRECT_OCC", '3', '3', 4);
    return k;
  }();
  AETrainKnobs k = once;
  k.ilp = digit("SML_AE_ILP", '1', '2', 3);
  k.direct_pairs = digit("SML_AE_DIRECT_PAIRS", '0', '0', 1) != 0;
  k.pair_occ = digit("SML_AE_PAIR_OCC", '2', '4', 4);
  k.pair_xp = digit("SML_AE_PAIR_XP", '0', '5', 5);
  k.occ = digit("SML_AE_OCC", '3', '3', 4);
  return k;
}
// The host sizes its partials buffer for 2 x this many workgroups per CU (16: above the largest
// default grid of any variant, the 4-wave pair variants' 3 rounds x 4 resident = 12); the launcher
// trims the grid it is given to the launched variant's own rounds x residency.
int ae_train_blocks_per_cu() { return 8; }
static int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || n <= 0)
      return 256;
    return n;
  }();
  return cus;
}

int ae_nslot() { return NSLOT; }
int ae_nparam() { return NPARAM; }
int ae_waves_per_block() { return WAVES; }

// What the calling thread's last ae_train_launch ran, for tests that A/B two instances in one
// process: the XP and TS of the 4-wave compact-ring packed-pair instances (-1 for every other
// variant; XP 3, 4 or 5) and the launched instance's static LDS size as the runtime reports it.
struct LastVariant {
  const void* fn = nullptr;
  int xp = -1, ts = -1;
};
static thread_local LastVariant last_variant;
void ae_train_last_variant(int out[3]) {
  out[0] = last_variant.xp;
  out[1] = last_variant.ts;
  out[2] = -1;
  hipFuncAttributes attr{};
  if (last_variant.fn && hipFuncGetAttributes(&attr, last_variant.fn) == hipSuccess) out[2] = (int)attr.sharedSizeBytes;
}

int ae_train_grid(int64_t n, int max_blocks) {
  const int64_t ntiles = (n + 15) / 16;
  int64_t blocks = (ntiles + WAVES - 1) / WAVES;
  if (blocks > max_blocks) blocks = max_blocks;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// the kernel of every row of kAEVariants, in the table's order
#define SML_AE_KERNEL(V) ae_train_kernel<aev::V>,
static void (*const kAETrainKernels[kAEVariantCount])(AEArgs) = {SML_AE_TRAIN_VARIANTS(SML_AE_KERNEL)};
#undef SML_AE_KERNEL

hipError_t ae_train_launch(const float* x, int64_t n, int64_t ld, const float* scale, const float* shift,
                           const float* params, float* partials, int64_t* iter, const int64_t* cursor,
                           const int* dims, const int* acts, float l1, int want_acc, int grid, const uint8_t* xpack,
                           hipStream_t stream, int* grid_used, unsigned xpack_live) {
  AEArgs a{};
  a.x = x; a.n = n; a.ld = ld; a.scale = scale; a.shift = shift; a.params = params;
  a.partials = partials; a.iter = iter; a.cursor = cursor; a.xpack = xpack;
  a.D = dims[0]; a.n1 = dims[1]; a.n2 = dims[2]; a.n3 = dims[3];
  a.a1 = acts[0]; a.a2 = acts[1]; a.a3 = acts[2]; a.a4 = acts[3];
  a.l1 = l1; a.want_acc = want_acc;
  AETrainRequest r{};
  r.pack = acts[0] | (acts[1] << 2) | (acts[2] << 4) | (acts[3] << 6);
  r.D = dims[0]; r.n1 = dims[1]; r.n2 = dims[2]; r.n3 = dims[3];
  r.n = n; r.ld = ld;
  r.want_acc = want_acc != 0; r.has_cursor = cursor != nullptr; r.has_xpack = xpack != nullptr;
  r.x_addr = (unsigned)(reinterpret_cast<uintptr_t>(x) & 15);
  r.xpack_addr = (unsigned)(reinterpret_cast<uintptr_t>(xpack) & 15);
  r.xpack_live = xpack_live;
  const AETrainKnobs k = ae_train_knobs();
  last_variant = LastVariant{};
  const AEVariantRow* v = ae_train_select(r, k);
  if (v == nullptr) return hipErrorInvalidValue;
  const int cap = ae_train_grid_cap(*v, k, device_cus());
  *grid_used = grid < cap ? grid : cap;
  void (*const kern)(AEArgs) = kAETrainKernels[v - kAEVariants];
  // the 4-wave compact-ring pair instances say which of them ran (ae_train_last_variant)
  if (v->xp_noted >= 0) last_variant = LastVariant{reinterpret_cast<const void*>(kern), v->xp_noted, v->ts_noted};
  hipLaunchKernelGGL(kern, dim3(*grid_used), dim3(WAVES * 64), 0, stream, a);
  return hipGetLastError();
}

hipError_t ae_forward_launch(const float* x, int64_t n, int64_t ld, const float* scale, const float* shift,
                             const float* params, float* recon, float* score, uint8_t* flag, float threshold,
                             const int* dims, const int* acts, int max_blocks, hipStream_t stream, float* metrics) {
  FwdArgs a{};
  a.metrics = metrics;
  a.x = x; a.n = n; a.ld = ld; a.scale = scale; a.shift = shift; a.params = params;
  a.recon = recon; a.score = score; a.flag = flag; a.threshold = threshold;
  a.D = dims[0]; a.n1 = dims[1]; a.n2 = dims[2]; a.n3 = dims[3];
  a.a1 = acts[0]; a.a2 = acts[1]; a.a3 = acts[2]; a.a4 = acts[3];
  const int grid = ae_train_grid(n, max_blocks);
  const bool vec = ((ld & 1) == 0) && ((dims[0] & 1) == 0) && dims[0] >= 2 &&
                   ((reinterpret_cast<uintptr_t>(x) & 7) == 0);
  const int pack = acts[0] | (acts[1] << 2) | (acts[2] << 4) | (acts[3] << 6);
  if (pack == PACK_REF) {
    if (vec) hipLaunchKernelGGL((ae_forward_kernel<PACK_REF, true>), dim3(grid), dim3(WAVES * 64), 0, stream, a);
    else hipLaunchKernelGGL((ae_forward_kernel<PACK_REF, false>), dim3(grid), dim3(WAVES * 64), 0, stream, a);
  } else {
    hipLaunchKernelGGL((ae_forward_kernel<PACK_DYN, false>), dim3(grid), dim3(WAVES * 64), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t reduce_adam_launch(const float* partials, int G, int S, int nparam, float* grad_out, float* params,
                              float* m, float* v, const int64_t* iter, float lr, float beta1, float beta2, float eps,
                              float gscale, float* metrics_acc, int flags, int64_t* cursor, int64_t cursor_step,
                              int64_t cursor_ring, hipStream_t stream) {
  AdamHP hp{lr, beta1, beta2, eps};
  CursorAdv adv{cursor, cursor_step, cursor_ring};
  if (S % 4 != 0) return hipErrorInvalidValue;
  const int grid = (S / 4 + 15) / 16;
  hipLaunchKernelGGL(reduce_adam_kernel, dim3(grid), dim3(256), 0, stream, partials, G, S, nparam, grad_out, params,
                     m, v, iter, hp, gscale, metrics_acc, flags, adv);
  return hipGetLastError();
}

int slab_adam_columns(int S) { return (S / 4 + 63) / 64; }

hipError_t slab_adam_launch(const float* partials, int G, int S, int nparam, float* scratch, unsigned* counters,
                            float* grad_out, float* params, float* m, float* v, const int64_t* iter, float lr,
                            float beta1, float beta2, float eps, float gscale, float* metrics_acc, int flags,
                            int64_t* cursor, int64_t cursor_step, int64_t cursor_ring, hipStream_t stream) {
  AdamHP hp{lr, beta1, beta2, eps};
  CursorAdv adv{cursor, cursor_step, cursor_ring};
  if (S % 4 != 0 || G < 1 || counters == nullptr || scratch == nullptr) return hipErrorInvalidValue;
  const int gy = (G + 31) / 32;
  hipLaunchKernelGGL(slab_adam_kernel, dim3(slab_adam_columns(S), gy), dim3(256), 0, stream, partials, G, S, nparam,
                     scratch, counters, grad_out, params, m, v, iter, hp, gscale, metrics_acc, flags, adv);
  return hipGetLastError();
}

}  // namespace sml
