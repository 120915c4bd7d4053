// Device code of a 32-row chunk on bf16 MFMAs, shared by the persistent small-batch trainer
// (kernels/dense_minibatch_bf16.hip: one workgroup, state in registers) and the large-batch step
// (kernels/dense_batch.hip: many workgroups, a gradient slab each).  Both run DenseMBPlanBF16
// (sml_dense_mb_plan.h) and the rounding points written at the head of dense_minibatch_bf16.hip:
// operand reads by rows and transposed, a layer's forward and backward product, the store of staged
// rows, the loss phase and the tile table's entries.  Who owns a parameter, what happens to a
// gradient and when Adam runs is in the kernel files.  Row staging from global memory, the penalty
// sum and the row merge, shared with the fp32 kernel too, are in sml_dense_mb_dev.h.
#pragma once

#include "sml_common.h"
#include "sml_ops.h"

#include "sml_dense_mb_dev.h"

namespace sml {
namespace dmb16 {

using namespace dmb;
constexpr int NW = NT / 64, SLOTS = DMB_TILES_BF16 / NW;
static_assert(CH == 32 && NW * SLOTS == DMB_TILES_BF16, "one MFMA K step per chunk; whole tiles per wave");

typedef unsigned char lds_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float* fptr(lds_t* S, int off) { return reinterpret_cast<float*>(S + off); }
__device__ __forceinline__ unsigned short to_bf16(float v) { return (unsigned short)(pack2(v, 0.0f) & 0xffffu); }

__device__ __forceinline__ f32x4 mma(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// MFMA operand read by rows: lane (c, g) gets elements k0 + 8g .. + 7 of row row0 + c of a bf16
// image with `stride` bytes between rows; zeros where k0 + 8g >= kmax
__device__ __forceinline__ s16x8 row8(const lds_t* S, int base, int stride, int row0, int k0, int kmax, int c, int g) {
  const int k = k0 + 8 * g;
  const bool in = k < kmax;
  const s16x8 v = *reinterpret_cast<const s16x8*>(S + base + (row0 + c) * stride + 2 * (in ? k : 0));
  const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return in ? v : z;
}

// MFMA operand read transposed: lane (c, g) gets column col0 + c of the image's rows k0 + 8g .. + 7
// (two ds_read_b64_tr_b16: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p + 3 of a
// 4 x 16 block); zeros where k0 + 8g >= kmax.  All 64 lanes must execute it.
__device__ __forceinline__ s16x8 tr8(lds_t* S, int base, int stride, int k0, int kmax, int col0, int c, int g) {
  const int k = k0 + 8 * g;
  const bool in = k < kmax;
  lds_t* p = S + base + ((in ? k : 0) + (c >> 2)) * stride + 2 * (col0 + 4 * (c & 3));
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)p);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p + 4 * stride));
  const s16x8 v = cat8(lo, hi);
  const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return in ? v : z;
}

// layer output, transposed product: C[unit j0 + 4g + e][row 16 rb + c] = b + sum_i W^T[j][i] h^T[i][r]
__device__ __forceinline__ void fwd_layer(lds_t* S, const DenseMBLayer& L, const DenseMBLayerPlanBF16& P, int lprev,
                                          int sprev, bool last, int wave, int c, int g) {
  const int ntile = (P.up >> 4) * 2;
  for (int t = wave; t < ntile; t += NW) {
    const int j0 = (t >> 1) << 4, r0 = (t & 1) << 4;
    f32x4 acc = ld4(fptr(S, P.lb) + j0 + 4 * g);
    for (int k0 = 0; k0 < P.ip; k0 += 32) {
      const s16x8 wa = row8(S, P.lw, 2 * P.ws, j0, k0, P.ip, c, g);
      const s16x8 hb = row8(S, lprev, 2 * sprev, r0, k0, P.ip, c, g);
      acc = mma(wa, hb, acc);
    }
    f32x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = j0 + 4 * g + e < L.units ? act_fwd(L.act, acc[e]) : 0.0f;
    st4(fptr(S, P.la) + (r0 + c) * P.hs + j0 + 4 * g, h);
    if (!last) *reinterpret_cast<bf16x4*>(S + P.lhb + 2 * ((r0 + c) * P.bs + j0 + 4 * g)) = pack4(h);
  }
}

// gradient of layer l - 1's output from layer l's, transposed product:
// C[input i0 + 4g + e][row 16 rb + c] = sum_j W[i][j] dz^T[j][r]; then dz_{l-1} replaces h_{l-1}
__device__ __forceinline__ void bwd_layer(lds_t* S, const DenseMBLayerPlanBF16& P, const DenseMBLayer& Lp,
                                          const DenseMBLayerPlanBF16& Pp, int rows, float inv_rows, int wave, int c, int g) {
  const int ntile = (P.ip >> 4) * 2;
  const bool pen = Lp.l1 != 0.0f || Lp.l2 != 0.0f;
  for (int t = wave; t < ntile; t += NW) {
    const int i0 = (t >> 1) << 4, r0 = (t & 1) << 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < P.up; k0 += 32) {
      const s16x8 wa = tr8(S, P.lw, 2 * P.ws, k0, P.up, i0, c, g);
      const s16x8 db = row8(S, P.ld, 2 * P.bs, r0, k0, P.up, c, g);
      acc = mma(wa, db, acc);
    }
    float* hp = fptr(S, Pp.la) + (r0 + c) * Pp.hs + i0 + 4 * g;
    const f32x4 h = ld4(hp);
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float gg = acc[e];
      if (pen) gg += pen_grad(Lp.l1, Lp.l2, h[e], inv_rows);
      gg = act_grad(Lp.act, h[e], gg);
      d[e] = (i0 + 4 * g + e < Lp.units && r0 + c < rows) ? gg : 0.0f;
    }
    st4(hp, d);
    *reinterpret_cast<bf16x4*>(S + Pp.ld + 2 * ((r0 + c) * Pp.bs + i0 + 4 * g)) = pack4(d);
  }
}

template <typename Run>
__device__ __forceinline__ void stage_store(lds_t* S, const Run& run, const DenseMBPlanBF16& P, int op, const Stage& st) {
  const int r = threadIdx.x / LPR, q = threadIdx.x % LPR;
  float* xr = fptr(S, P.la0) + r * P.xs;
  unsigned short* xb = reinterpret_cast<unsigned short*>(S + P.lxb) + r * P.xbs;
  float* yr = fptr(S, P.lyt) + r * P.ys;
#pragma unroll
  for (int e = 0; e < SE; ++e) {
    const int c = q + LPR * e;
    if (c < P.dp) {
      xr[c] = st.x[e];
      xb[c] = to_bf16(st.x[e]);
    }
    if (run.y != nullptr && c < op) yr[c] = st.y[e];
  }
}

// per row (LPR lanes each): squared error, categorical accuracy (ties -> lowest index), activity
// penalties; the last layer's output is replaced by its pre-activation gradient (fp32 and bf16)
__device__ __forceinline__ void loss_phase(lds_t* S, const DenseMBLayer* sL, const DenseMBLayerPlanBF16* sP, int nl, int lyt,
                                           int ys, int lstat, int rows, float inv_n, float inv_rows) {
  const int r = threadIdx.x / LPR, q = threadIdx.x % LPR;
  const bool rv = r < rows;
  const float pen = pen_sum(sL, nl, q, [&](int l) { return fptr(S, sP[l].la) + r * sP[l].hs; });
  const DenseMBLayer& L = sL[nl - 1];
  const DenseMBLayerPlanBF16& P = sP[nl - 1];
  const bool lpen = L.l1 != 0.0f || L.l2 != 0.0f;
  float* yrow = fptr(S, P.la) + r * P.hs;
  unsigned short* drow = reinterpret_cast<unsigned short*>(S + P.ld) + r * P.bs;
  const float* trow = fptr(S, lyt) + r * ys;
  float sq = 0.0f, by = -INFINITY, bt = -INFINITY;
  int iy = 1 << 30, it = 1 << 30;
  for (int j = q; j < P.up; j += LPR) {
    const bool valid = rv && j < L.units;
    const float yv = yrow[j], tv = j < L.units ? trow[j] : 0.0f;
    const float e = yv - tv;
    if (valid) {
      sq = fmaf(e, e, sq);
      if (yv > by) { by = yv; iy = j; }
      if (tv > bt) { bt = tv; it = j; }
    }
    float g = 2.0f * e * inv_n;
    if (lpen) g += pen_grad(L.l1, L.l2, yv, inv_rows);
    const float d = valid ? act_grad(L.act, yv, g) : 0.0f;
    yrow[j] = d;
    drow[j] = to_bf16(d);
  }
  row_stats(fptr(S, lstat), r, q, rv, sq, pen, by, iy, bt, it);
}

// the 16x16 tile of a slot of this wave from its table entry (wave-uniform, read once at launch, so
// it lives in SGPRs): false if the slot is empty (entry -1)
struct TilePos {
  int l, i0, j0;
};
__device__ __forceinline__ bool tile_of(int info, TilePos& t) {
  if (info < 0) return false;
  t.l = info >> 16;
  t.i0 = ((info >> 8) & 0xff) << 4;
  t.j0 = (info & 0xff) << 4;
  return true;
}

// one chunk's weight-gradient product of a tile: dW[i][j] += sum_r h^T[i][r] dz[r][j], both operands
// read transposed from the chunk's bf16 images (the input of layer 0 is the staged rows).
// sml_dense_mb_bf16_body.h keeps these five lines as text: at 255 VGPRs the call, though inlined,
// gives the trainer's kernels another register assignment.
__device__ __forceinline__ f32x4 wgrad_tile(lds_t* S, const DenseMBPlanBF16& P, const TilePos& t, f32x4 acc, int c, int g) {
  const int lp = t.l > 0 ? t.l - 1 : 0;
  const int lh = t.l == 0 ? P.lxb : P.L[lp].lhb, sh = t.l == 0 ? P.xbs : P.L[lp].bs;
  const s16x8 ha = tr8(S, lh, 2 * sh, 0, CH, t.i0, c, g);
  const s16x8 db = tr8(S, P.L[t.l].ld, 2 * P.L[t.l].bs, 0, CH, t.j0, c, g);
  return mma(ha, db, acc);
}

}  // namespace dmb16
}  // namespace sml
