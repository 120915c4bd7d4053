// Persistent small-batch trainer for Dense stacks of any depth with every contraction on
// v_mfma_f32_16x16x32_bf16 (sibling of dense_minibatch.hip: same launch shape, table, chunks,
// outputs and Adam; opt-in through DenseMBArgs::precision).
//
// ONE workgroup of DMB_NT threads (8 waves) runs nsteps sequential Keras steps in one launch.
// Rounding points (bf = round to nearest even bf16; everything else fp32):
//   forward   z_l = b_l + sum_k bf(h_{l-1}[r,k]) bf(W_l[k,j]),  h_l = act(z_l) in fp32, h_0 = x;
//             the fp32 h_l feeds the loss, the penalties, the accuracy and the activation derivative
//   backward  g_{l-1}[r,i] = sum_j bf(dz_l[r,j]) bf(W_l[i,j]),  dz_{l-1} = act'(h_{l-1}) (g_{l-1} + penalty) in fp32
//   weights   dW_l[i,j] = sum_r bf(h_{l-1}[r,i]) bf(dz_l[r,j]): K is the chunk's 32 rows, one MFMA per
//             16x16 tile per chunk, accumulated in fp32 over the chunks of a step
//   bias      db_l[j] = the fp32 column sum of the UNROUNDED dz_l, rows ascending (db_bf16 = False in
//             the test oracle)
//   Adam      sml_adam.h on fp32 masters; bf(W) is re-derived from the master after every update
//
// Memory plan (DenseMBPlanBF16, a pure function of the layer table; widths zero-padded to 16):
//   * wave w owns the 16x16 kernel tiles w, w + 8, ... (8 at most) in the MFMA C layout (lane (c, g):
//     kernel rows i0 + 4g .. + 3, column j0 + c) and keeps their fp32 master, gradient and both Adam
//     moments in registers from launch to exit: 128 VGPRs of state.
//   * LDS holds ONE bf16 weight image per layer, unit-major [up][ip + 8]: the forward pass reads its
//     rows (ds_read_b128), the backward pass reads it transposed (ds_read_b64_tr_b16).
//   * per 32-row chunk LDS holds the fp32 output of every layer (overwritten in place by its fp32
//     pre-activation gradient once that is known), a bf16 image of every layer input and a bf16
//     image of every pre-activation gradient, all [row][unit]: read by rows as the forward /
//     backward operand and transposed as the two weight-gradient operands.
//   * biases, their moments and gradients are fp32 in LDS, one thread per element.
//   * row strides carry 16 bytes of padding, so 16 rows' 16-byte pieces fall on different banks.
//   * the products are computed transposed (units or inputs on the C rows, batch rows on the lanes),
//     so a lane ends with four consecutive units of one row: one 16-byte and one 8-byte LDS store.
//   * padded units are forced to 0 on the way forward and padded units / rows to 0 gradient on the
//     way back, so padded parameters see exactly 0 gradient, stay 0 and are never written back
//     (sigmoid(0) = 0.5 cannot leak).  Every chunk computes all 32 rows: absent rows are zero inputs.
// Every transposed read is executed by all 64 lanes of every wave (wave-uniform control flow; out-of-
// range K pieces read a clamped address and are replaced by zeros).  The kernel synchronises with
// __syncthreads() only and every loop bound is known at launch.  dense_mb_bf16_fleet_kernel runs M models
// of one architecture side by side, workgroup b on model sched[b] (sml_dense_fleet.h): the same body
// (sml_dense_mb_bf16_body.h) on rebased arguments.  The limits, the plan and the check are in
// sml_dense_mb_plan.h; row staging, the loss phase's penalty sum and row merge, and the launch
// sequence, shared with the fp32 kernel, in sml_dense_mb_dev.h.
#include "sml_common.h"
#include "sml_ops.h"

#include "sml_adam.h"
#include "sml_dense_fleet.h"
#include "sml_dense_mb_dev.h"

namespace sml {
namespace {

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

__global__ __launch_bounds__(NT) void dense_mb_bf16_kernel(const DenseMBArgs a, const DenseMBPlanBF16 P) {
  const DenseMBArgs& run = a;
#include "sml_dense_mb_bf16_body.h"
}

// Fleet entry: workgroup b trains model sched[b] of M models of one architecture (sml_dense_fleet.h);
// rebased once before the first load, then the single-model launch.  Nothing outside the workgroup
// is waited on.
__global__ __launch_bounds__(NT) void dense_mb_bf16_fleet_kernel(const DenseMBArgs a, const DenseMBPlanBF16 P,
                                                                 const DenseMBFleetModel* __restrict__ models,
                                                                 const int32_t* __restrict__ sched, const int64_t stride) {
  const DenseMBRun run = fleet_run(SML_DENSE_MB_SINGLE_RUN(a), a.ldx, a.ldy, models, sched, stride);
#include "sml_dense_mb_bf16_body.h"
}

}  // namespace

// Both are reached through dense_mb_launch / dense_mb_fleet_launch, which have run dense_mb_check.  Its
// MAX_PARAMS_BF16 limit already keeps ntiles within the DMB_TILES_BF16 the waves can own; the test
// here is for a caller that comes another way.
hipError_t dense_mb_launch_bf16(const DenseMBArgs& a, hipStream_t stream) {
  const DenseMBPlanBF16 P = dense_mb_plan_bf16(a.L, a.nl, a.D, a.y != nullptr);
  if (P.ntiles > DMB_TILES_BF16) return hipErrorInvalidValue;
  return launch(dense_mb_bf16_kernel, 1, (size_t)P.lds_bytes, stream, a, P);
}

hipError_t dense_mb_fleet_launch_bf16(const DenseMBArgs& a, const DenseMBFleetModel* models, const int32_t* sched, int M,
                                      int64_t stride, hipStream_t stream) {
  const DenseMBPlanBF16 P = dense_mb_plan_bf16(a.L, a.nl, a.D, a.y != nullptr);
  if (P.ntiles > DMB_TILES_BF16 || M < 1) return hipErrorInvalidValue;
  return launch(dense_mb_bf16_fleet_kernel, M, (size_t)P.lds_bytes, stream, a, P, models, sched, stride);
}

}  // namespace sml
