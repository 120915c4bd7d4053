// What the fp32 and the bf16 kernel of the persistent small-batch Dense trainer share
// (kernels/dense_minibatch.hip, kernels/dense_minibatch_bf16.hip): device helpers for the row phases
// and ONE host helper, the launch sequence of the four launchers (dmb::launch, at the end).  Where
// the two differ -- the LDS images, the contractions, who owns a parameter -- is in the kernel files
// and their bodies (sml_dense_mb_body.h, sml_dense_mb_bf16_body.h).
//
// A "row phase" is a part of a chunk's work that goes by rows, not by tiles: staging a chunk's rows
// from global memory, and the loss.  LPR lanes serve each of the chunk's CH rows; a thread's row is
// threadIdx.x / LPR and it takes the columns threadIdx.x % LPR, + LPR, + 2 LPR, ...  The LPR lanes
// of a row are neighbours in one wave, so a row's sums and argmaxes are merged by lane shuffles.
#pragma once

#include "sml_common.h"
#include "sml_ops.h"

namespace sml {
namespace dmb {

constexpr int NT = DMB_NT, CH = DMB_CHUNK;
constexpr int STAT_SQ = 0, STAT_OK = CH, STAT_PEN = 2 * CH, STAT_TOT = 3 * CH;   // floats from lstat
constexpr int LPR = NT / CH;            // lanes per row in the row phases
constexpr int SE = DMB_MAXW / LPR;      // elements per lane of a row
static_assert(LPR * CH == NT && LPR <= 32 && (LPR & (LPR - 1)) == 0 && SE * LPR == DMB_MAXW, "row phases: lanes per row");
static_assert(ACT_LINEAR == 0 && ACT_SIGMOID == DMB_ACT_LAST, "dense_mb_check takes the activation codes act_fwd knows");

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// d(l1 * |h| + l2 * h^2) / dh, divided by the step's rows as Keras does
__device__ __forceinline__ float pen_grad(float l1, float l2, float h, float inv_rows) {
  const float sg = h > 0.0f ? 1.0f : h < 0.0f ? -1.0f : 0.0f;
  return (l1 * sg + 2.0f * l2 * h) * inv_rows;
}

// rows of one chunk on their way from global memory to LDS (each kernel file has its own stage_store)
struct Stage {
  float x[SE], y[SE];
};

template <typename Run>
__device__ __forceinline__ void stage_load(const DenseMBArgs& a, const Run& run, int O, int s, int k, int steps, Stage& st) {
  const int r = threadIdx.x / LPR, q = threadIdx.x % LPR;
  int rows = 0;
  int64_t pos = 0;
  if (s < steps) {
    const int64_t base = run.row0 + (int64_t)s * a.batch;
    const int64_t left = run.n - base;
    const int rows_s = left < a.batch ? (int)left : a.batch;
    rows = rows_s - k * CH < CH ? rows_s - k * CH : CH;
    pos = base + k * CH + r;
  }
  const bool rv = r < rows;
  int64_t src = 0;
  if (rv) {
    src = run.order ? (int64_t)run.order[pos] : pos;
    src = src < 0 ? 0 : src >= run.n ? run.n - 1 : src;
  }
#pragma unroll
  for (int e = 0; e < SE; ++e) {
    const int c = q + LPR * e;
    st.x[e] = (rv && c < a.D) ? run.x[src * a.ldx + c] : 0.0f;
    st.y[e] = (run.y != nullptr && rv && c < O) ? run.y[src * a.ldy + c] : 0.0f;
  }
}

// A row's activity penalties, this lane's share: sum over the layers with a regulariser of
// l1 * sum |h| + l2 * sum h^2 over the columns q, q + LPR, ...; hrow(l) is this row of layer l's fp32
// output in LDS
template <typename HRow>
__device__ __forceinline__ float pen_sum(const DenseMBLayer* sL, int nl, int q, HRow&& hrow) {
  float pen = 0.0f;
  for (int l = 0; l < nl; ++l) {
    const float l1 = sL[l].l1, l2 = sL[l].l2;
    if (l1 == 0.0f && l2 == 0.0f) continue;
    float s1 = 0.0f, s2 = 0.0f;
    const float* hr = hrow(l);
    for (int j = q; j < sL[l].units; j += LPR) {
      const float h = hr[j];
      s1 += fabsf(h);
      s2 = fmaf(h, h, s2);
    }
    pen += l1 * s1 + l2 * s2;
  }
  return pen;
}

// The LPR lanes of row r merge their squared error, penalty and the two argmaxes (output: by at iy,
// target: bt at it; ties -> lowest index), and lane q == 0 writes the row's three statistics (zeros
// for an absent row, rv false)
__device__ __forceinline__ void row_stats(float* stat, int r, int q, bool rv, float sq, float pen, float by, int iy, float bt,
                                          int it) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) {
    sq += __shfl_xor(sq, o, 64);
    pen += __shfl_xor(pen, o, 64);
    const float oy = __shfl_xor(by, o, 64), ot = __shfl_xor(bt, o, 64);
    const int oiy = __shfl_xor(iy, o, 64), oit = __shfl_xor(it, o, 64);
    if (oy > by || (oy == by && oiy < iy)) { by = oy; iy = oiy; }
    if (ot > bt || (ot == bt && oit < it)) { bt = ot; it = oit; }
  }
  if (q == 0) {
    stat[STAT_SQ + r] = rv ? sq : 0.0f;
    stat[STAT_OK + r] = (rv && iy == it) ? 1.0f : 0.0f;
    stat[STAT_PEN + r] = rv ? pen : 0.0f;
  }
}

// Host: the launch sequence of all four kernels (more than 64 KiB of dynamic LDS has to be allowed first).
template <typename Kernel, typename... Args>
inline hipError_t launch(Kernel* kernel, int grid, size_t lds, hipStream_t stream, const Args&... args) {
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), lds, stream, args...);
  return hipGetLastError();
}

}  // namespace dmb
}  // namespace sml
