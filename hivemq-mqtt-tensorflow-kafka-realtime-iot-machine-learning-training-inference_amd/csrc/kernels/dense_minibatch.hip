// Persistent small-batch trainer for Dense stacks of any depth (table-driven sibling of
// ae_minibatch.hip, state handling of lstm_ref_train.hip).
// sml-build: no-slp  (packed fp32 VALU is no faster here and costs the registers the launch-long
// state needs: with it the kernel gets a private segment)
//
// ONE workgroup of DMB_NT threads runs nsteps sequential Keras steps in one launch: forward, MSE
// loss + activity penalties, categorical accuracy, backward, weight / bias gradients, Adam
// (sml_adam.h).  fp32 end to end; every contraction is a k-ordered fmaf chain whose order is fixed
// by the shapes alone (no atomics), so a fit is bit-reproducible and splitting a launch in two
// gives the same bits.
//
// Memory plan (DenseMBPlan, a pure function of the layer table):
//   * LDS holds the fp32 weight image for the whole launch: per layer the kernel as [ip][ws] rows
//     (widths zero-padded to 4) and the bias [up].  ws is up or up + 4, whichever makes ws / 4
//     odd: the backward pass reads one 16-byte piece of 16 different kernel rows per 16-lane
//     group, and an odd slot stride puts them on 16 different slots.
//   * the batch is walked in chunks of DMB_CHUNK rows: LDS holds the chunk's input, every layer's
//     output and every layer's output gradient (the last layer's gradient overwrites its output),
//     so the activation footprint does not grow with the batch.
//   * thread t owns the 4x4 tiles t, t + DMB_NT, ... of the kernels (DMB_TPT at most; tiles of layer
//     l start at tile0[l], unit quads fastest); the tiles of a kernel's rows 0..3 also own four
//     bias elements.  The owner keeps
//     the tile's gradient accumulator and Adam moments in registers from launch to exit; the
//     gradient accumulates over a step's chunks, then Adam updates the LDS image in place.
//   * the next chunk's rows (of this step or the next) are fetched into registers while the
//     current chunk computes.
//   * padded units are forced to 0 on the way forward and to 0 gradient on the way back, and a
//     padded parameter is never updated or written, so a sigmoid's act(0) = 0.5 cannot leak.
// The kernel waits on nothing outside the workgroup: every loop bound is known at launch.
// That is what lets dense_mb_fleet_kernel run M models of one architecture side by side, workgroup b
// on model sched[b] (sml_dense_fleet.h): the same body (sml_dense_mb_body.h) on rebased arguments.
// What this kernel has in common with its bf16 sibling is not here: the limits, the plan and the
// check in sml_dense_mb_plan.h; row staging, the loss phase's penalty sum and row merge, and the
// launch sequence in sml_dense_mb_dev.h.
#include "sml_common.h"
#include "sml_ops.h"

#include "sml_adam.h"
#include "sml_dense_fleet.h"
#include "sml_dense_mb_dev.h"

#include <type_traits>

namespace sml {
namespace {

using namespace dmb;

// layer output for `rows` rows of the chunk: thread tile = RT rows x 4 units, k ascending
template <int RT>
__device__ __forceinline__ void fwd_layer(float* S, const DenseMBLayer& L, const DenseMBLayerPlan& P, int la_prev,
                                          int rows) {
  const int nq = P.up >> 2, niq = P.ip >> 2, nrt = (rows + RT - 1) / RT;
  for (int t = threadIdx.x; t < nrt * nq; t += NT) {
    const int rt = t / nq, jq = t - rt * nq;
    const float* ap = S + la_prev + rt * RT * P.ip;
    const float* wp = S + P.lw + 4 * jq;
    const f32x4 b = ld4(S + P.lb + 4 * jq);
    f32x4 acc[RT];
#pragma unroll
    for (int e = 0; e < RT; ++e) acc[e] = b;
#pragma nounroll
    for (int iq = 0; iq < niq; ++iq) {
      f32x4 w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = ld4(wp + (4 * iq + k) * P.ws);
#pragma unroll
      for (int e = 0; e < RT; ++e) {
        const f32x4 h = ld4(ap + e * P.ip + 4 * iq);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[e][c] = fmaf(h[k], w[k][c], acc[e][c]);
      }
    }
#pragma unroll
    for (int e = 0; e < RT; ++e) {
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = 4 * jq + c < L.units ? act_fwd(L.act, acc[e][c]) : 0.0f;
      st4(S + P.la + (rt * RT + e) * P.up + 4 * jq, o);
    }
  }
}

// gradient of layer l - 1's output from layer l's: thread tile = RT rows x inputs {q, q + nq,
// q + 2 nq, q + 3 nq}, unit index ascending
template <int RT>
__device__ __forceinline__ void bwd_layer(float* S, const DenseMBLayerPlan& P, const DenseMBLayer& Lp,
                                          const DenseMBLayerPlan& Pp, int rows, float inv_rows) {
  const int nq = P.ip >> 2, njq = P.up >> 2, nrt = (rows + RT - 1) / RT;
  const bool pen = Lp.l1 != 0.0f || Lp.l2 != 0.0f;
  for (int t = threadIdx.x; t < nrt * nq; t += NT) {
    const int rt = t / nq, q = t - rt * nq;
    const float* dp = S + P.ld + rt * RT * P.up;
    const float* wp = S + P.lw + q * P.ws;
    f32x4 acc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma nounroll
    for (int jq = 0; jq < njq; ++jq) {
      f32x4 w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = ld4(wp + e * nq * P.ws + 4 * jq);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const f32x4 d = ld4(dp + r * P.up + 4 * jq);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][e] = fmaf(d[c], w[e][c], acc[r][e]);
      }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const int row = rt * RT + r;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = q + e * nq;
        const float h = S[Pp.la + row * Pp.up + i];
        float g = acc[r][e];
        if (pen) g += pen_grad(Lp.l1, Lp.l2, h, inv_rows);
        g = act_grad(Lp.act, h, g);
        S[Pp.ld + row * Pp.up + i] = (i < Lp.units && row < rows) ? g : 0.0f;
      }
    }
  }
}

// The larger row tile halves the LDS reads per fmaf; it is taken while it still leaves every SIMD
// a wave of work.  (A 4-row tile does not fit the registers left beside the launch-long state.)
template <typename F>
__device__ __forceinline__ void by_row_tile(int rows, int nq, F&& f) {
  if (((rows + 1) >> 1) * nq >= 256) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 1>{});
}

template <typename Run>
__device__ __forceinline__ void stage_store(float* S, const DenseMBArgs& a, const Run& run, int op, const Stage& st) {
  const int r = threadIdx.x / LPR, q = threadIdx.x % LPR;
#pragma unroll
  for (int e = 0; e < SE; ++e) {
    const int c = q + LPR * e;
    if (c < a.P.dp) S[a.P.la0 + r * a.P.dp + c] = st.x[e];
    if (run.y != nullptr && c < op) S[a.P.lyt + r * op + c] = st.y[e];
  }
}

// per row (LPR lanes each): squared error, categorical accuracy (ties -> lowest index), activity
// penalties; the last layer's output is replaced by its pre-activation gradient
__device__ __forceinline__ void loss_phase(float* S, const DenseMBLayer* sL, const DenseMBLayerPlan* sP, int nl, int lyt,
                                           int lstat, int rows, float inv_n, float inv_rows) {
  const int r = threadIdx.x / LPR, q = threadIdx.x % LPR;
  const bool rv = r < rows;
  const float pen = pen_sum(sL, nl, q, [&](int l) { return S + sP[l].la + r * sP[l].up; });
  const DenseMBLayer& L = sL[nl - 1];
  const DenseMBLayerPlan& P = sP[nl - 1];
  const bool lpen = L.l1 != 0.0f || L.l2 != 0.0f;
  float* yrow = S + P.la + r * P.up;
  const float* trow = S + lyt + r * P.up;
  float sq = 0.0f, by = -INFINITY, bt = -INFINITY;
  int iy = 1 << 30, it = 1 << 30;
  for (int j = q; j < P.up; j += LPR) {
    const float yv = yrow[j], tv = trow[j];
    const bool valid = rv && j < L.units;
    const float e = yv - tv;
    if (valid) {
      sq = fmaf(e, e, sq);
      if (yv > by) { by = yv; iy = j; }
      if (tv > bt) { bt = tv; it = j; }
    }
    float g = 2.0f * e * inv_n;
    if (lpen) g += pen_grad(L.l1, L.l2, yv, inv_rows);
    yrow[j] = valid ? act_grad(L.act, yv, g) : 0.0f;
  }
  row_stats(S + lstat, r, q, rv, sq, pen, by, iy, bt, it);
}

// one owned 4x4 tile: where it sits, and its state for the whole launch
struct Tile {
  int l, iq, jq;       // layer (-1: none), input quad, unit quad
  f32x4 g[4], m[4], v[4], gb, mb, vb;
};

// fw(e, c, flat index, LDS address) for the tile's kernel elements, fb(c, flat index, LDS address)
// for its bias elements.  REAL: only the real ones (parameter loads and stores).  Otherwise the
// padded ones too: their gradient and moments are exactly 0 (a padded input is 0 on the way
// forward, a padded unit's gradient 0 on the way back), so Adam leaves them 0 and the update needs
// no per-element predicate.
template <bool REAL, typename FW, typename FB>
__device__ __forceinline__ void tile_params(float* S, const Tile& T, const DenseMBLayer* sL, const DenseMBLayerPlan* sP,
                                            FW&& fw, FB&& fb) {
  // the tile's place goes through an empty asm: addresses and predicates are then worked out
  // again at each use (launch, every Adam, exit) instead of being carried, and spilled, across
  // the whole launch
  int tl = T.l, iq = T.iq, jq = T.jq;
  asm volatile("" : "+v"(tl), "+v"(iq), "+v"(jq));
  if (tl < 0) return;
  const DenseMBLayer& L = sL[tl];
  const DenseMBLayerPlan& P = sP[tl];
  float* wl = S + P.lw + 4 * iq * P.ws + 4 * jq;
  const unsigned wflat = (unsigned)(L.w_off + 4 * iq * L.units + 4 * jq);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (!REAL || (4 * iq + e < L.in && 4 * jq + c < L.units))
        fw(e, c, wflat + (unsigned)(e * L.units + c), wl + e * P.ws + c);
    // one tile row's memory operations at a time: hoisting all of a thread's 40 loads (or Adam
    // updates) above their uses costs more registers than the launch-long state leaves
    asm volatile("" ::: "memory");
  }
  if (iq == 0 && L.has_bias) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (!REAL || 4 * jq + c < L.units) fb(c, (unsigned)(L.b_off + 4 * jq + c), S + P.lb + 4 * jq + c);
  }
}

__global__ __launch_bounds__(NT) void dense_mb_kernel(const DenseMBArgs a) {
  const DenseMBArgs& run = a;
#include "sml_dense_mb_body.h"
}

// Fleet entry: workgroup b trains model sched[b] of M models of one architecture (sml_dense_fleet.h).
// The rebase happens once, before the first load; from then on this is the single-model launch, and
// the workgroup leaves when its own model is done.
__global__ __launch_bounds__(NT) void dense_mb_fleet_kernel(const DenseMBArgs a, const DenseMBFleetModel* __restrict__ models,
                                                            const int32_t* __restrict__ sched, const int64_t stride) {
  const DenseMBRun run = fleet_run(SML_DENSE_MB_SINGLE_RUN(a), a.ldx, a.ldy, models, sched, stride);
#include "sml_dense_mb_body.h"
}

// what both launchers refuse before they look at the precision
bool launchable(const DenseMBArgs& a, int64_t nflat) {
  return a.nsteps >= 1 && dense_mb_check(a.L, a.nl, a.D, a.batch, nflat, a.y != nullptr, a.precision).empty();
}

}  // namespace

hipError_t dense_mb_launch(DenseMBArgs a, hipStream_t stream) {
  if (!launchable(a, INT64_MAX) || a.row0 < 0 || a.row0 >= a.n) return hipErrorInvalidValue;
  if (a.precision == DMB_BF16) return dense_mb_launch_bf16(a, stream);
  a.P = dense_mb_plan(a.L, a.nl, a.D, a.y != nullptr);
  return launch(dense_mb_kernel, 1, sizeof(float) * (size_t)a.P.lds_floats, stream, a);
}

hipError_t dense_mb_fleet_launch(DenseMBArgs a, const DenseMBFleetModel* models, const int32_t* sched, int M,
                                 int64_t stride, hipStream_t stream) {
  if (!launchable(a, stride) || M < 1 || models == nullptr || sched == nullptr) return hipErrorInvalidValue;
  if (a.precision == DMB_BF16) return dense_mb_fleet_launch_bf16(a, models, sched, M, stride, stream);
  a.P = dense_mb_plan(a.L, a.nl, a.D, a.y != nullptr);
  return launch(dense_mb_fleet_kernel, M, sizeof(float) * (size_t)a.P.lds_floats, stream, a, models, sched, stride);
}

}  // namespace sml
