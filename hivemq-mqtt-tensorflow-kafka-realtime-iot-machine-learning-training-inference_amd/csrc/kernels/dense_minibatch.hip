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
#include "sml_common.h"
#include "sml_ops.h"

#include "sml_adam.h"
#include "sml_dense_fleet.h"

#include <string>
#include <type_traits>

namespace sml {
namespace {

constexpr int NT = DMB_NT, CH = DMB_CHUNK;
constexpr int STAT_SQ = 0, STAT_OK = CH, STAT_PEN = 2 * CH, STAT_TOT = 3 * CH;   // floats from lstat

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// d(l1 * |h| + l2 * h^2) / dh, divided by the step's rows as Keras does
__device__ __forceinline__ float pen_grad(float l1, float l2, float h, float inv_rows) {
  const float sg = h > 0.0f ? 1.0f : h < 0.0f ? -1.0f : 0.0f;
  return (l1 * sg + 2.0f * l2 * h) * inv_rows;
}

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

// rows of one chunk on their way from global memory to LDS: row tid / LPR, columns tid % LPR + LPR e
constexpr int LPR = NT / CH;            // lanes per row in the staging and loss phases
constexpr int SE = DMB_MAXW / LPR;      // elements per lane of a row
static_assert(LPR * CH == NT && LPR <= 32 && (LPR & (LPR - 1)) == 0 && SE * LPR == DMB_MAXW, "row phases: lanes per row");
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
  float pen = 0.0f;
  for (int l = 0; l < nl; ++l) {
    const float l1 = sL[l].l1, l2 = sL[l].l2;
    if (l1 == 0.0f && l2 == 0.0f) continue;
    float s1 = 0.0f, s2 = 0.0f;
    for (int j = q; j < sL[l].units; j += LPR) {
      const float h = S[sP[l].la + r * sP[l].up + j];
      s1 += fabsf(h);
      s2 = fmaf(h, h, s2);
    }
    pen += l1 * s1 + l2 * s2;
  }
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
    S[lstat + STAT_SQ + r] = rv ? sq : 0.0f;
    S[lstat + STAT_OK + r] = (rv && iy == it) ? 1.0f : 0.0f;
    S[lstat + STAT_PEN + r] = rv ? pen : 0.0f;
  }
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

constexpr int pad4(int n) { return (n + 3) / 4 * 4; }
constexpr int STATIC_LDS = 1024;   // the kernel's layer table copy, rounded up

}  // namespace

DenseMBPlan dense_mb_plan(const DenseMBLayer* L, int nl, int D, bool own_targets) {
  DenseMBPlan P{};
  int off = 0, tiles = 0;
  P.dp = pad4(D);
  P.la0 = off;
  off += CH * P.dp;
  P.wimg0 = off;
  int prev = P.dp;
  for (int l = 0; l < nl; ++l) {
    DenseMBLayerPlan& q = P.L[l];
    q.ip = prev;
    q.up = pad4(L[l].units);
    q.ws = ((q.up >> 2) & 1) ? q.up : q.up + 4;
    q.lw = off;
    off += q.ip * q.ws;
    q.lb = off;
    off += q.up;
    q.tile0 = tiles;
    tiles += (q.ip >> 2) * (q.up >> 2);
    prev = q.up;
  }
  P.wimg1 = off;
  for (int l = 0; l < nl; ++l) {
    P.L[l].la = off;
    off += CH * P.L[l].up;
  }
  for (int l = 0; l < nl; ++l) {
    if (l == nl - 1) {
      P.L[l].ld = P.L[l].la;
    } else {
      P.L[l].ld = off;
      off += CH * P.L[l].up;
    }
  }
  if (own_targets) {
    P.lyt = off;
    off += CH * prev;
  } else {
    P.lyt = P.la0;
  }
  P.lstat = off;
  off += 4 * CH;
  P.ntiles = tiles;
  P.lds_floats = off;
  return P;
}

const char* dense_mb_check(const DenseMBLayer* L, int nl, int D, int batch, int64_t nflat, bool own_targets,
                           int precision) {
  static thread_local std::string why;
  why.clear();
  auto fail = [&](std::string s) {
    why = std::move(s);
    return why.c_str();
  };
  if (precision != DMB_FP32 && precision != DMB_BF16)
    return fail("precision " + std::to_string(precision) + " is neither fp32 (0) nor bf16 (1)");
  const bool bf16 = precision == DMB_BF16;
  auto pad = [&](int n) { return bf16 ? (n + 15) / 16 * 16 : pad4(n); };
  if (nl < 1 || nl > DMB_MAXLAYERS)
    return fail(std::to_string(nl) + " Dense layers: the persistent trainer takes 1.." + std::to_string(DMB_MAXLAYERS) +
                " (MAX_LAYERS)");
  if (batch < 1 || batch > DMB_MAXBATCH)
    return fail("batch " + std::to_string(batch) + " is outside 1.." + std::to_string(DMB_MAXBATCH) + " (MAX_BATCH)");
  if (D < 1 || D > DMB_MAXW)
    return fail("input width " + std::to_string(D) + " is outside 1.." + std::to_string(DMB_MAXW) + " (MAX_WIDTH)");
  int prev = D;
  int64_t padded = 0;
  for (int l = 0; l < nl; ++l) {
    if (L[l].in != prev) return fail("layer " + std::to_string(l) + " does not take the previous layer's width");
    if (L[l].units < 1 || L[l].units > DMB_MAXW)
      return fail("layer " + std::to_string(l) + " has " + std::to_string(L[l].units) + " units: the limit is " +
                  std::to_string(DMB_MAXW) + " (MAX_WIDTH)");
    if (L[l].act < ACT_LINEAR || L[l].act > ACT_SIGMOID) return fail("layer " + std::to_string(l) + ": unknown activation");
    const int64_t nw = (int64_t)L[l].in * L[l].units;
    if (L[l].w_off < 0 || L[l].w_off + nw > nflat ||
        (L[l].has_bias && (L[l].b_off < 0 || (int64_t)L[l].b_off + L[l].units > nflat)))
      return fail("layer " + std::to_string(l) + ": parameter offsets outside the flat buffer");
    padded += (int64_t)pad(L[l].in) * pad(L[l].units);
    prev = L[l].units;
  }
  if (bf16 && padded > DMB_MAXPARAMS_BF16)
    return fail(std::to_string(padded) + " kernel elements (widths rounded up to 16): the limit is " +
                std::to_string(DMB_MAXPARAMS_BF16) + " (MAX_PARAMS_BF16)");
  if (!bf16 && padded > DMB_MAXPARAMS)
    return fail(std::to_string(padded) + " kernel elements (widths rounded up to 4): the limit is " +
                std::to_string(DMB_MAXPARAMS) + " (MAX_PARAMS)");
  if (!own_targets && prev != D) return fail("y = x needs as many output units as inputs");
  const int64_t need = (bf16 ? (int64_t)dense_mb_plan_bf16(L, nl, D, own_targets).lds_bytes
                             : (int64_t)dense_mb_plan(L, nl, D, own_targets).lds_floats * 4) + STATIC_LDS;
  if (need > DMB_LDS_BYTES)
    return fail(std::to_string(need) + " bytes of LDS: the limit is " + std::to_string(DMB_LDS_BYTES) + " (LDS_BYTES)");
  return "";
}

hipError_t dense_mb_launch(DenseMBArgs a, hipStream_t stream) {
  const bool own_targets = a.y != nullptr;
  if (dense_mb_check(a.L, a.nl, a.D, a.batch, INT64_MAX, own_targets, a.precision)[0] != 0) return hipErrorInvalidValue;
  if (a.nsteps < 1 || a.row0 < 0 || a.row0 >= a.n) return hipErrorInvalidValue;
  if (a.precision == DMB_BF16) return dense_mb_launch_bf16(a, stream);
  a.P = dense_mb_plan(a.L, a.nl, a.D, own_targets);
  const size_t lds = sizeof(float) * (size_t)a.P.lds_floats;
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dense_mb_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(dense_mb_kernel, dim3(1), dim3(NT), lds, stream, a);
  return hipGetLastError();
}

hipError_t dense_mb_fleet_launch(DenseMBArgs a, const DenseMBFleetModel* models, const int32_t* sched, int M,
                                 int64_t stride, hipStream_t stream) {
  const bool own_targets = a.y != nullptr;
  if (dense_mb_check(a.L, a.nl, a.D, a.batch, stride, own_targets, a.precision)[0] != 0) return hipErrorInvalidValue;
  if (M < 1 || a.nsteps < 1 || models == nullptr || sched == nullptr) return hipErrorInvalidValue;
  if (a.precision == DMB_BF16) return dense_mb_fleet_launch_bf16(a, models, sched, M, stride, stream);
  a.P = dense_mb_plan(a.L, a.nl, a.D, own_targets);
  const size_t lds = sizeof(float) * (size_t)a.P.lds_floats;
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dense_mb_fleet_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(dense_mb_fleet_kernel, dim3(M), dim3(NT), lds, stream, a, models, sched, stride);
  return hipGetLastError();
}

}  // namespace sml
