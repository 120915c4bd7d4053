// Large-batch train step for Dense stacks: the bf16 persistent trainer's chunk spread over the machine.
// sml-build: no-packed-fp32
//
// A Keras step of `batch` rows (1 .. 2^24) is TWO launches and no host synchronisation:
//
//   dense_batch_grad_kernel   G workgroups of DMB_NT threads.  The batch is cut into 32-row chunks and
//     workgroup g takes the contiguous span [g n / G, (g + 1) n / G) of the n chunks: a static split, so
//     a result's bits depend on the batch and G alone.  Every chunk runs the phases of
//     dense_minibatch_bf16.hip (sml_dense_mb_bf16_dev.h) with that file's rounding points: bf(h) bf(W),
//     bf(dz) bf(W)^T and bf(h)^T bf(dz) on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; activations,
//     loss, l1 / l2 activity penalties, categorical accuracy and derivatives in fp32; the bias gradient
//     the fp32 column sum of the unrounded dz.  The mean and penalty divisors are the WHOLE batch's.
//   dense_batch_apply_kernel  elementwise over the flat parameters: sums the G slabs in ascending g and
//     applies sml_adam.h in place (or writes the summed gradient), folds the G loss pairs.
//
// What differs from the persistent trainer is who keeps what:
//   * nothing but the weight GRADIENT of the wave's 16x16 tiles lives in registers from launch to exit
//     (8 tiles, 32 VGPRs: MFMA C layout, lane (c, g) = kernel rows i0 + 4g .. + 3 of column j0 + c).  No
//     masters and no Adam moments, so the kernel stays within 128 VGPRs and two workgroups share a CU
//     whenever the plan's LDS is at most 80 KiB.
//   * every workgroup builds the bf16 weight image of DenseMBPlanBF16 (unit-major [up][ip + 8]) itself
//     at launch, from the fp32 masters in `flat`: the image is zeroed, then each thread takes 16-byte
//     quads of a kernel's [in, units] floats and scatters their four roundings.  The plan's words for
//     the bias moments stay unused; the bias and its gradient use the plan's first and fourth array.
//   * rows are staged as in the trainer, the next chunk's loads in flight under the current chunk's
//     phases; past the workgroup's span nothing is loaded.
//   * at the end of its span a workgroup writes ONE slab, slab[g][nflat], in the order of
//     FlatParams.flat: a 16-lane group stores 64 contiguous bytes of a kernel row, padded rows and
//     columns are skipped (their slab words, and those of any float no layer owns, stay the zeros the
//     host allocated), then its bias gradients and its pair (loss share incl. penalties, correct rows).
//     No atomics: every workgroup finishes on its own.
// With G = 1 the arithmetic and its order are the persistent trainer's, so the parameters, moments and
// per-step pairs are bit-identical to dense_mb_bf16_kernel's.
// The kernels synchronise with __syncthreads() only.  Limits and the split: sml_dense_batch.h.
#include "sml_common.h"
#include "sml_ops.h"

#include "sml_adam.h"
#include "sml_dense_mb_bf16_dev.h"

namespace sml {
namespace {

using namespace dmb16;

constexpr int APPLY_NT = 256;

// The launch's bf16 weight image and fp32 biases from the masters.  The image region of the plan
// (every layer's image and bias block, contiguous) is zeroed first: padded inputs and units must read
// as 0.  A kernel's floats w_off .. w_off + in * units - 1 are taken as 16-byte quads aligned in
// `flat`; a quad that straddles the kernel's ends is read element by element.
__device__ __forceinline__ void build_image(lds_t* S, const float* __restrict__ flat, const DenseMBLayer* sL,
                                            const DenseMBLayerPlanBF16* sP, int nl) {
  const int tid = threadIdx.x;
  const int z0 = sP[0].lw, z1 = sP[nl - 1].lb + 16 * sP[nl - 1].up;
  for (int o = z0 + 16 * tid; o < z1; o += 16 * NT) st4(fptr(S, o), f32x4{0.f, 0.f, 0.f, 0.f});
  __syncthreads();
  for (int l = 0; l < nl; ++l) {
    const int units = sL[l].units, w0 = sL[l].w_off, w1 = w0 + sL[l].in * units, ws = sP[l].ws;
    unsigned short* img = reinterpret_cast<unsigned short*>(S + sP[l].lw);
    const int f0 = w0 & ~3;
    for (int fb = f0 + 4 * tid; fb < w1; fb += 4 * NT) {
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      if (fb >= w0 && fb + 4 <= w1) {
        w = ld4(flat + fb);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (fb + e >= w0 && fb + e < w1) w[e] = flat[fb + e];
      }
      // element fb + e is kernel row i, column j; before the kernel's first float j counts up to 0
      int i = fb >= w0 ? (fb - w0) / units : 0;
      int j = fb - w0 - i * units;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (j >= 0 && fb + e < w1) img[j * ws + i] = to_bf16(w[e]);
        if (++j == units) {
          j = 0;
          ++i;
        }
      }
    }
  }
  for (int l = tid >> 7; l < nl; l += NT / DMB_MAXW) {
    const int j = tid & (DMB_MAXW - 1);
    if (sL[l].has_bias && j < sL[l].units) fptr(S, sP[l].lb)[j] = flat[sL[l].b_off + j];
  }
}

__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void dense_batch_grad_kernel(
    const DenseBatchArgs a, const DenseMBPlanBF16 P) {
  extern __shared__ __attribute__((aligned(16))) lds_t S[];
  __shared__ DenseMBLayer sL[DMB_MAXLAYERS];
  __shared__ DenseMBLayerPlanBF16 sP[DMB_MAXLAYERS];
  const int tid = threadIdx.x, nl = a.nl;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, c = lane & 15, g = lane >> 4;
  if (tid == 0) {
#pragma unroll
    for (int l = 0; l < DMB_MAXLAYERS; ++l) {
      sL[l] = a.L[l];
      sP[l] = P.L[l];
    }
  }
  if (tid < P.ntiles) {   // tile table: layer, input block, unit block (unit blocks fastest)
    int l = 0;
    for (int k = 1; k < nl; ++k)
      if (tid >= P.L[k].tile0) l = k;
    const int k = tid - P.L[l].tile0, nj = P.L[l].up >> 4;
    reinterpret_cast<int*>(S + P.ltile)[tid] = (l << 16) | ((k / nj) << 8) | (k % nj);
  }
  if (tid < 3) fptr(S, P.lstat)[STAT_TOT + tid] = 0.0f;
  __syncthreads();
  build_image(S, a.flat, sL, sP, nl);   // visible after the first chunk's barrier

  // ---- the tiles this wave owns: their gradient, and nothing else, stays in registers ----
  f32x4 Tg[SLOTS];
  int ti[SLOTS];
#pragma unroll
  for (int u = 0; u < SLOTS; ++u) {
    const int id = wave + NW * u;
    ti[u] = id < P.ntiles ? __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(S + P.ltile)[id]) : -1;
    Tg[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int O = sL[nl - 1].units, op = sP[nl - 1].up;
  const int chunks = dense_batch_chunks(a.batch), G = (int)gridDim.x, grp = (int)blockIdx.x;
  const int k_first = dense_batch_first_chunk(grp, G, chunks), k_end = dense_batch_first_chunk(grp + 1, G, chunks);
  const float inv_rows = 1.0f / (float)a.batch, inv_n = 1.0f / ((float)a.batch * (float)O);

  // stage_load's step is this launch (s = 0 of 1); s = 1 stages nothing
  Stage st;
  stage_load(a, a, O, 0, k_first, 1, st);
  for (int k = k_first; k < k_end; ++k) {
    const int rows = a.batch - k * CH < CH ? a.batch - k * CH : CH;
    stage_store(S, a, P, op, st);
    stage_load(a, a, O, k + 1 < k_end ? 0 : 1, k + 1, 1, st);
    __syncthreads();
    // ---- forward ----
    for (int l = 0; l < nl; ++l) {
      fwd_layer(S, a.L[l], P.L[l], l == 0 ? P.lxb : P.L[l - 1].lhb, l == 0 ? P.xbs : P.L[l - 1].bs, l == nl - 1, wave, c, g);
      __syncthreads();
    }
    loss_phase(S, sL, sP, nl, P.lyt, P.ys, P.lstat, rows, inv_n, inv_rows);
    __syncthreads();
    // ---- backward ----
    for (int l = nl - 1; l >= 1; --l) {
      bwd_layer(S, P.L[l], a.L[l - 1], P.L[l - 1], rows, inv_rows, wave, c, g);
      __syncthreads();
    }
    // ---- weight gradients into the owners' registers ----
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) {
      TilePos t;
      if (!tile_of(ti[u], t)) continue;
      Tg[u] = wgrad_tile(S, P, t, Tg[u], c, g);
    }
    // ---- bias gradients: fp32 column sums of the unrounded dz, rows ascending ----
    for (int l = tid >> 7; l < nl; l += NT / DMB_MAXW) {
      const int j = tid & (DMB_MAXW - 1), up = sP[l].up;
      if (j >= up || !sL[l].has_bias) continue;
      const float* dp = fptr(S, sP[l].la) + j;
      float* gb = fptr(S, sP[l].lb) + 3 * up + j;
      float sum = *gb;
      for (int r = 0; r < CH; ++r) sum += dp[r * sP[l].hs];
      *gb = sum;
    }
    if (tid < 3) {   // the span's squared error / correct rows / penalty, rows ascending
      float* stt = fptr(S, P.lstat);
      float tot = stt[STAT_TOT + tid];
      for (int r = 0; r < rows; ++r) tot += stt[CH * tid + r];
      stt[STAT_TOT + tid] = tot;
    }
    __syncthreads();
  }

  // ---- the slab: real kernel elements, real biases, the pair ----
  float* slab = a.slab + (int64_t)grp * a.nflat;
#pragma unroll
  for (int u = 0; u < SLOTS; ++u) {
    TilePos t;
    if (!tile_of(ti[u], t)) continue;
    const DenseMBLayer& L = sL[t.l];
    const int j = t.j0 + c;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = t.i0 + 4 * g + e;
      if (i < L.in && j < L.units) slab[(unsigned)(L.w_off + i * L.units + j)] = Tg[u][e];
    }
  }
  for (int l = tid >> 7; l < nl; l += NT / DMB_MAXW) {
    const int j = tid & (DMB_MAXW - 1);
    if (!sL[l].has_bias || j >= sL[l].units) continue;
    slab[(unsigned)(sL[l].b_off + j)] = fptr(S, sP[l].lb)[3 * sP[l].up + j];
  }
  if (tid == 0) {
    const float* tot = fptr(S, P.lstat) + STAT_TOT;
    a.pairs[2 * grp] = tot[0] * inv_n + tot[2] * inv_rows;
    a.pairs[2 * grp + 1] = tot[1];
  }
}

// One thread per 16 bytes of the flat parameters.  The Adam operands are loaded before the slab sum so
// that their latency lies under the slabs'.  Thread 0 of workgroup 0 folds the pairs; the step count
// comes from iter0, which no launch of the call writes, so no workgroup can read a count another has
// already advanced.
__global__ __launch_bounds__(APPLY_NT) void dense_batch_apply_kernel(const DenseBatchApplyArgs a) {
  const int f = 4 * (int)(blockIdx.x * APPLY_NT + threadIdx.x);
  const bool apply = a.flat != nullptr;
  const int64_t t = apply ? a.iter0[0] + a.step + 1 : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float loss = a.pairs[0], ok = a.pairs[1];
    for (int g = 1; g < a.G; ++g) {
      loss += a.pairs[2 * g];
      ok += a.pairs[2 * g + 1];
    }
    a.out[0] = loss;
    a.out[1] = ok;
    if (apply) *a.iter = t;
  }
  if (f >= a.nflat) return;
  f32x4 p = {0.f, 0.f, 0.f, 0.f}, m = p, v = p;
  if (apply) {
    p = ld4(a.flat + f);
    m = ld4(a.m + f);
    v = ld4(a.v + f);
  }
  const float* s = a.slab + f;
  f32x4 tot = ld4(s);
#pragma unroll 8
  for (int g = 1; g < a.G; ++g) tot += ld4(s + (int64_t)g * a.nflat);
  if (!apply) {
    st4(a.grad_out + f, tot);
    return;
  }
  const float lr_t = adam_lr_t(a.lr, a.beta1, a.beta2, (float)t);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float mm, vv, pn;
    adam_update(tot[e], m[e], v[e], p[e], lr_t, a.beta1, a.beta2, a.eps, 1.0f, mm, vv, pn);
    m[e] = mm;
    v[e] = vv;
    p[e] = pn;
  }
  st4(a.flat + f, p);
  st4(a.m + f, m);
  st4(a.v + f, v);
}

}  // namespace

int dense_batch_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      n <= 0)
    return 256;
  return n;
}

// Both launchers are reached through the bindings, which have run dense_batch_check; the tests here are
// for a caller that comes another way.
hipError_t dense_batch_grad_launch(const DenseBatchArgs& a, int G, hipStream_t stream) {
  const DenseMBPlanBF16 P = dense_mb_plan_bf16(a.L, a.nl, a.D, a.y != nullptr);
  if (P.ntiles > DMB_TILES_BF16 || a.batch < 1 || a.batch > DBT_MAXBATCH || a.row0 < 0 || a.row0 + a.batch > a.n ||
      G < 1 || G > dense_batch_chunks(a.batch) || (a.nflat & 3) || (reinterpret_cast<uintptr_t>(a.flat) & 15))
    return hipErrorInvalidValue;
  return launch(dense_batch_grad_kernel, G, (size_t)P.lds_bytes, stream, a, P);
}

hipError_t dense_batch_apply_launch(const DenseBatchApplyArgs& a, hipStream_t stream) {
  if (a.G < 1 || a.nflat < 4 || (a.nflat & 3) || (a.flat == nullptr && a.grad_out == nullptr))
    return hipErrorInvalidValue;
  const int grid = (a.nflat / 4 + APPLY_NT - 1) / APPLY_NT;
  hipLaunchKernelGGL(dense_batch_apply_kernel, dim3(grid), dim3(APPLY_NT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace sml
