// Fused fp32 train step of the MNIST classifier at batch 1..32: two launches per Keras step.
//
// Reference: python-scripts/tensorflow-kafka-mnist.py:39-47 (batch 1) and
// confluent-tensorflow-io-kafka-simplified.py:10-29 (Keras default batch 32) --
// Flatten -> Dense(H, relu) -> [Dropout] -> Dense(C, softmax), sparse categorical cross-entropy, Adam.
// The layer kernels (mlp.hip) take eight launches for such a step; at these batches that is all
// launch latency.  Here a step is
//
//   mlp_step_fwd_kernel  h = dropout(relu(x . W1 + b1)).  One workgroup per 64 hidden units stages the
//     step's rows (gathered through the epoch's permutation, uint8 scaled by 1/255) into LDS as fp32
//     and computes its units transposed on v_mfma_f32_16x16x4_f32: units on M, rows on N.  The eight
//     waves split k; lane (c, g) loads W1[4 ks + g][64 ub + 4c .. 4c + 3] with one 16-byte load that
//     feeds four MFMAs (component r serves the unit block {4c + r}), the next k-step's load in flight
//     under them.  The waves' partial tiles overwrite the dead x tile and are folded in wave order,
//     then bias, relu and the Dropout multiplier of mlp.hip's counter hash, and h goes to a global
//     scratch with 16-byte stores.  Workgroup 0 also snapshots W2 | b2.
//   mlp_step_bwd_kernel  G workgroups.  Each recomputes the small shared part from h and the snapshot:
//     z = h . W2 + b2 (fmaf chains over MLS_KSPLIT fixed k slices, folded in slice order), per row
//     softmax / cross-entropy / argmax / dz, and dh = (dz . W2^T) [h > 0] / keep in place over h.
//     Then it forms the gradient of the parameters it owns -- a span of W1's rows and a range of
//     b1 | W2 | b2, by the static split of sml_mlp_step.h -- as fmaf chains over the batch rows in
//     ascending order and applies sml_adam.h's update to (p, m, v) in place.
//
// Launch 2 reads W2 only through the snapshot, so its owners may update it while other workgroups
// still compute with the old values.  No atomics, no workgroup waits on another, and a gradient's
// bits depend on neither G nor the CU count.  Workgroup 0 of launch 2 is the single writer of the
// metric pair and of the step count.
#include "sml_common.h"
#include "sml_adam.h"
#include "sml_mlp_dropout.h"
#include "sml_mlp_step.h"
#include "sml_ops.h"

namespace sml {
namespace {

constexpr int NT = MLS_NT;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// row of x that holds sample row0 + r of the step, kept inside [0, n)
__device__ __forceinline__ int64_t sample_row(const MlpStepArgs& a, int r) {
  int64_t i = a.row0 + r;
  if (a.order) i = a.order[i];
  SML_DCHECK(i >= 0 && i < a.n);
  return i < 0 ? 0 : (i >= a.n ? a.n - 1 : i);
}

__device__ __forceinline__ float load_x(const MlpStepArgs& a, int64_t row, int k) {
  if (a.x_u8) return (float)static_cast<const uint8_t*>(a.x)[row * a.ldx + k] * (1.0f / 255.0f);
  return static_cast<const float*>(a.x)[row * a.ldx + k];
}

// ---------------------------------------------------------------- launch 1
template <int NTILE>
__global__ __launch_bounds__(NT) void mlp_step_fwd_kernel(const MlpStepArgs a, const MlpStepFwdPlan P) {
  extern __shared__ f32x4 mlp_step_lds[];
  float* S = reinterpret_cast<float*>(mlp_step_lds);
  constexpr int RT = 16 * NTILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int ub = blockIdx.x, ldx = P.ldx;

  // the step's rows as fp32 [RT][ldx], zero past `in` and past the batch
  const bool u8x4 = a.x_u8 && (a.in & 3) == 0 && (a.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 3) == 0;
  for (int r = wave; r < RT; r += MLS_WAVES) {
    float* dst = S + r * ldx;
    if (r >= a.batch) {
      for (int k = lane; k < ldx; k += 64) dst[k] = 0.0f;
    } else if (u8x4) {
      const uint8_t* src = static_cast<const uint8_t*>(a.x) + sample_row(a, r) * a.ldx;
      for (int k = 4 * lane; k < ldx; k += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < a.in) {
          const uint32_t w = *reinterpret_cast<const uint32_t*>(src + k);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (float)((w >> (8 * e)) & 0xffu) * (1.0f / 255.0f);
        }
        st4(dst + k, v);
      }
    } else {
      const int64_t row = sample_row(a, r);
      for (int k = lane; k < ldx; k += 64) dst[k] = k < a.in ? load_x(a, row, k) : 0.0f;
    }
  }
  __syncthreads();

  // wave w contracts the k-steps [nk w / 8, nk (w + 1) / 8) of 4
  const int nk = (a.in + 3) / 4;
  const int ks0 = nk * wave / MLS_WAVES, ks1 = nk * (wave + 1) / MLS_WAVES;
  const int u0 = MLS_UB * ub + 4 * c;
  const bool vec = (a.H & 3) == 0;
  auto load_w = [&](int ks) -> f32x4 {
    f32x4 w = {0.f, 0.f, 0.f, 0.f};
    const int k = 4 * ks + g;
    if (k < a.in && u0 < a.H) {
      const float* p = a.flat + (int64_t)k * a.H + u0;
      if (vec) {
        w = ld4(p);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (u0 + e < a.H) w[e] = p[e];
      }
    }
    return w;
  };
  f32x4 acc[4][NTILE];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < NTILE; ++t) acc[r][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 nxt = {0.f, 0.f, 0.f, 0.f};
  if (ks0 < ks1) nxt = load_w(ks0);
  for (int ks = ks0; ks < ks1; ++ks) {
    const f32x4 cur = nxt;
    if (ks + 1 < ks1) nxt = load_w(ks + 1);
    const float* xp = S + c * ldx + 4 * ks + g;
    float b[NTILE];
#pragma unroll
    for (int t = 0; t < NTILE; ++t) b[t] = xp[16 * t * ldx];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t = 0; t < NTILE; ++t) acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[r], b[t], acc[r][t], 0, 0, 0);
  }
  __syncthreads();   // the x tile is dead

  // MFMA r holds unit 16g + 4q + r of the block in register q, row c: the four MFMAs' registers q are
  // four adjacent units
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      st4(S + (wave * RT + 16 * t + c) * MLS_PSTRIDE + 16 * g + 4 * q,
          f32x4{acc[0][t][q], acc[1][t][q], acc[2][t][q], acc[3][t][q]});
  __syncthreads();

  if (tid < RT * 16) {
    const int row = tid >> 4, u = MLS_UB * ub + 4 * (tid & 15);
    if (row < a.batch && u < a.H) {
      const float* p = S + row * MLS_PSTRIDE + 4 * (tid & 15);
      f32x4 s = ld4(p);
#pragma unroll
      for (int w = 1; w < MLS_WAVES; ++w) s += ld4(p + w * RT * MLS_PSTRIDE);
      const float* b1 = a.flat + (int64_t)a.in * a.H;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = 0.0f;
        if (u + e < a.H) {
          v = fmaxf(s[e] + b1[u + e], 0.0f);
          if (a.keep < 1.0f) v = dropout_u(a.seed, a.step, (uint32_t)row, (uint32_t)(u + e)) < a.keep ? v * a.inv_keep : 0.0f;
        }
        s[e] = v;
      }
      st4(a.hbuf + row * mls_ldh(a.H) + u, s);
    }
  }

  if (ub == 0) {
    const float* w2 = a.flat + (int64_t)a.in * a.H + a.H;
    const int n2 = a.H * a.C + a.C;
    for (int i = tid; i < n2; i += NT) a.snap[i] = w2[i];
  }
}

// ---------------------------------------------------------------- launch 2
struct AdamK {
  float lr_t, b1, b2, eps;
};

__device__ __forceinline__ void adam1(const MlpStepArgs& a, const AdamK& k, int64_t i, float grad) {
  float mm, vv, pn;
  adam_update(grad, a.m[i], a.v[i], a.flat[i], k.lr_t, k.b1, k.b2, k.eps, 1.0f, mm, vv, pn);
  a.m[i] = mm;
  a.v[i] = vv;
  a.flat[i] = pn;
}

// cnt parameters from i on; 16-byte loads and stores where the quad is whole and aligned
__device__ __forceinline__ void adam4(const MlpStepArgs& a, const AdamK& k, int64_t i, int cnt, f32x4 grad) {
  if (cnt == 4 && (i & 3) == 0) {
    f32x4 p = ld4(a.flat + i), m = ld4(a.m + i), v = ld4(a.v + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float mm, vv, pn;
      adam_update(grad[e], m[e], v[e], p[e], k.lr_t, k.b1, k.b2, k.eps, 1.0f, mm, vv, pn);
      m[e] = mm;
      v[e] = vv;
      p[e] = pn;
    }
    st4(a.flat + i, p);
    st4(a.m + i, m);
    st4(a.v + i, v);
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < cnt) adam1(a, k, i + e, grad[e]);
}

__global__ __launch_bounds__(NT) void mlp_step_bwd_kernel(const MlpStepArgs a, const MlpStepBwdPlan P, const int G) {
  extern __shared__ f32x4 mlp_step_lds[];
  float* S = reinterpret_cast<float*>(mlp_step_lds);
  const int tid = threadIdx.x, grp = blockIdx.x;
  const int B = a.batch, H = a.H, C = a.C, ldh = P.ldh, BC = B * C;
  float* hs = S + P.o_h;
  float* zp = S + P.o_zpart;
  float* zs = S + P.o_z;
  float* xs = S + P.o_x;
  int* idx = reinterpret_cast<int*>(S + P.o_idx);
  int* lab = idx + MLS_MAXBATCH;
  float* red = S + P.o_red;
  // W2 | b2 of the step's forward: staged in LDS where it fits, else read from the snapshot
  const float* W2 = P.w2_in_lds ? S + P.o_w2 : a.snap;
  const float* b2 = W2 + H * C;

  const int64_t t = a.iter0[0] + a.s + 1;
  const AdamK ak = {adam_lr_t(a.lr, a.beta1, a.beta2, (float)t), a.beta1, a.beta2, a.eps};

  if (tid < B) {
    const int64_t row = sample_row(a, tid);
    const int64_t y = a.y[row];
    idx[tid] = (int)row;
    lab[tid] = (y >= 0 && y < C) ? (int)y : -1;
  }
  for (int i = tid; i < B * (ldh / 4); i += NT) st4(hs + 4 * i, ld4(a.hbuf + 4 * i));
  if (P.w2_in_lds)
    for (int i = tid; i < H * C + C; i += NT) S[P.o_w2 + i] = a.snap[i];
  __syncthreads();

  // z = h . W2 + b2: slice s of the contraction for every (row, class), then the slices in order
  for (int it = tid; it < MLS_KSPLIT * BC; it += NT) {
    const int s = it / BC, o = it - s * BC, row = o / C, cls = o - row * C;
    const int k1 = H * (s + 1) / MLS_KSPLIT;
    float acc = 0.0f;
    for (int k = H * s / MLS_KSPLIT; k < k1; ++k) acc = fmaf(hs[row * ldh + k], W2[k * C + cls], acc);
    zp[it] = acc;
  }
  __syncthreads();

  // one lane per row: softmax, cross-entropy, argmax match, dz = (p - onehot) / batch over z
  if (tid < B) {
    float* z = zs + tid * C;
    const int y = lab[tid];
    float mx = 0.0f, zy = 0.0f;
    int amax = 0;
    for (int j = 0; j < C; ++j) {
      float v = zp[tid * C + j];
      for (int s = 1; s < MLS_KSPLIT; ++s) v += zp[s * BC + tid * C + j];
      v += b2[j];
      z[j] = v;
      if (j == 0 || v > mx) {   // first maximal index (tf.argmax)
        mx = v;
        amax = j;
      }
      if (j == y) zy = v;
    }
    float sum = 0.0f;
    for (int j = 0; j < C; ++j) {
      const float e = __expf(z[j] - mx);
      z[j] = e;
      sum += e;
    }
    const float inv = __frcp_rn(sum), scale = 1.0f / (float)B;
    for (int j = 0; j < C; ++j) z[j] = y >= 0 ? (z[j] * inv - (j == y ? 1.0f : 0.0f)) * scale : 0.0f;
    red[tid] = y >= 0 ? (mx - zy) + __logf(sum) : 0.0f;
    red[MLS_MAXBATCH + tid] = (y >= 0 && amax == y) ? 1.0f : 0.0f;
  }
  __syncthreads();

  if (grp == 0 && tid == 0) {
    float loss = 0.0f, ok = 0.0f;
    for (int r = 0; r < B; ++r) {
      loss += red[r];
      ok += red[MLS_MAXBATCH + r];
    }
    a.acc[0] += loss;
    a.acc[1] += ok;
    *a.iter = t;
  }

  // this workgroup's range of the tail b1 | W2 | b2; W2 and b2 first, while LDS still holds h
  const int tail = mls_tail(H, C);
  const int t0 = mlp_step_first(grp, G, tail), t1 = mlp_step_first(grp + 1, G, tail);
  const int64_t tail0 = (int64_t)a.in * H;
  for (int e = (t0 > H ? t0 : H) + tid; e < t1; e += NT) {
    float grad = 0.0f;
    if (e < H + H * C) {
      const int j = (e - H) / C, cls = (e - H) - j * C;
      for (int b = 0; b < B; ++b) grad = fmaf(hs[b * ldh + j], zs[b * C + cls], grad);
    } else {
      const int cls = e - H - H * C;
      for (int b = 0; b < B; ++b) grad += zs[b * C + cls];
    }
    adam1(a, ak, tail0 + e, grad);
  }
  __syncthreads();

  // dh = (dz . W2^T) [h > 0] / keep, over h
  for (int it = tid; it < B * H; it += NT) {
    const int b = it / H, j = it - b * H;
    float acc = 0.0f;
    for (int cls = 0; cls < C; ++cls) acc = fmaf(zs[b * C + cls], W2[j * C + cls], acc);
    float* p = hs + b * ldh + j;
    *p = *p > 0.0f ? acc * a.inv_keep : 0.0f;
  }
  __syncthreads();

  for (int e = t0 + tid; e < (t1 < H ? t1 : H); e += NT) {   // b1
    float grad = 0.0f;
    for (int b = 0; b < B; ++b) grad += hs[b * ldh + e];
    adam1(a, ak, tail0 + e, grad);
  }

  // this workgroup's rows of W1, MLS_XCHUNK at a time: gather their x columns, then one quad of
  // units per thread, the chain over the batch rows in ascending order
  const int k0 = mlp_step_first(grp, G, a.in), k1 = mlp_step_first(grp + 1, G, a.in);
  const int nq = ldh / 4;
  for (int kc = k0; kc < k1; kc += MLS_XCHUNK) {
    const int nkc = k1 - kc < MLS_XCHUNK ? k1 - kc : MLS_XCHUNK;
    {
      const int kk = tid & (MLS_XCHUNK - 1), b = tid >> 4;   // NT = MLS_XCHUNK * MLS_MAXBATCH
      if (kk < nkc && b < B) xs[kk * MLS_MAXBATCH + b] = load_x(a, idx[b], kc + kk);
    }
    __syncthreads();
    for (int it = tid; it < nkc * nq; it += NT) {
      const int kk = it / nq, q = it - kk * nq;
      f32x4 grad = {0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < B; ++b) {
        const float xv = xs[kk * MLS_MAXBATCH + b];
        const f32x4 d = ld4(hs + b * ldh + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) grad[e] = fmaf(xv, d[e], grad[e]);
      }
      adam4(a, ak, (int64_t)(kc + kk) * H + 4 * q, H - 4 * q < 4 ? H - 4 * q : 4, grad);
    }
    __syncthreads();
  }
}

static_assert(NT == MLS_XCHUNK * MLS_MAXBATCH && MLS_XCHUNK == 16, "the backward's x gather: one element per thread");

template <typename Kernel>
hipError_t allow_lds(Kernel* kernel, int bytes) {
  if (bytes <= 65536) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace

// Reached through the binding, which has run mlp_step_check and sized the buffers; the tests here are
// for a caller that comes another way.
hipError_t mlp_train_steps_launch(MlpStepArgs a, int steps, int groups, hipStream_t st) {
  if (!mlp_step_check(a.batch, a.in, a.H, a.C, 1.0 - (double)a.keep, 1).empty() || steps < 1 || !a.flat || !a.m ||
      !a.v || !a.iter || !a.iter0 || !a.x || !a.y || !a.hbuf || !a.snap || !a.acc || a.row0 < 0 || a.n < 1 ||
      a.n > INT32_MAX || a.ldx < a.in || ((reinterpret_cast<uintptr_t>(a.flat) | reinterpret_cast<uintptr_t>(a.m) |
                                           reinterpret_cast<uintptr_t>(a.v) | reinterpret_cast<uintptr_t>(a.hbuf)) & 15))
    return hipErrorInvalidValue;
  if (!a.order && a.row0 + (int64_t)steps * a.batch > a.n) return hipErrorInvalidValue;
  const MlpStepFwdPlan fp = mlp_step_fwd_plan(a.batch, a.in);
  const MlpStepBwdPlan bp = mlp_step_bwd_plan(a.batch, a.H, a.C);
  const int G = mlp_step_groups(a.in, groups, dense_batch_cus());
  auto fwd = fp.rt == 16 ? mlp_step_fwd_kernel<1> : mlp_step_fwd_kernel<2>;
  hipError_t e = allow_lds(fwd, fp.lds_bytes);
  if (e != hipSuccess) return e;
  e = allow_lds(mlp_step_bwd_kernel, bp.lds_bytes);
  if (e != hipSuccess) return e;
  for (int s = 0; s < steps; ++s) {
    hipLaunchKernelGGL(fwd, dim3(mls_fwd_blocks(a.H)), dim3(NT), (size_t)fp.lds_bytes, st, a, fp);
    hipLaunchKernelGGL(mlp_step_bwd_kernel, dim3(G), dim3(NT), (size_t)bp.lds_bytes, st, a, bp, G);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    a.row0 += a.batch;
    a.step += 1;
    a.s += 1;
  }
  return hipSuccess;
}

}  // namespace sml
