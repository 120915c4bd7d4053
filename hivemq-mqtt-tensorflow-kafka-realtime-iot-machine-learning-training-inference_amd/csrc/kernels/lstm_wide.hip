// LSTM recurrence kernels for layers wider than 128 units (192 .. 512 in steps of 64) on gfx950.
//
// lstm.hip keeps the whole recurrent weight in registers; at U >= 192 the bf16 image of U
// (4U x U: 512 KB at U = 256, 2 MB at U = 512) no longer fits one CU, so here it is STREAMED:
// a pack kernel writes U once per call as bf16 in MFMA A-fragment order (one 16-byte load
// per lane per fragment, no LDS staging) and every workgroup re-reads that image each time
// step.  It stays in the XCD's L2 (4 MiB) and each fragment is used once per step.
//
// Forward: one workgroup (4 waves) owns NT tiles of 16 sequences for the whole time loop
// (NT = 1 is the only instance built: 32 sequences per workgroup measured 9 to 41 % slower at
// B = 64 and B = 4096, U = 256 and 512, profiles/r09/lstm_wide/SUMMARY.md).
// Wave w owns unit blocks [w UPW, (w+1) UPW), UPW = U / 64, with all four gate tiles
// (i, f, c~, o) of those units, so the gate math and c stay in-lane in registers.  The
// tile's h_{t-1} lives in LDS as bf16 in B-fragment order (both K = 16 halves of a
// v_mfma_f32_16x16x32_bf16 adjacent: one ds_read_b128 per k-step), double-buffered, one
// barrier per step.  The wave's weight fragments are contiguous in the image in the order
// it consumes them and are prefetched through a register ring that wraps from the end of
// one time step into the start of the next (the weights do not change).
//
// Backward: each wave forms dz for its own units from the saved gates / c, the tile's bf16
// dz meets in LDS (B-fragment order over the 4U gate features), and dh_{t-1} for the wave's
// units is U[units][all gates] . dz^T against a second image streamed the same way; each
// dz fragment read from LDS feeds all the wave's unit blocks.
//
// Every workgroup is independent.  Barriers sit inside the time loop, so no wave leaves
// early: the tile index is block-uniform, ragged tiles clamp their loads and mask their stores.
#include "sml_common.h"

using namespace sml;

namespace {

constexpr int WAVES = 4;

__device__ __forceinline__ float sig(float z) { return sigmoid_fast(z); }
__device__ __forceinline__ float act_f(int a, float z) { return a == ACT_RELU ? relu_fast(z) : tanh_fast(z); }
__device__ __forceinline__ float act_d(int a, float z, float y) {
  return a == ACT_RELU ? (z > 0.f ? 1.f : 0.f) : fmaf(-y, y, 1.0f);
}
__device__ __forceinline__ bf16x4 lo4(s16x8 v) { return __builtin_shufflevector(v, v, 0, 1, 2, 3); }
__device__ __forceinline__ bf16x4 hi4(s16x8 v) { return __builtin_shufflevector(v, v, 4, 5, 6, 7); }

// An offset of 0 the optimiser cannot see through.  The weight image is the same in every time
// step, so its loads are loop-invariant: without this they are all hoisted out of the time loop
// (the wave's whole slice in registers, hundreds of spilled VGPRs) instead of streamed per step.
__device__ __forceinline__ int opaque_zero() {
  int z = 0;
  asm volatile("" : "+s"(z));
  return z;
}

__device__ __forceinline__ short to_bf16(float v) { return __builtin_bit_cast(short, (__bf16)v); }

// Weight images, 16 bytes (8 bf16: K halves 0 and 1 of a 16x16x32 MFMA) per lane per fragment.
//   forward : entry ((b KS + ks) 4 + q) 64 + lane
//             A[m = gate q U + 16 b + c][k = unit 32 ks + 16 half + 4 g + j]
//   backward: entry ((w KSB + ksb) UPW + j) 64 + lane, unit block b = w UPW + j
//             A[m = unit 16 b + c][k = gate 32 ksb + 16 half + 4 g + jj]
// Both are contiguous per wave in the order the wave consumes them.
__global__ __launch_bounds__(256) void lstm_wide_pack_kernel(const float* __restrict__ Uw, s16x8* __restrict__ img,
                                                             int U, int bwd) {
  const int G4 = 4 * U, KS = U / 32, KSB = U / 8, UPW = U / 64;
  const int total = G4 * U / 8;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int lane = e & 63, c = lane & 15, g = lane >> 4;
  int r = e >> 6;
  s16x8 v;
  if (!bwd) {
    const int q = r & 3;
    r >>= 2;
    const int ks = r % KS, b = r / KS;
    const int gate = q * U + 16 * b + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int unit = 32 * ks + 16 * (i >> 2) + 4 * g + (i & 3);
      SML_DCHECK(unit < U && gate < G4);
      v[i] = to_bf16(Uw[(int64_t)unit * G4 + gate]);
    }
  } else {
    const int j = r % UPW;
    r /= UPW;
    const int ksb = r % KSB, w = r / KSB;
    const int unit = 16 * (w * UPW + j) + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int gate = 32 * ksb + 16 * (i >> 2) + 4 * g + (i & 3);
      SML_DCHECK(unit < U && gate < G4);
      v[i] = to_bf16(Uw[(int64_t)unit * G4 + gate]);
    }
  }
  img[e] = v;
}

struct WideFwdArgs {
  const float* zx;     // [B, T, 4U]  x.W + b
  const s16x8* img;    // forward weight image
  const float* h0;     // [B, U] or null
  const float* c0;     // [B, U] or null
  float* hseq;         // [B, T, U]
  float* cseq;         // [B, T, U]
  float* gates;        // [B, T, 4U]  post-activation i, f, c~, o
  int64_t B;
  int T;
  int act;
};

// register-ring depth: must divide the wave's fragment count so that the ring slot of a
// fragment is the same in every time step (the prefetch wraps across steps)
constexpr int ring_depth(int n) { return n % 4 == 0 ? 4 : n % 5 == 0 ? 5 : n % 3 == 0 ? 3 : n % 7 == 0 ? 7 : 2; }

template <int U, int NT>
__global__ __launch_bounds__(WAVES * 64) void lstm_wide_fwd_kernel(WideFwdArgs a) {
  constexpr int G4 = 4 * U, KS = U / 32, UPW = U / 64;
  constexpr int NIT = UPW * KS;          // k-steps per wave per time step (4 gate fragments each)
  constexpr int D = ring_depth(NIT);
  static_assert(NIT % D == 0 && D >= 2, "ring depth must divide the fragment count");
  __shared__ s16x8 hbuf[2][NT][KS][64];  // 64 NT U bytes: 64 KB at U = 512, NT = 2
  bf16x4* hb4 = reinterpret_cast<bf16x4*>(&hbuf[0][0][0][0]);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t s0 = (int64_t)blockIdx.x * (16 * NT);   // block-uniform
  bool valid[NT];
  int64_t sq[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int64_t seq = s0 + 16 * nt + c;
    valid[nt] = seq < a.B;
    sq[nt] = valid[nt] ? seq : a.B - 1;   // clamped for loads
    SML_DCHECK(sq[nt] >= 0 && sq[nt] < a.B);
  }
  f32x4 cs[UPW][NT];
#pragma unroll
  for (int j = 0; j < UPW; ++j)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int b = w * UPW + j;
      f32x4 h;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = 16 * b + 4 * g + i;
        h[i] = a.h0 ? a.h0[sq[nt] * U + u] : 0.f;
        cs[j][nt][i] = a.c0 ? a.c0[sq[nt] * U + u] : 0.f;
      }
      hb4[(((0 * NT + nt) * KS + (b >> 1)) * 64 + lane) * 2 + (b & 1)] = pack4(h);
    }
  // the wave's fragment stream: k-step `it`, gate q at wimg[(it * 4 + q) * 64]
  const s16x8* wimg = a.img + (int64_t)w * NIT * 4 * 64 + lane;
  s16x8 ring[D][4];
#pragma unroll
  for (int p = 0; p < D - 1; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) ring[p][q] = wimg[(p * 4 + q) * 64];
  __syncthreads();
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < a.T; ++t) {
    const int cur = t & 1;
    const s16x8* wt = wimg + opaque_zero();
#pragma unroll
    for (int j = 0; j < UPW; ++j) {
      const int b = w * UPW + j;
      f32x4 zin[4][NT], acc[4][NT];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          zin[q][nt] = *reinterpret_cast<const f32x4*>(a.zx + (sq[nt] * a.T + t) * (int64_t)G4 + q * U + 16 * b + 4 * g);
          acc[q][nt] = zero4;
        }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        constexpr int AHEAD = D - 1;
        const int it = j * KS + ks;
        const int nx = (it + AHEAD) % NIT;   // wraps into the next time step's first fragments
        SML_DCHECK((int64_t)w * NIT * 4 * 64 + (nx * 4 + 3) * 64 + lane < (int64_t)G4 * U / 8);
#pragma unroll
        for (int q = 0; q < 4; ++q) ring[(it + AHEAD) % D][q] = wt[(nx * 4 + q) * 64];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const s16x8 hb = hbuf[cur][nt][ks][lane];
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q][nt] = mfma32a(ring[it % D][q], lo4(hb), hi4(hb), acc[q][nt]);
        }
        // keep each k-step's loads where the ring puts them: unfenced, the scheduler hoists the
        // whole step's loads to the top and spills
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 gi, gf, gc, go, h;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          gi[i] = sig(acc[0][nt][i] + zin[0][nt][i]);
          gf[i] = sig(acc[1][nt][i] + zin[1][nt][i]);
          gc[i] = act_f(a.act, acc[2][nt][i] + zin[2][nt][i]);
          go[i] = sig(acc[3][nt][i] + zin[3][nt][i]);
          cs[j][nt][i] = fmaf(gf[i], cs[j][nt][i], gi[i] * gc[i]);
          h[i] = go[i] * act_f(a.act, cs[j][nt][i]);
        }
        if (valid[nt]) {
          const int64_t base_g = (sq[nt] * a.T + t) * (int64_t)G4;
          const int64_t base_u = (sq[nt] * a.T + t) * (int64_t)U;
          const int off = 16 * b + 4 * g;
          *reinterpret_cast<f32x4*>(a.gates + base_g + off) = gi;
          *reinterpret_cast<f32x4*>(a.gates + base_g + U + off) = gf;
          *reinterpret_cast<f32x4*>(a.gates + base_g + 2 * U + off) = gc;
          *reinterpret_cast<f32x4*>(a.gates + base_g + 3 * U + off) = go;
          *reinterpret_cast<f32x4*>(a.cseq + base_u + off) = cs[j][nt];
          *reinterpret_cast<f32x4*>(a.hseq + base_u + off) = h;
        }
        // read after this step's barrier
        hb4[((((cur ^ 1) * NT + nt) * KS + (b >> 1)) * 64 + lane) * 2 + (b & 1)] = pack4(h);
      }
    }
    __syncthreads();
  }
}

struct WideBwdArgs {
  const float* dh;     // [B, T, U] gradient w.r.t. the h sequence
  const float* gates;  // [B, T, 4U] post-activation
  const float* cseq;   // [B, T, U]
  const float* c0;     // [B, U] or null
  const s16x8* img;    // backward weight image
  float* dz;           // [B, T, 4U] pre-activation gate gradients
  float* dh0;          // [B, U] or null
  float* dc0;          // [B, U] or null
  int64_t B;
  int T;
  int act;
};

template <int U, int NT>
__global__ __launch_bounds__(WAVES * 64) void lstm_wide_bwd_kernel(WideBwdArgs a) {
  constexpr int G4 = 4 * U, UB = U / 16, KSB = U / 8, UPW = U / 64;
  constexpr int D = 4;                   // ring of k-steps, UPW fragments each
  static_assert(KSB % D == 0, "the k loop is unrolled by the ring depth");
  extern __shared__ __attribute__((aligned(16))) s16x8 dzbuf[];   // [NT][KSB][64]: 128 NT U bytes
  bf16x4* dz4 = reinterpret_cast<bf16x4*>(dzbuf);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t s0 = (int64_t)blockIdx.x * (16 * NT);   // block-uniform
  bool valid[NT];
  int64_t sq[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int64_t seq = s0 + 16 * nt + c;
    valid[nt] = seq < a.B;
    sq[nt] = valid[nt] ? seq : a.B - 1;
    SML_DCHECK(sq[nt] >= 0 && sq[nt] < a.B);
  }
  // the wave's fragment stream: k-step ksb, unit block j at wimg[(ksb * UPW + j) * 64]
  const s16x8* wimg = a.img + (int64_t)w * KSB * UPW * 64 + lane;
  s16x8 ring[D][UPW];
#pragma unroll
  for (int p = 0; p < D - 1; ++p)
#pragma unroll
    for (int j = 0; j < UPW; ++j) ring[p][j] = wimg[(p * UPW + j) * 64];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 dhr[UPW][NT], dcn[UPW][NT];
#pragma unroll
  for (int j = 0; j < UPW; ++j)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) dhr[j][nt] = dcn[j][nt] = zero4;

  for (int t = a.T - 1; t >= 0; --t) {
    const s16x8* wt = wimg + opaque_zero();
#pragma unroll
    for (int j = 0; j < UPW; ++j)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int b = w * UPW + j;
        const int off = 16 * b + 4 * g;
        const int64_t bg = (sq[nt] * a.T + t) * (int64_t)G4;
        const int64_t bu = (sq[nt] * a.T + t) * (int64_t)U;
        const f32x4 gi = *reinterpret_cast<const f32x4*>(a.gates + bg + off);
        const f32x4 gf = *reinterpret_cast<const f32x4*>(a.gates + bg + U + off);
        const f32x4 gc = *reinterpret_cast<const f32x4*>(a.gates + bg + 2 * U + off);
        const f32x4 go = *reinterpret_cast<const f32x4*>(a.gates + bg + 3 * U + off);
        const f32x4 ct = *reinterpret_cast<const f32x4*>(a.cseq + bu + off);
        f32x4 cp;
        if (t > 0) cp = *reinterpret_cast<const f32x4*>(a.cseq + bu - U + off);
        else if (a.c0) cp = *reinterpret_cast<const f32x4*>(a.c0 + sq[nt] * U + off);
        else cp = zero4;
        const f32x4 dho = valid[nt] ? *reinterpret_cast<const f32x4*>(a.dh + bu + off) : zero4;
        f32x4 dzt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dh = dho[i] + dhr[j][nt][i];
          const float ac = act_f(a.act, ct[i]);
          const float dc = dcn[j][nt][i] + dh * go[i] * act_d(a.act, ct[i], ac);
          dzt[0][i] = dc * gc[i] * gi[i] * (1.f - gi[i]);
          dzt[1][i] = dc * cp[i] * gf[i] * (1.f - gf[i]);
          const float gcd = a.act == ACT_RELU ? (gc[i] > 0.f ? 1.f : 0.f) : fmaf(-gc[i], gc[i], 1.f);
          dzt[2][i] = dc * gi[i] * gcd;
          dzt[3][i] = dh * ac * go[i] * (1.f - go[i]);
          dcn[j][nt][i] = dc * gf[i];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!valid[nt]) dzt[q] = zero4;
          const int mt = q * UB + b;   // gate tile = k half (mt & 1) of k-step mt >> 1
          if (valid[nt]) *reinterpret_cast<f32x4*>(a.dz + bg + 16 * mt + 4 * g) = dzt[q];
          dz4[((nt * KSB + (mt >> 1)) * 64 + lane) * 2 + (mt & 1)] = pack4(dzt[q]);
        }
        // two unit blocks' loads in flight at a time (28 VGPRs per block and tile)
        if ((j & 1) && nt == NT - 1) __builtin_amdgcn_sched_barrier(0);
      }
    __syncthreads();
    // recurrent gradient for step t-1 of the wave's units: dh^T = U . dz^T over all gates
    f32x4 acc[UPW][NT];
#pragma unroll
    for (int j = 0; j < UPW; ++j)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[j][nt] = zero4;
    // one k-step: prefetch k-step nx into the ring slot freed last, contract k-step k from slot p
    auto kstep = [&](int k, int nx, int p) {
      constexpr int AHEAD = D - 1;
      SML_DCHECK(nx >= 0 && nx < KSB && k >= 0 && k < KSB);
#pragma unroll
      for (int j = 0; j < UPW; ++j) ring[(p + AHEAD) % D][j] = wt[(nx * UPW + j) * 64];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const s16x8 db = dzbuf[(nt * KSB + k) * 64 + lane];
#pragma unroll
        for (int j = 0; j < UPW; ++j) acc[j][nt] = mfma32a(ring[p][j], lo4(db), hi4(db), acc[j][nt]);
      }
      __builtin_amdgcn_sched_barrier(0);   // as in the forward: no hoisting across k-steps
    };
    for (int k0 = 0; k0 < KSB - D; k0 += D) {
#pragma unroll
      for (int p = 0; p < D; ++p) kstep(k0 + p, k0 + p + D - 1, p);
    }
    // last group: the prefetch wraps into the next time step's first fragments
#pragma unroll
    for (int p = 0; p < D; ++p) kstep(KSB - D + p, (KSB - 1 + p) % KSB, p);
#pragma unroll
    for (int j = 0; j < UPW; ++j)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) dhr[j][nt] = acc[j][nt];
    __syncthreads();   // the next step overwrites dzbuf
  }
#pragma unroll
  for (int j = 0; j < UPW; ++j)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (valid[nt]) {
        const int off = 16 * (w * UPW + j) + 4 * g;
        if (a.dh0) *reinterpret_cast<f32x4*>(a.dh0 + sq[nt] * U + off) = dhr[j][nt];
        if (a.dc0) *reinterpret_cast<f32x4*>(a.dc0 + sq[nt] * U + off) = dcn[j][nt];
      }
}

template <int U, int NT>
hipError_t launch_fwd(const WideFwdArgs& a, hipStream_t stream) {
  const unsigned grid = (unsigned)((a.B + 16 * NT - 1) / (16 * NT));
  hipLaunchKernelGGL((lstm_wide_fwd_kernel<U, NT>), dim3(grid), dim3(WAVES * 64), 0, stream, a);
  return hipGetLastError();
}

template <int U, int NT>
hipError_t launch_bwd(const WideBwdArgs& a, hipStream_t stream) {
  const unsigned grid = (unsigned)((a.B + 16 * NT - 1) / (16 * NT));
  constexpr int lds = 128 * NT * U;
  static_assert(lds <= 128 * 1024, "dz tile must fit LDS");
  auto k = lstm_wide_bwd_kernel<U, NT>;
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(WAVES * 64), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

namespace sml {

bool lstm_wide_supported(int U) { return U > 128 && U <= 512 && U % 64 == 0; }

int64_t lstm_wide_image_bytes(int U) { return (int64_t)4 * U * U * 2; }

#define SML_WIDE_DISPATCH(FN, ARGS)                 \
  switch (U) {                                      \
    case 192: return FN<192, 1>(ARGS, stream);      \
    case 256: return FN<256, 1>(ARGS, stream);      \
    case 320: return FN<320, 1>(ARGS, stream);      \
    case 384: return FN<384, 1>(ARGS, stream);      \
    case 448: return FN<448, 1>(ARGS, stream);      \
    case 512: return FN<512, 1>(ARGS, stream);      \
    default: return hipErrorInvalidValue;           \
  }

hipError_t lstm_wide_fwd_launch(const float* zx, const float* Uw, void* image, const float* h0, const float* c0,
                                float* hseq, float* cseq, float* gates, int64_t B, int T, int U, int act,
                                hipStream_t stream) {
  if (!lstm_wide_supported(U) || B < 1 || T < 1) return hipErrorInvalidValue;
  const int entries = 4 * U * U / 8;
  hipLaunchKernelGGL(lstm_wide_pack_kernel, dim3((entries + 255) / 256), dim3(256), 0, stream, Uw,
                     static_cast<s16x8*>(image), U, 0);
  WideFwdArgs a{zx, static_cast<const s16x8*>(image), h0, c0, hseq, cseq, gates, B, T, act};
  SML_WIDE_DISPATCH(launch_fwd, a)
}

hipError_t lstm_wide_bwd_launch(const float* dh, const float* gates, const float* cseq, const float* c0,
                                const float* Uw, void* image, float* dz, float* dh0, float* dc0, int64_t B, int T,
                                int U, int act, hipStream_t stream) {
  if (!lstm_wide_supported(U) || B < 1 || T < 1) return hipErrorInvalidValue;
  const int entries = 4 * U * U / 8;
  hipLaunchKernelGGL(lstm_wide_pack_kernel, dim3((entries + 255) / 256), dim3(256), 0, stream, Uw,
                     static_cast<s16x8*>(image), U, 1);
  WideBwdArgs a{dh, gates, cseq, c0, static_cast<const s16x8*>(image), dz, dh0, dc0, B, T, act};
  SML_WIDE_DISPATCH(launch_bwd, a)
}

}  // namespace sml
