// Persistent per-event scorer for Dense stacks of any depth: 1..8 Dense layers, every width
// up to 512, rows of up to 32 features, the last layer one unit per feature (an autoencoder
// wider or deeper than the reference's 18-14-7-7-18, which ae_serve.hip is built around).
//
// The ring protocol, the pass, a layer's reduction, the exit conditions and the BIT-IDENTITY
// argument are described in sml_dense_serve_dev.h, shared with dense_serve_fleet.hip.  Here:
//
// The weights are an IMAGE built once per server (ops/serve.py: dense_serve_image): per layer
// float4 img[Kp / 4][Np] with img[g][o] = W[4g .. 4g + 3][o] (Kp = in rounded up to 4, Np = out
// rounded up to 32, zero-padded), followed by the padded bias [Np]; threads of consecutive o load
// consecutive 16 bytes.  The kernel body is a template on where that image lives:
//   "lds"     the whole image is copied to LDS at launch (it fits beside the activation and
//             partial-sum buffers: DSV_LDS_IMAGE_BYTES);
//   "stream"  every pass streams the image from L2.
//
// A thread loads each weight group of its slice once and uses it for every event of the pass,
// reading the events' activations as broadcast float4 from LDS into per-event accumulators
// (registers: the loops over events are fully unrolled).  The pass is instantiated for 1, 2, 4 and
// 8 accumulators (E is rounded up; the surplus accumulators read stale activations and their
// results are dropped), every instantiation with the same chains.
#include "sml_dense_serve_dev.h"

namespace sml {
namespace {

using namespace dense_serve_dev;

static_assert(FIXED_FLOATS * 4 + DSV_LDS_IMAGE_BYTES + 2048 <= 160 * 1024, "LDS budget");
static_assert(ACT_LINEAR == 0 && DSV_ACT_LAST == ACT_SIGMOID, "the check's activation range is Act's");

// One layer for EC accumulators (events 0 .. EC - 1 of the pass): in -> out, both in LDS with
// strides in_s / AS.  W: the layer's image, bias: its padded bias (LDS or global).
template <int EC>
__device__ __forceinline__ void layer_pass(const float4* __restrict__ W, const float* __restrict__ bias, int Kp, int Np,
                                           int KS, int out_n, int act, const float* in, int in_s, float* out,
                                           float* part, int tid) {
  const int G4 = Kp >> 2;
  const int KG = (G4 + KS - 1) / KS;   // groups per slice; the last slices may be short or empty
  if (tid < Np * KS) {
    const int ks = tid / Np, o = tid - ks * Np;
    const int g0 = ks * KG < G4 ? ks * KG : G4;
    const int g1 = g0 + KG < G4 ? g0 + KG : G4;
    float acc[EC];
#pragma unroll
    for (int e = 0; e < EC; ++e) acc[e] = 0.f;
    const float4* wp = W + (size_t)g0 * Np + o;
    int g = g0;
    // four 16-byte weight loads in flight; the chains stay in row order
    for (; g + 4 <= g1; g += 4, wp += 4 * (size_t)Np) {
      const float4 w0 = wp[0], w1 = wp[Np], w2 = wp[2 * (size_t)Np], w3 = wp[3 * (size_t)Np];
#pragma unroll
      for (int e = 0; e < EC; ++e) {
        const float4* xp = reinterpret_cast<const float4*>(in + e * in_s) + g;
        acc[e] = fma4(xp[0], w0, acc[e]);
        acc[e] = fma4(xp[1], w1, acc[e]);
        acc[e] = fma4(xp[2], w2, acc[e]);
        acc[e] = fma4(xp[3], w3, acc[e]);
      }
    }
    for (; g < g1; ++g, wp += Np) {
      const float4 w0 = wp[0];
#pragma unroll
      for (int e = 0; e < EC; ++e)
        acc[e] = fma4(reinterpret_cast<const float4*>(in + e * in_s)[g], w0, acc[e]);
    }
#pragma unroll
    for (int e = 0; e < EC; ++e) part[(ks * EB + e) * Np + o] = acc[e];
  }
  layer_finish([bias](int) { return bias; }, EC, Np, KS, DenseLayerOut{out_n, act}, out, part, tid);
}

template <bool LDSW>
__global__ __launch_bounds__(DSV_NT) void dense_serve_kernel(DenseServeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ __attribute__((aligned(16))) float s_xn[EB][32];   // the pass's normalised rows
  __shared__ float s_sc[32], s_sh[32];
  __shared__ int s_ctl[8];   // quit, E, -, seen sequence, t_seen lo / hi
  float* const act0 = smem;
  float* const act1 = smem + ACT_FLOATS;
  float* const part = smem + 2 * ACT_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int D = a.D;
  ServeCtl* const ctl = a.ctl;
  const float* wimg = a.img;
  if constexpr (LDSW) {
    float4* dst = reinterpret_cast<float4*>(smem + FIXED_FLOATS);
    const float4* src = reinterpret_cast<const float4*>(a.img);
    for (int i = tid; i < (a.img_floats >> 2); i += NT) dst[i] = src[i];
    wimg = smem + FIXED_FLOATS;
  }
  if (tid < 32) {
    s_sc[tid] = (tid < D && a.scale) ? a.scale[tid] : 1.f;
    s_sh[tid] = (tid < D && a.shift) ? a.shift[tid] : 0.f;
  }
  if (tid < 8) s_ctl[tid] = 0;
  __syncthreads();

  uint64_t tail = ld_sys(&ctl->done);
  const uint64_t st0 = ld_sys(a.stats);   // cumulative over launches
  uint32_t passes = (uint32_t)(st0 >> 32), events = (uint32_t)st0;
  uint64_t last = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) st_sys32(&ctl->alive, 1u);
  for (;;) {
    // ---------------- waves 0..3 poll the next request slot
    const int slot = (int)(tail % (uint64_t)a.nslots);
    const uint32_t want = (uint32_t)(tail + 1);
    if (wid < 4) {
      typedef __attribute__((address_space(3))) volatile int lds_vint;   // ds_* accesses, not flat
      lds_vint* seen = (lds_vint*)&s_ctl[3];
      lds_vint* quit_f = (lds_vint*)&s_ctl[0];
      const uint64_t* wp = lane < 32 ? &a.req[slot].w[lane] : &ctl->head;
      if (wid == 1) __builtin_amdgcn_s_sleep(10);
      else if (wid == 2) __builtin_amdgcn_s_sleep(20);
      else if (wid == 3) __builtin_amdgcn_s_sleep(30);
      for (uint32_t it = 0;; ++it) {
        if (*seen == (int)want || *quit_f) break;
        const uint64_t w = ld_sys(wp);
        const bool ok = lane >= D || (uint32_t)(w >> 32) == want;
        if (__ballot(ok) == ~0ull) {
          // the row arrived with the poll.  head was published after the rows: a head read
          // before the host's store landed only makes this pass smaller
          const uint32_t hlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, 32);
          const uint32_t hhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), 32);
          const uint64_t head = ((uint64_t)hhi << 32) | hlo;
          if (lane < 32) s_xn[0][lane] = lane < D ? fmaf(__uint_as_float((uint32_t)w), s_sc[lane], s_sh[lane]) : 0.f;
          if (lane == 0) {
            const uint64_t ts = __builtin_amdgcn_s_memrealtime();
            s_ctl[1] = head > tail ? (int)(head - tail < (uint64_t)EB ? head - tail : (uint64_t)EB) : 1;
            s_ctl[4] = (int)(uint32_t)ts;
            s_ctl[5] = (int)(uint32_t)(ts >> 32);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // row and E before the sequence
          if (lane == 0) *seen = (int)want;
          break;
        }
        if ((it & 63) == 63 && wid == 0) {   // exit conditions every wave reaches
          const uint64_t now = __builtin_amdgcn_s_memrealtime();
          if (ld_sys32(&ctl->stop) != 0 || now - last > a.idle_ticks) {
            if (lane == 0) *quit_f = 1;
            break;
          }
        }
      }
    }
    __syncthreads();
    if (s_ctl[0]) break;
    int E = s_ctl[1];
    E = E < 1 ? 1 : (E > EB ? EB : E);
    const uint64_t t_seen = (uint64_t)(uint32_t)s_ctl[4] | ((uint64_t)(uint32_t)s_ctl[5] << 32);
    // ---------------- backlog: wave e fetches row e (published before head)
    if (wid >= 1 && wid < E && lane < 32) {
      const uint64_t ev = tail + (uint64_t)wid;
      const uint32_t tag = (uint32_t)(ev + 1);
      const int sl = (int)(ev % (uint64_t)a.nslots);
      SML_DCHECK(sl >= 0 && sl < a.nslots);
      float xv = 0.f;
      if (lane < D) {
        // the host publishes head after the rows, so the spin normally never runs; bounded
        // so that a wave always reaches the exit conditions
        uint64_t v = ld_sys(&a.req[sl].w[lane]);
        for (int spin = 0; (uint32_t)(v >> 32) != tag && spin < (1 << 20); ++spin) v = ld_sys(&a.req[sl].w[lane]);
        xv = fmaf(__uint_as_float((uint32_t)v), s_sc[lane], s_sh[lane]);
      }
      s_xn[wid][lane] = xv;
    }
    if (E > 1) __syncthreads();   // E == 1: the row was in LDS before the barrier above
    const uint64_t t_load = __builtin_amdgcn_s_memrealtime();
    // ---------------- the stack, ping-pong between the two activation buffers
    const float* in = &s_xn[0][0];
    int in_s = 32;
    float* out = act0;
    for (int l = 0; l < a.nl; ++l) {
      const DenseServeLayer& L = a.L[l];
      const int Kp = dense_serve_kp(L.in), Np = dense_serve_np(L.out), KS = dense_serve_k_slices(L.in, L.out);
      const float4* W = reinterpret_cast<const float4*>(wimg + L.w_off);
      const float* bias = wimg + L.b_off;
      if (E == 1) layer_pass<1>(W, bias, Kp, Np, KS, L.out, L.act, in, in_s, out, part, tid);
      else if (E == 2) layer_pass<2>(W, bias, Kp, Np, KS, L.out, L.act, in, in_s, out, part, tid);
      else if (E <= 4) layer_pass<4>(W, bias, Kp, Np, KS, L.out, L.act, in, in_s, out, part, tid);
      else layer_pass<8>(W, bias, Kp, Np, KS, L.out, L.act, in, in_s, out, part, tid);
      in = out;
      in_s = AS;
      out = out == act0 ? act1 : act0;
    }
    const uint64_t t_comp = __builtin_amdgcn_s_memrealtime();
    // ---------------- results: wave e scores and stores event e
    if (wid < E) {
      const uint64_t ev = tail + (uint64_t)wid;
      const uint32_t tag = (uint32_t)(ev + 1);
      ServeResult* r = a.res + (int)(ev % (uint64_t)a.nslots);
      const float yv = lane < D ? in[wid * AS + lane] : 0.f;
      const float d = lane < D ? yv - s_xn[wid][lane & 31] : 0.f;
      const float se = wave_sum(__fmul_rn(d, d));
      if (lane < D) st_sys(&r->w[lane], tagged(tag, yv));
      if (lane == 0) {
        const float score = pass_score_word(r, tag, D, se);
        pass_flag_words(r, tag, score > a.threshold, t_seen, t_load, t_comp);
      }
    }
    tail += (uint64_t)E;
    passes += 1u;
    events += (uint32_t)E;
    last = __builtin_amdgcn_s_memrealtime();
    pass_done(ctl, a.stats, tail, passes, events, tid);
  }
  pass_exit(ctl, tid);
}

}  // namespace

hipError_t dense_serve_launch(const DenseServeArgs& args, hipStream_t stream) {
  if (dense_serve_check(args.L, args.nl, args.D, args.img_floats)[0] || args.nslots < 64 || !args.img || !args.stats)
    return hipErrorInvalidValue;
  const bool in_lds = dense_serve_in_lds(args.L, args.nl);
  const size_t lds = (size_t)FIXED_FLOATS * 4 + (in_lds ? (size_t)args.img_floats * 4 : 0);
  const void* fn = in_lds ? reinterpret_cast<const void*>(dense_serve_kernel<true>)
                          : reinterpret_cast<const void*>(dense_serve_kernel<false>);
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  if (in_lds) hipLaunchKernelGGL(dense_serve_kernel<true>, dim3(1), dim3(NT), lds, stream, args);
  else hipLaunchKernelGGL(dense_serve_kernel<false>, dim3(1), dim3(NT), lds, stream, args);
  return hipGetLastError();
}

}  // namespace sml
