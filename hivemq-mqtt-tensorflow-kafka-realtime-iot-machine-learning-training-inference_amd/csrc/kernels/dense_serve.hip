// Persistent per-event scorer for Dense stacks of any depth: 1..8 Dense layers, every width
// up to 512, rows of up to 32 features, the last layer one unit per feature (an autoencoder
// wider or deeper than the reference's 18-14-7-7-18, which ae_serve.hip is built around).
//
// Same protocol and semantics as ae_serve.hip: LL-framed request / result slots (sml_ops.h),
// xn = x * scale + shift, y = stack(xn), score = mean((y - xn)^2) over the D features,
// flag = score > threshold, the three timing words, `done`, `alive`, `stop` and the idle
// timeout.  fp32 throughout (the score is compared against a threshold).
//
// One workgroup of 1024 threads.  The weights are an IMAGE built once per server
// (ops/serve.py: dense_serve_image): per layer float4 img[Kp / 4][Np] with img[g][o] =
// W[4g .. 4g + 3][o] (Kp = in rounded up to 4, Np = out rounded up to 32, zero-padded),
// followed by the padded bias [Np]; threads of consecutive o load consecutive 16 bytes.  The
// kernel body is a template on where that image lives:
//   "lds"     the whole image is copied to LDS at launch (it fits beside the activation and
//             partial-sum buffers: DSV_LDS_IMAGE_BYTES);
//   "stream"  every pass streams the image from L2.
//
// A PASS serves E events at once, 1 <= E <= EB = 8.  Waves 0..3 poll the next request slot
// together with the host's head counter.  With one event outstanding E = 1 and the row has
// arrived with the poll; with a backlog E = min(head - tail, EB) and wave e fetches row e
// (rows below head were published before it; tag check, bounded spin).  Per layer the Np
// output columns times KS slices of the reduction are spread over the threads (KS: a power
// of two fixed by the layer's shape, dense_serve_k_slices); a thread loads each weight group
// once and uses it for every event of the pass, reading the events' activations as broadcast
// float4 from LDS into per-event accumulators (registers: the loops over events are fully
// unrolled).  The partial sums meet in LDS, are added to the bias in slice order 0 .. KS - 1,
// and the activation is applied.  Two workgroup barriers per layer.
//
// BIT-IDENTITY.  The sum of one output of one event is bias + p_0 + .. + p_{KS-1}, each p_s
// one fmaf chain over the slice's rows in order from 0.0f: it depends on the layer's shape
// only, never on E or on the event's position in the pass.  The pass is instantiated for 1,
// 2, 4 and 8 accumulators (E is rounded up; the surplus accumulators read stale activations
// and their results are dropped), every instantiation with the same chains, and the score is
// computed by one wave per event with the same lane-butterfly.  So an event's result bits do
// not depend on how the ring happened to batch it.
//
// After each pass thread 0 stores `done` and ONE 8-byte word {passes << 32 | events}
// (cumulative over launches) into the server's host-mapped stats block, after the pass's
// result words were issued: tests read it to prove which path ran.
//
// Exit conditions every wave reaches: the host's stop flag or `idle` without a request, decided
// by wave 0 every 64 polls and broadcast through LDS at the next barrier.  Every branch around
// a barrier is block-uniform: it depends only on kernel arguments and on values broadcast
// through LDS (quit, E).  Every spin on host memory is bounded.
#include "sml_common.h"
#include "sml_ops.h"
#include "sml_serve_dev.h"

namespace sml {
namespace {

using namespace serve_dev;

constexpr int NT = DSV_NT, EB = DSV_EB;
constexpr int AS = DSV_MAXW;             // stride of an event's activations in LDS (floats)
constexpr int ACT_FLOATS = EB * AS;      // one activation buffer
constexpr int PART_FLOATS = EB * NT;     // partial sums [KS][EB][Np], Np * KS <= NT
constexpr int FIXED_FLOATS = 2 * ACT_FLOATS + PART_FLOATS;   // dynamic LDS before the image

static_assert(DSV_MAXW % 4 == 0 && DSV_MAXW % DSV_TILE == 0, "padded widths stay within DSV_MAXW");
static_assert(FIXED_FLOATS * 4 + DSV_LDS_IMAGE_BYTES + 2048 <= 160 * 1024, "LDS budget");

__device__ __forceinline__ float fma4(const float4 x, const float4 w, float a) {
  return fmaf(x.w, w.w, fmaf(x.z, w.z, fmaf(x.y, w.y, fmaf(x.x, w.x, a))));
}

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
  __syncthreads();
  for (int it = tid; it < EC * Np; it += NT) {
    const int e = it / Np, o = it - e * Np;
    float s = bias[o];
    for (int ks = 0; ks < KS; ++ks) s += part[(ks * EB + e) * Np + o];
    out[e * AS + o] = o < out_n ? act_fwd(act, s) : 0.f;   // padded columns feed zero rows
  }
  __syncthreads();
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
    // ---------------- waves 0..3 poll the next request slot as in lstm_serve_wide.hip (staggered,
    // one synchronous cache-bypassing load per poll: lanes 0..31 the slot's words, lanes
    // 32..63 the host's head counter); the other waves wait at the barrier.  Two polling waves
    // may find the row at once and publish the same row and (possibly) different E: the barrier
    // below orders both before any reader, so every thread sees ONE value of E.
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
        const float score = se / (float)D;
        st_sys(&r->w[kServeScore], tagged(tag, score));
        st_sys(&r->w[kServeFlag], tagged_u(tag, score > a.threshold ? 1u : 0u));
        st_sys(&r->w[kServeTLoad], tagged_u(tag, (uint32_t)(t_load - t_seen)));
        st_sys(&r->w[kServeTComp], tagged_u(tag, (uint32_t)(t_comp - t_seen)));
        st_sys(&r->w[kServeTDone], tagged_u(tag, (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_seen)));
      }
    }
    tail += (uint64_t)E;
    passes += 1u;
    events += (uint32_t)E;
    last = __builtin_amdgcn_s_memrealtime();
    // every wave has issued its result stores and is done with s_xn / s_ctl before the next poll
    __syncthreads();
    if (tid == 0) {
      st_sys(&ctl->done, tail);   // back-pressure hint only: results carry their own tags
      st_sys(a.stats, ((uint64_t)passes << 32) | (uint64_t)events);
    }
  }
  __syncthreads();
  wait_stores();
  if (tid == 0) st_sys32(&ctl->alive, 0u);
}

}  // namespace

const char* dense_serve_check(const DenseServeLayer* L, int nl, int D, int64_t img_floats) {
  if (D < 1 || D > 32) return "rows must have 1..32 features (a request slot holds 32 words)";
  if (nl < 1 || nl > DSV_MAXLAYERS) return "the stack must have 1..8 Dense layers";
  int dim = D;
  int64_t total = 0;
  for (int l = 0; l < nl; ++l) {
    if (L[l].out < 1 || L[l].out > DSV_MAXW) return "Dense layers must have 1..512 units";
    if (L[l].in != dim) return "a layer's input width must match the layer below";
    if (L[l].act < ACT_LINEAR || L[l].act > ACT_SIGMOID) return "activations must be linear, relu, tanh or sigmoid";
    const int64_t wn = (int64_t)dense_serve_kp(L[l].in) * dense_serve_np(L[l].out);
    if (L[l].w_off < 0 || (L[l].w_off & 3) || (int64_t)L[l].w_off + wn > img_floats || L[l].b_off < 0 ||
        (L[l].b_off & 3) || (int64_t)L[l].b_off + dense_serve_np(L[l].out) > img_floats)
      return "a layer's weights lie outside the weight image";
    total += dense_serve_layer_floats(L[l].in, L[l].out);
    dim = L[l].out;
  }
  if (dim != D) return "the last layer must have one unit per feature";
  if (img_floats != total) return "the weight image has the wrong length";
  return "";
}

bool dense_serve_in_lds(const DenseServeLayer* L, int nl) {
  int64_t bytes = 0;
  for (int l = 0; l < nl && l < DSV_MAXLAYERS; ++l) bytes += 4 * (int64_t)dense_serve_layer_floats(L[l].in, L[l].out);
  return bytes <= DSV_LDS_IMAGE_BYTES;
}

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
