// Persistent per-event scorer for a FLEET of Dense stacks of one shape: every event names the
// model that scores it (one autoencoder per car, ops/dense_fleet.py trains them).
//
// The ring protocol, the pass, a layer's reduction, the exit conditions and the BIT-IDENTITY
// argument are described in sml_dense_serve_dev.h (KEYED), shared with dense_serve.hip.  What
// differs here:
//   * request word 31 carries the event's model index m as a tagged uint32, so rows have 1..31
//     features.  The host is the only writer of the ring and refuses m >= n_models before it
//     publishes (runtime/serve.cpp: DenseFleetServe::infer); the kernel trusts the word.
//   * the weights are n_models images stacked in device memory, img[n_models][stride], each laid
//     out as dense_serve.hip's single image; ONE layer table holds offsets relative to a model's
//     image.  They are always read from memory (L2 / HBM): a fleet does not fit the LDS.
//   * thr is a device array [n_models]: flag = score > thr[m].  One scale / shift pair for the fleet.
//
// Events cannot share a weight load, so per layer a thread (slice ks, column o) walks the pass's
// events in chunks of up to four: each event of a chunk has its own weight pointer and its own
// accumulator, and the chunk keeps 2 (four events) or 4 (one or two events) 16-byte weight loads
// per event in flight -- at most eight float4 of weights, which leaves launch_bounds(1024)'s 128
// VGPRs without a private segment.  A chunk of three runs the four-event body with the third
// event twice (same image, result dropped).
//
// There is no separate path for a pass whose events all name one model: sharing its weight loads
// through dense_serve.hip's layer_pass beside this code needed a private segment in every unroll
// tried, and a pass of one event is already that kernel's loop (slice_chunk<1, 4>).
#include "sml_dense_serve_dev.h"

namespace sml {
namespace {

using namespace dense_serve_dev;

static_assert(DSV_FLEET_MAXD == KEYW, "the model index follows the widest row");

// Partial sums of slice [g0, g1) of column o for EC events starting at e0, GU weight groups per
// event in flight.  Events e0 .. e0 + n - 1 exist (1 <= n <= EC); the surplus accumulators repeat
// the last of them and are not stored.
template <int EC, int GU>
__device__ __forceinline__ void slice_chunk(const float* __restrict__ img, size_t stride, int w_off,
                                            const int* model, int e0, int n, int g0, int g1, int Np, int o,
                                            const float* in, int in_s, float* part_ko) {
  const float4* wp[EC];
  const float4* xp[EC];
  float acc[EC];
#pragma unroll
  for (int c = 0; c < EC; ++c) {
    const int e = e0 + (c < n ? c : n - 1);
    wp[c] = reinterpret_cast<const float4*>(img + (size_t)model[e] * stride + w_off) + (size_t)g0 * Np + o;
    xp[c] = reinterpret_cast<const float4*>(in + e * in_s);
    acc[c] = 0.f;
  }
  int g = g0;
  for (; g + GU <= g1; g += GU) {
    float4 w[EC][GU];
#pragma unroll
    for (int c = 0; c < EC; ++c)
#pragma unroll
      for (int u = 0; u < GU; ++u) w[c][u] = wp[c][(size_t)u * Np];
#pragma unroll
    for (int c = 0; c < EC; ++c) {
#pragma unroll
      for (int u = 0; u < GU; ++u) acc[c] = fma4(xp[c][g + u], w[c][u], acc[c]);   // row order
      wp[c] += (size_t)GU * Np;
    }
  }
  for (; g < g1; ++g) {
    float4 w[EC];
#pragma unroll
    for (int c = 0; c < EC; ++c) w[c] = wp[c][0];
#pragma unroll
    for (int c = 0; c < EC; ++c) {
      acc[c] = fma4(xp[c][g], w[c], acc[c]);
      wp[c] += Np;
    }
  }
#pragma unroll
  for (int c = 0; c < EC; ++c)
    if (c < n) part_ko[(e0 + c) * Np] = acc[c];
}

// One layer for the pass's E events: in -> out, both in LDS with strides in_s / AS; event e reads
// the image of model[e].
__device__ __forceinline__ void fleet_layer(const float* __restrict__ img, size_t stride, const DenseServeLayer& L,
                                            const int* model, int E, const float* in, int in_s, float* out,
                                            float* part, int tid) {
  const int Kp = dense_serve_kp(L.in), Np = dense_serve_np(L.out), KS = dense_serve_k_slices(L.in, L.out);
  const int G4 = Kp >> 2;
  const int KG = (G4 + KS - 1) / KS;   // groups per slice; the last slices may be short or empty
  if (tid < Np * KS) {
    const int ks = tid / Np, o = tid - ks * Np;
    const int g0 = ks * KG < G4 ? ks * KG : G4;
    const int g1 = g0 + KG < G4 ? g0 + KG : G4;
    float* part_ko = part + (size_t)ks * EB * Np + o;   // part[(ks * EB + e) * Np + o]
    for (int e0 = 0; e0 < E; e0 += 4) {
      const int n = E - e0 < 4 ? E - e0 : 4;
      if (n == 1) slice_chunk<1, 4>(img, stride, L.w_off, model, e0, n, g0, g1, Np, o, in, in_s, part_ko);
      else if (n == 2) slice_chunk<2, 4>(img, stride, L.w_off, model, e0, n, g0, g1, Np, o, in, in_s, part_ko);
      else slice_chunk<4, 2>(img, stride, L.w_off, model, e0, n, g0, g1, Np, o, in, in_s, part_ko);
    }
  }
  layer_finish([img, stride, model, &L](int e) { return img + (size_t)model[e] * stride + L.b_off; }, E, Np, KS, L, out, part, tid);
}

__global__ __launch_bounds__(DSV_NT) void dense_serve_fleet_kernel(DenseFleetServeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ __attribute__((aligned(16))) float s_xn[EB][32];   // the pass's normalised rows
  __shared__ float s_sc[32], s_sh[32];
  __shared__ int s_model[EB];   // the pass's model indices
  __shared__ int s_ctl[8];      // quit, E, -, seen sequence, t_seen lo / hi
  float* const act0 = smem;
  float* const act1 = smem + ACT_FLOATS;
  float* const part = smem + 2 * ACT_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int D = a.D;
  const size_t stride = (size_t)a.stride;
  ServeCtl* const ctl = a.ctl;
  if (tid < 32) {
    s_sc[tid] = (tid < D && a.scale) ? a.scale[tid] : 1.f;
    s_sh[tid] = (tid < D && a.shift) ? a.shift[tid] : 0.f;
  }
  if (tid < 8) s_ctl[tid] = 0;
  if (tid < EB) s_model[tid] = 0;
  __syncthreads();

  uint64_t tail = ld_sys(&ctl->done);
  const uint64_t st0 = ld_sys(a.stats);   // cumulative over launches
  uint32_t passes = (uint32_t)(st0 >> 32), events = (uint32_t)st0;
  uint64_t last = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) st_sys32(&ctl->alive, 1u);
  for (;;) {
    // ---------------- waves 0..3 poll the next request slot (word 31: the model index)
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
        const bool ok = (lane >= D && lane != KEYW) || (uint32_t)(w >> 32) == want;
        if (__ballot(ok) == ~0ull) {
          // the row and its model index arrived with the poll.  head was published after the rows: a
          // head read before the host's store landed only makes this pass smaller
          const uint32_t hlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, 32);
          const uint32_t hhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), 32);
          const uint64_t head = ((uint64_t)hhi << 32) | hlo;
          if (lane < 32) s_xn[0][lane] = lane < D ? fmaf(__uint_as_float((uint32_t)w), s_sc[lane], s_sh[lane]) : 0.f;
          if (lane == KEYW) {
            SML_DCHECK((uint32_t)w < (uint32_t)a.n_models);
            s_model[0] = (int)(uint32_t)w;
          }
          if (lane == 0) {
            const uint64_t ts = __builtin_amdgcn_s_memrealtime();
            s_ctl[1] = head > tail ? (int)(head - tail < (uint64_t)EB ? head - tail : (uint64_t)EB) : 1;
            s_ctl[4] = (int)(uint32_t)ts;
            s_ctl[5] = (int)(uint32_t)(ts >> 32);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // row, index and E before the sequence
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
    // ---------------- backlog: wave e fetches row e and its model index (published before head)
    if (wid >= 1 && wid < E && lane < 32) {
      const uint64_t ev = tail + (uint64_t)wid;
      const uint32_t tag = (uint32_t)(ev + 1);
      const int sl = (int)(ev % (uint64_t)a.nslots);
      SML_DCHECK(sl >= 0 && sl < a.nslots);
      float xv = 0.f;
      if (lane < D || lane == KEYW) {
        // the host publishes head after the rows, so the spin normally never runs; bounded
        // so that a wave always reaches the exit conditions
        uint64_t v = ld_sys(&a.req[sl].w[lane]);
        for (int spin = 0; (uint32_t)(v >> 32) != tag && spin < (1 << 20); ++spin) v = ld_sys(&a.req[sl].w[lane]);
        if (lane == KEYW) {
          SML_DCHECK((uint32_t)v < (uint32_t)a.n_models);
          s_model[wid] = (int)(uint32_t)v;
        } else {
          xv = fmaf(__uint_as_float((uint32_t)v), s_sc[lane], s_sh[lane]);
        }
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
      fleet_layer(a.img, stride, a.L[l], s_model, E, in, in_s, out, part, tid);
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
        pass_flag_words(r, tag, score > a.thr[s_model[wid]], t_seen, t_load, t_comp);
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

hipError_t dense_fleet_serve_launch(const DenseFleetServeArgs& args, hipStream_t stream) {
  if (dense_fleet_serve_check(args.L, args.nl, args.D, args.img_floats, args.stride, args.n_models)[0] ||
      args.nslots < 64 || !args.img || !args.thr || !args.stats)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)FIXED_FLOATS * 4;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dense_serve_fleet_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dense_serve_fleet_kernel, dim3(1), dim3(NT), lds, stream, args);
  return hipGetLastError();
}

}  // namespace sml
