// Persistent per-event LSTM forecaster for WIDE stacks: any LSTM layer with more than 32
// units or inputs (up to 512), or a Dense head over more than 32 inputs.
//
// Same protocol and semantics as lstm_serve.hip (LL-framed request / result slots, per-key
// window ring + count + last forecast in HBM, append -> score against the key's previous
// forecast -> once the key has T events run the whole stack over the window from zero state,
// flags 0 / 1 / 2, stop flag and idle timeout).  What differs is where the weights live: a
// wide layer's [W ; U] fits neither LDS nor one workgroup's registers as fp32 (LSTM(512) over
// 512 inputs is 8 MB), so LSTMServe builds, once per server, a bf16 image of every LSTM
// layer's W and U (lstm_serve_wide_image) and this kernel streams them from L2 / HBM.
//
// One workgroup of 1024 threads, no cross-workgroup synchronisation.  Widths are zero-padded
// to multiples of 32 (up, Kp); a padded unit has zero weights and bias, so its gates are
// i = f = o = 1/2, g~ = act(0) = 0 and c = h = 0 exactly, and a padded input row multiplies
// a zero weight.  Per LSTM layer and event:
//   1. input projection, all steps at once: zx[t, g] = b[g] + sum_k x[t, k] W[k, g] for the
//      T <= 64 steps of the layer's input sequence (in LDS).  A thread owns one gate column g
//      and 8 steps; it reads W once per 8 steps as 16-byte groups of 8 input rows.  zx goes
//      to a global fp32 scratch [T, 4 up] (512 KB at u = 512, T = 64: it cannot live in LDS)
//      with agent-scope stores; every wave drains them before the barrier that ends the phase.
//   2. recurrence, step by step: z = zx[t] + h_{t-1} . U.  The 4 up gate columns times KS
//      slices of the reduction are spread over the 1024 threads (KS = 4 .. 1: narrow layers
//      split k so every thread has work); partial sums meet in LDS; thread j < up then owns
//      unit j: gates, cell state (a register), h.  Two workgroup barriers per step.  A layer
//      of up <= 128 units keeps its slice of U in registers for the whole recurrence (at most
//      8 x 16 bytes per thread), so its steps touch no memory but LDS; wider layers stream U
//      from L2 every step (2 MB at u = 512: the step is bound by that stream).  zx[t + 1] is
//      requested while step t runs.
// RepeatVector copies rows in LDS; the Dense / TimeDistributed head (the last layer) reads
// the last LSTM step's h and the fp32 master weights, 32 threads per output feature.
//
// PRECISION CONTRACT -- the exact rounding points (tests/helpers/lstm_serve_ref.py mirrors
// them with rounded=True).  Round-to-nearest-even to bf16:
//   * W and U of every LSTM layer, once, when the images are built;
//   * the normalised window x (the rows of the key's ring), when it is placed in LDS;
//   * h_t of every LSTM layer, where it is stored for the next step's recurrence
//     (h_{t-1} . U) and as the next layer's input sequence (also through a RepeatVector).
// Everything else is fp32: the bf16 pairs are multiplied and summed into fp32 accumulators
// by v_dot2_f32_bf16; biases, zx, gates, cell state, the h that the Dense head reads (NOT
// rounded), the head's weights and sums, the score and the forecast are fp32.
//
// Exit conditions every wave reaches: the host's stop flag or `idle` without a request
// (decided by wave 0, broadcast through LDS at the next barrier).  Every branch around a
// barrier is block-uniform: it depends only on kernel arguments (lanes among them) and on
// values broadcast through LDS (quit, the key's event count).
//
// LANES.  The launch has a.lanes workgroups; workgroup i is lane i, a complete server of its
// own: control block a.ctl[i] (its `done`, its `alive`), request and result rings a.req / a.res
// + i * nslots, projection scratch a.wide_zx + i * rows * gmax.  The host sends key k to lane
// k % lanes, so a key's window, count and forecast (indexed by key, shared arrays) are touched
// by one lane only and in the key's event order: every result has the bits the one-lane server
// gives.  Weight images, master weights, scale and shift are read-only and shared.  No lane
// waits for another: there is no grid barrier and no lane reads what another lane computes,
// so the launch is correct whether its workgroups run side by side or one after the other
// (a lane that has not started yet only delays its own keys).  Waiting is what a resident
// grid cannot afford: a workgroup spinning on a lane that the dispatcher has not placed yet
// would never be released.
//
// LEAVING is collective and one-way.  With one idle timer per lane a quiet lane would leave
// while a busy one keeps the launch (and the stream) alive, and the quiet lane's next event
// would wait until the busy lane goes quiet too, because the host can only relaunch a
// drained stream.  So the lanes share two words of lane 0's host-mapped control block, read
// and written at system scope like `stop` (host memory: no per-XCD L2 holds a copy):
//   active  s_memrealtime of the latest pick-up on any lane (stored by the lane that picks up);
//   leave   the latch.  A lane whose own last event is idle_ticks old reads `active`; if the
//           whole server has been idle that long, or the host's stop flag is up, it sets
//           `leave`.  Every lane tests `leave` every 64 polls and after each event and leaves
//           once it is set.  The host clears it before each launch, which it issues only on
//           a drained stream, so no lane of the previous launch can still set it.
// Races, all benign.  (1) A lane picks up an event as another sets the latch (the `active`
// store still in flight, or the clocks of two XCDs a few ticks apart; the age is compared
// signed): the lane finishes the event, stores its results and `done`, then leaves.  (2) An
// event published after the latch, or to a lane that has left, stays in its ring; the host
// sees the stream drain, relaunches, and every lane resumes at its own `done`.  (3) Two lanes
// set the latch at once: same value.  With one lane the two words are not used at all.
#include <type_traits>

#include "sml_common.h"
#include "sml_ops.h"
#include "sml_serve_dev.h"

namespace sml {
namespace {

using namespace serve_dev;

constexpr int WNT = 1024;      // threads of a lane's workgroup
constexpr int KEY_WORD = 31;   // request word carrying the car key
constexpr int TB = 8;          // steps of the input projection per thread

__device__ __forceinline__ float sigm(float z) { return 1.0f / (1.0f + __expf(-z)); }
__device__ __forceinline__ float act_lstm(int a, float z) { return a == ACT_RELU ? fmaxf(z, 0.f) : tanhf(z); }

// Per-key state and the zx scratch are written by one wave and read by others later:
// agent-scope relaxed atomics go around the per-CU L1.
template <typename T>
__device__ __forceinline__ T ld_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void st_agent(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// fp32 bits -> nearest-even bf16 bits
__host__ __device__ inline uint32_t bf16_bits(uint32_t u) { return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16; }
__device__ __forceinline__ uint16_t bf16r(float x) { return (uint16_t)bf16_bits(__float_as_uint(x)); }

// acc + w[0] v[0] + w[1] v[1] on one pair of bf16 values
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dot2(uint32_t w, uint32_t v, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2v, w), __builtin_bit_cast(bf16x2v, v), acc, false);
}
// the 8 rows of one 16-byte group: one chain, or two
__device__ __forceinline__ float dot8(const uint4 w, const uint4 v, float a) {
  return dot2(w.w, v.w, dot2(w.z, v.z, dot2(w.y, v.y, dot2(w.x, v.x, a))));
}
__device__ __forceinline__ void dot8(const uint4 w, const uint4 v, float& a0, float& a1) {
  a0 = dot2(w.x, v.x, a0);
  a1 = dot2(w.y, v.y, a1);
  a0 = dot2(w.z, v.z, a0);
  a1 = dot2(w.w, v.w, a1);
}

// slices of a layer's recurrent reduction: the largest power of two with 4 up * KS <= WNT and
// at least 8 rows per slice (16-byte groups); 1 for up >= 160
__host__ __device__ inline int k_slices(int up) {
  int ks = 1;
  while (4 * up * ks * 2 <= WNT && up / (ks * 2) >= 8 && (up / (ks * 2)) % 8 == 0) ks *= 2;
  return ks;
}

// sum_k v[k] * W[k, g] over the 8-row groups [g0, g1) of an image, v: bf16 values in LDS.
// g1 - g0 is a multiple of 4 (a streamed layer has up >= 160, one slice, up / 8 groups and up
// a multiple of 32): four 16-byte loads in flight per trip and no remainder loop (a `#pragma
// unroll 4` with its remainder loop cost the kernel a 36-byte private segment).
__device__ __forceinline__ float dot_groups(const uint4* __restrict__ img, int G, int g, int g0, int g1,
                                            const uint16_t* v) {
  float a0 = 0.f, a1 = 0.f;
  const uint4* wp = img + (size_t)g0 * G + g;
  const uint4* vp = reinterpret_cast<const uint4*>(v);
  for (int i = g0; i < g1; i += 4, wp += 4 * (size_t)G) {
    const uint4 w0 = wp[0], w1 = wp[G], w2 = wp[2 * (size_t)G], w3 = wp[3 * (size_t)G];
    dot8(w0, vp[i], a0, a1);
    dot8(w1, vp[i + 1], a0, a1);
    dot8(w2, vp[i + 2], a0, a1);
    dot8(w3, vp[i + 3], a0, a1);
  }
  return a0 + a1;
}

// The recurrence of one LSTM layer over tcur steps, instantiated for a register-resident and
// for a streamed U, so that neither carries the other's registers.  Returns h of the last step.
template <bool CACHED>
__device__ __forceinline__ float wide_steps(const uint4* __restrict__ uimg, const float* zx, int up, int G, int KS,
                                            int KG, int tcur, int act, int ret, uint16_t* seq, int S, float* s_part,
                                            uint16_t* s_hq, float* s_hf, int tid) {
  float c = 0.f, h = 0.f;
  const int cks = tid / G, cg = tid - cks * G;
  uint4 wc[CACHED ? 8 : 1];
  if constexpr (CACHED) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      wc[i] = (tid < G * KS && i < KG) ? uimg[(size_t)(cks * KG + i) * G + cg] : uint4{0u, 0u, 0u, 0u};
  }
  float zn[4] = {0.f, 0.f, 0.f, 0.f};
  if (tid < up) {
#pragma unroll
    for (int q = 0; q < 4; ++q) zn[q] = ld_agent(&zx[q * up + tid]);
  }
  for (int t = 0; t < tcur; ++t) {
    float zv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) zv[q] = zn[q];
    if (tid < up && t + 1 < tcur) {   // the next step's, requested a step ahead
#pragma unroll
      for (int q = 0; q < 4; ++q) zn[q] = ld_agent(&zx[(size_t)(t + 1) * G + q * up + tid]);
    }
    if (t > 0) {   // h_{-1} = 0
      if constexpr (CACHED) {
        if (tid < G * KS) {
          const uint4* vp = reinterpret_cast<const uint4*>(s_hq) + cks * KG;
          float a0 = 0.f, a1 = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (i < KG) dot8(wc[i], vp[i], a0, a1);
          s_part[tid] = a0 + a1;
        }
      } else {
        for (int item = tid; item < G * KS; item += WNT) {
          const int ks = item / G, g = item - ks * G;
          s_part[item] = dot_groups(uimg, G, g, ks * KG, (ks + 1) * KG, s_hq);
        }
      }
    }
    __syncthreads();
    if (tid < up) {
      if (t > 0) {
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
          for (int q = 0; q < 4; ++q) zv[q] += s_part[ks * G + q * up + tid];
        }
      }
      const float ig = sigm(zv[0]), fg = sigm(zv[1]);
      const float gg = act_lstm(act, zv[2]), og = sigm(zv[3]);
      c = fmaf(fg, c, ig * gg);
      h = og * act_lstm(act, c);
      const uint16_t hb = bf16r(h);
      s_hq[tid] = hb;
      s_hf[tid] = h;
      if (ret) seq[t * S + tid] = hb;
    }
    __syncthreads();
  }
  return h;
}

__global__ __launch_bounds__(WNT) void lstm_serve_wide_kernel(LstmServeArgs a, int rows, int S, int zx_lane) {
  extern __shared__ __attribute__((aligned(16))) uint16_t smem_w[];
  __shared__ __attribute__((aligned(16))) float s_part[4 * LSW_MAXW];   // partial sums [KS][4 up] / head [32][32]
  __shared__ __attribute__((aligned(16))) uint16_t s_hq[LSW_MAXW];      // h_{t-1}, bf16
  __shared__ __attribute__((aligned(16))) float s_hf[LSW_MAXW];         // h of the last step computed, fp32
  __shared__ float s_xrow[32], s_pred[32], s_sc[32], s_sh[32];
  __shared__ int s_ctl[8];   // quit, key, count, seen sequence, t_seen lo / hi
  uint16_t* seq = smem_w;    // [rows][S]: the current layer's input / output sequence, bf16
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int D = a.D, T = a.T;
  // this lane's control block, rings and scratch; stop / leave / active are lane 0's
  const int ln = blockIdx.x;
  const bool multi = a.lanes > 1;
  ServeCtl* const ctl = a.ctl + ln;
  ServeCtl* const ctl0 = a.ctl;
  const ServeReq* const req = a.req + (size_t)ln * a.nslots;
  ServeResult* const res = a.res + (size_t)ln * a.nslots;
  float* const zx_mine = a.wide_zx + (size_t)ln * zx_lane;
  if (tid < 32) {
    s_sc[tid] = (tid < D && a.scale) ? a.scale[tid] : 1.f;
    s_sh[tid] = (tid < D && a.shift) ? a.shift[tid] : 0.f;
  }
  if (tid < 8) s_ctl[tid] = 0;
  __syncthreads();

  uint64_t tail = ld_sys(&ctl->done);
  uint64_t last = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) st_sys32(&ctl->alive, 1u);
  for (;;) {
    // ---------------- waves 0..3 poll the next request slot as in lstm_serve.hip (staggered,
    // one synchronous cache-bypassing load per poll); the other waves wait at the barrier
    const int slot = (int)(tail % (uint64_t)a.nslots);
    const uint32_t want = (uint32_t)(tail + 1);
    if (wid < 4) {
      typedef __attribute__((address_space(3))) volatile int lds_vint;   // ds_* accesses, not flat
      lds_vint* seen = (lds_vint*)&s_ctl[3];
      lds_vint* quit_f = (lds_vint*)&s_ctl[0];
      const uint64_t* wp = &req[slot].w[lane & 31];
      if (wid == 1) __builtin_amdgcn_s_sleep(10);
      else if (wid == 2) __builtin_amdgcn_s_sleep(20);
      else if (wid == 3) __builtin_amdgcn_s_sleep(30);
      for (uint32_t it = 0;; ++it) {
        if (*seen == (int)want || *quit_f) break;
        const uint64_t w = ld_sys(wp);
        const bool ok = (lane >= D && lane != KEY_WORD) || lane >= 32 || (uint32_t)(w >> 32) == want;
        if (__ballot(ok) == ~0ull) {
          if (lane < D) s_xrow[lane] = fmaf(__uint_as_float((uint32_t)w), s_sc[lane], s_sh[lane]);
          if (lane == KEY_WORD) s_ctl[1] = (int)(uint32_t)w;
          if (lane == 0) {
            const uint64_t ts = __builtin_amdgcn_s_memrealtime();
            s_ctl[4] = (int)(uint32_t)ts;
            s_ctl[5] = (int)(uint32_t)(ts >> 32);
            if (multi) st_sys(&ctl0->active, ts);   // the server is busy: no lane may call it idle
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // row and key before the sequence
          if (lane == 0) *seen = (int)want;
          break;
        }
        if ((it & 63) == 63 && wid == 0) {   // exit conditions every wave reaches
          const uint64_t now = __builtin_amdgcn_s_memrealtime();
          bool out = ld_sys32(&ctl0->stop) != 0;
          if (!multi) {
            out = out || now - last > a.idle_ticks;
          } else {
            out = out || ld_sys32(&ctl0->leave) != 0;
            // this lane is idle: is the whole server?  (signed: clocks of two XCDs may differ)
            if (!out && now - last > a.idle_ticks)
              out = (int64_t)(now - ld_sys(&ctl0->active)) > (int64_t)a.idle_ticks;
            if (out && lane == 0) st_sys32(&ctl0->leave, 1u);   // one-way: every lane follows
          }
          if (out) {
            if (lane == 0) *quit_f = 1;
            break;
          }
        }
      }
    }
    __syncthreads();
    if (s_ctl[0]) break;
    int key = s_ctl[1];
    key = key < 0 ? 0 : (key >= a.nkeys ? a.nkeys - 1 : key);   // the host validates; never leave the table
    float* hist = a.hist + (int64_t)key * T * D;
    float* lastp = a.lastpred + (int64_t)key * D;
    // events of this key before this one and its previous forecast: read once, broadcast, so
    // every wave takes the same branches
    if (tid == 0) s_ctl[2] = ld_agent(&a.hcount[key]);
    if (tid >= 64 && tid < 64 + D) s_pred[tid - 64] = ld_agent(&lastp[tid - 64]);
    __syncthreads();
    const int cnt = s_ctl[2];
    const bool full = cnt + 1 >= T;
    // ---------------- append the event, score it against the previous forecast
    float err = 0.f;
    if (tid < D) {
      const float xn = s_xrow[tid];
      st_agent(&hist[(cnt % T) * D + tid], xn);
      if (cnt >= T) {
        const float d = xn - s_pred[tid];
        err = d * d;
      }
    }
    if (wid == 0) err = wave_sum(err);
    // ---------------- the window, oldest first, bf16-rounded, into seq [t][k < 32] (columns
    // past D are zero; the newest row comes from LDS, its ring slot still holds the evicted one)
    if (full) {
      const int rot = (cnt + 1) % T;   // window step t is ring slot (t + rot) mod T
      for (int e = tid; e < T * 32; e += WNT) {
        const int t = e >> 5, k = e & 31;
        float v = 0.f;
        if (k < D) {
          int r = t + rot;
          r = r >= T ? r - T : r;
          v = t == T - 1 ? s_xrow[k] : ld_agent(&hist[r * D + k]);
        }
        seq[t * S + k] = bf16r(v);
      }
    }
    __syncthreads();
    const uint64_t t_rec = __builtin_amdgcn_s_memrealtime();   // key state + window gathered
    if (full) {
      int tcur = T, li = 0;
      for (int l = 0; l < a.nl; ++l) {
        const LstmServeLayer& L = a.L[l];
        if (L.kind == LS_LSTM) {
          const int up = lstm_serve_wide_pad(L.u), Kp = lstm_serve_wide_pad(L.in), G = 4 * up;
          const uint4* wimg = reinterpret_cast<const uint4*>(a.wide_w[li]);
          const uint4* uimg = reinterpret_cast<const uint4*>(a.wide_u[li]);
          const float* bias = a.wide_b[li];
          float* zx = zx_mine;
          // ---- 1. input projection: thread = (column g, block of TB steps)
          const int ntb = (tcur + TB - 1) / TB;
          for (int item = tid; item < G * ntb; item += WNT) {
            const int tb = item / G, g = item - tb * G, t0 = tb * TB;
            int xr[TB];   // row offsets, in 16-byte groups
#pragma unroll
            for (int q = 0; q < TB; ++q) xr[q] = (t0 + q < tcur ? t0 + q : tcur - 1) * (S / 8);
            float acc[TB];
            const float bg = bias[g];
#pragma unroll
            for (int q = 0; q < TB; ++q) acc[q] = bg;
            const uint4* wp = wimg + g;
            const uint4* xs = reinterpret_cast<const uint4*>(seq);
            for (int i = 0; i < Kp / 8; ++i, wp += G) {
              const uint4 w = *wp;
#pragma unroll
              for (int q = 0; q < TB; ++q) acc[q] = dot8(w, xs[xr[q] + i], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < TB; ++q)
              if (t0 + q < tcur) st_agent(&zx[(size_t)(t0 + q) * G + g], acc[q]);
          }
          if (tid < up) s_hq[tid] = 0;
          wait_stores();   // zx is in L2 before any wave passes the barrier
          __syncthreads();
          // ---- 2. recurrence
          const int KS = k_slices(up), KG = up / KS / 8;   // slices, 8-row groups per slice
          // up <= 128: this thread's slice of its one column of U stays in registers
          // (one item per thread, at most 8 groups); wider: KS = 1 and up / 8 groups, a multiple of 4
          const bool cached = up <= 128;
          const float h = cached ? wide_steps<true>(uimg, zx, up, G, KS, KG, tcur, L.act, L.ret, seq, S, s_part, s_hq,
                                                    s_hf, tid)
                                 : wide_steps<false>(uimg, zx, up, G, KS, KG, tcur, L.act, L.ret, seq, S, s_part, s_hq,
                                                     s_hf, tid);
          if (!L.ret && tid < up) seq[tid] = bf16r(h);
          tcur = L.ret ? tcur : 1;
          ++li;
        } else if (L.kind == LS_REPEAT) {
          // row 0 holds one vector (the previous layer's h_T) over the whole padded stride
          for (int e = tid; e < (L.n - 1) * S; e += WNT) seq[S + e] = seq[e % S];
          tcur = L.n;
        } else {   // the Dense / TimeDistributed head on the last step: fp32 h, fp32 master weights
          const int U = L.u, o = tid & 31, kp = tid >> 5;
          float acc = 0.f;
          if (o < U)
            for (int k = kp; k < L.in; k += 32) acc = fmaf(s_hf[k], a.wts[L.woff + k * U + o], acc);
          s_part[kp * 32 + o] = acc;
          __syncthreads();
          if (tid < U) {
            float s = a.wts[L.boff + tid];
            for (int p = 0; p < 32; ++p) s += s_part[p * 32 + tid];
            s_pred[tid] = s;
          }
        }
        __syncthreads();
      }
    }
    const uint64_t t_comp = __builtin_amdgcn_s_memrealtime();
    const uint64_t t_seen = (uint64_t)(uint32_t)s_ctl[4] | ((uint64_t)(uint32_t)s_ctl[5] << 32);
    // ---------------- results (wave 0), the key's state, completion counter
    // the latch, requested before the result stores so that its round trip hides behind them
    uint32_t leave = 0;
    if (multi && tid == 0) leave = ld_sys32(&ctl0->leave);
    if (wid == 0) {
      ServeResult* r = res + slot;
      const float p = (full && lane < D) ? s_pred[lane] : 0.f;
      if (lane < D) {
        st_sys(&r->w[lane], tagged(want, p));
        if (full) st_agent(&lastp[lane], p);
      }
      if (lane == 0) {
        const float score = cnt >= T ? err / (float)D : __builtin_nanf("");
        const uint32_t flag = cnt >= T ? (score > a.threshold ? 1u : 0u) : 2u;
        st_agent(&a.hcount[key], cnt + 1);
        st_sys(&r->w[kServeScore], tagged(want, score));
        st_sys(&r->w[kServeFlag], tagged_u(want, flag));
        st_sys(&r->w[kServeTLoad], tagged_u(want, (uint32_t)(t_rec - t_seen)));
        st_sys(&r->w[kServeTComp], tagged_u(want, (uint32_t)(t_comp - t_seen)));
        st_sys(&r->w[kServeTDone], tagged_u(want, (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_seen)));
        st_sys(&ctl->done, tail + 1);
      }
    }
    tail += 1;
    last = __builtin_amdgcn_s_memrealtime();
    wait_stores();     // key state stored before the next event may read it
    if (leave) s_ctl[0] = 1;   // reaches all 16 waves through LDS, as quit does
    __syncthreads();
  }
  __syncthreads();
  wait_stores();
  if (tid == 0) st_sys32(&ctl->alive, 0u);
}

}  // namespace

bool lstm_serve_is_wide(const LstmServeArgs& x) {
  int nlstm = 0;
  for (int l = 0; l < x.nl && l < LS_MAXLAYERS; ++l) {
    const LstmServeLayer& L = x.L[l];
    if (L.kind == LS_LSTM && (L.u > 32 || L.in > 32)) return true;
    if (L.kind == LS_DENSE && L.in > 32) return true;
    nlstm += L.kind == LS_LSTM;
  }
  return nlstm > 4;   // more LSTM layers than the LDS-resident kernels hold in registers
}

const char* lstm_serve_wide_check(const LstmServeArgs& x) {
  if (x.D < 1 || x.D > 31) return "rows must have 1..31 features (request word 31 carries the key)";
  if (x.T < 1 || x.T > LSW_MAXT) return "look_back must be 1..64";
  if (x.nl < 1 || x.nl > LS_MAXLAYERS) return "1..8 layers";
  int dim = x.D, tlen = x.T, nlstm = 0;
  for (int l = 0; l < x.nl; ++l) {
    const LstmServeLayer& L = x.L[l];
    if (L.kind == LS_LSTM) {
      if (L.u < 1 || L.u > LSW_MAXW) return "LSTM layers must have 1..512 units";
      if (L.in != dim || L.in > LSW_MAXW) return "layer inputs must be 1..512 wide and match the layer below";
      dim = L.u;
      tlen = L.ret ? tlen : 1;
      ++nlstm;
    } else if (L.kind == LS_REPEAT) {
      if (tlen != 1 || L.n < 1 || L.n > LSW_MAXT) return "RepeatVector needs a single vector and 1..64 repeats";
      tlen = L.n;
    } else if (L.kind == LS_DENSE) {
      if (l != x.nl - 1) return "a stack with layers wider than 32 takes a Dense layer only as its head";
      if (L.in != dim || L.in > LSW_MAXW) return "the head's input must be 1..512 wide and match the layer below";
      if (L.u != x.D) return "the head must produce one value per feature";
      dim = L.u;
    } else {
      return "unknown layer kind";
    }
  }
  if (x.L[x.nl - 1].kind != LS_DENSE) return "the stack must end in a Dense head";
  if (nlstm < 1) return "the stack needs an LSTM layer";
  return "";
}

LstmServeWideDims lstm_serve_wide_dims(const LstmServeArgs& x) {
  LstmServeWideDims d{x.T, 32, 128};
  for (int l = 0; l < x.nl && l < LS_MAXLAYERS; ++l) {
    const LstmServeLayer& L = x.L[l];
    if (L.kind == LS_LSTM) {
      const int up = lstm_serve_wide_pad(L.u), kp = lstm_serve_wide_pad(L.in);
      d.stride = up > d.stride ? up : d.stride;
      d.stride = kp > d.stride ? kp : d.stride;
      d.gmax = 4 * up > d.gmax ? 4 * up : d.gmax;
    } else if (L.kind == LS_REPEAT) {
      d.rows = L.n > d.rows ? L.n : d.rows;
    }
  }
  return d;
}

size_t lstm_serve_wide_lds_bytes(const LstmServeArgs& x) {
  const LstmServeWideDims d = lstm_serve_wide_dims(x);
  return (size_t)d.rows * d.stride * sizeof(uint16_t);
}

void lstm_serve_wide_image(const float* w, int K, int u, int Kp, int up, uint16_t* out) {
  const int G = 4 * up;
  for (int k = 0; k < Kp; ++k)
    for (int g = 0; g < G; ++g) {
      const int q = g / up, j = g - q * up;
      uint32_t bits = 0;
      if (k < K && j < u) {
        const float v = w[(size_t)k * 4 * u + q * u + j];
        __builtin_memcpy(&bits, &v, 4);
        bits = bf16_bits(bits);
      }
      out[((size_t)(k / 8) * G + g) * 8 + (k & 7)] = (uint16_t)bits;
    }
}

hipError_t lstm_serve_wide_launch(const LstmServeArgs& args, hipStream_t stream) {
  if (lstm_serve_wide_check(args)[0] || args.nslots < 64 || args.nkeys < 1 || !args.wide_zx || args.lanes < 1 ||
      args.lanes > LSW_MAXLANES)
    return hipErrorInvalidValue;
  int li = 0;
  for (int l = 0; l < args.nl; ++l)
    if (args.L[l].kind == LS_LSTM) {
      if (!args.wide_w[li] || !args.wide_u[li] || !args.wide_b[li]) return hipErrorInvalidValue;
      ++li;
    }
  const LstmServeWideDims d = lstm_serve_wide_dims(args);
  const size_t lds = lstm_serve_wide_lds_bytes(args);
  if (lds + 16 * 1024 > 160 * 1024) return hipErrorInvalidValue;   // + 11.6 KB of static LDS
  if (lds > 49152) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_serve_wide_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  // one launch, one workgroup per lane: lanes on streams of their own would share hardware
  // queues, and a resident kernel queued behind another never starts (runtime/queues.h)
  hipLaunchKernelGGL(lstm_serve_wide_kernel, dim3(args.lanes), dim3(WNT), lds, stream, args, d.rows, d.stride,
                     d.rows * d.gmax);
  return hipGetLastError();
}

}  // namespace sml
