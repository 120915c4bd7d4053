// Persistent per-event scorer for Dense stacks on v_mfma_f32_16x16x32_bf16: the stacks dense_serve.hip
// serves (1..8 Dense layers, every width up to 512, rows of up to 32 features, the last layer one unit per
// feature), with the arithmetic and the weight image of the wide bulk forward (dense_forward_wide.hip,
// sml_dense_fwdw_plan.h).  Limits, LDS plan and check: sml_dense_serve_bf16.h.
//
// ARITHMETIC.  xn = fmaf(x, scale, shift) in fp32; z_l = b_l + bf16(h_{l-1}) . bf16(W_l): the accumulator
// starts as the fp32 bias and ONE chain per unit walks kb ascending, the weight fragment as the A
// operand and the activations as the B operand; h_l = act_fwd(z_l) in fp32; only the copy that feeds
// the next contraction is rounded (pack4); the last layer leaves unrounded.  These are the bulk
// kernel's chains, so an event's reconstruction has the bits ops.dense_forward_wide.forward returns for
// that row.  score = mean((y - xn)^2) against the unrounded xn as dense_serve.hip computes it: one wave
// per event, wave_sum, se / D.
//
// PROTOCOL.  sml_dense_serve_dev.h's, unchanged (LL-framed slots, waves 0..3 poll the slot together with
// head, bounded spins, the stop and idle exits decided by wave 0 and broadcast through LDS, every
// branch around a barrier block-uniform, pass_done / pass_exit and the stats word), with a pass of up
// to DSVB_EB = 16 events: the 16 columns of the MFMA.  Wave e fetches row e; columns past E hold zeros
// or stale rows, and their results are dropped.
//
// A LAYER.  The pass's activations live in LDS as bf16 [16][stride] in two buffers used ping-pong: a
// layer reads one and writes the other, so it costs ONE barrier.  Wave w owns the unit blocks w and
// w + 16 for all 16 columns (2 x 4 accumulator VGPRs).  Per k-step it reads the B fragment (lane (c, g):
// event c, k = 32 kb + 8 g .. + 7; one ds_read_b128, bank-conflict free) and issues one MFMA per owned
// block; its weight fragments come through a ring of DSVB_RING k-steps in flight ahead of the MFMAs
// (a slot is refilled as soon as its fragment has been issued).  Waves past nub skip to the barrier.
// The result layout (units on registers, events on lanes) is the store layout of the next layer's k:
// 8-byte LDS stores at [event c][16 ub + 4 g .. + 3].  After an odd nub the wave that would own block nub
// zeroes the second half of the next layer's last k-step.  The last layer (at most two blocks) writes
// fp32 to s_y, from where wave e scores and stores event e.
//
// BIT-IDENTITY.  MFMA columns are independent and a unit's k order is fixed (k is never split across
// waves), so an event's result bits depend on neither E nor the event's column.
//
// WEIGHTS.  The kernel body is a template on where the image lives:
//   "bf16-lds"     copied to LDS at launch (at most DSVB_LDS_IMAGE_BYTES); a lane reads its fragment
//                  with one ds_read_b128, consecutive lanes consecutive addresses;
//   "bf16-stream"  16-byte global loads from L2 on every pass.
#include "sml_common.h"
#include "sml_dense_serve_bf16.h"
#include "sml_dense_serve_dev.h"
#include "sml_ops.h"

namespace sml {
namespace {

using namespace serve_dev;
using dense_serve_dev::pass_done;
using dense_serve_dev::pass_exit;
using dense_serve_dev::pass_flag_words;
using dense_serve_dev::pass_score_word;

constexpr int NT = DSVB_NT, EB = DSVB_EB, NWV = DSVB_WAVES, RING = DSVB_RING;
static_assert(ACT_LINEAR == 0 && DFW_ACT_LAST == ACT_SIGMOID, "the check's activation range is Act's");
static_assert(EB == 16 && NT == 1024, "a pass is the 16 columns of one MFMA; 1024 threads leave 128 VGPRs");

__device__ __forceinline__ f32x4 mfma_k32(s16x8 a, s16x8 b, f32x4 c) {
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ uint16_t bf16_of(float v) { return (uint16_t)(pack2(v, 0.f) & 0xffffu); }

// One layer of the pass for a wave that owns up to UBN unit blocks (ub = wid + 16 j): in -> out (bf16,
// stride S words), or, for the last layer, -> y (fp32 [16][32]).  img: the image (LDS or global).
template <int UBN>
__device__ __forceinline__ void layer_pass(const uint16_t* __restrict__ img, const DenseFwdLayer& L, bool last,
                                           const uint16_t* in, uint16_t* out, float* y, int S, int lane, int wid) {
  const int c = lane & 15, g = lane >> 4;
  const int nkb = (L.in + 31) >> 5, nub = (L.out + 15) >> 4;
  if (wid < nub) {
    const int wstep = nub * 64;   // fragments between two k-steps of one unit block
    const s16x8* W[UBN];
    s16x8 ring[RING][UBN];
    f32x4 acc[UBN];
#pragma unroll
    for (int j = 0; j < UBN; ++j) {
      // a block past nub runs on block nub - 1's fragments (the loads stay inside the image) and is
      // never written
      const int ub = wid + NWV * j < nub ? wid + NWV * j : nub - 1;
      W[j] = reinterpret_cast<const s16x8*>(img + L.w_off) + ub * 64 + lane;
      acc[j] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(img + L.b_off) + 16 * ub + 4 * g);
    }
#pragma unroll
    for (int i = 0; i < RING; ++i) {
      const int kb = i < nkb ? i : nkb - 1;
#pragma unroll
      for (int j = 0; j < UBN; ++j) ring[i][j] = W[j][kb * wstep];
    }
    const uint16_t* brow = in + c * S + 8 * g;
#pragma unroll 1
    for (int kb0 = 0; kb0 < nkb; kb0 += RING) {
#pragma unroll
      for (int i = 0; i < RING; ++i) {
        const int kb = kb0 + i;
        if (kb < nkb) {   // wave-uniform
          const s16x8 b = *reinterpret_cast<const s16x8*>(brow + 32 * kb);
          s16x8 a[UBN];
#pragma unroll
          for (int j = 0; j < UBN; ++j) a[j] = ring[i][j];
          if (kb + RING < nkb) {
#pragma unroll
            for (int j = 0; j < UBN; ++j) ring[i][j] = W[j][(kb + RING) * wstep];
          }
#pragma unroll
          for (int j = 0; j < UBN; ++j) acc[j] = mfma_k32(a[j], b, acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < UBN; ++j) {
      const int ub = wid + NWV * j;
      if (ub < nub) {
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = act_fwd(L.act, acc[j][r]);
        if (last) {
          // nub <= 2: units 16 ub + 4 g + r < 32
          *reinterpret_cast<f32x4*>(y + c * DSVB_MAXD + 16 * ub + 4 * g) = h;
        } else {
          *reinterpret_cast<bf16x4*>(out + c * S + 16 * ub + 4 * g) = pack4(h);
        }
      }
    }
  }
  // the second half of the next layer's last k-step
  if (!last && (nub & 1) && wid == (nub & (NWV - 1)))
    *reinterpret_cast<bf16x4*>(out + c * S + 16 * nub + 4 * g) = bf16x4{0, 0, 0, 0};
  __syncthreads();
}

template <bool LDSW>
__global__ __launch_bounds__(DSVB_NT) void dense_serve_bf16_kernel(DenseServeBf16Args a, int S) {
  extern __shared__ __attribute__((aligned(16))) uint16_t smem[];   // act0, act1 [16][S]; then the image
  __shared__ __attribute__((aligned(16))) float s_xn[EB][DSVB_MAXD];   // the pass's normalised rows
  __shared__ __attribute__((aligned(16))) float s_y[EB][DSVB_MAXD];    // the last layer's outputs
  __shared__ float s_sc[32], s_sh[32];
  __shared__ int s_ctl[8];   // quit, E, -, seen sequence, t_seen lo / hi
  uint16_t* const act0 = smem;
  uint16_t* const act1 = smem + EB * S;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int D = a.D;
  ServeCtl* const ctl = a.ctl;
  const uint16_t* wimg = a.image;
  if constexpr (LDSW) {
    uint16_t* const limg = smem + 2 * EB * S;
    f32x4* dst = reinterpret_cast<f32x4*>(limg);
    const f32x4* src = reinterpret_cast<const f32x4*>(a.image);
    for (int i = tid; i < (a.img_words >> 3); i += NT) dst[i] = src[i];
    wimg = limg;
  }
  // columns a pass does not fill read finite values from the first pass on
  for (int i = tid; i < EB * S; i += NT) reinterpret_cast<uint32_t*>(smem)[i] = 0u;   // both buffers
  if (tid < 32) {
    s_sc[tid] = (tid < D && a.scale) ? a.scale[tid] : 1.f;
    s_sh[tid] = (tid < D && a.shift) ? a.shift[tid] : 0.f;
  }
  if (tid < 8) s_ctl[tid] = 0;
  __syncthreads();
  const bool norm = a.scale != nullptr;

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
          if (lane < 32) {
            float xv = 0.f;
            if (lane < D) {
              xv = __uint_as_float((uint32_t)w);
              if (norm) xv = fmaf(xv, s_sc[lane], s_sh[lane]);
            }
            s_xn[0][lane] = xv;
            act0[lane] = bf16_of(xv);
          }
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
        xv = __uint_as_float((uint32_t)v);
        if (norm) xv = fmaf(xv, s_sc[lane], s_sh[lane]);
      }
      s_xn[wid][lane] = xv;
      act0[wid * S + lane] = bf16_of(xv);
    }
    if (E > 1) __syncthreads();   // E == 1: the row was in LDS before the barrier above
    const uint64_t t_load = __builtin_amdgcn_s_memrealtime();
    // ---------------- the stack, ping-pong between the two activation buffers
    const uint16_t* in = act0;
    uint16_t* out = act1;
#pragma unroll 1
    for (int l = 0; l < a.nl; ++l) {
      const bool lastl = l == a.nl - 1;
      if (a.L[l].out <= 16 * NWV) layer_pass<1>(wimg, a.L[l], lastl, in, out, &s_y[0][0], S, lane, wid);
      else layer_pass<2>(wimg, a.L[l], lastl, in, out, &s_y[0][0], S, lane, wid);
      uint16_t* const t = const_cast<uint16_t*>(in);
      in = out;
      out = t;
    }
    const uint64_t t_comp = __builtin_amdgcn_s_memrealtime();
    // ---------------- results: wave e scores and stores event e
    if (wid < E) {
      const uint64_t ev = tail + (uint64_t)wid;
      const uint32_t tag = (uint32_t)(ev + 1);
      ServeResult* r = a.res + (int)(ev % (uint64_t)a.nslots);
      const float yv = lane < D ? s_y[wid][lane & 31] : 0.f;
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

hipError_t dense_serve_bf16_launch(const DenseServeBf16Args& args, hipStream_t stream) {
  if (args.nl < 1 || args.nl > DFWW_MAXLAYERS || !dense_serve_bf16_check(args.L, args.nl, args.D, args.img_words).empty() ||
      args.nslots < 64 || !args.image || ((uintptr_t)args.image & 15) || !args.stats ||
      (args.scale == nullptr) != (args.shift == nullptr))
    return hipErrorInvalidValue;
  const DenseServeBf16Plan P = dense_serve_bf16_plan(args.L, args.nl);
  const void* fn = P.in_lds ? reinterpret_cast<const void*>(dense_serve_bf16_kernel<true>)
                            : reinterpret_cast<const void*>(dense_serve_bf16_kernel<false>);
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes);
  if (e != hipSuccess) return e;
  if (P.in_lds) hipLaunchKernelGGL(dense_serve_bf16_kernel<true>, dim3(1), dim3(NT), (size_t)P.lds_bytes, stream, args, P.stride);
  else hipLaunchKernelGGL(dense_serve_bf16_kernel<false>, dim3(1), dim3(NT), (size_t)P.lds_bytes, stream, args, P.stride);
  return hipGetLastError();
}

}  // namespace sml
