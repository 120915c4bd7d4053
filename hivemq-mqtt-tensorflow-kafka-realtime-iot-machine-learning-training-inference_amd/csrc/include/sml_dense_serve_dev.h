// What the per-event Dense scorers share on the device: dense_serve.hip (one model) and
// dense_serve_fleet.hip (KEYED: a model index per event).  The LDS geometry of a pass, fma4, the
// second half of a layer, lane 0's result words, the `done` + stats store and the exit sequence
// are here once.  The kernels keep the inner product loops, the image, the threshold and -- in their
// old form in both files, because every shared form tried moved an instruction stream -- the
// prologue, the poll, the backlog fetch, a thread's slice bounds and the reconstruction's store
// (profiles/r20/dense_serve_shared/SUMMARY.md).  Nothing here owns __shared__ storage, and the
// pieces take kernel-argument words as values the kernels read where they always did: where an
// argument is loaded is part of the instruction stream.
//
// PROTOCOL (as ae_serve.hip: LL-framed request / result slots of sml_ops.h, xn = x * scale + shift,
// score = mean((y - xn)^2) over the D features, flag = score > threshold, three timing words, `done`,
// `alive`, `stop`, the idle timeout; fp32 throughout).  One workgroup of 1024 threads.  A PASS serves
// E events at once, 1 <= E <= EB = 8.  Waves 0..3 poll the next request slot together with the
// host's head counter (staggered as in lstm_serve_wide.hip; one synchronous cache-bypassing load per
// poll: lanes 0..31 the slot's words, lanes 32..63 head); the other waves wait at the barrier.  Two
// polling waves may find the row at once and publish the same row and (possibly) different E: the
// barrier orders both before any reader, so every thread sees ONE value of E.  With one event
// outstanding E = 1 and the row has arrived with the poll; with a backlog E = min(head - tail, EB)
// and wave e fetches row e (rows below head were published before it; tag check, bounded spin).
// KEYED: request word 31 carries the event's model index as a tagged uint32, fetched with the row
// into s_model[e], so rows have at most 31 features.  After the stack wave e scores event e and
// stores its result words.  Then thread 0 stores `done` and ONE 8-byte word {passes << 32 | events}
// (cumulative over launches) into the server's host-mapped stats block, after the pass's result
// words were issued: tests read it to prove which path ran.
//
// A LAYER spreads its Np output columns times KS slices of the reduction over the threads (KS: a
// power of two fixed by the layer's shape, dense_serve_k_slices): thread tid < Np * KS owns slice
// ks = tid / Np of column o = tid % Np, the 4-row groups [g0, g1) with KG = ceil(Kp / 4 / KS) groups
// per slice (the last slices may be short or empty).  The partial sums meet in LDS
// (part[(ks * EB + e) * Np + o]), are added to the bias in slice order and the activation is
// applied (layer_finish).  Two workgroup barriers per layer.
//
// BIT-IDENTITY.  The sum of one output of one event is bias[o] + p_0 + .. + p_{KS-1}, each p_s one
// fma4 chain over the slice's groups g0 .. g1 - 1 in order from 0.0f: it depends on the layer's
// shape only, never on E, on the event's position in the pass or on which kernel's inner loop ran,
// and the score is computed by one wave per event with the same lane-butterfly.  So an event's
// result bits do not depend on how the ring happened to batch it, and the fleet's are those of the
// single-model server holding the event's model.
//
// Exit conditions every wave reaches: the host's stop flag or `idle` without a request, decided by
// wave 0 every 64 polls and broadcast through LDS at the next barrier.  Every branch around a
// barrier is block-uniform: it depends only on kernel arguments and on values broadcast through
// LDS (quit, E).  Every spin on host memory is bounded.
#pragma once
#include "sml_common.h"
#include "sml_ops.h"
#include "sml_serve_dev.h"

namespace sml {
namespace dense_serve_dev {

using namespace serve_dev;

constexpr int NT = DSV_NT, EB = DSV_EB;
constexpr int AS = DSV_MAXW;             // stride of an event's activations in LDS (floats)
constexpr int ACT_FLOATS = EB * AS;      // one activation buffer
constexpr int PART_FLOATS = EB * NT;     // partial sums [KS][EB][Np], Np * KS <= NT
constexpr int FIXED_FLOATS = 2 * ACT_FLOATS + PART_FLOATS;   // dynamic LDS before any image
constexpr int KEYW = 31;                 // KEYED: request word of the model index

static_assert(DSV_MAXW % 4 == 0 && DSV_MAXW % DSV_TILE == 0, "padded widths stay within DSV_MAXW");
static_assert(FIXED_FLOATS * 4 + 2048 <= 160 * 1024, "LDS budget");

__device__ __forceinline__ float fma4(const float4 x, const float4 w, float a) {
  return fmaf(x.w, w.w, fmaf(x.z, w.z, fmaf(x.y, w.y, fmaf(x.x, w.x, a))));
}

// units and activation of a layer, for a caller that holds them as values
struct DenseLayerOut {
  int out, act;
};

// Second half of a layer for events 0 .. n - 1: bias + partial sums in slice order 0 .. KS - 1,
// activation.  bias_of(e): event e's padded bias [Np].
template <class BiasOf, class Layer>
__device__ __forceinline__ void layer_finish(BiasOf bias_of, int n, int Np, int KS, const Layer& L,
                                             float* out, const float* part, int tid) {
  __syncthreads();
  for (int it = tid; it < n * Np; it += NT) {
    const int e = it / Np, o = it - e * Np;
    float s = bias_of(e)[o];
    for (int ks = 0; ks < KS; ++ks) s += part[(ks * EB + e) * Np + o];
    out[e * AS + o] = o < L.out ? act_fwd(L.act, s) : 0.f;   // padded columns feed zero rows
  }
  __syncthreads();
}

// Lane 0 of the wave that scored an event (its tag, its slot r) stores the result words in two
// steps: the kernel reads the event's threshold between them, where it always did.
__device__ __forceinline__ float pass_score_word(ServeResult* r, uint32_t tag, int D, float se) {
  const float score = se / (float)D;
  st_sys(&r->w[kServeScore], tagged(tag, score));
  return score;
}
__device__ __forceinline__ void pass_flag_words(ServeResult* r, uint32_t tag, bool flag, uint64_t t_seen,
                                                uint64_t t_load, uint64_t t_comp) {
  st_sys(&r->w[kServeFlag], tagged_u(tag, flag ? 1u : 0u));
  st_sys(&r->w[kServeTLoad], tagged_u(tag, (uint32_t)(t_load - t_seen)));
  st_sys(&r->w[kServeTComp], tagged_u(tag, (uint32_t)(t_comp - t_seen)));
  st_sys(&r->w[kServeTDone], tagged_u(tag, (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_seen)));
}

// The pass is counted: once every wave has issued its result stores and is done with the LDS rows
// and control words, thread 0 stores `done` and the stats word.
__device__ __forceinline__ void pass_done(ServeCtl* ctl, uint64_t* stats, uint64_t tail, uint32_t passes,
                                          uint32_t events, int tid) {
  __syncthreads();
  if (tid == 0) {
    st_sys(&ctl->done, tail);   // back-pressure hint only: results carry their own tags
    st_sys(stats, ((uint64_t)passes << 32) | (uint64_t)events);
  }
}

__device__ __forceinline__ void pass_exit(ServeCtl* ctl, int tid) {
  __syncthreads();
  wait_stores();
  if (tid == 0) st_sys32(&ctl->alive, 0u);
}

}  // namespace dense_serve_dev
}  // namespace sml
