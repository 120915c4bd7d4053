// sml-build: no-packed-fp32
// Fused bulk forward of a FLEET of Dense stacks: M stacks of one shape (the limits of
// dense_forward.hip), model m over its own slice table[m] = {first row, rows} of one flat row array,
// all in ONE launch.  The arithmetic is dense_forward.hip's, from the same device code
// (sml_dense_fwd_dev.h): a row's reconstruction and score bits are those the single-model kernel gives
// with that member's image.  What is this kernel's own is how the work is split and how the weights move.
//
// PAIR SPACE (sml_dense_fleet_fwd.h).  Tile pairs of 32 rows are aligned to each model's first row and
// masked at first + rows, so a tile never mixes models.  pair_base[M + 1] is the prefix sum of the
// models' pair counts and G its last entry.  Workgroup b of a persistent grid owns the global pairs
// [G b / grid, G (b + 1) / grid): no tickets, no atomics.  It finds its first model by binary search
// in pair_base and walks the models its range overlaps, one SEGMENT per model (models without rows
// are stepped over); inside a segment the waves split the local pair range as the single-model kernel
// splits its rows, each wave prefetching its next pair's rows under the current chain.  A workgroup
// loads each image at most once, and a launch has at most M + grid - 1 segments.
//
// IMAGES.  With two image buffers in LDS (the plan: two images, the normaliser and staging for half
// the instance's waves fit) segment s + 1's image is copied while segment s runs, and ONE
// __syncthreads() separates segments.  The copy is the global-to-LDS 16-byte load of ae_fused.hip and
// lstm_fused_split.hip (LDS address M0 + 16 lane, a 1 KiB chunk per wave instruction, no registers
// held).  Every wave issues its chunks right after it staged its first pair of segment s -- not before
// that pair's row loads, whose compiler-placed vmcnt wait would drain the copy at once -- so the copy
// flies under that pair's chain and is waited for at the barrier.  args.plain_copy copies through
// registers at the same place instead (the fallback, kept for measuring).  With one buffer, switching
// is barrier, copy, barrier.
//
// SUMS.  The (loss, correct rows) of segment (b, m) go to slot m + b of [M + grid][2] doubles, with m
// written beside it: consecutive workgroups share at most one model, so the slot is the segment's
// alone.  Waves fold into s_part[segment parity], and thread 0 adds the waves in index order after
// the segment's barrier; the host folds the slots in slot order.
//
// Three instances by padded width, as dense_forward.hip; built without packed fp32 like it.
#include "sml_common.h"
#include "sml_dense_fwd_dev.h"
#include "sml_dense_fwd_launch.h"
#include "sml_ops.h"

namespace sml {
namespace {

// global -> LDS, 16 bytes per lane: LDS destination = m0 + 16 lane, wave-uniform global base + lane offset
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // m0 is deliberately clobbered
__device__ __forceinline__ void dma16(const void* gbase, unsigned voff, unsigned m0) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0), "v"(voff), "s"(gbase) : "memory", "m0");
}
#pragma clang diagnostic pop
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int MB>
__global__ __launch_bounds__(MB == 8 ? 256 : 512) void dense_fwd_fleet_kernel(DenseFleetFwdArgs a, DenseFleetFwdPlan F) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double s_part[2][DFW_MAXWAVES][2];
  const DenseFwdPlan& P = F.one;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), NW = (int)blockDim.x >> 6;
  const int D = a.D, Dp = dfw_pad16(D), nkb0 = Dp >> 4;
  const int out = a.L[a.nl - 1].out, nubL = (out + 15) >> 4;
  const int64_t b = blockIdx.x, G = a.pairs;
  const int64_t g0 = G * b / (int64_t)gridDim.x, g1 = G * (b + 1) / (int64_t)gridDim.x;
  if (g0 >= g1) return;   // the whole workgroup: a grid larger than G

  float* const s_sc = smem + P.norm_off;
  float* const s_sh = s_sc + Dp;
  for (int i = tid; i < Dp; i += (int)blockDim.x) {
    s_sc[i] = (i < D && a.scale) ? a.scale[i] : 1.f;   // padded inputs stay 0 * 1 + 0
    s_sh[i] = (i < D && a.shift) ? a.shift[i] : 0.f;
  }
  const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) float*)smem);
  const int chunks = dff_img_pad(P.img_floats) / DFF_IMG_ALIGN;   // of 1 KiB; stride holds them all
  auto copy_image = [&](int64_t m, int buf) {   // this thread's share; visible after wait_vm0 and a barrier
    const float* src = a.images + m * a.stride;
    const int off = buf ? F.img2_off : 0;
    if (a.plain_copy) {
      f32x4* dst = reinterpret_cast<f32x4*>(smem + off);
      const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
      for (int i = tid; i < (P.img_floats >> 2); i += (int)blockDim.x) dst[i] = s4[i];
    } else {
      for (int k = wid; k < chunks; k += NW)
        dma16(reinterpret_cast<const char*>(src) + (int64_t)k * 1024, (unsigned)lane * 16u,
              lds0 + (unsigned)off * 4u + (unsigned)k * 1024u);
    }
  };

  int64_t m;
  {
    int64_t lo = 0, hi = a.M;   // pair_base[lo] <= g0 < pair_base[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (a.pair_base[mid] <= g0) lo = mid; else hi = mid;
    }
    m = lo;
  }

  const int S = P.stride;
  float* const st0 = smem + P.stage_off + wid * (NT2 * DFW_TILE * S);
  const uint64_t magicD = magic_of(D), magicO = magic_of(out);
  const bool norm = a.scale != nullptr;
  const bool want_target = a.score != nullptr || a.slot_sums != nullptr;
  const bool two = F.nbuf == 2;
  auto flush = [&](int parity, int64_t model) {   // thread 0, after the segment's barrier
    double s = 0.0, k = 0.0;
    for (int w = 0; w < NW; ++w) {
      s += s_part[parity][w][0];
      k += s_part[parity][w][1];
    }
    a.slot_sums[2 * (model + b)] = s;
    a.slot_sums[2 * (model + b) + 1] = k;
    a.slot_model[model + b] = (int32_t)model;
  };

  double lsum = 0.0, lcnt = 0.0;   // sums: lanes 0..15, their rows of the segment
  float pre[NT2][4 * MB];
  int64_t mprev = -1;
  copy_image(m, 0);
  for (int s = 0;; ++s) {
    const int64_t pb0 = a.pair_base[m], pb1 = a.pair_base[m + 1];
    int64_t mn = -1;   // the next model with rows, if this workgroup's range reaches it
    if (pb1 < g1) {
      mn = m + 1;
      while (a.pair_base[mn + 1] == pb1) ++mn;   // pair_base[M] >= g1 > pb1 ends it
    }
    wait_vm0();
    __syncthreads();   // segment s's image is in; everyone is done with segment s - 1
    if (s > 0 && tid == 0 && a.slot_sums) flush((s - 1) & 1, mprev);
    const float* img = smem + ((two && (s & 1)) ? F.img2_off : 0);
    bool pending = two && mn >= 0;

    const int64_t first = a.table[2 * m], end = first + a.table[2 * m + 1];
    const int64_t l0 = (g0 > pb0 ? g0 : pb0) - pb0, cnt = (g1 < pb1 ? g1 : pb1) - pb0 - l0;
    int64_t p = l0 + cnt * wid / NW;
    const int64_t p1 = l0 + cnt * (wid + 1) / NW;
    const PairOut o{a.rec, a.score, a.flag, a.thr ? a.thr[m] : 0.f, a.slot_sums, a.y, a.ldy, end};
    if (p < p1) pair_load<MB>(pre, a.x, a.ldx, first + 32 * p, end, D, magicD, opaque(lane));   // not hoisted: see opaque
    for (; p < p1; ++p) {
      const int64_t row0 = first + 32 * p;
      const int ln = opaque(lane);
      pair_stage<MB>(pre, st0, S, D, magicD, ln);
      wave_lds_sync();
      if (pending) {   // uniform
        copy_image(mn, (s + 1) & 1);
        pending = false;
      }
      if (p + 1 < p1) pair_load<MB>(pre, a.x, a.ldx, row0 + 32, end, D, magicD, ln);
      float h[NT2][4 * MB], z[NT2][4 * MB];
      first_fragments<MB>(h, st0, S, s_sc, s_sh, nkb0, norm, c, g);
      stack_chain<MB>(h, z, img, a.L, a.nl, lane, g);
      pair_epilogue<MB>(h, z, st0, S, s_sc, s_sh, norm, o, want_target, row0, out, nubL, magicO, ln, lane, c, g,
                        lsum, lcnt);
    }
    if (pending) copy_image(mn, (s + 1) & 1);   // a wave without pairs in this segment
    if (a.slot_sums) {
      wave_fold(lsum, lcnt);
      if (lane == 0) {
        s_part[s & 1][wid][0] = lsum;
        s_part[s & 1][wid][1] = lcnt;
      }
      lsum = lcnt = 0.0;
    }
    mprev = m;
    if (mn < 0) {
      __syncthreads();
      if (tid == 0 && a.slot_sums) flush(s & 1, mprev);
      return;
    }
    if (!two) {
      __syncthreads();   // everyone is done with the only buffer
      copy_image(mn, 0);
    }
    m = mn;
  }
}

// what the launcher can check without reading device memory; the binding checks the table's host copy
bool args_ok(const DenseFleetFwdArgs& a) {
  if (a.nl < 1 || a.nl > DFW_MAXLAYERS) return false;
  const bool scored = a.score != nullptr || (a.slot_sums && !a.y);
  if (!dense_fleet_fwd_check(a.L, a.nl, a.D, a.img_floats, scored, a.M, nullptr, a.n, a.stride).empty()) return false;
  if (*dense_fwd_args_why(a, a.images, a.slot_sums)) return false;
  if (!a.table || !a.pair_base) return false;
  if (a.pairs < 1 || a.pairs > (a.n + DFF_PAIR_ROWS - 1) / DFF_PAIR_ROWS + a.M) return false;
  if (a.flag && !a.thr) return false;
  return !a.slot_sums || a.slot_model;
}

DenseFwdLdsMark<3> lds_mark;   // of dense_fwd_fleet_kernel<2 / 4 / 8>

}  // namespace

int dense_fleet_fwd_grid(const DenseFwdLayer* L, int nl, int D, int64_t pairs, int max_blocks) {
  const DenseFleetFwdPlan F = dense_fleet_fwd_plan(L, nl, D);
  const int64_t want = (pairs + F.waves - 1) / F.waves;   // a pair per wave at least
  const int64_t cap = max_blocks > 0 ? max_blocks : dense_fwd_cu_count();
  return (int)(want < cap ? want : cap);
}

hipError_t dense_fleet_fwd_launch(const DenseFleetFwdArgs& a, hipStream_t stream) {
  if (!args_ok(a)) return hipErrorInvalidValue;
  const int grid = dense_fleet_fwd_grid(a.L, a.nl, a.D, a.pairs, a.max_blocks);
  const DenseFleetFwdPlan F = dense_fleet_fwd_plan(a.L, a.nl, a.D);
  const int mb = F.one.mb, inst = mb == 2 ? 0 : mb == 4 ? 1 : 2;
  const void* fn = mb == 2   ? reinterpret_cast<const void*>(dense_fwd_fleet_kernel<2>)
                   : mb == 4 ? reinterpret_cast<const void*>(dense_fwd_fleet_kernel<4>)
                             : reinterpret_cast<const void*>(dense_fwd_fleet_kernel<8>);
  const hipError_t e = lds_mark.ensure(fn, inst, F.one.lds_bytes);
  if (e != hipSuccess) return e;
  const dim3 block(64 * F.waves);
  const size_t lds = (size_t)F.one.lds_bytes;
  if (mb == 2) hipLaunchKernelGGL(dense_fwd_fleet_kernel<2>, dim3(grid), block, lds, stream, a, F);
  else if (mb == 4) hipLaunchKernelGGL(dense_fwd_fleet_kernel<4>, dim3(grid), block, lds, stream, a, F);
  else hipLaunchKernelGGL(dense_fwd_fleet_kernel<8>, dim3(grid), block, lds, stream, a, F);
  return hipGetLastError();
}

}  // namespace sml
