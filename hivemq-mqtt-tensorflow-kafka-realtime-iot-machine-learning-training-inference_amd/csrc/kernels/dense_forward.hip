// sml-build: no-packed-fp32
// Fused bulk forward of a Dense stack: 1..8 Dense layers, every width (input included) up to 128,
// over n rows in ONE launch.  Rows are read once, activations never leave registers, every
// contraction is v_mfma_f32_16x16x4_f32 (an fp32 fma chain).  It writes reconstructions, per-row
// scores and flags, or per-workgroup loss / accuracy sums (nn.Model.predict / score / detect /
// evaluate through ops/dense_forward.py).  Limits, image layout and LDS plan: sml_dense_fwd_plan.h.
//
// MFMA CHAIN.  Every layer is computed transposed, Y^T = W^T . X^T, on 16-row tiles; lane l has
// c = l % 16 (the tile's row) and g = l / 16.  The A operand is a weight fragment W[k][unit = c],
// the B operand the activations h[row = c][k], and the result leaves register r holding
// y[row = c][unit = 16 ub + 4 g + r].  The contraction index of the NEXT layer is numbered the same
// way: MFMA r of k-block kb contracts k = 16 kb + 4 g + r, so register r of output block kb is,
// unchanged, the B operand of that MFMA.  Activations chain in VGPRs: no LDS round trip, no
// transposes and no barriers between layers.  The bias is the accumulator's initial value; the
// activation is sml_common.h's act_fwd, as in the per-event scorers.
//
// WEIGHTS.  Every workgroup copies the packed image to LDS once and then loops.  A lane fetches the
// four A values of a (kb, ub) pair with one ds_read_b128, and the two row tiles a wave runs at once
// share it.  MFMAs whose whole k-slice is padding (16 kb + r >= in) are skipped under uniform
// branches: with 18 inputs, two of the second block's four.
//
// ROWS.  A persistent grid; every WAVE takes a contiguous span of tile pairs (32 rows) and needs no
// barrier with the others once the image is in.  A tile's elements are loaded element-coalesced
// (element e of the tile is row e / D, column e % D, at x + row * ldx + column: contiguous bytes when
// ldx == D, only the D columns of a strided view) into registers, then written to the wave's staging
// tile in LDS, zero-filled up to the padded width; the first layer's B fragments are 16-byte reads of
// it, normalised (xn = x * scale + shift) as they are formed.  The NEXT pair's loads are issued before
// the current pair's chain and written to the staging tile after its epilogue.  The staging tile is
// single: a second one per tile would halve the waves that fit beside a 64 KiB image, and the
// registers hold the prefetch anyway.
//
// EPILOGUE.  The target fragment (xn again from the staging tile, or the caller's y staged through
// the same tile) has the layout of the output registers.  score = (sum over the lane's units, then
// + lane ^ 16, then + lane ^ 32) / out: a fixed order, the same in all four lane groups.  argmax:
// first maximal index, per lane in unit order, then merged across the lane groups by (value, index).
// Reconstructions go back through the staging tile and leave as element-coalesced stores.  sums:
// lanes 0..15 add their rows in doubles, the wave and then the workgroup fold them in a fixed order
// into sums[block]; no atomics.
//
// A ROW'S BITS depend on the row and the weights only: column c of an MFMA's result depends on
// column c of B alone, and nothing else in the row's path looks at the grid, the span or c.
//
// Register arrays are statically indexed: the block loops are fully unrolled under uniform bounds,
// in three instances by the widest padded width (<= 32 / 64 / 128: MB = 2 / 4 / 8 blocks).  MB = 8
// keeps 2 x 32 input, 2 x 32 output and 2 x 32 prefetch registers, so it runs 4 waves of up to 512
// registers; the others run 8.
//
// BUILD.  "sml-build: no-packed-fp32" (line 1, read by _build.py) compiles this file without the
// packed-fp32 target feature.  With the feature the compiler pairs the normaliser's fmaf into 56
// v_pk_fma_f32 that sit between MFMAs, where the packed form issues slower than the two scalar ones
// (_build.py's note on no-slp); without it there are none, at the same 113 / 182 / 296 VGPRs.  The
// feature switch is used rather than no-slp because it holds for every pass, not the SLP vectoriser alone.
#include "sml_common.h"
#include "sml_dense_fwd_dev.h"
#include "sml_dense_fwd_launch.h"
#include "sml_ops.h"

namespace sml {
namespace {

template <int MB>
__global__ __launch_bounds__(MB == 8 ? 256 : 512) void dense_fwd_kernel(DenseFwdArgs a, DenseFwdPlan P) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ double s_part[DFW_MAXWAVES][2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
  const int NW = (int)blockDim.x >> 6;
  const int D = a.D, Dp = dfw_pad16(D), nkb0 = Dp >> 4;
  const int out = a.L[a.nl - 1].out, nubL = (out + 15) >> 4;
  float* const s_sc = smem + P.norm_off;
  float* const s_sh = s_sc + Dp;
  {
    f32x4* dst = reinterpret_cast<f32x4*>(smem);
    const f32x4* src = reinterpret_cast<const f32x4*>(a.image);
    for (int i = tid; i < (P.img_floats >> 2); i += (int)blockDim.x) dst[i] = src[i];
    for (int i = tid; i < Dp; i += (int)blockDim.x) {
      s_sc[i] = (i < D && a.scale) ? a.scale[i] : 1.f;   // padded inputs stay 0 * 1 + 0
      s_sh[i] = (i < D && a.shift) ? a.shift[i] : 0.f;
    }
  }
  __syncthreads();

  const int S = P.stride;
  float* const st0 = smem + P.stage_off + wid * (NT2 * DFW_TILE * S);
  const uint64_t magicD = magic_of(D), magicO = magic_of(out);
  const bool norm = a.scale != nullptr;
  const bool want_target = a.score != nullptr || a.sums != nullptr;
  const PairOut o{a.rec, a.score, a.flag, a.threshold, a.sums, a.y, a.ldy, a.n};

  // this wave's span of tile pairs
  const int64_t tiles = (a.n + 15) >> 4, pairs = (tiles + 1) >> 1;
  const int64_t gw = (int64_t)blockIdx.x * NW + wid, GW = (int64_t)gridDim.x * NW;
  int64_t p = pairs * gw / GW;
  const int64_t p1 = pairs * (gw + 1) / GW;

  double lsum = 0.0, lcnt = 0.0;   // sums: lanes 0..15, their rows
  float pre[NT2][4 * MB];
  if (p < p1) pair_load<MB>(pre, a.x, a.ldx, 32 * p, a.n, D, magicD, lane);
  for (; p < p1; ++p) {
    const int64_t row0 = 32 * p;
    const int ln = opaque(lane);
    pair_stage<MB>(pre, st0, S, D, magicD, ln);
    wave_lds_sync();
    if (p + 1 < p1) pair_load<MB>(pre, a.x, a.ldx, row0 + 32, a.n, D, magicD, ln);
    float h[NT2][4 * MB], z[NT2][4 * MB];
    first_fragments<MB>(h, st0, S, s_sc, s_sh, nkb0, norm, c, g);
    stack_chain<MB>(h, z, smem, a.L, a.nl, lane, g);
    pair_epilogue<MB>(h, z, st0, S, s_sc, s_sh, norm, o, want_target, row0, out, nubL, magicO, ln, lane, c, g,
                      lsum, lcnt);
  }
  if (a.sums) {
    wave_fold(lsum, lcnt);
    if (lane == 0) {
      s_part[wid][0] = lsum;
      s_part[wid][1] = lcnt;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0, k = 0.0;
      for (int w = 0; w < NW; ++w) {
        s += s_part[w][0];
        k += s_part[w][1];
      }
      a.sums[2 * blockIdx.x] = s;
      a.sums[2 * blockIdx.x + 1] = k;
    }
  }
}

std::string args_check(const DenseFwdArgs& a) {
  if (a.nl < 1 || a.nl > DFW_MAXLAYERS) return dense_fwd_check(a.L, a.nl, a.D, -1, false);
  const std::string why = dense_fwd_check(a.L, a.nl, a.D, a.img_floats, a.score != nullptr || (a.sums && !a.y));
  return why.empty() ? dense_fwd_args_why(a, a.image, a.sums) : why;
}

DenseFwdLdsMark<3> lds_mark;   // of dense_fwd_kernel<2 / 4 / 8>

}  // namespace

int dense_fwd_grid(const DenseFwdLayer* L, int nl, int D, int64_t n, int max_blocks) {
  const DenseFwdPlan P = dense_fwd_plan(L, nl, D);
  const int64_t pairs = ((n + 15) / 16 + 1) / 2;
  const int64_t want = (pairs + P.waves - 1) / P.waves;   // a pair per wave at least
  const int64_t cap = max_blocks > 0 ? max_blocks : dense_fwd_cu_count();
  return (int)(want < cap ? want : cap);
}

hipError_t dense_fwd_launch(const DenseFwdArgs& a, hipStream_t stream) {
  if (!args_check(a).empty()) return hipErrorInvalidValue;
  const int grid = dense_fwd_grid(a.L, a.nl, a.D, a.n, a.max_blocks);
  const DenseFwdPlan P = dense_fwd_plan(a.L, a.nl, a.D);
  const void* fn = P.mb == 2   ? reinterpret_cast<const void*>(dense_fwd_kernel<2>)
                   : P.mb == 4 ? reinterpret_cast<const void*>(dense_fwd_kernel<4>)
                               : reinterpret_cast<const void*>(dense_fwd_kernel<8>);
  const hipError_t e = lds_mark.ensure(fn, P.mb == 2 ? 0 : P.mb == 4 ? 1 : 2, P.lds_bytes);
  if (e != hipSuccess) return e;
  const dim3 block(64 * P.waves);
  if (P.mb == 2) hipLaunchKernelGGL(dense_fwd_kernel<2>, dim3(grid), block, (size_t)P.lds_bytes, stream, a, P);
  else if (P.mb == 4) hipLaunchKernelGGL(dense_fwd_kernel<4>, dim3(grid), block, (size_t)P.lds_bytes, stream, a, P);
  else hipLaunchKernelGGL(dense_fwd_kernel<8>, dim3(grid), block, (size_t)P.lds_bytes, stream, a, P);
  return hipGetLastError();
}

}  // namespace sml
