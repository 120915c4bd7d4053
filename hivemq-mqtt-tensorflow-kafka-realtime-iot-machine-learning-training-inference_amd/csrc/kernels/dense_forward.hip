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
#include <atomic>

#include "sml_common.h"
#include "sml_ops.h"

namespace sml {
namespace {

static_assert(ACT_LINEAR == 0 && DFW_ACT_LAST == ACT_SIGMOID, "the check's activation range is Act's");
static_assert(DFW_WAVE_TILES == 2 && DFW_TILE == 16, "the kernel is written for two 16-row tiles per wave");

constexpr int NT2 = DFW_WAVE_TILES;

// one wave's own LDS traffic in program order: what it wrote is what its other lanes read next
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// e / w for e < 4096, w <= 128, from magic = ceil(2^32 / w)
__device__ __forceinline__ int div_magic(int e, uint64_t magic) { return (int)(((uint64_t)(uint32_t)e * magic) >> 32); }

// The element loops below compute (row, column) of element e = lane + 64 i from the lane.  Everything
// in them is invariant in the persistent loop, and hoisted out of it the 4 MB offsets per matrix would
// cost more registers than the activations: `ln` is the lane behind an empty asm inside the loop, so
// they are recomputed (five VALU per element) where they are used.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Element-coalesced load of a pair of 16-row tiles [16][w] at rows row0.. and row0 + 16.. of a matrix
// with leading dimension ld; rows past n read as zero (the load is predicated off).
template <int MB>
__device__ __forceinline__ void pair_load(float (&v)[NT2][4 * MB], const float* __restrict__ base, int64_t ld,
                                          int64_t row0, int64_t n, int w, uint64_t magic, int ln) {
  const float* b0 = base + row0 * ld;   // uniform
#pragma unroll
  for (int i = 0; i < 4 * MB; ++i) {
    if (64 * i < 16 * w) {
      const int e = ln + 64 * i;
      const int r = div_magic(e, magic), col = e - r * w;
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
        const int rr = r + 16 * t;
        v[t][i] = (e < 16 * w && row0 + rr < n) ? b0[(int64_t)rr * ld + col] : 0.f;
      }
    }
  }
}

// ... into the wave's staging tiles [NT2][16][stride], columns w .. pad16(w) - 1 zeroed
template <int MB>
__device__ __forceinline__ void pair_stage(const float (&v)[NT2][4 * MB], float* st, int stride, int w, uint64_t magic,
                                           int ln) {
#pragma unroll
  for (int i = 0; i < 4 * MB; ++i) {
    if (64 * i < 16 * w) {
      const int e = ln + 64 * i;
      const int r = div_magic(e, magic), col = e - r * w;
      if (e < 16 * w) {
#pragma unroll
        for (int t = 0; t < NT2; ++t) st[(r + 16 * t) * stride + col] = v[t][i];
      }
    }
  }
  const int c = ln & 15, g = ln >> 4, wp = dfw_pad16(w);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = w + g + 4 * j;
    if (col < wp) {
#pragma unroll
      for (int t = 0; t < NT2; ++t) st[(c + 16 * t) * stride + col] = 0.f;
    }
  }
}

// the staging tiles' [16][w] out to a contiguous [n, w] matrix, element-coalesced
template <int MB>
__device__ __forceinline__ void pair_store(float* __restrict__ base, const float* st, int stride, int64_t row0, int64_t n,
                                           int w, uint64_t magic, int ln) {
  float* b0 = base + row0 * w;   // uniform
#pragma unroll
  for (int i = 0; i < 4 * MB; ++i) {
    if (64 * i < 16 * w) {
      const int e = ln + 64 * i;
      const int r = div_magic(e, magic), col = e - r * w;
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
        const int rr = r + 16 * t;
        if (e < 16 * w && row0 + rr < n) b0[rr * w + col] = st[rr * stride + col];
      }
    }
  }
}

__device__ __forceinline__ f32x4 lds4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

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
  const uint64_t magicD = (0x100000000ull + (uint64_t)D - 1) / (uint64_t)D;
  const uint64_t magicO = (0x100000000ull + (uint64_t)out - 1) / (uint64_t)out;
  const bool norm = a.scale != nullptr;
  const bool want_target = a.score != nullptr || a.sums != nullptr;

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
    // ---------------- the first layer's B fragments
    float h[NT2][4 * MB], z[NT2][4 * MB];
#pragma unroll
    for (int kb = 0; kb < MB; ++kb) {
      if (kb < nkb0) {
        const f32x4 sc = lds4(s_sc + 16 * kb + 4 * g), sh = lds4(s_sh + 16 * kb + 4 * g);
#pragma unroll
        for (int t = 0; t < NT2; ++t) {
          const f32x4 v = lds4(st0 + (t * DFW_TILE + c) * S + 16 * kb + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) h[t][4 * kb + r] = norm ? fmaf(v[r], sc[r], sh[r]) : v[r];
        }
      }
    }
    // ---------------- the stack
    for (int l = 0; l < a.nl; ++l) {
      const int K = a.L[l].in, N = a.L[l].out, act = a.L[l].act;
      const int nub = (N + 15) >> 4;
      const f32x4* W4 = reinterpret_cast<const f32x4*>(smem + a.L[l].w_off) + lane;
      const float* bias = smem + a.L[l].b_off + 4 * g;
#pragma unroll
      for (int ub = 0; ub < MB; ++ub) {
        if (ub < nub) {
          f32x4 acc[NT2];
          acc[0] = lds4(bias + 16 * ub);
          acc[1] = acc[0];
#pragma unroll
          for (int kb = 0; kb < MB; ++kb) {
            if (16 * kb + 16 <= K) {
              const f32x4 w = W4[(kb * nub + ub) * 64];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                acc[0] = mfma4(w[r], h[0][4 * kb + r], acc[0]);
                acc[1] = mfma4(w[r], h[1][4 * kb + r], acc[1]);
              }
            } else if (16 * kb < K) {   // the ragged last block: MFMA r holds k = 16 kb + 4 g + r >= 16 kb + r
              const f32x4 w = W4[(kb * nub + ub) * 64];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                if (16 * kb + r < K) {
                  acc[0] = mfma4(w[r], h[0][4 * kb + r], acc[0]);
                  acc[1] = mfma4(w[r], h[1][4 * kb + r], acc[1]);
                }
              }
            }
          }
#pragma unroll
          for (int t = 0; t < NT2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) z[t][4 * ub + r] = acc[t][r];
        }
      }
      // every block of h was read: the activation writes the next layer's B fragments over it.
      // Units past `out` are act(0), finite, and meet zero weights only.
#pragma unroll
      for (int ub = 0; ub < MB; ++ub) {
        if (ub < nub) {
#pragma unroll
          for (int t = 0; t < NT2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[t][4 * ub + r] = act_fwd(act, z[t][4 * ub + r]);
        }
      }
    }
    // ---------------- epilogue: h holds y[row = c][unit = 16 ub + 4 g + r]
    if (want_target) {
      if (a.y) {   // own targets through the staging tiles (the rows are done with them, z is free)
        pair_load<MB>(z, a.y, a.ldy, row0, a.n, out, magicO, ln);
        pair_stage<MB>(z, st0, S, out, magicO, ln);
        wave_lds_sync();
      }
      const bool tnorm = norm && !a.y;
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
        float se = 0.f, by = -INFINITY, bt = -INFINITY;
        int iy = 0x7fffffff, it = 0x7fffffff;
#pragma unroll
        for (int ub = 0; ub < MB; ++ub) {
          if (ub < nubL) {
            f32x4 tg = lds4(st0 + (t * DFW_TILE + c) * S + 16 * ub + 4 * g);
            if (tnorm) {
              const f32x4 sc = lds4(s_sc + 16 * ub + 4 * g), sh = lds4(s_sh + 16 * ub + 4 * g);
#pragma unroll
              for (int r = 0; r < 4; ++r) tg[r] = fmaf(tg[r], sc[r], sh[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int u = 16 * ub + 4 * g + r;
              if (u < out) {
                const float yv = h[t][4 * ub + r], d = yv - tg[r];
                se = fmaf(d, d, se);
                if (yv > by) { by = yv; iy = u; }
                if (tg[r] > bt) { bt = tg[r]; it = u; }
              }
            }
          }
        }
        se += xor16(se, lane);
        se += xor32(se, lane);
        const float score = se / (float)out;
        const int64_t row = row0 + 16 * t + c;
        const bool live = g == 0 && row < a.n;
        if (a.score && live) {
          a.score[row] = score;
          if (a.flag) a.flag[row] = score > a.threshold ? 1 : 0;
        }
        if (a.sums) {   // uniform
#pragma unroll
          for (int m = 16; m <= 32; m += 16) {
            const float oy = m == 16 ? xor16(by, lane) : xor32(by, lane);
            const float ot = m == 16 ? xor16(bt, lane) : xor32(bt, lane);
            const int ojy = m == 16 ? xor16i(iy, lane) : xor32i(iy, lane);
            const int ojt = m == 16 ? xor16i(it, lane) : xor32i(it, lane);
            if (oy > by || (oy == by && ojy < iy)) { by = oy; iy = ojy; }
            if (ot > bt || (ot == bt && ojt < it)) { bt = ot; it = ojt; }
          }
          if (live) {
            lsum += (double)score;
            lcnt += iy == it ? 1.0 : 0.0;
          }
        }
      }
    }
    if (a.rec) {
      wave_lds_sync();   // the target reads are done with the tile
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
#pragma unroll
        for (int ub = 0; ub < MB; ++ub) {
          if (ub < nubL) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = h[t][4 * ub + r];
            *reinterpret_cast<f32x4*>(st0 + (t * DFW_TILE + c) * S + 16 * ub + 4 * g) = v;
          }
        }
      }
      wave_lds_sync();
      pair_store<MB>(a.rec, st0, S, row0, a.n, out, magicO, ln);
    }
    wave_lds_sync();   // before the next pair's rows overwrite the tile
  }
  if (a.sums) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lsum += __shfl_xor(lsum, o, 64);
      lcnt += __shfl_xor(lcnt, o, 64);
    }
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
  if (!why.empty()) return why;
  if (!a.x || !a.image || ((uintptr_t)a.image & 15) || a.n < 1 || a.ldx < a.D) return "bad rows or image";
  if ((a.scale == nullptr) != (a.shift == nullptr)) return "scale and shift come together";
  if (a.flag && !a.score) return "flags need scores";
  if (a.y && (!a.sums || a.score || a.ldy < a.L[a.nl - 1].out)) return "own targets are for sums alone";
  if (!a.rec && !a.score && !a.sums) return "nothing to compute";
  if (a.max_blocks < 0) return "max_blocks is negative";
  return "";
}

constexpr int MAXDEV = 64;

int cur_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAXDEV ? dev : -1;
}

// CUs of the current device, asked once per device
int cu_count() {
  static std::atomic<int> cus[MAXDEV];
  const int dev = cur_device();
  int n = dev >= 0 ? cus[dev].load(std::memory_order_relaxed) : 0;
  if (n < 1) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev < 0 ? 0 : dev) != hipSuccess || n < 1) n = 256;
    if (dev >= 0) cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// hipFuncAttributeMaxDynamicSharedMemorySize only grows: set once per device and instance for the
// largest plan seen
hipError_t ensure_lds(const void* fn, int instance, int bytes) {
  static std::atomic<int> have[MAXDEV][3];
  const int dev = cur_device();
  if (dev >= 0 && have[dev][instance].load(std::memory_order_relaxed) >= bytes) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && dev >= 0) have[dev][instance].store(bytes, std::memory_order_relaxed);
  return e;
}

}  // namespace

int dense_fwd_grid(const DenseFwdLayer* L, int nl, int D, int64_t n, int max_blocks) {
  const DenseFwdPlan P = dense_fwd_plan(L, nl, D);
  const int64_t pairs = ((n + 15) / 16 + 1) / 2;
  const int64_t want = (pairs + P.waves - 1) / P.waves;   // a pair per wave at least
  const int64_t cap = max_blocks > 0 ? max_blocks : cu_count();
  return (int)(want < cap ? want : cap);
}

hipError_t dense_fwd_launch(const DenseFwdArgs& a, hipStream_t stream) {
  if (!args_check(a).empty()) return hipErrorInvalidValue;
  const int grid = dense_fwd_grid(a.L, a.nl, a.D, a.n, a.max_blocks);
  const DenseFwdPlan P = dense_fwd_plan(a.L, a.nl, a.D);
  const void* fn = P.mb == 2   ? reinterpret_cast<const void*>(dense_fwd_kernel<2>)
                   : P.mb == 4 ? reinterpret_cast<const void*>(dense_fwd_kernel<4>)
                               : reinterpret_cast<const void*>(dense_fwd_kernel<8>);
  const hipError_t e = ensure_lds(fn, P.mb == 2 ? 0 : P.mb == 4 ? 1 : 2, P.lds_bytes);
  if (e != hipSuccess) return e;
  const dim3 block(64 * P.waves);
  if (P.mb == 2) hipLaunchKernelGGL(dense_fwd_kernel<2>, dim3(grid), block, (size_t)P.lds_bytes, stream, a, P);
  else if (P.mb == 4) hipLaunchKernelGGL(dense_fwd_kernel<4>, dim3(grid), block, (size_t)P.lds_bytes, stream, a, P);
  else hipLaunchKernelGGL(dense_fwd_kernel<8>, dim3(grid), block, (size_t)P.lds_bytes, stream, a, P);
  return hipGetLastError();
}

}  // namespace sml
