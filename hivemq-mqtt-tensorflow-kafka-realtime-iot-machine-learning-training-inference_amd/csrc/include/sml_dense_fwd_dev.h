// Device code the fused bulk forwards of Dense stacks share (kernels/dense_forward.hip: one model over
// all rows; kernels/dense_forward_fleet.hip: a fleet, every model over its own rows): the element-
// coalesced movement of a pair of 16-row tiles, the first layer's B fragments, the MFMA chain over the
// stack and the epilogue.  The layouts and the orders of every sum are described at the top of
// dense_forward.hip; a row's bits depend on the row and the weight image only, whichever kernel and
// whichever wave runs it.  Everything is force-inlined: the callers' loops own the registers.
#pragma once

#include "sml_common.h"
#include "sml_dense_fwd_plan.h"

namespace sml {
namespace {

static_assert(ACT_LINEAR == 0 && DFW_ACT_LAST == ACT_SIGMOID, "the check's activation range is Act's");
static_assert(DFW_WAVE_TILES == 2 && DFW_TILE == 16, "the kernels are written for two 16-row tiles per wave");

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
__device__ __forceinline__ uint64_t magic_of(int w) { return (0x100000000ull + (uint64_t)w - 1) / (uint64_t)w; }

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

// The first layer's B fragments from the wave's staging tiles, normalised as they are formed.
template <int MB>
__device__ __forceinline__ void first_fragments(float (&h)[NT2][4 * MB], const float* st0, int S, const float* s_sc,
                                                const float* s_sh, int nkb0, bool norm, int c, int g) {
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
}

// The stack over the two tiles: h holds the first layer's B fragments on entry and the last layer's
// activations y[row = c][unit = 16 ub + 4 g + r] on return.  img is the packed image in LDS.
template <int MB>
__device__ __forceinline__ void stack_chain(float (&h)[NT2][4 * MB], float (&z)[NT2][4 * MB], const float* img,
                                            const DenseFwdLayer* L, int nl, int lane, int g) {
  for (int l = 0; l < nl; ++l) {
    const int K = L[l].in, N = L[l].out, act = L[l].act;
    const int nub = (N + 15) >> 4;
    const f32x4* W4 = reinterpret_cast<const f32x4*>(img + L[l].w_off) + lane;
    const float* bias = img + L[l].b_off + 4 * g;
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
}

// What the epilogue writes for the rows row0 .. of a pair, rows at and past `n` masked.
struct PairOut {
  float* rec;          // [.., out] contiguous, or null
  float* score;        // or null
  uint8_t* flag;       // or null (needs score)
  float threshold;
  const double* sums;  // not null: add to lsum / lcnt
  const float* y;      // own targets of sums, or null
  int64_t ldy;
  int64_t n;
};

// h holds y[row = c][unit = 16 ub + 4 g + r]; z is free.  The staging tiles still hold the rows.
template <int MB>
__device__ __forceinline__ void pair_epilogue(float (&h)[NT2][4 * MB], float (&z)[NT2][4 * MB], float* st0, int S,
                                              const float* s_sc, const float* s_sh, bool norm, const PairOut& o,
                                              bool want_target, int64_t row0, int out, int nubL, uint64_t magicO,
                                              int ln, int lane, int c, int g, double& lsum, double& lcnt) {
  if (want_target) {
    if (o.y) {   // own targets through the staging tiles (the rows are done with them, z is free)
      pair_load<MB>(z, o.y, o.ldy, row0, o.n, out, magicO, ln);
      pair_stage<MB>(z, st0, S, out, magicO, ln);
      wave_lds_sync();
    }
    const bool tnorm = norm && !o.y;
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
      const bool live = g == 0 && row < o.n;
      if (o.score && live) {
        o.score[row] = score;
        if (o.flag) o.flag[row] = score > o.threshold ? 1 : 0;
      }
      if (o.sums) {   // uniform
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
  if (o.rec) {
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
    pair_store<MB>(o.rec, st0, S, row0, o.n, out, magicO, ln);
  }
  wave_lds_sync();   // before the next pair's rows overwrite the tile
}

// lanes 0..15 hold the sums of their rows: the wave's total, in a fixed order, in every lane
__device__ __forceinline__ void wave_fold(double& lsum, double& lcnt) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lsum += __shfl_xor(lsum, o, 64);
    lcnt += __shfl_xor(lcnt, o, 64);
  }
}

}  // namespace
}  // namespace sml
