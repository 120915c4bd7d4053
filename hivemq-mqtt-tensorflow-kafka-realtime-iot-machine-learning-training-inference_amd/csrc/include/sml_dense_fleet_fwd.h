// The fused bulk forward of a FLEET of Dense stacks (kernels/dense_forward_fleet.hip): M stacks of one
// shape, each over its own slice of one flat row array, in one launch.  Its LDS plan, the check that
// names the limit a launch exceeds and the walk over (workgroup, model) segments.  Plain C++17 with no
// HIP header, in the manner of sml_dense_fwd_plan.h, whose limits, layer table and image layout hold
// here unchanged; ops/dense_fleet_forward.py mirrors the plan and the check (csrc/tests/dense_fwd_check.cpp
// asks both on the host).
//
// PAIR SPACE.  A tile pair is 32 rows, aligned to its model's first row, so no tile holds rows of two
// models.  pair_base[M + 1] is the prefix sum of ceil(rows / 32); G = pair_base[M].  Workgroup b of
// `grid` owns the global pairs [G b / grid, G (b + 1) / grid) and walks the models that range overlaps,
// one SEGMENT per model.  Consecutive workgroups share at most one model, so the segment (b, m) has
// slot m + b of an [M + grid] array to itself: the per-model sums need no atomics.
//
// IMAGES.  images[M][stride] floats, each the single-model image; stride is a multiple of
// DFF_IMG_ALIGN floats (1 KiB, the unit of a global-to-LDS copy of one wave).
#pragma once

#include <cstdint>
#include <string>

#include "sml_dense_fwd_plan.h"

namespace sml {

enum : int {
  DFF_IMG_ALIGN = 256,          // floats: image stride and LDS image buffers are whole 1 KiB chunks
  DFF_MAXMODELS = 1 << 24,      // exclusive, as the fleet trainer's
  DFF_PAIR_ROWS = DFW_WAVE_TILES * DFW_TILE
};

struct DenseFleetFwdPlan {
  DenseFwdPlan one;    // mb, img_floats and stride as the single-model plan; offsets and waves are the fleet's
  int nbuf;            // image buffers in LDS: 2 when two fit beside staging for enough waves, else 1
  int img2_off;        // float offset of the second buffer (the first is at 0); 0 when nbuf == 1
  int waves;           // waves of a workgroup (== one.waves)
};

constexpr int dff_img_pad(int floats) { return (floats + DFF_IMG_ALIGN - 1) / DFF_IMG_ALIGN * DFF_IMG_ALIGN; }

// waves == 0: not even one wave's staging fits beside one image
inline DenseFleetFwdPlan dense_fleet_fwd_plan(const DenseFwdLayer* L, int nl, int D) {
  DenseFleetFwdPlan F{};
  F.one = dense_fwd_plan(L, nl, D);
  DenseFwdPlan& P = F.one;
  const int buf = dff_img_pad(P.img_floats), dp = dfw_pad16(D);
  const int wave_floats = DFW_WAVE_TILES * DFW_TILE * P.stride;
  const int maxw = P.mb == 8 ? DFW_MAXWAVES / 2 : DFW_MAXWAVES;
  auto fits = [&](int nbuf, int waves) {
    return (int64_t)(nbuf * buf + 2 * dp + waves * wave_floats) * 4 + DFW_STATIC_LDS <= DFW_LDS_BYTES;
  };
  F.nbuf = fits(2, maxw / 2) ? 2 : 1;
  int waves = maxw;
  while (waves > 0 && !fits(F.nbuf, waves)) waves >>= 1;
  F.img2_off = F.nbuf == 2 ? buf : 0;
  P.norm_off = F.nbuf * buf;
  P.stage_off = P.norm_off + 2 * dp;
  P.waves = F.waves = waves;
  P.lds_bytes = (P.stage_off + waves * wave_floats) * 4;
  return F;
}

// pair_base[M + 1] from table[M][2] = {first row, rows}
inline void dense_fleet_fwd_pair_base(const int64_t* table, int64_t M, int64_t* pair_base) {
  pair_base[0] = 0;
  for (int64_t m = 0; m < M; ++m) pair_base[m + 1] = pair_base[m] + (table[2 * m + 1] + DFF_PAIR_ROWS - 1) / DFF_PAIR_ROWS;
}

// The segment walk of workgroup b, as the kernel does it: calls seg(m, slot, first local pair, end)
// for every model whose pairs the workgroup's range holds, in model order.  Returns the segments.
template <class F>
inline int64_t dense_fleet_fwd_walk(const int64_t* pair_base, int64_t M, int64_t grid, int64_t b, F&& seg) {
  const int64_t G = pair_base[M];
  const int64_t g0 = G * b / grid, g1 = G * (b + 1) / grid;
  if (g0 >= g1) return 0;
  int64_t lo = 0, hi = M;   // pair_base[lo] <= g0 < pair_base[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (pair_base[mid] <= g0) lo = mid; else hi = mid;
  }
  int64_t m = lo, count = 0;
  for (;;) {
    const int64_t pb0 = pair_base[m], pb1 = pair_base[m + 1];
    seg(m, m + b, (g0 > pb0 ? g0 : pb0) - pb0, (g1 < pb1 ? g1 : pb1) - pb0);
    ++count;
    if (pb1 >= g1) return count;
    ++m;
    while (pair_base[m + 1] == pb1) ++m;   // models without rows; pair_base[M] >= g1 > pb1 ends it
  }
}

// empty if the kernel takes the launch, else the limit it exceeds: the single-model check, then the
// fleet's size, the slices and the image stride.  table may be null (the shape alone is asked about).
inline std::string dense_fleet_fwd_check(const DenseFwdLayer* L, int nl, int D, int64_t img_floats, bool score, int64_t M,
                                         const int64_t* table, int64_t n_rows, int64_t stride) {
  using std::to_string;
  const std::string why = dense_fwd_check(L, nl, D, img_floats, score);
  if (!why.empty()) return why;
  if (dense_fleet_fwd_plan(L, nl, D).waves < 1)
    return "an image in whole 1 KiB chunks leaves no staging: the limit is " + to_string((int)DFW_LDS_BYTES) + " (LDS_BYTES)";
  if (M < 1 || M >= DFF_MAXMODELS)
    return "a fleet of " + to_string(M) + " models: the fused fleet forward takes 1.." + to_string(DFF_MAXMODELS - 1);
  if (table)
    for (int64_t m = 0; m < M; ++m) {
      const int64_t first = table[2 * m], rows = table[2 * m + 1];
      if (first < 0 || rows < 0 || first > n_rows || rows > n_rows - first)
        return "model " + to_string(m) + ": rows " + to_string(first) + " .. " + to_string(first) + " + " + to_string(rows) +
               " lie outside the " + to_string(n_rows) + " rows";
    }
  DenseFwdLayer T[DFW_MAXLAYERS];
  for (int l = 0; l < nl; ++l) T[l] = L[l];
  const int want = dense_fwd_image_offsets(T, nl);
  if (stride >= 0 && (stride < want || stride % DFF_IMG_ALIGN))
    return "an image stride of " + to_string(stride) + " floats: it must be a multiple of " + to_string((int)DFF_IMG_ALIGN) +
           " that holds the " + to_string(want) + " floats of an image";
  return "";
}

}  // namespace sml
