// The fused bulk forward of Dense stacks (kernels/dense_forward.hip): its limits, its layer table, the
// offsets of the packed weight image, its LDS plan and the check that names the limit a stack exceeds.
// Plain C++17 with no HIP header, in the manner of sml_dense_mb_plan.h.  ops/dense_forward.py mirrors
// the check and the plan in Python, because supports() must answer without a built extension.
//
// SHARED.  The layer table, dense_fwd_check_rows, dense_fwd_offsets / dense_fwd_check_image and
// dense_fwd_args_why hold what the three fused forwards (this one, sml_dense_fwdw_plan.h and
// sml_dense_fleet_fwd.h) have in common, once; a variant passes its width limit, its k padding, the units
// of a bias entry and its words.  csrc/tests/dense_fwd_check.cpp asks the checks and plans on the host.
//
// IMAGE (fp32, offsets in floats).  Per layer, blocks of 16 inputs (kb) by 16 units (ub):
//   img[w_off + ((kb * nub + ub) * 64 + lane) * 4 + r] = W[16 kb + 4 (lane / 16) + r][16 ub + lane % 16]
// zero past `in` and `out`, so a lane fetches the four A values of a (kb, ub) pair with one 16-byte
// read; then the layer's bias [16 nub], zero past `out` (all zero for a layer without bias).
#pragma once

#include <cstdint>
#include <string>

namespace sml {

enum : int {
  DFW_MAXLAYERS = 8,
  DFW_MAXW = 128,             // units / inputs of a layer
  DFW_TILE = 16,              // rows of an MFMA tile; widths are padded to it
  DFW_WAVE_TILES = 2,         // row tiles a wave runs at once (they share each weight fragment)
  DFW_MAXWAVES = 8,           // waves of a workgroup; 4 for the widest class (its registers)
  DFW_LDS_BYTES = 160 * 1024,
  DFW_STATIC_LDS = 1024,      // the kernel's own static LDS, rounded up
  DFW_ACT_LAST = 3,           // activation codes 0 .. 3 (Act of sml_common.h: ACT_LINEAR .. ACT_SIGMOID)
  DFW_STAGE_PAD = 4           // floats added to a staging row (16-byte aligned, off the bank stride)
};

// a layer of any of the fused forwards
struct DenseFwdLayer {
  int in, out;
  int act;             // ACT_* code
  int w_off, b_off;    // offsets of the layer's blocks and of its padded bias in the image (floats; words when wide)
};

struct DenseFwdPlan {
  int mb;              // 16-wide blocks of the widest padded width, rounded up to 2 / 4 / 8: the kernel instance
  int img_floats;
  int norm_off;        // scale [Dp], shift [Dp]
  int stage_off;       // staging tiles [waves][DFW_WAVE_TILES][16][stride]
  int stride;          // floats between two rows of a staging tile
  int waves;           // waves of a workgroup: the most that fit
  int lds_bytes;       // dynamic LDS
};

constexpr int dfw_pad16(int n) { return (n + 15) / 16 * 16; }

constexpr int dfw_pad(int n, int m) { return (n + m - 1) / m * m; }

// fills w_off / b_off from in / out for blocks of `kpad` inputs by 16 units and `bias_units` image units per
// bias entry; returns the units of the image
inline int dense_fwd_offsets(DenseFwdLayer* L, int nl, int kpad, int bias_units) {
  int off = 0;
  for (int l = 0; l < nl; ++l) {
    L[l].w_off = off;
    off += dfw_pad(L[l].in, kpad) * dfw_pad16(L[l].out);
    L[l].b_off = off;
    off += bias_units * dfw_pad16(L[l].out);
  }
  return off;
}
inline int dense_fwd_image_offsets(DenseFwdLayer* L, int nl) { return dense_fwd_offsets(L, nl, 16, 1); }

// The rules of a stack that every fused forward has: layer count, input width, chaining, units, activation
// and, for scores against the input row, out == D.  `who`: "fused" or "wide fused".
inline std::string dense_fwd_check_rows(const DenseFwdLayer* L, int nl, int D, bool score, int max_width, const char* who) {
  using std::to_string;
  if (nl < 1 || nl > DFW_MAXLAYERS)
    return to_string(nl) + " Dense layers: the " + who + " forward takes 1.." + to_string(DFW_MAXLAYERS) + " (MAX_LAYERS)";
  if (D < 1 || D > max_width)
    return "input width " + to_string(D) + " is outside 1.." + to_string(max_width) + " (MAX_WIDTH)";
  int prev = D;
  for (int l = 0; l < nl; ++l) {
    if (L[l].in != prev) return "layer " + to_string(l) + " does not take the previous layer's width";
    if (L[l].out < 1 || L[l].out > max_width)
      return "layer " + to_string(l) + " has " + to_string(L[l].out) + " units: the limit is " + to_string(max_width) +
             " (MAX_WIDTH)";
    if (L[l].act < 0 || L[l].act > DFW_ACT_LAST) return "layer " + to_string(l) + ": unknown activation";
    prev = L[l].out;
  }
  if (score && prev != D)
    return "scores against the input row need as many output units as inputs (" + to_string(prev) + " units, " +
           to_string(D) + " inputs)";
  return "";
}

// an image of img_units `unit`s ("floats" / "words") against the packed layout of a stack that passed
// dense_fwd_check_rows; img_units < 0: the offsets may lie anywhere
inline std::string dense_fwd_check_image(const DenseFwdLayer* L, int nl, int64_t img_units, int kpad, int bias_units,
                                         const char* unit) {
  using std::to_string;
  if (img_units < 0) return "";
  DenseFwdLayer T[DFW_MAXLAYERS];
  for (int l = 0; l < nl; ++l) T[l] = L[l];
  const int want = dense_fwd_offsets(T, nl, kpad, bias_units);
  if (img_units != want)
    return "an image of " + to_string(img_units) + " " + unit + ": the stack packs into " + to_string(want);
  for (int l = 0; l < nl; ++l)
    if (L[l].w_off != T[l].w_off || L[l].b_off != T[l].b_off)
      return "layer " + to_string(l) + ": image offsets are not those of the packed layout";
  return "";
}

// What a launcher can say about the arguments every fused forward takes (A: an *Args of sml_ops.h; its
// image and sums fields are named differently, so they come beside it), after the stack's own check.
// The bindings use the same words for the same rules.
constexpr const char* DFW_WHY_PAIRED = "scale and shift come together";
constexpr const char* DFW_WHY_FLAGS = "flags need scores";
constexpr const char* DFW_WHY_OWN_TARGETS = "own targets are for sums alone";
constexpr const char* DFW_WHY_NOTHING = "nothing to compute";
template <class A>
inline const char* dense_fwd_args_why(const A& a, const void* image, const double* sums) {
  if (!a.x || !image || ((uintptr_t)image & 15) || a.n < 1 || a.ldx < a.D) return "bad rows or image";
  if ((a.scale == nullptr) != (a.shift == nullptr)) return DFW_WHY_PAIRED;
  if (a.flag && !a.score) return DFW_WHY_FLAGS;
  if (a.y && (!sums || a.score || a.ldy < a.L[a.nl - 1].out)) return DFW_WHY_OWN_TARGETS;
  if (!a.rec && !a.score && !sums) return DFW_WHY_NOTHING;
  if (a.max_blocks < 0) return "max_blocks is negative";
  return "";
}

// waves == 0: not even one wave's staging fits beside the image
inline DenseFwdPlan dense_fwd_plan(const DenseFwdLayer* L, int nl, int D) {
  DenseFwdPlan P{};
  const int dp = dfw_pad16(D);
  int maxw = dp, off = 0;
  for (int l = 0; l < nl; ++l) {
    const int np = dfw_pad16(L[l].out);
    maxw = np > maxw ? np : maxw;
    off += dfw_pad16(L[l].in) * np + np;
  }
  const int blocks = maxw / 16;
  P.mb = blocks <= 2 ? 2 : blocks <= 4 ? 4 : 8;
  P.img_floats = off;
  P.norm_off = off;
  off += 2 * dp;
  P.stage_off = off;
  const int op = dfw_pad16(L[nl - 1].out);
  P.stride = (dp > op ? dp : op) + DFW_STAGE_PAD;   // a tile stages rows, targets and reconstructions in turn
  const int wave_floats = DFW_WAVE_TILES * DFW_TILE * P.stride;
  int waves = P.mb == 8 ? DFW_MAXWAVES / 2 : DFW_MAXWAVES;
  while (waves > 0 && (int64_t)(off + waves * wave_floats) * 4 + DFW_STATIC_LDS > DFW_LDS_BYTES) waves >>= 1;
  P.waves = waves;
  P.lds_bytes = (off + waves * wave_floats) * 4;
  return P;
}

// empty if the kernel takes the stack (D inputs, nl layers whose image offsets lie inside img_floats
// floats, or anywhere if that is negative; score: the target is the input row, so out == D), else the
// limit it exceeds
inline std::string dense_fwd_check(const DenseFwdLayer* L, int nl, int D, int64_t img_floats, bool score) {
  using std::to_string;
  std::string why = dense_fwd_check_rows(L, nl, D, score, DFW_MAXW, "fused");
  if (why.empty()) why = dense_fwd_check_image(L, nl, img_floats, 16, 1, "floats");
  if (!why.empty()) return why;
  const DenseFwdPlan P = dense_fwd_plan(L, nl, D);
  if (P.waves < 1)
    return to_string((int64_t)(P.stage_off + DFW_WAVE_TILES * DFW_TILE * P.stride) * 4 + DFW_STATIC_LDS) +
           " bytes of LDS: the limit is " + to_string(DFW_LDS_BYTES) + " (LDS_BYTES)";
  return "";
}

}  // namespace sml
