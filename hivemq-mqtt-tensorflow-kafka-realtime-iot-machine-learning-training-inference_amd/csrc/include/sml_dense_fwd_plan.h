// The fused bulk forward of Dense stacks (kernels/dense_forward.hip): its limits, its layer table, the
// offsets of the packed weight image, its LDS plan and the check that names the limit a stack exceeds.
// Plain C++17 with no HIP header, in the manner of sml_dense_mb_plan.h.  ops/dense_forward.py mirrors
// the check and the plan in Python, because supports() must answer without a built extension.
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

struct DenseFwdLayer {
  int in, out;
  int act;             // ACT_* code
  int w_off, b_off;    // float offsets of the layer's blocks and of its padded bias in the image
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

// fills w_off / b_off from in / out; returns the floats of the image
inline int dense_fwd_image_offsets(DenseFwdLayer* L, int nl) {
  int off = 0;
  for (int l = 0; l < nl; ++l) {
    L[l].w_off = off;
    off += dfw_pad16(L[l].in) * dfw_pad16(L[l].out);
    L[l].b_off = off;
    off += dfw_pad16(L[l].out);
  }
  return off;
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
  if (nl < 1 || nl > DFW_MAXLAYERS)
    return to_string(nl) + " Dense layers: the fused forward takes 1.." + to_string(DFW_MAXLAYERS) + " (MAX_LAYERS)";
  if (D < 1 || D > DFW_MAXW)
    return "input width " + to_string(D) + " is outside 1.." + to_string(DFW_MAXW) + " (MAX_WIDTH)";
  int prev = D;
  for (int l = 0; l < nl; ++l) {
    if (L[l].in != prev) return "layer " + to_string(l) + " does not take the previous layer's width";
    if (L[l].out < 1 || L[l].out > DFW_MAXW)
      return "layer " + to_string(l) + " has " + to_string(L[l].out) + " units: the limit is " + to_string(DFW_MAXW) +
             " (MAX_WIDTH)";
    if (L[l].act < 0 || L[l].act > DFW_ACT_LAST) return "layer " + to_string(l) + ": unknown activation";
    prev = L[l].out;
  }
  if (score && prev != D)
    return "scores against the input row need as many output units as inputs (" + to_string(prev) + " units, " +
           to_string(D) + " inputs)";
  DenseFwdLayer T[DFW_MAXLAYERS];
  for (int l = 0; l < nl; ++l) T[l] = L[l];
  const int want = dense_fwd_image_offsets(T, nl);
  if (img_floats >= 0) {
    if (img_floats != want)
      return "an image of " + to_string(img_floats) + " floats: the stack packs into " + to_string(want);
    for (int l = 0; l < nl; ++l)
      if (L[l].w_off != T[l].w_off || L[l].b_off != T[l].b_off)
        return "layer " + to_string(l) + ": image offsets are not those of the packed layout";
  }
  const DenseFwdPlan P = dense_fwd_plan(L, nl, D);
  if (P.waves < 1)
    return to_string((int64_t)(P.stage_off + DFW_WAVE_TILES * DFW_TILE * P.stride) * 4 + DFW_STATIC_LDS) +
           " bytes of LDS: the limit is " + to_string(DFW_LDS_BYTES) + " (LDS_BYTES)";
  return "";
}

}  // namespace sml
