// The fused bulk forward of WIDE Dense stacks (kernels/dense_forward_wide.hip): its limits, its layer
// table, the offsets of the packed bf16 weight image, its LDS plan and the check that names the limit a
// stack exceeds.  Plain C++17 with no HIP header, over sml_dense_fwd_plan.h: the layer table (DenseFwdLayer,
// offsets in words here), DFW_MAXLAYERS, DFW_ACT_LAST and the shared rules of the check are that header's.
// ops/dense_forward_wide.py mirrors the plan in Python (the check is ops/dense_forward.py's), because
// supports() must answer without a built extension.
//
// IMAGE (16-bit words; offsets in words).  Per layer, blocks of 32 inputs (kb) by 16 units (ub) in the
// order of a v_mfma_f32_16x16x32_bf16 A fragment:
//   img[w_off + ((kb * nub + ub) * 64 + lane) * 8 + j] = bf16(W[32 kb + 8 (lane / 16) + j][16 ub + lane % 16])
// zero past `in` and `out`, so a lane fetches its eight k-values of a (kb, ub) block with one 16-byte
// load; then the layer's bias as fp32 [16 nub] (two words each), zero past `out` (all zero for a layer
// without bias).  Every offset is a multiple of 8 words: 16-byte loads stay aligned.
#pragma once

#include <cstdint>
#include <string>

#include "sml_dense_fwd_plan.h"

namespace sml {

enum : int {
  DFWW_MAXLAYERS = DFW_MAXLAYERS,
  DFWW_MAXW = 512,             // units / inputs of a layer
  DFWW_WAVES = 8,              // waves of a workgroup; wave w owns the unit blocks w, w + 8, w + 16, w + 24
  DFWW_MAXUB = 4,              // unit blocks a wave owns at most: DFWW_MAXW / 16 / DFWW_WAVES
  DFWW_ROWS_SMALL = 64,        // rows of a workgroup's tile: 4 or 8 MFMA row tiles
  DFWW_ROWS_LARGE = 128,
  DFWW_ROW_PAD = 8,            // words added to an activation row in LDS (16-byte aligned, off the bank stride)
  DFWW_PART_WORDS = 5,         // a wave's epilogue partial of a row: squared error, (max, argmax) of y and of the target;
                               // under a softmax head (max, argmax) of its logits, sum of exp(z - max), the label's logit
  DFWW_LDS_BYTES = 160 * 1024,
  DFWW_STATIC_LDS = 2048       // the kernel's own static LDS
};
static_assert(DFWW_MAXUB * DFWW_WAVES * 16 == DFWW_MAXW, "a wave's accumulators hold its whole unit slice");

struct DenseFwdWPlan {
  int img_words;
  int rows;            // rows of a tile (DFWW_ROWS_SMALL or DFWW_ROWS_LARGE)
  int stride;          // words between two activation rows in LDS
  int lds_bytes;       // dynamic LDS: the activation tile, which the epilogue's partials reuse
};

constexpr int dfww_pad16(int n) { return (n + 15) / 16 * 16; }
constexpr int dfww_pad32(int n) { return (n + 31) / 32 * 32; }

// fills w_off / b_off from in / out; returns the words of the image
inline int dense_fwdw_image_offsets(DenseFwdLayer* L, int nl) { return dense_fwd_offsets(L, nl, 32, 2); }

// tile == 0: the kernel's own choice of the rows of a tile for n rows on `cus` CUs.  One workgroup
// runs per CU either way (153 / 229 VGPRs); the large tile fetches each weight fragment half as often
// per row, the small one fills the CUs from half as many rows.
inline int dense_fwdw_rows(int64_t n, int cus, int tile) {
  if (tile == DFWW_ROWS_SMALL || tile == DFWW_ROWS_LARGE) return tile;
  return n >= (int64_t)DFWW_ROWS_LARGE * cus ? DFWW_ROWS_LARGE : DFWW_ROWS_SMALL;
}

inline DenseFwdWPlan dense_fwdw_plan(const DenseFwdLayer* L, int nl, int rows) {
  DenseFwdWPlan P{};
  int kmax = 0, off = 0;
  for (int l = 0; l < nl; ++l) {
    const int kp = dfww_pad32(L[l].in), np = dfww_pad16(L[l].out);
    kmax = kp > kmax ? kp : kmax;
    off += kp * np + 2 * np;
  }
  P.img_words = off;
  P.rows = rows;
  P.stride = kmax + DFWW_ROW_PAD;
  const int act = rows * P.stride * 2, part = DFWW_WAVES * rows * DFWW_PART_WORDS * 4;
  P.lds_bytes = act > part ? act : part;
  return P;
}
// the widest plan fits: LDS never refuses a stack inside the width limit
static_assert(DFWW_ROWS_LARGE * (DFWW_MAXW + DFWW_ROW_PAD) * 2 + DFWW_STATIC_LDS <= DFWW_LDS_BYTES, "LDS plan");

// empty if the kernel takes the stack (D inputs, nl layers whose image offsets lie inside img_words
// words, or anywhere if that is negative; score: the target is the input row, so out == D), else the
// limit it exceeds.  head: 0, or 1 for softmax over the last layer's units (its table entry is linear)
constexpr const char* DFWW_WHY_HEAD_SCORE = "scores need a reconstruction, not a softmax head";
constexpr const char* DFWW_WHY_HEAD = "a softmax head needs 2..512 units in the last layer and a linear last entry in the table";
inline std::string dense_fwdw_check(const DenseFwdLayer* L, int nl, int D, int64_t img_words, bool score, int head = 0) {
  if (head != 0 && score) return DFWW_WHY_HEAD_SCORE;
  const std::string why = dense_fwd_check_rows(L, nl, D, score, DFWW_MAXW, "wide fused");
  if (!why.empty()) return why;
  if (head != 0 && (head != 1 || L[nl - 1].out < 2 || L[nl - 1].act != 0)) return DFWW_WHY_HEAD;
  return dense_fwd_check_image(L, nl, img_words, 32, 2, "words");
}

}  // namespace sml
