// The per-event Dense scorer on bf16 MFMAs (kernels/dense_serve_bf16.hip): its limits, its LDS plan and
// the check that names the limit a stack exceeds.  Plain C++17 with no HIP header, over
// sml_dense_fwdw_plan.h: the scorer reads the wide bulk forward's image (DenseFwdLayer, offsets in 16-bit
// words, dense_fwdw_image_offsets) and runs its arithmetic, so an event's reconstruction has the bits
// dense_forward_wide.hip gives that row.  ops/serve.py mirrors the check and the placement in Python
// (DenseScoringServer.supports / kernel_for with precision="bf16"), because they must answer without a
// built extension; csrc/tests/dense_serve_bf16_check.cpp asks this header on the host.
//
// LDS PLAN of the one resident workgroup (DSVB_NT threads, DSVB_WAVES waves; a pass serves up to DSVB_EB
// events, the 16 columns of a v_mfma_f32_16x16x32_bf16):
//   dynamic   two bf16 activation buffers [DSVB_EB][stride], stride = the widest padded k + DFWW_ROW_PAD
//             words (the bulk kernel's row: a B fragment is one 16-byte read, 16 rows on distinct banks),
//             used ping-pong; then, for "bf16-lds", the whole image
//   static    the pass's fp32 rows xn [DSVB_EB][32], the last layer's fp32 outputs [DSVB_EB][32], scale,
//             shift and the control words: DSVB_STATIC_LDS bytes, rounded up
#pragma once

#include <cstdint>
#include <string>

#include "sml_dense_fwdw_plan.h"

namespace sml {

enum : int {
  DSVB_MAXD = 32,              // features of a row: a request slot holds 32 words
  DSVB_EB = 16,                // events per pass: the columns of the MFMA
  DSVB_WAVES = 16,             // wave w owns the unit blocks w and w + 16
  DSVB_NT = 64 * DSVB_WAVES,   // threads of the workgroup: at most 128 VGPRs each
  DSVB_MAXUB = 2,              // unit blocks a wave owns at most: DFWW_MAXW / 16 / DSVB_WAVES
  DSVB_RING = 4,               // k-steps of weight fragments a wave keeps in flight
  DSVB_LDS_BYTES = 160 * 1024,
  DSVB_STATIC_LDS = 2 * DSVB_EB * DSVB_MAXD * 4 + 1024,
  // the widest plan's activation buffers
  DSVB_ACT_BYTES_MAX = 2 * DSVB_EB * (DFWW_MAXW + DFWW_ROW_PAD) * 2,
  // bytes of image that fit beside them at every stack inside the limits, in whole KiB: at or below
  // this the image is copied to LDS at launch ("bf16-lds"), above it every pass streams it from L2
  // ("bf16-stream")
  DSVB_LDS_IMAGE_BYTES = (DSVB_LDS_BYTES - DSVB_STATIC_LDS - DSVB_ACT_BYTES_MAX) / 1024 * 1024
};
static_assert(DSVB_MAXUB * DSVB_WAVES * 16 == DFWW_MAXW, "a wave's accumulators hold its whole unit slice");
static_assert(DSVB_ACT_BYTES_MAX + DSVB_LDS_IMAGE_BYTES + DSVB_STATIC_LDS <= 160 * 1024, "LDS plan");
static_assert(DSVB_LDS_IMAGE_BYTES == 122 * 1024, "ops/serve.py DenseScoringServer.LDS_IMAGE_BYTES_BF16");

struct DenseServeBf16Plan {
  int img_words;
  int stride;          // words between two activation rows in LDS
  int act_bytes;       // both activation buffers
  bool in_lds;         // the image follows them in LDS
  int lds_bytes;       // dynamic LDS
};

inline DenseServeBf16Plan dense_serve_bf16_plan(const DenseFwdLayer* L, int nl) {
  const DenseFwdWPlan W = dense_fwdw_plan(L, nl, DSVB_EB);
  DenseServeBf16Plan P{};
  P.img_words = W.img_words;
  P.stride = W.stride;
  P.act_bytes = 2 * DSVB_EB * W.stride * 2;
  P.in_lds = 2 * (int64_t)W.img_words <= DSVB_LDS_IMAGE_BYTES;
  P.lds_bytes = P.act_bytes + (P.in_lds ? 2 * W.img_words : 0);
  return P;
}

// empty if the scorer can serve the stack (D features, nl layers, the wide forward's image of img_words
// words, or any image if that is negative), else the limit it exceeds: the wide forward's rules, then the
// serving rules
inline std::string dense_serve_bf16_check(const DenseFwdLayer* L, int nl, int D, int64_t img_words) {
  const std::string why = dense_fwdw_check(L, nl, D, img_words, false);
  if (!why.empty()) return why;
  if (D > DSVB_MAXD) return "rows must have 1..32 features (a request slot holds 32 words)";
  if (L[nl - 1].out != D) return "the last layer must have one unit per feature";
  return "";
}

}  // namespace sml
