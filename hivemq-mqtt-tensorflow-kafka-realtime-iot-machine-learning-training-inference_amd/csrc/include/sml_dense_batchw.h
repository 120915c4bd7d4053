// The large-batch train step of WIDE Dense stacks (kernels/dense_batch_wide.hip): its limits, the
// offsets of its two bf16 weight images, of the step's activation workspace and of the per-workgroup
// buffers, the splits of a step over workgroups, and the check that names the limit a stack or a batch
// exceeds.  Plain C++17 with no HIP header, over sml_dense_mb_plan.h (the layer table DenseMBLayer:
// widths, activation, bias, penalties and the FlatParams offsets) and sml_dense_fwdw_plan.h (the
// fragment-order image of a layer and the padded LDS row).  ops/dense_batch_wide.py mirrors the check
// in Python, because supports() must answer without a built extension.
//
// IMAGES (16-bit words).  Per layer the forward image of sml_dense_fwdw_plan.h,
//   img[fw + ((kb * nub + ub) * 64 + lane) * 8 + j] = bf16(W[32 kb + 8 (lane / 16) + j][16 ub + lane % 16]),
// the fp32 bias [16 nub] (two words each), and the image of W^T in the same block layout with inputs
// and units swapped,
//   img[tw + ((kb * nib + ib) * 64 + lane) * 8 + j] = bf16(W[16 ib + lane % 16][32 kb + 8 (lane / 16) + j]),
// so the backward contraction g = dz . W^T is the forward's loop over the second image.
//
// WORKSPACE (16-bit words, rows padded to whole 64-row tiles).  For every layer l its bf16 input
// H_l [rows][pad32(in_l)] (H_0 is the staged x) and its bf16 pre-activation gradient
// DZ_l [rows][pad32(out_l)], row-major: the operands of the weight-gradient kernel.
#pragma once

#include <cstdint>
#include <string>

#include "sml_dense_fwdw_plan.h"
#include "sml_dense_mb_plan.h"

namespace sml {

enum : int {
  DBW_MAXLAYERS = DMB_MAXLAYERS,
  DBW_MAXW = DFWW_MAXW,        // units / inputs of a layer
  DBW_MAXBATCH = 1 << 24,      // a chosen bound, the narrow step's
  DBW_ROWS = DFWW_ROWS_SMALL,  // rows of a forward / backward tile
  DBW_KROWS = 32,              // rows of one k-step of the weight-gradient contraction
  DBW_WTILE = 128,             // a weight-gradient work item is DBW_WTILE inputs x DBW_WTILE units
  DBW_WTHREADS = 256,          // of the weight-gradient kernel: 2 x 2 waves of 64 x 64
  DBW_MAXSPLIT = 32,           // row splits (= gradient slabs) of a step at most
  DBW_LDS_BYTES = DFWW_LDS_BYTES
};
constexpr int64_t DBW_WS_BYTES = int64_t(1) << 30;   // the budget of a step's activation workspace

struct DenseBatchWLayerPlan {
  int fw, fb, tw;      // words into the image: W blocks, fp32 bias, W^T blocks
  int db;              // floats into a workgroup's bias-gradient partial
  int slot;            // floats into a workgroup's fp32 activation slot, -1: the layer keeps none
  int hw, dw;          // pad32(in), pad32(out): words of a workspace row of H_l and DZ_l
  int64_t h, dz;       // words into the workspace
};
struct DenseBatchWPlan {
  int img_words;
  int ndb;             // floats of a workgroup's bias-gradient partial
  int slot_floats;     // floats of a workgroup's activation slot
  int stride;          // words between two activation rows in LDS
  int act_bytes;       // the activation tile in LDS
  int db_off, part_off;   // bytes into the dynamic LDS: bias-gradient sums, epilogue partials
  int lds_bytes;
  int rows;            // workspace rows: the batch rounded up to DBW_ROWS
  int wtiles;          // weight-gradient tiles of all layers
  int64_t ws_words;
  DenseBatchWLayerPlan L[DBW_MAXLAYERS];
};

constexpr int dense_batchw_tiles(int batch) { return (batch + DBW_ROWS - 1) / DBW_ROWS; }

// forward / backward workgroups of a step: `groups` (<= 0: one per CU), never more than it has tiles
constexpr int dense_batchw_groups(int batch, int groups, int cus) {
  const int want = groups > 0 ? groups : cus, n = dense_batchw_tiles(batch);
  return want < n ? (want < 1 ? 1 : want) : n;
}

// a hidden layer's unrounded output is kept for its derivative unless that is 1 and no penalty needs it
inline bool dense_batchw_keeps(const DenseMBLayer& L) { return L.act != 0 || L.l1 != 0.0f || L.l2 != 0.0f; }

inline DenseBatchWPlan dense_batchw_plan(const DenseMBLayer* L, int nl, int batch) {
  DenseBatchWPlan P{};
  int off = 0, kmax = 0;
  P.rows = dense_batchw_tiles(batch) * DBW_ROWS;
  for (int l = 0; l < nl; ++l) {
    DenseBatchWLayerPlan& q = P.L[l];
    const int in = L[l].in, out = L[l].units;
    q.fw = off;
    off += dfww_pad32(in) * dfww_pad16(out);
    q.fb = off;
    off += 2 * dfww_pad16(out);
    q.tw = off;
    off += dfww_pad32(out) * dfww_pad16(in);
    q.db = P.ndb;
    P.ndb += dfww_pad16(out);
    q.slot = -1;
    if (l < nl - 1 && dense_batchw_keeps(L[l])) {
      q.slot = P.slot_floats;
      P.slot_floats += DBW_ROWS * dfww_pad16(out);
    }
    q.hw = dfww_pad32(in);
    q.dw = dfww_pad32(out);
    kmax = q.hw > kmax ? q.hw : kmax;
    kmax = q.dw > kmax ? q.dw : kmax;
    q.h = P.ws_words;
    P.ws_words += (int64_t)P.rows * q.hw;
    q.dz = P.ws_words;
    P.ws_words += (int64_t)P.rows * q.dw;
    P.wtiles += ((in + DBW_WTILE - 1) / DBW_WTILE) * ((out + DBW_WTILE - 1) / DBW_WTILE);
  }
  P.img_words = off;
  P.stride = kmax + DFWW_ROW_PAD;
  P.act_bytes = DBW_ROWS * P.stride * 2;
  P.db_off = P.act_bytes;
  P.part_off = P.db_off + P.ndb * 4;
  P.lds_bytes = P.part_off + DFWW_WAVES * DBW_ROWS * DFWW_PART_WORDS * 4;
  return P;
}
// the widest plan fits: LDS never refuses a stack inside the limits
static_assert(DBW_ROWS * (DBW_MAXW + DFWW_ROW_PAD) * 2 + DBW_MAXLAYERS * DBW_MAXW * 4 +
                      DFWW_WAVES * DBW_ROWS * DFWW_PART_WORDS * 4 + 8192 <= DBW_LDS_BYTES, "LDS plan");

// row splits of the weight-gradient contraction (= slabs the apply step sums): `splits` (<= 0: enough to
// give every CU two work items), never more than the step has k-steps or than DBW_MAXSPLIT.  Static in
// the batch, the CU count and the stack, so a result's bits depend on the batch, the grid and S alone.
inline int dense_batchw_splits(int batch, int splits, int cus, int wtiles) {
  const int ksteps = dense_batchw_tiles(batch) * (DBW_ROWS / DBW_KROWS);
  int want = splits > 0 ? splits : (2 * cus + wtiles - 1) / (wtiles > 0 ? wtiles : 1);
  want = want < 1 ? 1 : want;
  want = want < DBW_MAXSPLIT ? want : (int)DBW_MAXSPLIT;
  return want < ksteps ? want : ksteps;
}

// the loss head of the step's last layer: none (mean squared error on the layer's own activation), or
// softmax over its units with sparse categorical cross-entropy against integer labels
enum : int { DBW_HEAD_NONE = 0, DBW_HEAD_SOFTMAX = 1 };
constexpr const char* DBW_WHY_HEAD =
    "a softmax head needs 2..512 units in the last layer, a linear last entry in the table, no penalty on the last "
    "layer, and labels";

// empty if the step can train the stack at this batch (D inputs, nl layers, parameter offsets inside
// nflat floats, targets of their own or y = x; head: own_targets says that labels came), else the limit
// it exceeds
inline std::string dense_batchw_check(const DenseMBLayer* L, int nl, int D, int64_t batch, int64_t nflat, bool own_targets,
                                      int head = DBW_HEAD_NONE) {
  using std::to_string;
  if (nl < 1 || nl > DBW_MAXLAYERS)
    return to_string(nl) + " Dense layers: the wide trainer takes 1.." + to_string((int)DBW_MAXLAYERS) + " (MAX_LAYERS)";
  if (D < 1 || D > DBW_MAXW)
    return "input width " + to_string(D) + " is outside 1.." + to_string((int)DBW_MAXW) + " (MAX_WIDTH)";
  int prev = D;
  for (int l = 0; l < nl; ++l) {
    if (L[l].in != prev) return "layer " + to_string(l) + " does not take the previous layer's width";
    if (L[l].units < 1 || L[l].units > DBW_MAXW)
      return "layer " + to_string(l) + " has " + to_string(L[l].units) + " units: the limit is " + to_string((int)DBW_MAXW) +
             " (MAX_WIDTH)";
    if (L[l].act < 0 || L[l].act > DMB_ACT_LAST) return "layer " + to_string(l) + ": unknown activation";
    const int64_t nw = (int64_t)L[l].in * L[l].units;
    if (L[l].w_off < 0 || L[l].w_off + nw > nflat ||
        (L[l].has_bias && (L[l].b_off < 0 || (int64_t)L[l].b_off + L[l].units > nflat)))
      return "layer " + to_string(l) + ": parameter offsets outside the flat buffer";
    prev = L[l].units;
  }
  if (head != DBW_HEAD_NONE) {
    const DenseMBLayer& H = L[nl - 1];
    if (head != DBW_HEAD_SOFTMAX) return "unknown head " + to_string(head);
    if (H.units < 2 || H.act != 0 || H.l1 != 0.0f || H.l2 != 0.0f || !own_targets) return DBW_WHY_HEAD;
  }
  if (!own_targets && prev != D) return "y = x needs as many output units as inputs";
  if (batch < 1 || batch > DBW_MAXBATCH)
    return "batch " + to_string(batch) + " is outside 1.." + to_string((int)DBW_MAXBATCH) + " (MAX_BATCH)";
  const int64_t need = dense_batchw_plan(L, nl, (int)batch).ws_words * 2;
  if (need > DBW_WS_BYTES)
    return to_string(need) + " bytes of activation workspace at batch " + to_string(batch) + ": the budget is " +
           to_string(DBW_WS_BYTES) + " (WS_BYTES)";
  return "";
}

}  // namespace sml
