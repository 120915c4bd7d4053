// The persistent small-batch Dense trainer's limits, its layer table and its two LDS plans (fp32:
// kernels/dense_minibatch.hip, bf16 MFMAs: kernels/dense_minibatch_bf16.hip), with the check that says
// which stacks the kernels take.  Plain C++17 with no HIP header, so a host program can include it and
// walk the check without a GPU (csrc/tests/dense_mb_plan_walk.cpp).  ops/dense_persistent.py mirrors
// the check and the LDS sizes in Python, because supports() must answer without a built extension;
// tests/test_dense_mb_plan.py holds the two together on the CPU.  What a plan's regions are for is
// written at the head of the kernel file that reads them.
#pragma once

#include <cstdint>
#include <string>

namespace sml {

enum : int {
  DMB_MAXLAYERS = 8,
  DMB_MAXW = 128,             // units / inputs of a layer
  DMB_MAXBATCH = 128,
  DMB_NT = 512,               // threads of the workgroup
  DMB_TPT = 2,                // 4x4 parameter tiles a thread can own (fp32)
  DMB_CHUNK = 32,             // rows of a batch in LDS at a time
  DMB_MAXPARAMS = DMB_NT * DMB_TPT * 16,   // kernel elements with both widths rounded up to 4 (fp32)
  DMB_LDS_BYTES = 160 * 1024,
  DMB_STATIC_LDS = 1024,      // a kernel's own copy of the layer table and plan, rounded up
  DMB_ACT_LAST = 3,           // activation codes 0 .. 3 (Act of sml_common.h: ACT_LINEAR .. ACT_SIGMOID)
  DMB_FP32 = 0,
  DMB_BF16 = 1,
  DMB_TILES_BF16 = 64,                        // 16x16 parameter tiles: 8 per wave
  DMB_MAXPARAMS_BF16 = DMB_TILES_BF16 * 256   // kernel elements with both widths rounded up to 16
};
struct DenseMBLayer {
  int in, units;
  int act;             // ACT_* code
  int has_bias;
  float l1, l2;        // activity regulariser of the layer's output
  int w_off, b_off;    // float offsets of the [in, units] kernel and the bias in flat / m / v
};

// ---- fp32: float offsets from the start of the dynamic LDS, derived from the table alone ----
struct DenseMBLayerPlan {
  int ip, up;          // in / units rounded up to 4
  int ws;              // floats between two rows of the kernel image (up, or up + 4: see the kernel)
  int lw, lb;          // kernel image [ip][ws], bias [up]
  int la, ld;          // the layer's output [DMB_CHUNK][up] and its gradient (the last layer's share one buffer)
  int tile0;           // first 4x4 tile (= owning thread) of the layer
};
struct DenseMBPlan {
  int dp;              // input width rounded up to 4
  int la0;             // input rows [DMB_CHUNK][dp]
  int lyt;             // target rows [DMB_CHUNK][op] (= la0 when y is null)
  int lstat;           // per-row loss / correct / penalty, then the step's totals
  int wimg0, wimg1;    // the weight image (zero-filled at launch)
  int ntiles;
  int lds_floats;
  DenseMBLayerPlan L[DMB_MAXLAYERS];
};

// ---- bf16: byte offsets from the start of the dynamic LDS, all multiples of 16 ----
struct DenseMBLayerPlanBF16 {
  int ip, up;          // in / units rounded up to 16
  int ws;              // bf16 elements between two rows of the weight image [up][ws] (unit-major), ip + 8
  int lw;              // the weight image
  int lb;              // fp32 bias, its two Adam moments and its gradient: 4 x [up]
  int hs, la;          // the layer's fp32 output [DMB_CHUNK][hs], hs = up + 4; overwritten by its fp32 gradient
  int bs;              // bf16 elements between two rows of the bf16 images, up + 8
  int lhb;             // bf16 output [DMB_CHUNK][bs] (the last layer has none)
  int ld;              // bf16 pre-activation gradient [DMB_CHUNK][bs]
  int tile0;           // first 16x16 tile of the layer; tile t belongs to wave t % 8, slot t / 8
};
struct DenseMBPlanBF16 {
  int dp;              // input width rounded up to 16
  int xs, la0;         // fp32 input rows [DMB_CHUNK][xs], xs = dp + 4
  int xbs, lxb;        // bf16 input rows [DMB_CHUNK][xbs], xbs = dp + 8
  int ys, lyt;         // fp32 target rows [DMB_CHUNK][ys] (= the input rows when y is null)
  int lstat;           // per-row loss / correct / penalty, then the step's totals
  int ltile;           // DMB_TILES_BF16 ints: layer << 16 | input block << 8 | unit block
  int ntiles;
  int lds_bytes;
  DenseMBLayerPlanBF16 L[DMB_MAXLAYERS];
};

constexpr int dmb_pad4(int n) { return (n + 3) / 4 * 4; }
constexpr int dmb_pad16(int n) { return (n + 15) / 16 * 16; }

inline DenseMBPlan dense_mb_plan(const DenseMBLayer* L, int nl, int D, bool own_targets) {
  constexpr int CH = DMB_CHUNK;
  DenseMBPlan P{};
  int off = 0, tiles = 0;
  P.dp = dmb_pad4(D);
  P.la0 = off;
  off += CH * P.dp;
  P.wimg0 = off;
  int prev = P.dp;
  for (int l = 0; l < nl; ++l) {
    DenseMBLayerPlan& q = P.L[l];
    q.ip = prev;
    q.up = dmb_pad4(L[l].units);
    q.ws = ((q.up >> 2) & 1) ? q.up : q.up + 4;
    q.lw = off;
    off += q.ip * q.ws;
    q.lb = off;
    off += q.up;
    q.tile0 = tiles;
    tiles += (q.ip >> 2) * (q.up >> 2);
    prev = q.up;
  }
  P.wimg1 = off;
  for (int l = 0; l < nl; ++l) {
    P.L[l].la = off;
    off += CH * P.L[l].up;
  }
  for (int l = 0; l < nl; ++l) {
    if (l == nl - 1) {
      P.L[l].ld = P.L[l].la;
    } else {
      P.L[l].ld = off;
      off += CH * P.L[l].up;
    }
  }
  if (own_targets) {
    P.lyt = off;
    off += CH * prev;
  } else {
    P.lyt = P.la0;
  }
  P.lstat = off;
  off += 4 * CH;
  P.ntiles = tiles;
  P.lds_floats = off;
  return P;
}

inline DenseMBPlanBF16 dense_mb_plan_bf16(const DenseMBLayer* L, int nl, int D, bool own_targets) {
  constexpr int CH = DMB_CHUNK;
  DenseMBPlanBF16 P{};
  int off = 0, tiles = 0;
  P.dp = dmb_pad16(D);
  P.xs = P.dp + 4;
  P.la0 = off;
  off += CH * P.xs * 4;
  P.xbs = P.dp + 8;
  P.lxb = off;
  off += CH * P.xbs * 2;
  int prev = P.dp;
  for (int l = 0; l < nl; ++l) {
    DenseMBLayerPlanBF16& q = P.L[l];
    q.ip = prev;
    q.up = dmb_pad16(L[l].units);
    q.ws = q.ip + 8;
    q.lw = off;
    off += q.up * q.ws * 2;
    q.lb = off;
    off += 4 * q.up * 4;
    q.tile0 = tiles;
    tiles += (q.ip >> 4) * (q.up >> 4);
    prev = q.up;
  }
  for (int l = 0; l < nl; ++l) {
    P.L[l].hs = P.L[l].up + 4;
    P.L[l].la = off;
    off += CH * P.L[l].hs * 4;
  }
  for (int l = 0; l < nl; ++l) {
    P.L[l].bs = P.L[l].up + 8;
    P.L[l].lhb = 0;
    if (l < nl - 1) {
      P.L[l].lhb = off;
      off += CH * P.L[l].bs * 2;
    }
  }
  for (int l = 0; l < nl; ++l) {
    P.L[l].ld = off;
    off += CH * P.L[l].bs * 2;
  }
  if (own_targets) {
    P.ys = prev + 4;
    P.lyt = off;
    off += CH * P.ys * 4;
  } else {
    P.ys = P.xs;
    P.lyt = P.la0;
  }
  P.lstat = off;
  off += 4 * CH * 4;
  P.ltile = off;
  off += DMB_TILES_BF16 * 4;
  P.ntiles = tiles;
  P.lds_bytes = off;
  return P;
}

// empty if the kernel of this precision can train the stack (D inputs, nl layers, parameter offsets
// inside nflat floats, this batch size, targets of their own or y = x), else the limit it exceeds
inline std::string dense_mb_check(const DenseMBLayer* L, int nl, int D, int batch, int64_t nflat, bool own_targets,
                                  int precision = DMB_FP32) {
  using std::to_string;
  if (precision != DMB_FP32 && precision != DMB_BF16)
    return "precision " + to_string(precision) + " is neither fp32 (0) nor bf16 (1)";
  const bool bf16 = precision == DMB_BF16;
  auto pad = [&](int n) { return bf16 ? dmb_pad16(n) : dmb_pad4(n); };
  if (nl < 1 || nl > DMB_MAXLAYERS)
    return to_string(nl) + " Dense layers: the persistent trainer takes 1.." + to_string(DMB_MAXLAYERS) + " (MAX_LAYERS)";
  if (batch < 1 || batch > DMB_MAXBATCH)
    return "batch " + to_string(batch) + " is outside 1.." + to_string(DMB_MAXBATCH) + " (MAX_BATCH)";
  if (D < 1 || D > DMB_MAXW)
    return "input width " + to_string(D) + " is outside 1.." + to_string(DMB_MAXW) + " (MAX_WIDTH)";
  int prev = D;
  int64_t padded = 0;
  for (int l = 0; l < nl; ++l) {
    if (L[l].in != prev) return "layer " + to_string(l) + " does not take the previous layer's width";
    if (L[l].units < 1 || L[l].units > DMB_MAXW)
      return "layer " + to_string(l) + " has " + to_string(L[l].units) + " units: the limit is " + to_string(DMB_MAXW) +
             " (MAX_WIDTH)";
    if (L[l].act < 0 || L[l].act > DMB_ACT_LAST) return "layer " + to_string(l) + ": unknown activation";
    const int64_t nw = (int64_t)L[l].in * L[l].units;
    if (L[l].w_off < 0 || L[l].w_off + nw > nflat ||
        (L[l].has_bias && (L[l].b_off < 0 || (int64_t)L[l].b_off + L[l].units > nflat)))
      return "layer " + to_string(l) + ": parameter offsets outside the flat buffer";
    padded += (int64_t)pad(L[l].in) * pad(L[l].units);
    prev = L[l].units;
  }
  // 256 padded elements make one 16x16 tile (a layer's padded input is the padded width before it),
  // so the bf16 limit also keeps the bf16 plan's ntiles within DMB_TILES_BF16
  if (bf16 && padded > DMB_MAXPARAMS_BF16)
    return to_string(padded) + " kernel elements (widths rounded up to 16): the limit is " + to_string(DMB_MAXPARAMS_BF16) +
           " (MAX_PARAMS_BF16)";
  if (!bf16 && padded > DMB_MAXPARAMS)
    return to_string(padded) + " kernel elements (widths rounded up to 4): the limit is " + to_string(DMB_MAXPARAMS) +
           " (MAX_PARAMS)";
  if (!own_targets && prev != D) return "y = x needs as many output units as inputs";
  const int64_t need = (bf16 ? (int64_t)dense_mb_plan_bf16(L, nl, D, own_targets).lds_bytes
                             : (int64_t)dense_mb_plan(L, nl, D, own_targets).lds_floats * 4) + DMB_STATIC_LDS;
  if (need > DMB_LDS_BYTES)
    return to_string(need) + " bytes of LDS: the limit is " + to_string(DMB_LDS_BYTES) + " (LDS_BYTES)";
  return "";
}

}  // namespace sml
