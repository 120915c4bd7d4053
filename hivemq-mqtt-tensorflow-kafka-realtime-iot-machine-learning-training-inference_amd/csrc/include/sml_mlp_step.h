// The fused MNIST-classifier train step (kernels/mlp_step.hip): its limits, the LDS plans of its two
// kernels and the split of the flat parameters over the workgroups of the second.  Plain C++17 with no
// HIP header, like sml_dense_batch.h; ops/mlp_step.py mirrors the check and the splits in Python.
#pragma once

#include <cstdint>
#include <string>

namespace sml {

enum : int {
  MLS_MAXBATCH = 32,      // two 16-row MFMA tiles
  MLS_MAXIN = 1024,       // the step's rows as fp32 in LDS: 32 x 1028 floats
  MLS_MAXHIDDEN = 512,
  MLS_MINCLASSES = 2,
  MLS_MAXCLASSES = 64,
  MLS_NT = 512,           // threads of both kernels
  MLS_WAVES = MLS_NT / 64,
  MLS_UB = 64,            // hidden units a workgroup of the forward owns
  MLS_PSTRIDE = MLS_UB + 4,   // floats per row of a wave's partial tile (16-byte aligned, off the bank period)
  MLS_KSPLIT = 8,         // slices of the head's contraction: fixed, so z's bits depend on no launch shape
  MLS_XCHUNK = 16,        // rows of W1 whose x columns the backward stages at a time
  MLS_ROWS_PER_GROUP = 8, // default: one backward workgroup per 8 rows of W1
  MLS_MAXGROUPS = 1024,
  MLS_LDS_LIMIT = 160 * 1024
};

constexpr int mls_pad4(int n) { return (n + 3) / 4 * 4; }
constexpr int mls_row_tile(int batch) { return batch <= 16 ? 16 : 32; }
// LDS stride of a staged row of x: a multiple of 4 with an odd quarter, so that the 16 rows x 4 k of
// a B-fragment read (address row * ldx + k) fall on 64 different banks
constexpr int mls_ldx(int in) { return (mls_pad4(in) / 4) & 1 ? mls_pad4(in) : mls_pad4(in) + 4; }
// stride of the h scratch, in global memory and in the backward's LDS
constexpr int mls_ldh(int hidden) { return mls_pad4(hidden); }
constexpr int mls_fwd_blocks(int hidden) { return (hidden + MLS_UB - 1) / MLS_UB; }
// parameters after W1 in the flat buffer: b1 | W2 | b2
constexpr int mls_tail(int hidden, int classes) { return hidden + hidden * classes + classes; }
constexpr int64_t mls_nparams(int in, int hidden, int classes) { return (int64_t)in * hidden + mls_tail(hidden, classes); }

// forward: the x tile [rt][ldx], overwritten by the waves' partial tiles [8][rt][MLS_PSTRIDE]
struct MlpStepFwdPlan {
  int rt, ldx, lds_bytes;
};
constexpr MlpStepFwdPlan mlp_step_fwd_plan(int batch, int in) {
  const int rt = mls_row_tile(batch), ldx = mls_ldx(in);
  const int x = rt * ldx, p = MLS_WAVES * rt * MLS_PSTRIDE;
  return {rt, ldx, 4 * (x > p ? x : p)};
}

// backward (offsets in floats): h -> dh [batch][ldh] | z slices [8][batch * C] | z -> dz [batch * C] |
// x columns [MLS_XCHUNK][32] | row index, label [2][32] (int) | loss, correct [2][32] | W2 | b2 if it fits
struct MlpStepBwdPlan {
  int ldh, o_h, o_zpart, o_z, o_x, o_idx, o_red, o_w2, w2_in_lds, lds_bytes;
};
constexpr MlpStepBwdPlan mlp_step_bwd_plan(int batch, int hidden, int classes) {
  MlpStepBwdPlan p{};
  p.ldh = mls_ldh(hidden);
  const int bc = mls_pad4(batch * classes);
  p.o_h = 0;
  p.o_zpart = p.o_h + batch * p.ldh;
  p.o_z = p.o_zpart + MLS_KSPLIT * bc;
  p.o_x = p.o_z + bc;
  p.o_idx = p.o_x + MLS_XCHUNK * MLS_MAXBATCH;
  p.o_red = p.o_idx + 2 * MLS_MAXBATCH;
  p.o_w2 = p.o_red + 2 * MLS_MAXBATCH;
  const int w2 = mls_pad4(hidden * classes + classes);
  p.w2_in_lds = 4 * (p.o_w2 + w2) <= MLS_LDS_LIMIT ? 1 : 0;
  p.lds_bytes = 4 * (p.o_w2 + (p.w2_in_lds ? w2 : 0));
  return p;
}

// workgroups of the backward: `groups` (<= 0: one per MLS_ROWS_PER_GROUP rows of W1, at most one per CU)
constexpr int mlp_step_groups(int in, int groups, int cus) {
  const int per = (in + MLS_ROWS_PER_GROUP - 1) / MLS_ROWS_PER_GROUP;
  const int want = groups > 0 ? groups : (per < cus ? per : cus);
  return want < 1 ? 1 : want > MLS_MAXGROUPS ? MLS_MAXGROUPS : want;
}

// Workgroup g of G owns the rows [first(g, G, in), first(g + 1, G, in)) of W1 and the elements
// [first(g, G, tail), first(g + 1, G, tail)) of b1 | W2 | b2: every parameter has exactly one owner.
constexpr int mlp_step_first(int g, int G, int n) { return (int)((int64_t)g * n / G); }

inline std::string mls_outside(const char* what, int64_t v, int lo, int hi, const char* name) {
  return std::string(what) + " " + std::to_string(v) + " is outside " + std::to_string(lo) + ".." + std::to_string(hi) +
         " (" + name + ")";
}

// empty if the fused step can train the model at this batch, else the limit it exceeds
inline std::string mlp_step_check(int64_t batch, int64_t in, int64_t hidden, int64_t classes, double rate, int64_t world) {
  if (batch < 1 || batch > MLS_MAXBATCH) return mls_outside("batch", batch, 1, MLS_MAXBATCH, "MLS_MAXBATCH");
  if (in < 1 || in > MLS_MAXIN) return mls_outside("in_features", in, 1, MLS_MAXIN, "MLS_MAXIN");
  if (hidden < 1 || hidden > MLS_MAXHIDDEN) return mls_outside("hidden", hidden, 1, MLS_MAXHIDDEN, "MLS_MAXHIDDEN");
  if (classes < MLS_MINCLASSES || classes > MLS_MAXCLASSES)
    return mls_outside("classes", classes, MLS_MINCLASSES, MLS_MAXCLASSES, "MLS_MAXCLASSES");
  if (!(rate >= 0.0 && rate < 1.0)) return "dropout rate " + std::to_string(rate) + " is outside [0, 1)";
  if (world != 1) return "world size " + std::to_string(world) + ": the fused step trains on one device (MLS_WORLD)";
  return "";
}

static_assert(mlp_step_fwd_plan(MLS_MAXBATCH, MLS_MAXIN).lds_bytes <= MLS_LDS_LIMIT, "forward LDS at the limits");
static_assert(mlp_step_bwd_plan(MLS_MAXBATCH, MLS_MAXHIDDEN, MLS_MAXCLASSES).lds_bytes <= MLS_LDS_LIMIT,
              "backward LDS at the limits");
static_assert(mlp_step_bwd_plan(32, 512, 10).w2_in_lds == 1, "the MNIST heads keep W2 in LDS");

}  // namespace sml
