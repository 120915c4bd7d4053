// The per-event Dense scorers' limits and layer table (kernels/dense_serve.hip: one model;
// kernels/dense_serve_fleet.hip: a fleet of models of one shape, a model index per event), the fleet
// kernel's arguments and the checks that say which stacks and fleets they take.  Plain C++17 with no
// HIP header, so a host program can include it and ask the checks without a GPU
// (csrc/tests/dense_fleet_serve_check.cpp).  ops/serve.py mirrors the checks in Python, because
// supports() must answer without a built extension; tests/test_dense_serve_limits.py and
// tests/test_dense_fleet_serve.py hold the two together on the CPU.  sml_ops.h includes this header.
#pragma once

#include <cstdint>

namespace sml {

struct ServeCtl;
struct ServeReq;
struct ServeResult;

// Same rings, framing and result words as ae_serve: 1..DSV_MAXLAYERS Dense layers, every width
// 1..DSV_MAXW, the last layer one unit per feature.  fp32 throughout.  One resident workgroup
// scores up to DSV_EB events per pass; an event's result bits do not depend on how the ring
// batched it.
enum : int {
  DSV_MAXW = 512,             // units / inputs of a layer
  DSV_MAXLAYERS = 8,
  DSV_EB = 8,                 // events per pass
  DSV_NT = 1024,              // threads of the workgroup
  DSV_TILE = 32,              // output widths are zero-padded to this, input widths to 4
  DSV_MAXKS = 16,             // slices of a layer's reduction
  // bytes of weight image that fit the CU's 160 KiB of LDS beside the activation and
  // partial-sum buffers (64 KiB) and the kernel's small static arrays: at or below this
  // the image is copied to LDS at launch ("lds"), above it every pass streams it ("stream")
  DSV_LDS_IMAGE_BYTES = 92 * 1024,
  DSV_ACT_LAST = 3,           // activation codes 0 .. 3 (Act of sml_common.h: ACT_LINEAR .. ACT_SIGMOID)
  DSV_FLEET_MAXD = 31,        // fleet rows: request word 31 carries the event's model index
  DSV_FLEET_MAXMODELS = 1 << 24   // exclusive
};
struct DenseServeLayer {
  int in, out;         // input width, units
  int act;             // ACT_* code
  int w_off, b_off;    // float offsets of the layer's weight image and padded bias in the image
};
constexpr int dense_serve_kp(int in) { return (in + 3) / 4 * 4; }
constexpr int dense_serve_np(int out) { return (out + DSV_TILE - 1) / DSV_TILE * DSV_TILE; }
// slices of a layer's reduction: a power of two fixed by the layer's shape alone -- the largest
// with Np * KS <= DSV_NT threads, at least one 4-row group per slice and KS <= DSV_MAXKS
constexpr int dense_serve_k_slices(int in, int out) {
  int ks = 1;
  while (dense_serve_np(out) * ks * 2 <= DSV_NT && ks * 2 <= dense_serve_kp(in) / 4 && ks * 2 <= DSV_MAXKS) ks *= 2;
  return ks;
}
// floats of one layer in the image: float4 img[Kp / 4][Np] (img[g][o] = W[4g .. 4g + 3][o]), then bias[Np]
constexpr int dense_serve_layer_floats(int in, int out) {
  return dense_serve_kp(in) * dense_serve_np(out) + dense_serve_np(out);
}

// ---- a fleet of Dense stacks of one shape (dense_serve_fleet.hip) ----
// The n_models images lie one after the other in device memory, img[n_models][stride], each laid
// out as the single-model image; ONE layer table serves them all, its offsets relative to a
// model's image.  Request word 31 carries the event's model index (tagged like the row's words),
// so rows have 1..DSV_FLEET_MAXD features.  One scale / shift pair normalises every model's rows.
struct DenseFleetServeArgs {
  ServeCtl* ctl;
  const ServeReq* req;
  ServeResult* res;
  int nslots;
  int D;
  const float* img;    // [n_models][stride] (device)
  const float* thr;    // [n_models] thresholds (device)
  int img_floats;      // floats of one image
  int stride;          // floats between two images: >= img_floats, a multiple of 4
  int n_models;
  int nl;
  DenseServeLayer L[DSV_MAXLAYERS];
  const float* scale;  // [D] or null
  const float* shift;
  uint64_t idle_ticks;
  uint64_t* stats;     // host-mapped: {passes << 32 | events}, cumulative, stored after each pass
};

// floats between two images of a fleet whose single image has img_floats floats
constexpr int64_t dense_fleet_serve_stride(int64_t img_floats) { return (img_floats + 3) / 4 * 4; }

// The layer-table rules of both scorers: empty if a stack of this table (D features in rows of at
// most max_D, nl layers, offsets inside an image of img_floats floats) can be served, else the limit
// it exceeds (rows_why: the message of the row limit)
inline const char* dense_serve_check_rows(const DenseServeLayer* L, int nl, int D, int64_t img_floats, int max_D,
                                          const char* rows_why) {
  if (D < 1 || D > max_D) return rows_why;
  if (nl < 1 || nl > DSV_MAXLAYERS) return "the stack must have 1..8 Dense layers";
  int dim = D;
  int64_t total = 0;
  for (int l = 0; l < nl; ++l) {
    if (L[l].out < 1 || L[l].out > DSV_MAXW) return "Dense layers must have 1..512 units";
    if (L[l].in != dim) return "a layer's input width must match the layer below";
    if (L[l].act < 0 || L[l].act > DSV_ACT_LAST) return "activations must be linear, relu, tanh or sigmoid";
    const int64_t wn = (int64_t)dense_serve_kp(L[l].in) * dense_serve_np(L[l].out);
    if (L[l].w_off < 0 || (L[l].w_off & 3) || (int64_t)L[l].w_off + wn > img_floats || L[l].b_off < 0 ||
        (L[l].b_off & 3) || (int64_t)L[l].b_off + dense_serve_np(L[l].out) > img_floats)
      return "a layer's weights lie outside the weight image";
    total += dense_serve_layer_floats(L[l].in, L[l].out);
    dim = L[l].out;
  }
  if (dim != D) return "the last layer must have one unit per feature";
  if (img_floats != total) return "the weight image has the wrong length";
  return "";
}

// empty if the single-model kernel can serve the stack, else the limit it exceeds
inline const char* dense_serve_check(const DenseServeLayer* L, int nl, int D, int64_t img_floats) {
  return dense_serve_check_rows(L, nl, D, img_floats, 32, "rows must have 1..32 features (a request slot holds 32 words)");
}

// the single-model kernel copies the whole image to LDS: a pure function of the layer table and
// DSV_LDS_IMAGE_BYTES
inline bool dense_serve_in_lds(const DenseServeLayer* L, int nl) {
  int64_t bytes = 0;
  for (int l = 0; l < nl && l < DSV_MAXLAYERS; ++l) bytes += 4 * (int64_t)dense_serve_layer_floats(L[l].in, L[l].out);
  return bytes <= DSV_LDS_IMAGE_BYTES;
}

// empty if the fleet kernel can serve n_models stacks of this table (images stride floats apart),
// else the limit it exceeds: the single-model rules with rows of at most 31 features, then the
// stride's and the fleet size's
inline const char* dense_fleet_serve_check(const DenseServeLayer* L, int nl, int D, int64_t img_floats, int64_t stride,
                                           int64_t n_models) {
  const char* why = dense_serve_check_rows(L, nl, D, img_floats, DSV_FLEET_MAXD,
                                           "rows must have 1..31 features (request word 31 carries the model index)");
  if (why[0]) return why;
  if (stride % 4 != 0 || stride < img_floats)
    return "the image stride must be a multiple of 4 floats and at least one image long";
  if (n_models < 1 || n_models >= DSV_FLEET_MAXMODELS) return "a fleet must have 1..16777215 models";
  return "";
}

}  // namespace sml
