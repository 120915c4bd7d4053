// The softmax + sparse categorical cross-entropy head of the wide Dense kernels (dense_batch_wide.hip,
// dense_forward_wide.hip): device code, shared so that the train step and the bulk forward give a row
// the same bits.
//
// In both kernels wave w holds, for every row of the tile, the logits of the unit blocks w, w + 8, ...
// in its accumulators: lane (c, g) has z[row c][unit 16 ub + 4 g + r].  A row's softmax spans all eight
// waves, so it is an online-softmax merge through the epilogue's partial array (DFWW_PART_WORDS words
// per wave and row), with one barrier between the two halves:
//   head_wave_partial  per wave and row: m_w = max of the wave's live logits with its first index,
//                      s_w = sum exp(z - m_w), and the label's logit if the wave owns that unit, folded
//                      over the four lane groups by lane ^ 16, lane ^ 32; lane group 0 writes them.  A
//                      wave without a block (wid >= nub) writes the neutral element (-inf, INT_MAX, 0, 0).
//   head_merge         after the barrier, by any lane: M = max m_w (lowest index on a tie), S = sum s_w
//                      exp(m_w - M) in ascending w, the label's logit.
// p_u = exp(z_u - M) / S and loss = log S + M - z_label follow in fp32.  Padded units (u >= N) take no
// part.  Every order is fixed, so the bits depend on the row and the weights alone.
#pragma once

#include <climits>

#include "sml_common.h"
#include "sml_dense_fwdw_plan.h"

namespace sml {

// (value, index) of the larger, the lower index on a tie
__device__ __forceinline__ void take_max(float& b, int& i, float ob, int oi) {
  if (ob > b || (ob == b && oi < i)) {
    b = ob;
    i = oi;
  }
}

struct DenseHeadRow {
  float M, S, zl;   // the row's largest logit, sum exp(z - M), the label's logit
  int arg;          // the first unit that holds M
};

// z[j][r]: the logit of unit 16 (wid + DFWW_WAVES j) + 4 (lane / 16) + r of the lane's row; p: this wave's
// and row's words of the partial array.  All 64 lanes of every wave must come here.
template <int UBN>
__device__ __forceinline__ void head_wave_partial(const f32x4 (&z)[UBN], int wid, int nub, int N, int label, int lane, float* p) {
  const int g = lane >> 4;
  float m = -INFINITY, s = 0.f, zl = 0.f;
  int im = INT_MAX;
  if (wid < nub) {
#pragma unroll
    for (int j = 0; j < UBN; ++j) {
      const int ub = wid + DFWW_WAVES * j;
      if (ub < nub) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int u = 16 * ub + 4 * g + r;
          if (u < N) {
            if (z[j][r] > m) { m = z[j][r]; im = u; }
            if (u == label) zl = z[j][r];
          }
        }
      }
    }
  }
  take_max(m, im, xor16(m, lane), xor16i(im, lane));
  take_max(m, im, xor32(m, lane), xor32i(im, lane));
  if (wid < nub) {   // m is finite: block wid has a live unit
#pragma unroll
    for (int j = 0; j < UBN; ++j) {
      const int ub = wid + DFWW_WAVES * j;
      if (ub < nub) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (16 * ub + 4 * g + r < N) s += expf(z[j][r] - m);
      }
    }
  }
  s += xor16(s, lane);
  s += xor32(s, lane);
  zl += xor16(zl, lane);
  zl += xor32(zl, lane);
  if (g == 0) {
    p[0] = m;
    p[1] = __int_as_float(im);
    p[2] = s;
    p[3] = zl;
  }
}

// the eight waves' partials of row `row` of a tile of `rows` rows, in wave order
__device__ __forceinline__ DenseHeadRow head_merge(const float* part, int rows, int row) {
  DenseHeadRow h = {-INFINITY, 0.f, 0.f, INT_MAX};
  const float* p = part + row * DFWW_PART_WORDS;
  for (int w = 0; w < DFWW_WAVES; ++w) take_max(h.M, h.arg, p[w * rows * DFWW_PART_WORDS], __float_as_int(p[w * rows * DFWW_PART_WORDS + 1]));
  for (int w = 0; w < DFWW_WAVES; ++w) {
    const float* q = p + w * rows * DFWW_PART_WORDS;
    h.S += q[2] * expf(q[0] - h.M);   // the neutral element: 0 * exp(-inf) = 0
    h.zl += q[3];
  }
  return h;
}

__device__ __forceinline__ float head_prob(float z, const DenseHeadRow& h) { return expf(z - h.M) / h.S; }
__device__ __forceinline__ float head_loss(const DenseHeadRow& h) { return logf(h.S) + h.M - h.zl; }

}  // namespace sml
