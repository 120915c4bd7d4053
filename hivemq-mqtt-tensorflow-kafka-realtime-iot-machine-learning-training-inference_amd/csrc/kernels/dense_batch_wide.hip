// Large-batch train step for WIDE Dense stacks: 1..8 Dense layers, every width (input included) up to
// 512, any batch the activation workspace holds, for nn.Model.fit(engine="wide") through
// ops/dense_batch_wide.py.  Limits, image and workspace layout, the splits: sml_dense_batchw.h.
// sml-build: no-packed-fp32
//
// A Keras step is FOUR launches on one stream and no host synchronisation: the three of this file and
// dense_batch.hip's dense_batch_apply_launch (slab sum in ascending order, Adam on the fp32 masters).
//
// ARITHMETIC.  The rounding points of the bf16 trainers: z_l = b_l + bf(h_{l-1}) . bf(W_l) with fp32
// accumulation, h_l = act(z_l) unrounded; the unrounded h_l feeds the loss, the l1 / l2 penalties, the
// accuracy and the derivative; g_{l-1} = bf(dz_l) . bf(W_l)^T; dW_l = bf(h_{l-1})^T . bf(dz_l); db_l the
// fp32 column sum of the unrounded dz_l; the mean and penalty divisors are the whole batch's.
//
// 1. dense_batchw_image_kernel: one thread per 16 bytes of the image.  From the masters in FlatParams
//    order it writes, per layer, bf(W) and bf(W^T) in MFMA A-fragment order and the fp32 bias; zero in
//    every padded place.  A W^T fragment is eight consecutive floats of a kernel row: two 16-byte loads
//    where they are aligned.
//
// 2. dense_batchw_fb_kernel: forward and backward, the split of dense_forward_wide.hip.  A persistent grid
//    of G workgroups with static contiguous spans of 64-row tiles; 8 waves; the tile's current activation
//    is bf16 in LDS, [64][stride].  Every layer is computed transposed on v_mfma_f32_16x16x32_bf16: wave w
//    owns the unit blocks w, w + 8, w + 16, w + 24 for all rows, streams its A fragments from the image
//    (L2) with the next k-step's in flight, and writes its results back in place behind a barrier.
//    FORWARD adds: every layer's bf16 input (the staged bf(x) first) leaves LDS row-major for the
//    workspace in 16-byte stores; the unrounded h_l of a hidden layer whose derivative or penalty needs
//    it goes to the workgroup's fp32 slot in global memory at the lane's own (row, 4 units), 16 bytes,
//    and is read back once by the same lane in the backward pass: the slot is reused tile after tile.
//    LAST LAYER: the epilogue forms dz_L from the unrounded output and the target (x again, or y), and
//    folds squared error and argmax match as the forward kernel does: lane, lane ^ 16, lane ^ 32, one
//    partial per wave and row in LDS, waves in order; no atomics.
//    BACKWARD, l = L .. 2: bf(dz_l) is the LDS tile (and leaves for the workspace); the same MFMA loop over
//    the W^T image gives g_{l-1} in the accumulators of the lanes that held h_{l-1}; times act'(h_{l-1})
//    plus the penalty gradient is dz_{l-1}.  Layer 1 needs no g_0.
//    BIAS: a unit belongs to one wave; the lane adds its four row tiles in order, the 16 row lanes fold
//    by xor 1, 2, 4, 8, and lane c = 0 adds into the workgroup's fp32 LDS array.  One partial per
//    workgroup leaves at the end, with its [loss, correct] pair (sums kept in doubles per thread and
//    folded in index order).
//    SOFTMAX HEAD (a.head = DBW_HEAD_SOFTMAX, the kernel's second instance; sml_dense_head.h): the last
//    layer is linear in the table and its loss is sparse categorical cross-entropy against a.labels
//    (int32 per sample, addressed through order / row0 as target rows are; a.y is null).  A row's
//    softmax spans the eight waves, so the epilogue is an online-softmax merge through s_part with ONE
//    more barrier: per wave and row (max, argmax, sum exp(z - max), the label's logit), a wave without a
//    block writing the neutral element; after the barrier every lane merges the eight partials of its
//    rows in wave order and forms dz = (p - [u == label]) / batch from the logits still in its
//    accumulators.  bf16 dz to LDS and the workspace, unrounded column sums and the zero-fill are the
//    squared-error path's; the row's thread adds log S + M - z_label and the argmax match, and the
//    workgroup's loss is their sum / batch + penalties / batch.  Padded units take no part, a row past
//    `live` gets dz = 0.  The accumulators live across that barrier: the instance without a head keeps
//    the 153 VGPRs it had (layer<1>, <2> and <4> are inlined into one kernel, so the count is the
//    kernel's: 153 before the head existed, 153 / 161 without / with it now); neither uses scratch.
//    Rows past the batch are staged as zero and their dz is zero; padded k and units meet zero weights
//    only; with an odd number of unit blocks the wave that would own the next block zero-fills it, in
//    both directions.
//
// 3. dense_batchw_wgrad_kernel: one grouped launch for all layers.  A work item is (layer, 128 inputs x
//    128 units, row split s of S) from a host-built table; 2 x 2 waves of 64 x 64.  The contraction runs
//    over the rows of split s, 32 at a time: both operands are row-major in the workspace, so rows lie on
//    k; a k-step's [32][128] slices are staged through LDS with 16-byte loads (the next step's in
//    registers under the MFMAs) and read as fragments with ds_read_b64_tr_b16.  The fp32 tile goes to
//    slab s at its FlatParams offsets.  S more items fold the workgroups' bias partials and pairs into
//    slabs / pairs 0 .. S - 1 over static contiguous ranges, in ascending order.
#include <climits>

#include "sml_common.h"
#include "sml_dense_fwd_launch.h"
#include "sml_dense_head.h"
#include "sml_ops.h"

namespace sml {
namespace {

constexpr int NWV = DFWW_WAVES, NTHR = 64 * DFWW_WAVES, R = DBW_ROWS, RT = DBW_ROWS / 16;
constexpr int IMG_NT = 256;
constexpr int WG_STRIDE = (DBW_WTILE + 8) * 2;   // bytes between two staged rows of the weight-gradient kernel

__device__ __forceinline__ f32x4 mfma_k32(s16x8 a, s16x8 b, f32x4 c) {
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float pen_grad(float l1, float l2, float h, float inv_rows) {
  const float sg = h > 0.0f ? 1.0f : h < 0.0f ? -1.0f : 0.0f;
  return (l1 * sg + 2.0f * l2 * h) * inv_rows;
}

// ---------------------------------------------------------------- 1. the images
__global__ __launch_bounds__(IMG_NT) void dense_batchw_image_kernel(const DenseBatchWArgs a) {
  const int w = 8 * (int)(blockIdx.x * IMG_NT + threadIdx.x);   // first word of this thread's 16 bytes
  if (w >= a.P.img_words) return;
  for (int l = 0; l < a.nl; ++l) {   // l stays uniform: the tables are read with scalar loads
    const DenseBatchWLayerPlan& q = a.P.L[l];
    const int end = l + 1 < a.nl ? a.P.L[l + 1].fw : a.P.img_words;
    if (w < q.fw || w >= end) continue;
    const int in = a.L[l].in, out = a.L[l].units;
    const float* W = a.flat + a.L[l].w_off;
    if (w >= q.fb && w < q.tw) {   // four bias floats
      const int u0 = (w - q.fb) >> 1;
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (a.L[l].has_bias && u0 + j < out) b[j] = a.flat[a.L[l].b_off + u0 + j];
      st4(reinterpret_cast<float*>(a.image + w), b);
      return;
    }
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (w < q.fb) {   // W: lane (c, g) of block (kb, ub) holds W[32 kb + 8 g + j][16 ub + c]
      const int e = (w - q.fw) >> 3, lane = e & 63, blk = e >> 6, nub = dfww_pad16(out) >> 4;
      const int kb = blk / nub, ub = blk - kb * nub, u = 16 * ub + (lane & 15), k0 = 32 * kb + 8 * (lane >> 4);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k0 + j < in && u < out) v[j] = W[(k0 + j) * out + u];
    } else {          // W^T: lane (c, g) of block (kb, ib) holds W[16 ib + c][32 kb + 8 g + j]
      const int e = (w - q.tw) >> 3, lane = e & 63, blk = e >> 6, nib = dfww_pad16(in) >> 4;
      const int kb = blk / nib, ib = blk - kb * nib, i = 16 * ib + (lane & 15), k0 = 32 * kb + 8 * (lane >> 4);
      if (i < in) {
        const int f = a.L[l].w_off + i * out + k0;
        if (k0 + 8 <= out && (f & 3) == 0) {
          const f32x4 lo = ld4(a.flat + f), hi = ld4(a.flat + f + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = lo[j];
            v[4 + j] = hi[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k0 + j < out) v[j] = a.flat[f + j];
        }
      }
    }
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 p = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
    *reinterpret_cast<u32x4*>(a.image + w) = p;
    return;
  }
}

// ---------------------------------------------------------------- 2. forward and backward
struct Tile {
  uint16_t* s_act;
  float* s_db;
  float* s_part;
  float* slot;         // the workgroup's fp32 activations
  int64_t pos0;        // the tile's first position in the step's row sequence (order / x index)
  int64_t wrow0;       // its first workspace row
  int live;
  float inv_n, inv_rows;
};

// the LDS tile's first `width` words of every row -> workspace rows wrow0 .., 16 bytes a thread
__device__ __forceinline__ void copy_out(const DenseBatchWArgs& a, const Tile& T, int64_t dst, int width, int tid) {
  const int per = width >> 3;
  uint16_t* out = a.ws + dst + T.wrow0 * width;
  for (int i = tid; i < R * per; i += NTHR) {
    const int r = i / per, q = i - r * per;
    *reinterpret_cast<s16x8*>(out + r * width + 8 * q) = *reinterpret_cast<const s16x8*>(T.s_act + r * a.P.stride + 8 * q);
  }
}

// acc[t][j] = (bias or 0) + image block row (wid + 8 j) . the LDS tile, for K inputs and N outputs.  The
// loop of dense_forward_wide.hip: no branch inside, a block past nub runs on block nub - 1's fragments
// (the loads stay inside the image) and is never used.
template <int UBN>
__device__ __forceinline__ void mfma_loop(const uint16_t* img, const float* bias, int K, int N, const uint16_t* s_act, int S,
                                          int lane, int wid, f32x4 (&acc)[RT][UBN]) {
  const int c = lane & 15, g = lane >> 4;
  const int nkb = (K + 31) >> 5, nub = (N + 15) >> 4;
  if (wid >= nub) return;
  const s16x8* W[UBN];
  s16x8 wc[UBN], wn[UBN];
#pragma unroll
  for (int j = 0; j < UBN; ++j) {
    const int ub = wid + NWV * j < nub ? wid + NWV * j : nub - 1;
    W[j] = reinterpret_cast<const s16x8*>(img) + ub * 64 + lane;
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (bias) b = ld4(bias + 16 * ub + 4 * g);
    wc[j] = *W[j];
    wn[j] = wc[j];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t][j] = b;
  }
  const uint16_t* brow = s_act + c * S + 8 * g;
  const int wstep = nub * 64;
#pragma unroll 1
  for (int kb = 0; kb < nkb; ++kb) {
    if (kb + 1 < nkb) {
#pragma unroll
      for (int j = 0; j < UBN; ++j) {
        W[j] += wstep;
        wn[j] = *W[j];
      }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const s16x8 b = *reinterpret_cast<const s16x8*>(brow + 16 * t * S);
#pragma unroll
      for (int j = 0; j < UBN; ++j) acc[t][j] = mfma_k32(wc[j], b, acc[t][j]);
    }
    brow += 32;
#pragma unroll
    for (int j = 0; j < UBN; ++j) wc[j] = wn[j];
  }
}

// One contraction over the tile and what follows it.  Forward (bwd false): layer l's output from its
// input; a hidden layer's h goes back to LDS (and to the slot), the last layer's becomes dz_L.
// Backward: dz_{l-1} from dz_l.  `lo` is the layer whose output units the accumulators hold.
template <int UBN, bool HEAD>
__device__ __forceinline__ void layer(const DenseBatchWArgs& a, const Tile& T, int l, bool bwd, int tid, double& lsum,
                                      double& lcnt, double& lpen) {
  const int lane = opaque(tid) & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
  const int lo = bwd ? l - 1 : l;
  const DenseBatchWLayerPlan& Po = a.P.L[lo];
  const int K = bwd ? a.L[l].units : a.L[l].in, N = a.L[lo].units, act = a.L[lo].act;
  const int nub = (N + 15) >> 4, np = 16 * nub, S = a.P.stride;
  const float l1 = a.L[lo].l1, l2 = a.L[lo].l2;
  const bool pen = l1 != 0.0f || l2 != 0.0f, last = !bwd && l == a.nl - 1, is_dz = bwd || last;
  const bool head = HEAD && last;
  f32x4 acc[RT][UBN];
  mfma_loop<UBN>(a.image + (bwd ? a.P.L[l].tw : a.P.L[l].fw),
                 bwd ? nullptr : reinterpret_cast<const float*>(a.image + a.P.L[l].fb), K, N, T.s_act, S, lane, wid, acc);
  __syncthreads();   // every wave has read the contraction's input: the tile is free

  int lab[RT];
  if (head) {   // uniform: every wave's partial of every row, then the head's one barrier
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int rr = 16 * t + c;
      lab[t] = -1;
      if (rr < T.live) {
        const int64_t pos = T.pos0 + rr;
        lab[t] = a.labels[a.order ? (int64_t)a.order[pos] : pos];
      }
      head_wave_partial<UBN>(acc[t], wid, nub, N, lab[t], lane, T.s_part + (wid * R + rr) * DFWW_PART_WORDS);
    }
    __syncthreads();
  }

  f32x4 dbs[UBN];
#pragma unroll
  for (int j = 0; j < UBN; ++j) dbs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int rr = 16 * t + c;
    const bool rlive = rr < T.live;
    const float* trow = nullptr;
    DenseHeadRow hr = {};
    if (head) hr = head_merge(T.s_part, R, rr);
    if (last && !head && rlive) {
      const int64_t pos = T.pos0 + rr, smp = a.order ? (int64_t)a.order[pos] : pos;
      trow = a.y ? a.y + smp * a.ldy : a.x + smp * a.ldx;
    }
    float se = 0.f, by = -INFINITY, bt = -INFINITY;
    int iy = INT_MAX, it = INT_MAX;
    if (wid < nub) {
#pragma unroll
      for (int j = 0; j < UBN; ++j) {
        const int ub = wid + NWV * j;
        if (ub < nub) {
          const int u0 = 16 * ub + 4 * g;
          f32x4 v;
          if (!bwd) {
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = act_fwd(act, acc[t][j][r]);
            if (pen) {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (rlive && u0 + r < N) {
                  s1 += fabsf(h[r]);
                  s2 = fmaf(h[r], h[r], s2);
                }
            }
            if (!last) {
              if (Po.slot >= 0) st4(T.slot + Po.slot + rr * np + u0, h);
              v = h;
            } else if (head) {   // dz = (p - [u == label]) / batch from the logits the accumulators still hold
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int u = u0 + r;
                const float p = head_prob(acc[t][j][r], hr) - (u == lab[t] ? 1.0f : 0.0f);
                v[r] = (rlive && u < N) ? p * T.inv_rows : 0.0f;
              }
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int u = u0 + r;
                const bool ok = rlive && u < N;
                const float tg = ok ? trow[u] : 0.0f, d = h[r] - tg;
                if (ok) {
                  se = fmaf(d, d, se);
                  if (h[r] > by) { by = h[r]; iy = u; }
                  if (tg > bt) { bt = tg; it = u; }
                }
                float gg = 2.0f * d * T.inv_n;
                if (pen) gg += pen_grad(l1, l2, h[r], T.inv_rows);
                v[r] = ok ? act_grad(act, h[r], gg) : 0.0f;
              }
            }
          } else {
            f32x4 h = {0.f, 0.f, 0.f, 0.f};
            if (Po.slot >= 0) h = ld4(T.slot + Po.slot + rr * np + u0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float gg = acc[t][j][r];
              if (pen) gg += pen_grad(l1, l2, h[r], T.inv_rows);
              v[r] = (rlive && u0 + r < N) ? act_grad(act, h[r], gg) : 0.0f;
            }
          }
          if (is_dz) dbs[j] += v;   // the lane's rows in ascending order
          *reinterpret_cast<bf16x4*>(T.s_act + rr * S + u0) = pack4(v);
        }
      }
    }
    if (last && !head) {   // uniform: the row's squared error and argmaxes over the wave's units
      se += xor16(se, lane);
      se += xor32(se, lane);
      take_max(by, iy, xor16(by, lane), xor16i(iy, lane));
      take_max(bt, it, xor16(bt, lane), xor16i(it, lane));
      take_max(by, iy, xor32(by, lane), xor32i(iy, lane));
      take_max(bt, it, xor32(bt, lane), xor32i(it, lane));
      if (g == 0) {
        float* p = T.s_part + (wid * R + rr) * DFWW_PART_WORDS;
        p[0] = se;
        p[1] = by;
        p[2] = __int_as_float(iy);
        p[3] = bt;
        p[4] = __int_as_float(it);
      }
    }
  }
  if ((nub & 1) && wid == (nub & (NWV - 1))) {   // the second half of the next contraction's last k-step
#pragma unroll
    for (int t = 0; t < RT; ++t) *reinterpret_cast<bf16x4*>(T.s_act + (16 * t + c) * S + 16 * nub + 4 * g) = bf16x4{0, 0, 0, 0};
  }
  if (is_dz && a.L[lo].has_bias && wid < nub) {   // column sums of the unrounded dz: 16 row lanes, fixed order
#pragma unroll
    for (int j = 0; j < UBN; ++j) {
      const int ub = wid + NWV * j;
      if (ub < nub) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = dbs[j][r];
          s += __shfl_xor(s, 1, 64);
          s += __shfl_xor(s, 2, 64);
          s += __shfl_xor(s, 4, 64);
          s += __shfl_xor(s, 8, 64);
          if (c == 0) T.s_db[Po.db + 16 * ub + 4 * g + r] += s;
        }
      }
    }
  }
  if (pen && !bwd) lpen += (double)(l1 * s1 + l2 * s2);
  __syncthreads();
  if (head && tid < T.live) {   // the row's thread: cross-entropy and argmax match
    const DenseHeadRow hr = head_merge(T.s_part, R, tid);
    const int64_t pos = T.pos0 + tid;
    lsum += (double)head_loss(hr);
    lcnt += hr.arg == a.labels[a.order ? (int64_t)a.order[pos] : pos] ? 1.0 : 0.0;
  }
  if (last && !head && tid < T.live) {   // waves in order
    float se = 0.f, by = -INFINITY, bt = -INFINITY;
    int iy = INT_MAX, it = INT_MAX;
    for (int w = 0; w < NWV; ++w) {
      const float* p = T.s_part + (w * R + tid) * DFWW_PART_WORDS;
      se += p[0];
      take_max(by, iy, p[1], __float_as_int(p[2]));
      take_max(bt, it, p[3], __float_as_int(p[4]));
    }
    lsum += (double)se;
    lcnt += iy == it ? 1.0 : 0.0;
  }
  copy_out(a, T, is_dz ? Po.dz : a.P.L[l + 1].h, Po.dw, tid);
}

template <bool HEAD>
__device__ __forceinline__ void run_layer(const DenseBatchWArgs& a, const Tile& T, int l, bool bwd, int tid, double& lsum,
                                          double& lcnt, double& lpen) {
  const int nub = ((bwd ? a.L[l].in : a.L[l].units) + 15) >> 4;
  if (nub <= NWV) layer<1, HEAD>(a, T, l, bwd, tid, lsum, lcnt, lpen);
  else if (nub <= 2 * NWV) layer<2, HEAD>(a, T, l, bwd, tid, lsum, lcnt, lpen);
  else layer<4, HEAD>(a, T, l, bwd, tid, lsum, lcnt, lpen);
}

// HEAD: the instance for a.head == DBW_HEAD_SOFTMAX; the other one is untouched by the head
template <bool HEAD>
__global__ __launch_bounds__(NTHR) void dense_batchw_fb_kernel(const DenseBatchWArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double s_red[NTHR];
  const int tid = threadIdx.x, grp = (int)blockIdx.x, G = (int)gridDim.x;
  const int D = a.D, hw0 = a.P.L[0].hw >> 1, O = a.L[a.nl - 1].units;   // hw0: column pairs of a staged row
  Tile T;
  T.s_act = reinterpret_cast<uint16_t*>(smem);
  T.s_db = reinterpret_cast<float*>(smem + a.P.db_off);
  T.s_part = reinterpret_cast<float*>(smem + a.P.part_off);
  T.slot = a.slots + (int64_t)grp * a.P.slot_floats;
  T.inv_rows = 1.0f / (float)a.batch;
  T.inv_n = 1.0f / ((float)a.batch * (float)O);
  for (int i = tid; i < a.P.ndb; i += NTHR) T.s_db[i] = 0.0f;

  const int tiles = dense_batchw_tiles(a.batch);
  int tile = (int)((int64_t)tiles * grp / G);
  const int tile1 = (int)((int64_t)tiles * (grp + 1) / G);
  double lsum = 0.0, lcnt = 0.0, lpen = 0.0;   // squared error and matches of row tid; this thread's penalties
  for (; tile < tile1; ++tile) {
    T.wrow0 = (int64_t)tile * R;
    T.pos0 = a.row0 + T.wrow0;
    T.live = a.batch - tile * R < R ? a.batch - tile * R : R;
    __syncthreads();   // the previous tile's last copy has read the LDS tile
    // ---- rows -> LDS: bf(x), zero past D and past the live rows
    for (int i = tid; i < R * hw0; i += NTHR) {
      const int r = i / hw0, col = 2 * (i - r * hw0);
      float v[2] = {0.f, 0.f};
      if (r < T.live) {
        const int64_t pos = T.pos0 + r, smp = a.order ? (int64_t)a.order[pos] : pos;
        const float* xr = a.x + smp * a.ldx;
#pragma unroll
        for (int e = 0; e < 2; ++e)
          if (col + e < D) v[e] = xr[col + e];
      }
      *reinterpret_cast<unsigned*>(T.s_act + r * a.P.stride + col) = pack2(v[0], v[1]);
    }
    __syncthreads();
    copy_out(a, T, a.P.L[0].h, a.P.L[0].hw, tid);
#pragma unroll 1
    for (int l = 0; l < a.nl; ++l) run_layer<HEAD>(a, T, l, false, tid, lsum, lcnt, lpen);
#pragma unroll 1
    for (int l = a.nl - 1; l >= 1; --l) run_layer<HEAD>(a, T, l, true, tid, lsum, lcnt, lpen);
  }
  __syncthreads();
  for (int i = tid; i < a.P.ndb; i += NTHR) a.dbp[(int64_t)grp * a.P.ndb + i] = T.s_db[i];
  // the workgroup's pair: rows' squared errors and matches, then the threads' penalties, in index order
  double part[3] = {lsum, lcnt, lpen}, tot[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s_red[tid] = part[k];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < (k == 2 ? NTHR : R); ++i) tot[k] += s_red[i];
    __syncthreads();
  }
  if (tid == 0) {
    const double rows = (double)a.batch;   // a head's loss is a mean over rows, the squared error's over rows and units
    a.wpairs[2 * grp] = (float)(tot[0] / (HEAD ? rows : rows * (double)O) + tot[2] / rows);
    a.wpairs[2 * grp + 1] = (float)tot[1];
  }
}

// ---------------------------------------------------------------- 3. weight gradients
// MFMA operand read transposed from a staged [32 rows][128] bf16 slice: lane (c, g) gets column col0 + c
// of rows 8 g .. 8 g + 7 (two ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group addresses row q,
// columns 4 p .. 4 p + 3 of a 4 x 16 block).  All 64 lanes must execute it.
__device__ __forceinline__ s16x8 tr_frag(unsigned char* base, int col0, int c, int g) {
  unsigned char* p = base + (8 * g + (c >> 2)) * WG_STRIDE + 2 * (col0 + 4 * (c & 3));
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)p);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p + 4 * WG_STRIDE));
  return cat8(lo, hi);
}

__device__ __forceinline__ void bias_item(const DenseBatchWArgs& a, int s, float* slab, int tid) {
  const int g0 = (int)((int64_t)s * a.G / a.S), g1 = (int)((int64_t)(s + 1) * a.G / a.S);
  for (int l = 0; l < a.nl; ++l) {
    if (!a.L[l].has_bias) continue;
    for (int u = tid; u < a.L[l].units; u += DBW_WTHREADS) {
      float sum = 0.0f;
      for (int g = g0; g < g1; ++g) sum += a.dbp[(int64_t)g * a.P.ndb + a.P.L[l].db + u];
      slab[a.L[l].b_off + u] = sum;
    }
  }
  if (tid == 0) {
    float loss = 0.0f, ok = 0.0f;
    for (int g = g0; g < g1; ++g) {
      loss += a.wpairs[2 * g];
      ok += a.wpairs[2 * g + 1];
    }
    a.pairs[2 * s] = loss;
    a.pairs[2 * s + 1] = ok;
  }
}

__global__ __launch_bounds__(DBW_WTHREADS) void dense_batchw_wgrad_kernel(const DenseBatchWArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sA[DBW_KROWS * WG_STRIDE];
  __shared__ __attribute__((aligned(16))) unsigned char sB[DBW_KROWS * WG_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wid = uniform(tid >> 6), c = lane & 15, g = lane >> 4;
  const int32_t* item = a.items + 4 * (int64_t)blockIdx.x;
  const int l = uniform(item[0]), i0 = uniform(item[1]), j0 = uniform(item[2]), s = uniform(item[3]);
  float* slab = a.slab + (int64_t)s * a.nflat;
  if (l < 0) {
    bias_item(a, s, slab, tid);
    return;
  }
  const int in = a.L[l].in, out = a.L[l].units, hw = a.P.L[l].hw, dw = a.P.L[l].dw;
  const uint16_t* A = a.ws + a.P.L[l].h;
  const uint16_t* B = a.ws + a.P.L[l].dz;
  const int ksteps = a.P.rows / DBW_KROWS;
  const int ks0 = (int)((int64_t)s * ksteps / a.S), ks1 = (int)((int64_t)(s + 1) * ksteps / a.S);
  const int wi = 64 * (wid >> 1), wj = 64 * (wid & 1);   // this wave's 64 x 64 inside the tile
  int ni = (dfww_pad16(in) - i0 - wi) >> 4, nj = (dfww_pad16(out) - j0 - wj) >> 4;
  ni = ni < 0 ? 0 : ni > 4 ? 4 : ni;
  nj = nj < 0 ? 0 : nj > 4 ? 4 : nj;

  f32x4 acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};

  // a k-step's slices: 32 rows x 16 runs of 16 bytes per operand, two runs a thread
  const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  s16x8 ra[2], rb[2];
  auto load = [&](int ks) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + DBW_WTHREADS * u, r = e >> 4, q = e & 15;
      const int64_t row = (int64_t)ks * DBW_KROWS + r;
      ra[u] = i0 + 8 * q < hw ? *reinterpret_cast<const s16x8*>(A + row * hw + i0 + 8 * q) : zero;
      rb[u] = j0 + 8 * q < dw ? *reinterpret_cast<const s16x8*>(B + row * dw + j0 + 8 * q) : zero;
    }
  };
  if (ks0 < ks1) load(ks0);
  for (int ks = ks0; ks < ks1; ++ks) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + DBW_WTHREADS * u, r = e >> 4, q = e & 15;
      *reinterpret_cast<s16x8*>(sA + r * WG_STRIDE + 16 * q) = ra[u];
      *reinterpret_cast<s16x8*>(sB + r * WG_STRIDE + 16 * q) = rb[u];
    }
    __syncthreads();
    if (ks + 1 < ks1) load(ks + 1);
    if (ni > 0 && nj > 0) {
      s16x8 fb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) fb[q] = tr_frag(sB, wj + 16 * q, c, g);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p < ni) {
          const s16x8 fa = tr_frag(sA, wi + 16 * p, c, g);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < nj) acc[p][q] = mfma_k32(fa, fb[q], acc[p][q]);
        }
      }
    }
    __syncthreads();
  }
  // C layout: lane (c, g) holds inputs 4 g .. 4 g + 3 of unit column c of each 16 x 16 block
  float* Wg = slab + a.L[l].w_off;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + wj + 16 * q + c;
      if (p < ni && q < nj && j < out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = i0 + wi + 16 * p + 4 * g + e;
          if (i < in) Wg[i * out + j] = acc[p][q][e];
        }
      }
    }
}

DenseFwdLdsMark<2> lds_mark;   // of dense_batchw_fb_kernel<no head / head>

}  // namespace

// Reached through the bindings, which have run dense_batchw_check; the tests here are for a caller that
// comes another way.
hipError_t dense_batchw_launch(const DenseBatchWArgs& a, hipStream_t stream) {
  if (a.nl < 1 || a.nl > DBW_MAXLAYERS) return hipErrorInvalidValue;
  const bool head = a.head != DBW_HEAD_NONE;
  if ((a.labels != nullptr) != head || (head && a.y)) return hipErrorInvalidValue;
  if (!dense_batchw_check(a.L, a.nl, a.D, a.batch, a.nflat, a.y != nullptr || head, a.head).empty()) return hipErrorInvalidValue;
  const DenseBatchWPlan P = dense_batchw_plan(a.L, a.nl, a.batch);
  if (P.ws_words != a.P.ws_words || P.img_words != a.P.img_words || P.lds_bytes != a.P.lds_bytes || P.rows != a.P.rows ||
      a.row0 < 0 || a.row0 + a.batch > a.n || a.G < 1 || a.G > dense_batchw_tiles(a.batch) || a.S < 1 ||
      a.S > P.rows / DBW_KROWS || a.S > DBW_MAXSPLIT || a.nitems != a.S * (P.wtiles + 1) || (a.nflat & 3) ||
      (reinterpret_cast<uintptr_t>(a.flat) & 15) || (reinterpret_cast<uintptr_t>(a.image) & 15) ||
      (reinterpret_cast<uintptr_t>(a.ws) & 15) || (reinterpret_cast<uintptr_t>(a.slots) & 15) || !a.items || !a.slab ||
      !a.pairs || !a.dbp || !a.wpairs)
    return hipErrorInvalidValue;
  void (*const fb)(const DenseBatchWArgs) = head ? dense_batchw_fb_kernel<true> : dense_batchw_fb_kernel<false>;
  const hipError_t e = lds_mark.ensure(reinterpret_cast<const void*>(fb), head ? 1 : 0, P.lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dense_batchw_image_kernel, dim3((P.img_words / 8 + IMG_NT - 1) / IMG_NT), dim3(IMG_NT), 0, stream, a);
  hipLaunchKernelGGL(fb, dim3(a.G), dim3(NTHR), (size_t)P.lds_bytes, stream, a);
  hipLaunchKernelGGL(dense_batchw_wgrad_kernel, dim3(a.nitems), dim3(DBW_WTHREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace sml
