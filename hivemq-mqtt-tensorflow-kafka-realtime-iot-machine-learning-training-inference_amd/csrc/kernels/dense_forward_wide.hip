// Fused bulk forward of a WIDE Dense stack: 1..8 Dense layers, every width (input included) up to 512,
// over n rows in ONE launch, on v_mfma_f32_16x16x32_bf16.  It writes what dense_forward.hip writes
// (reconstructions, per-row scores and flags, or per-workgroup loss / accuracy sums) for
// nn.Model.predict / score / detect / evaluate(engine="wide") through ops/dense_forward_wide.py.
// Limits, image layout and LDS plan: sml_dense_fwdw_plan.h.
//
// ARITHMETIC.  The rounding points of the bf16 trainers' forward: xn = x * scale + shift in fp32;
// z_l = b_l + bf16(h_{l-1}) . bf16(W_l) with fp32 accumulation; h_l = act_fwd(z_l) in fp32; only the
// copy of h_l that feeds the next contraction is rounded to bf16; the last layer's h leaves unrounded;
// score = mean((y - xn)^2) against the unrounded fp32 xn.
//
// WORK SPLIT.  A workgroup of 8 waves owns a tile of R = 16 RT rows (RT = 4 or 8).  The tile's
// activations live in LDS as bf16, [R][stride], stride = the widest padded k + 8 words: a B fragment
// (lane (c, g): row c, k = 32 kb + 8 g .. + 7) is one ds_read_b128, and 16 rows of one g fall on
// distinct banks.  Every layer is computed transposed, Y^T = W^T . X^T: wave w owns the unit blocks
// ub = w, w + 8, w + 16, w + 24 (up to 4 x 16 units) for ALL R rows, so its accumulators
// acc[RT][4] (64 or 128 VGPRs) hold its whole slice of the layer.  Per k-step it loads its (up to) four
// A fragments straight from the image in global memory (L2; 16 bytes a lane, once per workgroup and
// tile), reads the RT B fragments from LDS and issues RT x 4 MFMAs; the next k-step's A fragments are
// in flight under them.  Because a wave finishes all of k before it writes, the layer's results go
// back IN PLACE: barrier (every wave has read the layer's input), bias came in as the accumulator's
// initial value, act_fwd, round, 8-byte LDS stores at [row c][16 ub + 4 g .. + 3], barrier.  The result
// layout of one layer (units on registers, rows on lanes) is the store layout of the next layer's k.
// No activation goes to HBM and nothing spills.
//
// PADDING.  k is padded to 32 and units to 16 with zero weights.  A padded unit is act(0), finite,
// and meets zero weights only; when a layer has an odd number of unit blocks the wave that would own
// the next block writes zeros there, so the next layer's last k-step reads no stale LDS.
//
// ROWS.  A persistent grid with static contiguous tile spans per workgroup.  A tile's rows are read
// element-coalesced, normalised, rounded and stored to LDS two columns a thread; rows past n are
// zero.  One workgroup runs per CU (153 VGPRs at RT = 4, 229 at RT = 8; no scratch); the host takes
// RT = 8 when the rows fill every CU with 128-row tiles, since it halves the weight traffic per row.
// The epilogue reads its target (xn again from the row, or the caller's y) at the lanes that hold
// the matching outputs: 16-byte runs that the staging pass left in L2.
//
// EPILOGUE.  A lane holds y[row c][unit 16 ub + 4 g + r] of its wave's blocks.  Reconstructions leave
// from the registers.  Squared error and argmax: per lane in unit order, then + lane ^ 16, + lane ^ 32
// (argmax merged by (value, index): the first maximal index), then one partial per wave and row in LDS
// (over the activation tile, which is free by then), folded in wave order by the row's thread.  sums:
// every thread adds its rows in doubles, thread 0 folds the workgroup's in index order; no atomics.
//
// SOFTMAX HEAD (a.head = 1: the kernel's HEAD instances, one per tile size; sml_dense_head.h).  The last
// layer is linear in the table; its logits go through the train step's online-softmax merge: per wave and
// row (max, argmax, sum exp(z - max), the label's logit) into the partials, one barrier, then every lane
// merges the eight partials of its rows in wave order.  rec takes the probabilities exp(z - M) / S from
// the accumulators, sums the per-workgroup [sum of log S + M - z_label, rows whose argmax is the label]
// against a.labels (int32 [n]).  Scores and flags are refused with a head.  157 / 233 VGPRs at RT = 4 / 8
// (153 / 229 without a head, as before), no scratch.
//
// A ROW'S BITS depend on the row and the weights only: the k order of a unit is kb ascending whatever
// RT, the grid or the row's place in the tile, and the fold over lanes and waves is fixed.
#include <climits>

#include "sml_common.h"
#include "sml_dense_fwd_launch.h"
#include "sml_dense_head.h"
#include "sml_ops.h"

namespace sml {
namespace {

static_assert(ACT_LINEAR == 0 && DFW_ACT_LAST == ACT_SIGMOID, "the check's activation range is Act's");
constexpr int NWV = DFWW_WAVES, NTHR = 64 * DFWW_WAVES;

__device__ __forceinline__ f32x4 mfma_k32(s16x8 a, s16x8 b, f32x4 c) {
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// One layer over the tile, for a layer whose waves own up to UBN unit blocks (ub = wid + 8 j).  The
// MFMA loop has no branch: a block past nub runs on block nub - 1's fragments (the loads stay inside
// the image) and is never written.  The last layer ends in the epilogue.
template <int RT, int UBN, bool HEAD>
__device__ __forceinline__ void run_layer(const DenseFwdWArgs& a, int l, uint16_t* s_act, int S, int64_t row0, int live,
                                          int tid, double& lsum, double& lcnt) {
  constexpr int R = 16 * RT;
  // everything below that depends on the lane alone is invariant in the tile and layer loops; kept
  // there it would cost more registers than the accumulators, so the lane comes from behind an empty asm
  const int lane = opaque(tid) & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
  const int K = a.L[l].in, N = a.L[l].out, act = a.L[l].act;
  const int nkb = (K + 31) >> 5, nub = (N + 15) >> 4;
  f32x4 acc[RT][UBN];
  if (wid < nub) {
    const s16x8* W[UBN];
    s16x8 wc[UBN], wn[UBN];
#pragma unroll
    for (int j = 0; j < UBN; ++j) {
      const int ub = wid + NWV * j < nub ? wid + NWV * j : nub - 1;
      W[j] = reinterpret_cast<const s16x8*>(a.image + a.L[l].w_off) + ub * 64 + lane;
      const f32x4 b = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.image + a.L[l].b_off) + 16 * ub + 4 * g);
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
  __syncthreads();   // every wave has read the layer's input: the tile is free

  if (l < a.nl - 1) {
    if (wid < nub) {
#pragma unroll
      for (int j = 0; j < UBN; ++j) {
        const int ub = wid + NWV * j;
        if (ub < nub) {
#pragma unroll
          for (int t = 0; t < RT; ++t) {
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = act_fwd(act, acc[t][j][r]);
            *reinterpret_cast<bf16x4*>(s_act + (16 * t + c) * S + 16 * ub + 4 * g) = pack4(h);
          }
        }
      }
    }
    if ((nub & 1) && wid == (nub & (NWV - 1))) {   // the second half of the next layer's last k-step
#pragma unroll
      for (int t = 0; t < RT; ++t) *reinterpret_cast<bf16x4*>(s_act + (16 * t + c) * S + 16 * nub + 4 * g) = bf16x4{0, 0, 0, 0};
    }
    __syncthreads();
    return;
  }

  // ---- epilogue: the lane holds y[row c][unit 16 ub + 4 g + r] of its wave's blocks
  const int out = N;
  const bool norm = a.scale != nullptr;
  const bool want_target = a.score != nullptr || a.sums != nullptr;
  float* const s_part = reinterpret_cast<float*>(s_act);
  if constexpr (HEAD) {   // softmax over the logits; rec takes the probabilities, sums the cross-entropy
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int64_t row = row0 + 16 * t + c;
      const int lab = a.sums && row < a.n ? a.labels[row] : -1;
      head_wave_partial<UBN>(acc[t], wid, nub, out, lab, lane, s_part + (wid * R + 16 * t + c) * DFWW_PART_WORDS);
    }
    __syncthreads();
    if (a.rec && wid < nub) {
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int64_t row = row0 + 16 * t + c;
        const DenseHeadRow hr = head_merge(s_part, R, 16 * t + c);
        float* const rr = a.rec + row * out;
#pragma unroll
        for (int j = 0; j < UBN; ++j) {
          const int ub = wid + NWV * j;
          if (ub < nub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int u = 16 * ub + 4 * g + r;
              if (u < out && row < a.n) rr[u] = head_prob(acc[t][j][r], hr);
            }
          }
        }
      }
    }
    if (a.sums && tid < live) {
      const DenseHeadRow hr = head_merge(s_part, R, tid);
      lsum += (double)head_loss(hr);
      lcnt += hr.arg == a.labels[row0 + tid] ? 1.0 : 0.0;
    }
    __syncthreads();   // before the next tile's rows overwrite the partials
    return;
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t row = row0 + 16 * t + c;
    const bool rlive = row < a.n;
    const float* const xr = a.x + row * a.ldx;
    const float* const yr = a.y + row * a.ldy;
    float* const rr = a.rec + row * out;
    float se = 0.f, by = -INFINITY, bt = -INFINITY;
    int iy = INT_MAX, it = INT_MAX;
    if (wid < nub) {
#pragma unroll
      for (int j = 0; j < UBN; ++j) {
        const int ub = wid + NWV * j;
        if (ub < nub) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int u = 16 * ub + 4 * g + r;
            const float yv = act_fwd(act, acc[t][j][r]);
            if (u < out && rlive) {
              if (a.rec) rr[u] = yv;
              if (want_target) {
                float tg;
                if (a.y) {
                  tg = yr[u];
                } else {
                  tg = xr[u];
                  if (norm) tg = fmaf(tg, a.scale[u], a.shift[u]);
                }
                const float d = yv - tg;
                se = fmaf(d, d, se);
                if (yv > by) { by = yv; iy = u; }
                if (tg > bt) { bt = tg; it = u; }
              }
            }
          }
        }
      }
    }
    if (want_target) {   // uniform
      se += xor16(se, lane);
      se += xor32(se, lane);
      take_max(by, iy, xor16(by, lane), xor16i(iy, lane));
      take_max(bt, it, xor16(bt, lane), xor16i(it, lane));
      take_max(by, iy, xor32(by, lane), xor32i(iy, lane));
      take_max(bt, it, xor32(bt, lane), xor32i(it, lane));
      if (g == 0) {
        float* p = s_part + (wid * R + 16 * t + c) * DFWW_PART_WORDS;
        p[0] = se;
        p[1] = by;
        p[2] = __int_as_float(iy);
        p[3] = bt;
        p[4] = __int_as_float(it);
      }
    }
  }
  if (want_target) {
    __syncthreads();
    if (tid < live) {
      float se = 0.f, by = -INFINITY, bt = -INFINITY;
      int iy = INT_MAX, it = INT_MAX;
      for (int w = 0; w < NWV; ++w) {
        const float* p = s_part + (w * R + tid) * DFWW_PART_WORDS;
        se += p[0];
        take_max(by, iy, p[1], __float_as_int(p[2]));
        take_max(bt, it, p[3], __float_as_int(p[4]));
      }
      const float score = se / (float)out;
      if (a.score) {
        a.score[row0 + tid] = score;
        if (a.flag) a.flag[row0 + tid] = score > a.threshold ? 1 : 0;
      }
      lsum += (double)score;
      lcnt += iy == it ? 1.0 : 0.0;
    }
    __syncthreads();   // before the next tile's rows overwrite the partials
  }
}

// HEAD: the instance whose epilogue is the softmax head; the other one is untouched by it
template <int RT, bool HEAD>
__global__ __launch_bounds__(NTHR) void dense_fwdw_kernel(DenseFwdWArgs a, int S) {
  constexpr int R = 16 * RT;
  extern __shared__ __attribute__((aligned(16))) uint16_t s_act[];   // [R][S] bf16; the epilogue's partials
  __shared__ double s_red[2][R];
  const int tid = threadIdx.x;
  const int D = a.D, hw0 = dfww_pad32(D) >> 1;   // column pairs of a staged row
  const bool norm = a.scale != nullptr;

  const int64_t tiles = (a.n + R - 1) / R;
  int64_t tile = tiles * blockIdx.x / gridDim.x;
  const int64_t tile1 = tiles * (blockIdx.x + 1) / gridDim.x;
  double lsum = 0.0, lcnt = 0.0;   // sums: thread tid < R, its rows

  for (; tile < tile1; ++tile) {
    const int64_t row0 = tile * R;
    const int live = (int)(a.n - row0 < R ? a.n - row0 : R);

    // ---- rows -> LDS: xn rounded to bf16, zero past D and past the live rows
    for (int i = tid; i < R * hw0; i += NTHR) {
      const int r = i / hw0, col = 2 * (i - r * hw0);
      float v[2] = {0.f, 0.f};
      if (r < live) {
        const float* xr = a.x + (row0 + r) * a.ldx;
#pragma unroll
        for (int e = 0; e < 2; ++e)
          if (col + e < D) v[e] = norm ? fmaf(xr[col + e], a.scale[col + e], a.shift[col + e]) : xr[col + e];
      }
      *reinterpret_cast<unsigned*>(s_act + r * S + col) = pack2(v[0], v[1]);
    }
    __syncthreads();

#pragma unroll 1
    for (int l = 0; l < a.nl; ++l) {
      const int nub = (a.L[l].out + 15) >> 4;
      if (nub <= NWV) run_layer<RT, 1, HEAD>(a, l, s_act, S, row0, live, tid, lsum, lcnt);
      else if (nub <= 2 * NWV) run_layer<RT, 2, HEAD>(a, l, s_act, S, row0, live, tid, lsum, lcnt);
      else run_layer<RT, 4, HEAD>(a, l, s_act, S, row0, live, tid, lsum, lcnt);
    }
  }
  if (a.sums) {
    if (tid < R) {
      s_red[0][tid] = lsum;
      s_red[1][tid] = lcnt;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0, k = 0.0;
      for (int i = 0; i < R; ++i) {
        s += s_red[0][i];
        k += s_red[1][i];
      }
      a.sums[2 * blockIdx.x] = s;
      a.sums[2 * blockIdx.x + 1] = k;
    }
  }
}

std::string args_check(const DenseFwdWArgs& a) {
  if (a.nl < 1 || a.nl > DFW_MAXLAYERS) return dense_fwdw_check(a.L, a.nl, a.D, -1, false);
  std::string why = dense_fwdw_check(a.L, a.nl, a.D, a.img_words, a.score != nullptr || (a.sums && !a.y && !a.head), a.head);
  if (why.empty()) why = dense_fwd_args_why(a, a.image, a.sums);
  if (!why.empty()) return why;
  if (a.head ? (a.y || (a.sums != nullptr) != (a.labels != nullptr)) : a.labels != nullptr)
    return "labels come with a softmax head's sums, and with nothing else";
  if (a.tile != 0 && a.tile != DFWW_ROWS_SMALL && a.tile != DFWW_ROWS_LARGE) return "a tile has 64 or 128 rows";
  return "";
}

DenseFwdLdsMark<4> lds_mark;   // of dense_fwdw_kernel<4 / 8, no head / head>

}  // namespace

int dense_fwdw_grid(const DenseFwdLayer* L, int nl, int64_t n, int max_blocks, int tile) {
  const int cus = dense_fwd_cu_count();
  const DenseFwdWPlan P = dense_fwdw_plan(L, nl, dense_fwdw_rows(n, cus, tile));
  const int64_t tiles = (n + P.rows - 1) / P.rows;
  const int64_t cap = max_blocks > 0 ? max_blocks : cus;
  return (int)(tiles < cap ? tiles : cap);
}

hipError_t dense_fwdw_launch(const DenseFwdWArgs& a, hipStream_t stream) {
  if (!args_check(a).empty()) return hipErrorInvalidValue;
  const DenseFwdWPlan P = dense_fwdw_plan(a.L, a.nl, dense_fwdw_rows(a.n, dense_fwd_cu_count(), a.tile));
  const int grid = dense_fwdw_grid(a.L, a.nl, a.n, a.max_blocks, a.tile);
  const bool large = P.rows == DFWW_ROWS_LARGE, head = a.head != 0;
  void (*const fn)(DenseFwdWArgs, int) = large ? (head ? dense_fwdw_kernel<8, true> : dense_fwdw_kernel<8, false>)
                                               : (head ? dense_fwdw_kernel<4, true> : dense_fwdw_kernel<4, false>);
  const hipError_t e = lds_mark.ensure(reinterpret_cast<const void*>(fn), (large ? 1 : 0) + (head ? 2 : 0), P.lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(NTHR), (size_t)P.lds_bytes, stream, a, P.stride);
  return hipGetLastError();
}

}  // namespace sml
