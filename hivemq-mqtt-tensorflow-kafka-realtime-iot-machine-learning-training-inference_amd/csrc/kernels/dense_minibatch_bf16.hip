// Persistent small-batch trainer for Dense stacks of any depth with every contraction on
// v_mfma_f32_16x16x32_bf16 (sibling of dense_minibatch.hip: same launch shape, table, chunks,
// outputs and Adam; opt-in through DenseMBArgs::precision).
//
// ONE workgroup of DMB_NT threads (8 waves) runs nsteps sequential Keras steps in one launch.
// Rounding points (bf = round to nearest even bf16; everything else fp32):
//   forward   z_l = b_l + sum_k bf(h_{l-1}[r,k]) bf(W_l[k,j]),  h_l = act(z_l) in fp32, h_0 = x;
//             the fp32 h_l feeds the loss, the penalties, the accuracy and the activation derivative
//   backward  g_{l-1}[r,i] = sum_j bf(dz_l[r,j]) bf(W_l[i,j]),  dz_{l-1} = act'(h_{l-1}) (g_{l-1} + penalty) in fp32
//   weights   dW_l[i,j] = sum_r bf(h_{l-1}[r,i]) bf(dz_l[r,j]): K is the chunk's 32 rows, one MFMA per
//             16x16 tile per chunk, accumulated in fp32 over the chunks of a step
//   bias      db_l[j] = the fp32 column sum of the UNROUNDED dz_l, rows ascending (db_bf16 = False in
//             the test oracle)
//   Adam      sml_adam.h on fp32 masters; bf(W) is re-derived from the master after every update
//
// Memory plan (DenseMBPlanBF16, a pure function of the layer table; widths zero-padded to 16):
//   * wave w owns the 16x16 kernel tiles w, w + 8, ... (8 at most) in the MFMA C layout (lane (c, g):
//     kernel rows i0 + 4g .. + 3, column j0 + c) and keeps their fp32 master, gradient and both Adam
//     moments in registers from launch to exit: 128 VGPRs of state.
//   * LDS holds ONE bf16 weight image per layer, unit-major [up][ip + 8]: the forward pass reads its
//     rows (ds_read_b128), the backward pass reads it transposed (ds_read_b64_tr_b16).
//   * per 32-row chunk LDS holds the fp32 output of every layer (overwritten in place by its fp32
//     pre-activation gradient once that is known), a bf16 image of every layer input and a bf16
//     image of every pre-activation gradient, all [row][unit]: read by rows as the forward /
//     backward operand and transposed as the two weight-gradient operands.
//   * biases, their moments and gradients are fp32 in LDS, one thread per element.
//   * row strides carry 16 bytes of padding, so 16 rows' 16-byte pieces fall on different banks.
//   * the products are computed transposed (units or inputs on the C rows, batch rows on the lanes),
//     so a lane ends with four consecutive units of one row: one 16-byte and one 8-byte LDS store.
//   * padded units are forced to 0 on the way forward and padded units / rows to 0 gradient on the
//     way back, so padded parameters see exactly 0 gradient, stay 0 and are never written back
//     (sigmoid(0) = 0.5 cannot leak).  Every chunk computes all 32 rows: absent rows are zero inputs.
// Every transposed read is executed by all 64 lanes of every wave (wave-uniform control flow; out-of-
// range K pieces read a clamped address and are replaced by zeros).  The kernel synchronises with
// __syncthreads() only and every loop bound is known at launch.  dense_mb_bf16_fleet_kernel runs M models
// of one architecture side by side, workgroup b on model sched[b] (sml_dense_fleet.h): the same body
// (sml_dense_mb_bf16_body.h) on rebased arguments.  The limits, the plan and the check are in
// sml_dense_mb_plan.h; row staging, the loss phase's penalty sum and row merge, and the launch
// sequence, shared with the fp32 kernel, in sml_dense_mb_dev.h; a chunk's operand reads, layer
// products, loss phase and tile table, shared with the large-batch step (dense_batch.hip), in
// sml_dense_mb_bf16_dev.h.
#include "sml_common.h"
#include "sml_ops.h"

#include "sml_adam.h"
#include "sml_dense_fleet.h"
#include "sml_dense_mb_bf16_dev.h"

namespace sml {
namespace {

using namespace dmb16;

__global__ __launch_bounds__(NT) void dense_mb_bf16_kernel(const DenseMBArgs a, const DenseMBPlanBF16 P) {
  const DenseMBArgs& run = a;
#include "sml_dense_mb_bf16_body.h"
}

// Fleet entry: workgroup b trains model sched[b] of M models of one architecture (sml_dense_fleet.h);
// rebased once before the first load, then the single-model launch.  Nothing outside the workgroup
// is waited on.
__global__ __launch_bounds__(NT) void dense_mb_bf16_fleet_kernel(const DenseMBArgs a, const DenseMBPlanBF16 P,
                                                                 const DenseMBFleetModel* __restrict__ models,
                                                                 const int32_t* __restrict__ sched, const int64_t stride) {
  const DenseMBRun run = fleet_run(SML_DENSE_MB_SINGLE_RUN(a), a.ldx, a.ldy, models, sched, stride);
#include "sml_dense_mb_bf16_body.h"
}

}  // namespace

// Both are reached through dense_mb_launch / dense_mb_fleet_launch, which have run dense_mb_check.  Its
// MAX_PARAMS_BF16 limit already keeps ntiles within the DMB_TILES_BF16 the waves can own; the test
// here is for a caller that comes another way.
hipError_t dense_mb_launch_bf16(const DenseMBArgs& a, hipStream_t stream) {
  const DenseMBPlanBF16 P = dense_mb_plan_bf16(a.L, a.nl, a.D, a.y != nullptr);
  if (P.ntiles > DMB_TILES_BF16) return hipErrorInvalidValue;
  return launch(dense_mb_bf16_kernel, 1, (size_t)P.lds_bytes, stream, a, P);
}

hipError_t dense_mb_fleet_launch_bf16(const DenseMBArgs& a, const DenseMBFleetModel* models, const int32_t* sched, int M,
                                      int64_t stride, hipStream_t stream) {
  const DenseMBPlanBF16 P = dense_mb_plan_bf16(a.L, a.nl, a.D, a.y != nullptr);
  if (P.ntiles > DMB_TILES_BF16 || M < 1) return hipErrorInvalidValue;
  return launch(dense_mb_bf16_fleet_kernel, M, (size_t)P.lds_bytes, stream, a, P, models, sched, stride);
}

}  // namespace sml
