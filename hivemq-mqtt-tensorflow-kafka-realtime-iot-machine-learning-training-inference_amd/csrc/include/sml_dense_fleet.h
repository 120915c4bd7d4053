// What differs between the members of a fleet of Dense stacks, for the kernel bodies of
// dense_minibatch.hip and dense_minibatch_bf16.hip (sml_dense_mb_body.h, sml_dense_mb_bf16_body.h) and
// for the row staging they share (stage_load of sml_dense_mb_dev.h).  A
// body reads what a fleet shares (layer table, plan, batch, Adam constants) from the launch's
// DenseMBArgs where they are, in the kernel arguments, and everything else from `run`: the arguments
// themselves in a single-model entry, a DenseMBRun in a fleet entry, rebased once per workgroup from
// the descriptor of model sched[blockIdx.x].  Every value of a run is the same for all lanes of the
// workgroup; the ones read from memory go through readfirstlane so that they live in SGPRs beside the
// kernel arguments (both kernels have no VGPR to spare).  A run holds no array, so it never needs
// memory of its own.
#pragma once

#include "sml_ops.h"

namespace sml {

struct DenseMBRun {
  float* flat;
  float* m;
  float* v;
  int64_t* iter;
  const float* x;
  const float* y;          // null: y = x
  const int32_t* order;    // null: rows in storage order
  int64_t n, row0;
  int nsteps;
  float lr;
  float* out;              // [nsteps, 2]
};

// the launch's arguments as a run (a macro: the kernel's argument struct is read where it is, never
// handed on by address)
#define SML_DENSE_MB_SINGLE_RUN(a) \
  ::sml::DenseMBRun { (a).flat, (a).m, (a).v, (a).iter, (a).x, (a).y, (a).order, (a).n, (a).row0, (a).nsteps, (a).lr, (a).out }

__device__ __forceinline__ int fleet_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t fleet_uniform(int64_t v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v & 0xffffffff));
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// all: the launch's shared arguments as a run (SML_DENSE_MB_SINGLE_RUN: whole arrays, nsteps = the out
// rows per model); models, sched, stride: see dense_mb_fleet_launch
__device__ __forceinline__ DenseMBRun fleet_run(const DenseMBRun a, int64_t ldx, int64_t ldy,
                                                const DenseMBFleetModel* __restrict__ models,
                                                const int32_t* __restrict__ sched, int64_t stride) {
  const int b = fleet_uniform(sched[blockIdx.x]);
  const DenseMBFleetModel* fm = models + b;
  const int64_t first = fleet_uniform(fm->first_row);
  const int64_t state = (int64_t)b * stride;
  DenseMBRun r;
  r.flat = a.flat + state;
  r.m = a.m + state;
  r.v = a.v + state;
  r.iter = a.iter + b;
  r.x = a.x + first * ldx;
  r.y = a.y != nullptr ? a.y + first * ldy : nullptr;
  r.order = a.order != nullptr ? a.order + first : nullptr;
  r.n = fleet_uniform(fm->rows);
  r.row0 = fleet_uniform(fm->row0);
  r.nsteps = fleet_uniform(fm->nsteps);
  r.lr = __builtin_bit_cast(float, fleet_uniform(__builtin_bit_cast(int, fm->lr)));
  r.out = a.out + (int64_t)b * a.nsteps * 2;
  return r;
}

}  // namespace sml
