// The large-batch Dense train step's limits and its split of a batch over workgroups
// (kernels/dense_batch.hip).  Plain C++17 with no HIP header, like sml_dense_mb_plan.h, whose layer
// table, bf16 LDS plan and stack limits the step takes over unchanged; ops/dense_batch.py mirrors the
// check in Python.
#pragma once

#include <cstdint>
#include <string>

#include "sml_dense_mb_plan.h"

namespace sml {

enum : int {
  DBT_MAXBATCH = 1 << 24   // a chosen bound: row and chunk indices of a step stay in int32 (and exact in fp32)
};

// 32-row chunks of a step of `rows` rows
constexpr int dense_batch_chunks(int rows) { return (rows + DMB_CHUNK - 1) / DMB_CHUNK; }

// workgroups of a step: `groups` (<= 0: one per CU), never more than the step has chunks
constexpr int dense_batch_groups(int rows, int groups, int cus) {
  const int want = groups > 0 ? groups : cus, n = dense_batch_chunks(rows);
  return want < n ? (want < 1 ? 1 : want) : n;
}

// the chunks [first, second) of workgroup g of G: a static split, so a result's bits depend on the
// batch and G alone
constexpr int dense_batch_first_chunk(int g, int G, int chunks) { return (int)((int64_t)g * chunks / G); }

// empty if the step can train the stack (dense_mb_check's arguments), else the limit it exceeds:
// the bf16 persistent trainer's limits on the stack, 1 .. DBT_MAXBATCH on the batch
inline std::string dense_batch_check(const DenseMBLayer* L, int nl, int D, int64_t batch, int64_t nflat, bool own_targets) {
  const std::string why = dense_mb_check(L, nl, D, 1, nflat, own_targets, DMB_BF16);
  if (!why.empty()) return why;
  if (batch < 1 || batch > DBT_MAXBATCH)
    return "batch " + std::to_string(batch) + " is outside 1.." + std::to_string((int)DBT_MAXBATCH) + " (MAX_BATCH)";
  return "";
}

}  // namespace sml
