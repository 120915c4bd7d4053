// Key -> lane sharding of the multi-lane forecaster (runtime/serve.cpp), host only and pure.
//
// Key k is served by lane k % lanes.  serve_lane_partition() groups a batch's events by lane,
// keeping batch order within each lane (a counting sort, stable): event j of lane l in this
// batch is batch row order[start[l] + j].  The same table read the other way gathers results
// back into batch order: the result of lane l's j-th event belongs to row order[start[l] + j],
// so order is the permutation and its inverse restores the batch.
#pragma once
#include <cstdint>
#include <vector>

namespace sml {

inline int serve_lane_of(uint32_t key, int lanes) { return (int)(key % (uint32_t)lanes); }

struct ServeLanePartition {
  std::vector<int> order;   // [k] batch rows grouped by lane, batch order within a lane
  std::vector<int> start;   // [lanes + 1] lane l owns order[start[l] .. start[l + 1])
};

inline ServeLanePartition serve_lane_partition(const uint32_t* keys, int k, int lanes) {
  ServeLanePartition p;
  p.order.resize(k > 0 ? (size_t)k : 0);
  p.start.assign((size_t)lanes + 1, 0);
  for (int i = 0; i < k; ++i) ++p.start[(size_t)serve_lane_of(keys[i], lanes) + 1];
  for (int l = 0; l < lanes; ++l) p.start[(size_t)l + 1] += p.start[(size_t)l];
  std::vector<int> at(p.start.begin(), p.start.end() - 1);
  for (int i = 0; i < k; ++i) p.order[(size_t)at[(size_t)serve_lane_of(keys[i], lanes)]++] = i;
  return p;
}

}  // namespace sml
