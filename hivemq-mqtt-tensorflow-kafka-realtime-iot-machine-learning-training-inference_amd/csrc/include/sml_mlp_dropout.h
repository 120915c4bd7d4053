// The MNIST classifier's Dropout mask: a counter hash of (seed, step, row, column), shared by the layer
// kernels (kernels/mlp.hip) and the fused train step (kernels/mlp_step.hip), so both drop the same units.
#pragma once

#include <stdint.h>

namespace sml {

__device__ __forceinline__ uint32_t mix32(uint32_t h) {   // murmur3 finaliser
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// uniform [0, 1) with 24 bits, keyed by (seed, step, row, col)
__device__ __forceinline__ float dropout_u(uint32_t seed, uint32_t step, uint32_t row, uint32_t col) {
  uint32_t h = mix32(seed ^ 0x9e3779b9u);
  h = mix32(h ^ (step * 0x632be5abu));
  h = mix32(h ^ (row * 0x85157af5u));
  h = mix32(h ^ col);
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

}  // namespace sml
