// prt_blas_cost_gpu.h -- launch of the device SAH measure (prt_blas_cost.hip; the definition: prt_blas_cost.h).
#pragma once
#include <hip/hip_runtime.h>

#include "prt_scene.h"

namespace prt {

// nodes per block of the node pass = its block size: one partial sum per block
constexpr uint32_t kCostBlock = 256;
inline uint32_t blas_cost_blocks(uint64_t n_nodes) { return (uint32_t)((n_nodes + kCostBlock - 1) / kCostBlock); }

// The cost of the tree nodes[0 .. n_nodes) (nodes[0] = its root; n_nodes >= 1) into *cost (device memory, 8 bytes),
// on stream s.  partials: room for blas_cost_blocks(n_nodes) + 1 doubles (the blocks' sums, then the root area).
// No atomics, one fixed order of additions: the same tree gives the same bits.
hipError_t launch_blas_cost(hipStream_t s, const Node8* nodes, uint32_t n_nodes, double* partials, double* cost);

}  // namespace prt
