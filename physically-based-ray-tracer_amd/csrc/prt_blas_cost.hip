// prt_blas_cost.hip -- the device SAH measure of prt_blas_cost (definition and per-node code: prt_blas_cost.h).
// Its own translation unit: every earlier kernel keeps its machine code.
//
//   k_cost_nodes   one lane per node: its five 16-B words loaded, cost_node8 in f64; the block's lanes summed within
//                  each wave (six shuffle steps over 64 lanes), then the four waves' sums through 32 B of LDS in wave
//                  order; one f64 per block stored by its lane 0.  The lane of node 0 also stores the root area.
//   k_cost_total   one block: lane t sums its contiguous run of the partials in index order, the block's lanes are
//                  summed as above, lane 0 divides by the root area and stores the cost
// No atomics anywhere: the additions have one fixed order, so two calls on the same tree return the same bits.
// The block size: the node pass streams 80 B per lane against some 150 f64 operations, and the f64 vector rate keeps
// that ahead of the HBM stream; 256 lanes (four waves, 20 KiB in flight per block) is the size of the other per-node
// kernels, and the LDS is one f64 per wave.
#include "prt_blas_cost.h"
#include "prt_blas_cost_gpu.h"

namespace prt {

namespace {

constexpr int kCB = (int)kCostBlock;
constexpr int kCW = kCB / 64;  // waves per block

// the block's sum of v, valid in thread 0: within each wave by shuffles, then the waves in order
__device__ __forceinline__ double block_sum(double v, double* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63u) == 0u) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kCW; w++) t += sm[w];
  }
  return t;
}

__global__ void __launch_bounds__(kCB) k_cost_nodes(const Node8* __restrict__ nodes, uint32_t n,
                                                    double* __restrict__ partials, uint32_t nblocks) {
  __shared__ double sm[kCW];
  const uint32_t j = blockIdx.x * kCB + threadIdx.x;
  double v = 0.0;
  if (j < n) {
    const uint4* raw = reinterpret_cast<const uint4*>(nodes + j);
    union { Node8 nd; uint4 q[5]; } u;
#pragma unroll
    for (int k = 0; k < 5; k++) u.q[k] = raw[k];
    v = cost_node8(u.nd);
    if (j == 0) partials[nblocks] = cost_root_area(u.nd);
  }
  const double t = block_sum(v, sm);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ void __launch_bounds__(kCB) k_cost_total(const double* __restrict__ partials, uint32_t nblocks,
                                                    double* __restrict__ cost) {
  __shared__ double sm[kCW];
  const uint32_t run = (nblocks + kCB - 1) / kCB;
  const uint32_t b = threadIdx.x * run, e = b + run < nblocks ? b + run : nblocks;
  double v = 0.0;
  for (uint32_t i = b; i < e; i++) v += partials[i];
  const double t = block_sum(v, sm);
  if (threadIdx.x == 0) *cost = cost_finish(t, partials[nblocks]);
}

}  // namespace

hipError_t launch_blas_cost(hipStream_t s, const Node8* nodes, uint32_t n_nodes, double* partials, double* cost) {
  if (!n_nodes) return hipErrorInvalidValue;
  const uint32_t nb = blas_cost_blocks(n_nodes);
  hipLaunchKernelGGL(k_cost_nodes, dim3(nb), dim3(kCB), 0, s, nodes, n_nodes, partials, nb);
  hipLaunchKernelGGL(k_cost_total, dim3(1), dim3(kCB), 0, s, partials, nb, cost);
  return hipGetLastError();
}

}  // namespace prt
