// prt_tlas_build.hip -- the device side of prt_rebuild_instances around the device builder (bvh_gpu.hip
// gpu_build_blas8 with max_leaf = 1; the definitions and per-record code: prt_tlas_build.h).  Its own translation unit:
// every earlier kernel keeps its machine code.
//
//   k_tlas_prims    one lane per instance: the record's box as two 16-B loads (InstDev words 8 and 9: bmin | mesh,
//                   bmax | kind), the builder's fat triangle {lo, hi, centre} stored as three 16-B words
//   k_tlas_level    one block per tree level: the canonical order of the next level's nodes (see there)
//   k_tlas_finish   one lane per node of the builder's tree: 80 B of node loaded as five 16-B words from the build
//                   scratch, the prim word of the record behind each leaf slot, the node at its canonical position p
//                   with tri_base = 8p and its eight instance-slot words stored as seven 16-B words to the next copy
//                   of the instance state
// All move a few hundred KiB at 10,000 instances: launch-bound, one launch each and one per tree level.
#include "prt_tlas_build.h"

#include "prt_launch.h"

namespace prt {

namespace {

constexpr int kTB = 256;
static_assert(sizeof(InstDev) == 160 && offsetof(InstDev, bmin) == 128 && offsetof(InstDev, bmax) == 144,
              "k_tlas_prims reads an InstDev's box as its 16-byte words 8 and 9");

__global__ void __launch_bounds__(kTB) k_tlas_prims(const float4* __restrict__ inst, int32_t n, float4* __restrict__ fat) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  if (i >= (uint32_t)n) return;
  const float4 lo = inst[10 * (size_t)i + 8], hi = inst[10 * (size_t)i + 9];
  const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
  union { float f[12]; float4 q[3]; } u;
  tlas_fat_record(l, h, u.f);
  float4* o = fat + 3 * (size_t)i;
  o[0] = u.q[0];
  o[1] = u.q[1];
  o[2] = u.q[2];
}

// The builder hands out node positions by atomic counters: within a level the blocks of children come in the order the
// lanes reached the counter, which differs from run to run once a level takes more than one wavefront.  k_tlas_level
// gives level d + 1 its canonical order -- the children of the level-d nodes in the order of those nodes' canonical
// positions, each node's children in slot order, as the builder placed them -- so that the same tree always gives the
// same bytes.  One block per launch, one launch per level (an exclusive scan over the level in chunks of the block;
// levels are a few thousand nodes at most at 10,000 instances).  pos[j]: the canonical position of the builder's node
// j (pos[0] = 0; 0xFFFFFFFF until its parent's level has run); base[j]: the canonical child_base of node j; inv:
// scratch, the level's nodes by canonical position.  [lo, hi): the level, in both numberings.
__global__ void __launch_bounds__(kTB) k_tlas_level(const Node8* __restrict__ nodes, uint32_t n_nodes, uint32_t lo,
                                                    uint32_t hi, uint32_t* pos, uint32_t* base, uint32_t* inv) {
  __shared__ uint32_t sh[kTB];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x;
  for (uint32_t j = lo + t; j < hi; j += kTB) inv[j] = 0xFFFFFFFFu;
  if (t == 0) carry = 0u;
  __syncthreads();
  for (uint32_t j = lo + t; j < hi; j += kTB) {
    const uint32_t p = pos[j];
    if (p >= lo && p < hi) inv[p] = j;
  }
  __syncthreads();
  for (uint32_t p0 = lo; p0 < hi; p0 += kTB) {
    const uint32_t p = p0 + t;
    const uint32_t j = p < hi ? inv[p] : 0xFFFFFFFFu;
    const bool ok = j >= lo && j < hi;
    const uint32_t cnt = ok ? (uint32_t)__popc((uint32_t)nodes[j].imask) : 0u;
    sh[t] = cnt;
    __syncthreads();
    for (uint32_t o = 1; o < (uint32_t)kTB; o <<= 1) {  // inclusive scan of the chunk
      const uint32_t v = t >= o ? sh[t - o] : 0u;
      __syncthreads();
      sh[t] += v;
      __syncthreads();
    }
    const uint32_t first = hi + carry + sh[t] - cnt;  // the next level starts at hi
    if (ok) {
      base[j] = cnt ? first : 0u;
      const uint32_t old = nodes[j].child_base;
      for (uint32_t k = 0; k < cnt; k++)
        if (old + k < n_nodes && first + k < n_nodes) pos[old + k] = first + k;
    }
    __syncthreads();
    if (t == kTB - 1) carry += sh[t];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kTB) k_tlas_finish(const Node8* __restrict__ nodes, const TriMT* __restrict__ tris,
                                                     uint32_t n_tris, uint32_t n_nodes, uint32_t ninst,
                                                     const uint32_t* __restrict__ pos, const uint32_t* __restrict__ base,
                                                     Node8* dst, uint32_t* dst_slot) {
  const uint32_t j = blockIdx.x * kTB + threadIdx.x;
  if (j >= n_nodes) return;
  const uint32_t p = pos[j];
  if (p >= n_nodes) return;  // (a node no parent names: the builder emits none)
  const uint4* raw = reinterpret_cast<const uint4*>(nodes + j);
  union { Node8 nd; uint4 q[5]; } u;
  union { uint32_t id[8]; uint4 q[2]; } sl;
#pragma unroll
  for (int k = 0; k < 5; k++) u.q[k] = raw[k];
  tlas_finish_node8(u.nd, p, tris, n_tris, ninst, sl.id);
  u.nd.child_base = base[j];
  uint4* out = reinterpret_cast<uint4*>(dst + p);
  uint4* sout = reinterpret_cast<uint4*>(dst_slot + 8 * (size_t)p);
#pragma unroll
  for (int k = 0; k < 5; k++) out[k] = u.q[k];
  sout[0] = sl.q[0];
  sout[1] = sl.q[1];
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kTB - 1) / kTB); }

}  // namespace

hipError_t launch_tlas_prims(hipStream_t s, const InstDev* inst, int32_t n, float4* fat) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_tlas_prims, dim3(blocks_of((uint64_t)n)), dim3(kTB), 0, s, reinterpret_cast<const float4*>(inst), n,
                     fat);
  return hipGetLastError();
}

hipError_t launch_tlas_finish(hipStream_t s, const Node8* nodes, const TriMT* tris, uint32_t n_tris, uint32_t n_nodes,
                              uint32_t ninst, const uint32_t* level_ends, size_t levels, uint32_t* order_scratch,
                              Node8* dst, uint32_t* dst_slot) {
  if (!n_nodes) return hipSuccess;
  uint32_t *pos = order_scratch, *base = pos + n_nodes, *inv = base + n_nodes;
  hipError_t e = hipMemsetAsync(pos, 0xFF, 4 * (size_t)n_nodes, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(pos, 0, 4, s)) != hipSuccess) return e;  // the root keeps its place
  for (size_t d = 0; d < levels; d++) {
    const uint32_t lo = d ? level_ends[d - 1] : 0u, hi = level_ends[d];
    if (lo >= hi || hi > n_nodes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tlas_level, dim3(1), dim3(kTB), 0, s, nodes, n_nodes, lo, hi, pos, base, inv);
  }
  hipLaunchKernelGGL(k_tlas_finish, dim3(blocks_of(n_nodes)), dim3(kTB), 0, s, nodes, tris, n_tris, n_nodes, ninst, pos,
                     base, dst, dst_slot);
  return hipGetLastError();
}

}  // namespace prt
