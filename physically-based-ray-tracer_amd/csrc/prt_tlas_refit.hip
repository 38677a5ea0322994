// prt_tlas_refit.hip -- the device side of prt_update_instances (definition and per-node code: prt_tlas_refit.h).
// Its own translation unit: every earlier kernel keeps its machine code.
//
//   k_inst_src           one lane per instance: its 64-B transform as four 16-B loads, its mesh id and kind, the mesh's
//                        box (two 16-B loads from the per-mesh table); one InstSrc stored as six 16-B words.  k_refit
//                        (prt_render.hip) then writes the InstDev records, as after every prt_set_instances
//   k_tlas_refit_level   one lane per node of one tree level, deepest level first (separate launches: no lane ever
//                        waits for another block's progress).  80 B of node and 32 B of slot words loaded as seven
//                        16-B words from the current copy of the instance state and stored to the next one; six
//                        floats of scratch per node.  One lane per node, as k_refit_level, whose eight-lane form
//                        measured slower: the encode's double arithmetic is what a level waits for
#include "prt_tlas_refit.h"
#include "prt_tlas_refit_gpu.h"

namespace prt {

namespace {

constexpr int kTB = 256;

// (the table's members as separate arguments: the struct by value was copied to a private array, which the compiler
// moved to 24 B of LDS per lane)
__global__ void __launch_bounds__(kTB) k_inst_src(const float4* xf, uint32_t stride4, const uint32_t* __restrict__ mesh,
                                                  const uint32_t* __restrict__ kind,
                                                  const float4* __restrict__ mesh_box, uint32_t nmesh, int32_t n,
                                                  InstSrc* out) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  if (i >= (uint32_t)n) return;
  const float4* t = xf + (size_t)stride4 * i;
  const float4 r0 = t[0], r1 = t[1], r2 = t[2], r3 = t[3];
  uint32_t m = mesh[i];
  if (m >= nmesh) m = 0;  // (refused on the host: never an out-of-range read)
  float4 lo = mesh_box[2 * (size_t)m], hi = mesh_box[2 * (size_t)m + 1];
  lo.w = __uint_as_float(m);
  hi.w = __uint_as_float(kind[i]);
  float4* o = reinterpret_cast<float4*>(out + i);
  o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
  o[4] = lo; o[5] = hi;
}

__global__ void __launch_bounds__(kTB) k_tlas_refit_level(const Node8* src, const uint32_t* src_slot, Node8* dst,
                                                          uint32_t* dst_slot, const InstDev* __restrict__ inst,
                                                          uint32_t ninst, float* boxes,
                                                          const uint32_t* __restrict__ order, uint32_t n,
                                                          uint32_t n_nodes) {
  const uint32_t i = blockIdx.x * kTB + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = order[i];
  if (j >= n_nodes) return;
  const uint4* raw = reinterpret_cast<const uint4*>(src + j);
  const uint4* sraw = reinterpret_cast<const uint4*>(src_slot + 8 * (size_t)j);
  union { Node8 nd; uint4 q[5]; } u;
  union { uint32_t id[8]; uint4 q[2]; } sl;
#pragma unroll
  for (int k = 0; k < 5; k++) u.q[k] = raw[k];
  sl.q[0] = sraw[0];
  sl.q[1] = sraw[1];
  float box[6];
  refit_tlas_node8(u.nd, sl.id, inst, ninst, boxes, n_nodes, box);
  uint4* out = reinterpret_cast<uint4*>(dst + j);
  uint4* sout = reinterpret_cast<uint4*>(dst_slot + 8 * (size_t)j);
#pragma unroll
  for (int k = 0; k < 5; k++) out[k] = u.q[k];
  sout[0] = sl.q[0];
  sout[1] = sl.q[1];
#pragma unroll
  for (int k = 0; k < 6; k++) boxes[6 * (size_t)j + k] = box[k];
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kTB - 1) / kTB); }

}  // namespace

hipError_t launch_inst_src(hipStream_t s, const float4* xf, uint32_t stride4, const InstTabDev& tab, int32_t n,
                           InstSrc* out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_inst_src, dim3(blocks_of((uint64_t)n)), dim3(kTB), 0, s, xf, stride4, tab.mesh, tab.kind,
                     tab.mesh_box, tab.nmesh, n, out);
  return hipGetLastError();
}

hipError_t launch_tlas_refit_level(hipStream_t s, const Node8* src, const uint32_t* src_slot, Node8* dst,
                                   uint32_t* dst_slot, const InstDev* inst, uint32_t ninst, float* boxes,
                                   const uint32_t* order, uint32_t n, uint32_t n_nodes) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_tlas_refit_level, dim3(blocks_of(n)), dim3(kTB), 0, s, src, src_slot, dst, dst_slot, inst, ninst,
                     boxes, order, n, n_nodes);
  return hipGetLastError();
}

}  // namespace prt
