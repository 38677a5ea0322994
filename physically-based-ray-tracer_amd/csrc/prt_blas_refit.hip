// prt_blas_refit.hip -- the device BLAS refit of prt_update_mesh (definition and per-node code: prt_blas_refit.h).
// Its own translation unit: every earlier kernel keeps its machine code.
//
//   k_refit_tris    one lane per TriMT record: 48 B read (prim, pads), the primitive's 48-B triangle read, 48 B stored
//   k_refit_shade   one lane per ShadeTri: 27 words gathered, stored as 7 x 16 B (pad[0] kept, pad[1..4] untouched)
//                   (eight lanes per ShadeTri, 16 B each, so that a wave's store covers whole lines, measured slower:
//                   83.3 against 73.6 us on C4)
//   k_refit_level   one lane per node of one tree level, deepest level first (separate launches: no lane ever waits
//                   for another block's progress); the per-node code is refit_node8
#include "prt_blas_refit.h"
#include "prt_blas_refit_gpu.h"

namespace prt {

namespace {

constexpr int kRB = 256;

__global__ void __launch_bounds__(kRB) k_refit_tris(TriMT* __restrict__ tris, uint32_t n,
                                                    const float* __restrict__ triangles) {
  const uint32_t g = blockIdx.x * kRB + threadIdx.x;
  if (g >= n) return;
  uint4* rec = reinterpret_cast<uint4*>(tris + g);
  union { TriMT t; uint4 q[3]; } u;
  u.q[0] = rec[0]; u.q[1] = rec[1]; u.q[2] = rec[2];
  const float4* a = reinterpret_cast<const float4*>(triangles) + 3 * (size_t)u.t.prim;
  const float4 v0 = a[0], v1 = a[1], v2 = a[2];
  u.t.v0[0] = v0.x; u.t.v0[1] = v0.y; u.t.v0[2] = v0.z;
  u.t.e1[0] = v1.x - v0.x; u.t.e1[1] = v1.y - v0.y; u.t.e1[2] = v1.z - v0.z;
  u.t.e2[0] = v2.x - v0.x; u.t.e2[1] = v2.y - v0.y; u.t.e2[2] = v2.z - v0.z;
  rec[0] = u.q[0]; rec[1] = u.q[1]; rec[2] = u.q[2];
}

// words 4q .. 4q+3 of primitive p's ShadeTri (q = 0..6; word 27 is pad[0], kept)
__device__ __forceinline__ void shade_quad(ShadeTri* stri, uint32_t p, int q, const RefitMeshDev& m, uint32_t* bad) {
  float4* dst = reinterpret_cast<float4*>(stri + p) + q;
  float w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = 4 * q + k;
    w[k] = i < 27 ? refit_shade_word(i, p, m.fixed_normals, m.fixed_uvs, m.indices, m.vertices, m.face_normals,
                                     m.vertex_count, bad)
                  : __uint_as_float(stri[p].pad[0]);
  }
  *dst = make_float4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(kRB) k_refit_shade(ShadeTri* __restrict__ stri, RefitMeshDev m, RefitResult* res) {
  const uint32_t p = blockIdx.x * kRB + threadIdx.x;
  if (p >= (uint32_t)m.tri_count) return;
  uint32_t bad = 0;
#pragma unroll
  for (int q = 0; q < 7; q++) shade_quad(stri, p, q, m, &bad);
  if (bad) res->bad_index = 1u;
}

// (Eight lanes per node -- a lane per slot gathering its box, lane 0 encoding -- measured slower on C4: 21.2 against
// 16.0 us per level on average.  The encode's double arithmetic, not the gathers, is what a level waits for, and
// it then ran on one lane in eight of eight times as many waves)
__global__ void __launch_bounds__(kRB) k_refit_level(Node8* __restrict__ nodes8, const TriMT* __restrict__ tris,
                                                     const float* __restrict__ triangles, float* boxes,
                                                     const uint32_t* __restrict__ order, uint32_t n, uint32_t root,
                                                     RefitResult* res) {
  const uint32_t i = blockIdx.x * kRB + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = order[i];
  uint4* raw = reinterpret_cast<uint4*>(nodes8 + j);
  union { Node8 nd; uint4 q[5]; } u;
#pragma unroll
  for (int k = 0; k < 5; k++) u.q[k] = raw[k];
  float box[6];
  refit_node8(u.nd, tris, triangles, boxes, box);
#pragma unroll
  for (int k = 0; k < 5; k++) raw[k] = u.q[k];
#pragma unroll
  for (int k = 0; k < 6; k++) boxes[6 * (size_t)j + k] = box[k];
  if (j == root) {
    for (int k = 0; k < 3; k++) { res->bmin[k] = box[k]; res->bmax[k] = box[3 + k]; }
  }
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kRB - 1) / kRB); }

}  // namespace

hipError_t launch_refit_records(hipStream_t s, TriMT* tris, uint32_t n_recs, ShadeTri* stri, const RefitMeshDev& m,
                                RefitResult* res) {
  if (n_recs) hipLaunchKernelGGL(k_refit_tris, dim3(blocks_of(n_recs)), dim3(kRB), 0, s, tris, n_recs, m.triangles);
  if (m.tri_count > 0)
    hipLaunchKernelGGL(k_refit_shade, dim3(blocks_of((uint64_t)m.tri_count)), dim3(kRB), 0, s, stri, m, res);
  return hipGetLastError();
}

hipError_t launch_refit_level(hipStream_t s, Node8* nodes8, const TriMT* tris, const float* triangles, float* boxes,
                              const uint32_t* order, uint32_t n, uint32_t root, RefitResult* res) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_refit_level, dim3(blocks_of(n)), dim3(kRB), 0, s, nodes8, tris, triangles, boxes, order, n, root,
                     res);
  return hipGetLastError();
}

}  // namespace prt
