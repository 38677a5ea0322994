// prt_skin.hip -- the device skinning of prt_skin_mesh (definition and per-vertex / per-primitive code: prt_skin.h).
// Its own translation unit: every earlier kernel keeps its machine code.
//
//   k_skin_vertices  one lane per vertex: 24 B of bind pose, the weights as one 16-B load, the joints as one 8-B
//                    load, four 48-B joint matrices (from LDS when the binding's matrices fit kSkinLdsJoints, staged
//                    by the block; otherwise gathered through L2), 2 x 16 B stored: (P', 0) and (N', 0)
//   k_skin_prims     one lane per primitive: 12 B of indices, 3 x 2 x 16 B gathered from the skinned vertices, the fat
//                    triangle stored as 3 x 16 B (what k_refit_tris and k_refit_level then read), and the ShadeTri's
//                    words n[9], p[9], fn[3] as 7 x 16-B stores with uv[6] and pad[0] read back and kept (three 16-B
//                    loads; pad[1..4] untouched)
#include "prt_skin.h"
#include "prt_skin_gpu.h"

namespace prt {

namespace {

constexpr int kSB = 256;

__device__ __forceinline__ void load12(const float4* q, float* m) {
  const float4 a = q[0], b = q[1], c = q[2];
  m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
  m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
  m[8] = c.x; m[9] = c.y; m[10] = c.z; m[11] = c.w;
}

template <bool kLds>
__global__ void __launch_bounds__(kSB) k_skin_vertices(SkinDev m) {
  __shared__ float4 sm[kLds ? 3 * kSkinLdsJoints : 1];
  if (kLds) {
    for (int i = threadIdx.x; i < 3 * m.joint_count; i += kSB) sm[i] = m.matrices[i];
    __syncthreads();
  }
  const uint32_t v = blockIdx.x * kSB + threadIdx.x;
  if (v >= (uint32_t)m.vertex_count) return;
  const uint2 jj = m.joints[v];
  const float4 w4 = m.weights[v];
  const uint32_t j[4] = {jj.x & 0xFFFFu, jj.x >> 16, jj.y & 0xFFFFu, jj.y >> 16};
  float mj[4][12];
#pragma unroll
  for (int k = 0; k < 4; k++) load12((kLds ? sm : m.matrices) + 3 * (size_t)j[k], mj[k]);
  const float w[4] = {w4.x, w4.y, w4.z, w4.w};
  float B[12];
  skin_blend(mj[0], mj[1], mj[2], mj[3], w, B);
  const float* pp = m.positions + 3 * (size_t)v;
  const float* pn = m.normals + 3 * (size_t)v;
  const float P[3] = {pp[0], pp[1], pp[2]}, N[3] = {pn[0], pn[1], pn[2]};
  float Po[3], No[3];
  skin_vertex(B, P, N, Po, No);
  m.vpos[v] = make_float4(Po[0], Po[1], Po[2], 0.0f);
  m.vnrm[v] = make_float4(No[0], No[1], No[2], 0.0f);
}

__global__ void __launch_bounds__(kSB) k_skin_prims(SkinDev m, ShadeTri* __restrict__ stri) {
  const uint32_t p = blockIdx.x * kSB + threadIdx.x;
  if (p >= (uint32_t)m.tri_count) return;
  const int32_t* ix = m.indices + 3 * (size_t)p;
  const int32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
  const float4 a = m.vpos[i0], b = m.vpos[i1], c = m.vpos[i2];
  const float4 na = m.vnrm[i0], nb = m.vnrm[i1], nc = m.vnrm[i2];
  float4* tri = m.triangles + 3 * (size_t)p;
  tri[0] = a; tri[1] = b; tri[2] = c;
  const float pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z}, pc[3] = {c.x, c.y, c.z};
  float fn[3];
  skin_face_normal(pa, pb, pc, fn);
  // ShadeTri words: n[9] 0..8 | uv[6] 9..14 | p[9] 15..23 | fn[3] 24..26 | pad[0] 27
  float4* q = reinterpret_cast<float4*>(stri + p);
  const float4 q2 = q[2], q3 = q[3], q6 = q[6];
  q[0] = make_float4(na.x, na.y, na.z, nb.x);
  q[1] = make_float4(nb.y, nb.z, nc.x, nc.y);
  q[2] = make_float4(nc.z, q2.y, q2.z, q2.w);
  q[3] = make_float4(q3.x, q3.y, q3.z, a.x);
  q[4] = make_float4(a.y, a.z, b.x, b.y);
  q[5] = make_float4(b.z, c.x, c.y, c.z);
  q[6] = make_float4(fn[0], fn[1], fn[2], q6.w);
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kSB - 1) / kSB); }

}  // namespace

hipError_t launch_skin_mesh(hipStream_t s, const SkinDev& m, ShadeTri* stri) {
  if (m.vertex_count > 0) {
    const dim3 g(blocks_of((uint64_t)m.vertex_count)), b(kSB);
    if (m.joint_count <= kSkinLdsJoints) hipLaunchKernelGGL(k_skin_vertices<true>, g, b, 0, s, m);
    else hipLaunchKernelGGL(k_skin_vertices<false>, g, b, 0, s, m);
  }
  if (m.tri_count > 0)
    hipLaunchKernelGGL(k_skin_prims, dim3(blocks_of((uint64_t)m.tri_count)), dim3(kSB), 0, s, m, stri);
  return hipGetLastError();
}

}  // namespace prt
