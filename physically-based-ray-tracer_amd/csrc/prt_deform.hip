// prt_deform.hip -- temporal reprojection that follows deforming meshes (gfx950).
//
// k_snapshot_mesh:    the object-space corners of a mesh's primitives (ShadeTri::p) copied into the mesh's snapshot,
//                     nine floats per primitive in prim order.
// k_aov_deform:       HitOut of k_primary_hits -> the first hit's object-space displacement from where its surface
//                     point is now to where it was at the snapshot, the corners' differences interpolated with the
//                     hit's barycentrics; (0, 0, 0, 0) for a miss and for a mesh without a snapshot.
// k_reproject_deform: k_reproject_moments (prt_variance.hip) with that displacement, under the upper-left 3 x 3 of the
//                     instance's previous transform, added to the point carried back (prt_reproject_dev.h).
// DESIGN.md "Deforming meshes" has the definitions.  Every operation is a correctly rounded f32 + - * / or sqrt in a
// fixed order (no FMA contraction, IEEE division), so tests/deform_ref.py reproduces the passes bit for bit.
#include "prt_deform.h"
#include "prt_path.h"
#include "prt_reproject_dev.h"

namespace prt {

namespace {
constexpr uint32_t kCornerWord = 15;  // ShadeTri: n[9] | uv[6] | p[9] | ...
static_assert(offsetof(ShadeTri, p) == 4 * kCornerWord, "ShadeTri::p");
}  // namespace

// One thread per float: the reads are 36 of every 128 bytes of the records, the writes contiguous.
__global__ void __launch_bounds__(kBlock) k_snapshot_mesh(uint64_t n, const ShadeTri* __restrict__ stri,
                                                          float* __restrict__ snap) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t p = i / 9;
  snap[i] = stri[p].p[(uint32_t)(i - 9 * p)];
}

// One thread per pixel, no LDS.  Per lane: the 20-B HitOut, the instance's mesh word, the mesh's prim_base and its
// snapshot pointer, then 36 B of the primitive's record and 36 B of the snapshot.
__global__ void __launch_bounds__(kBlock) k_aov_deform(int32_t n, const HitOut* __restrict__ hits,
                                                       const InstDev* __restrict__ inst,
                                                       const MeshDev* __restrict__ mesh,
                                                       const ShadeTri* __restrict__ stri,
                                                       const float* const* __restrict__ snaps,
                                                       float4* __restrict__ offset) {
  const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= n) return;
  const HitOut h = hits[p];
  float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (h.t < kFar && snaps) {
    const uint32_t mi = inst[h.inst].mesh;
    const float* q = snaps[mi];
    if (q) {
      const float* c = stri[mesh[mi].prim_base + h.prim].p;
      q += 9 * (size_t)h.prim;
      const float w0 = (1.0f - h.u) - h.v;
      float d[3];
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const float d0 = q[j] - c[j], d1 = q[3 + j] - c[3 + j], d2 = q[6 + j] - c[6 + j];
        d[j] = (w0 * d0 + h.u * d1) + h.v * d2;
      }
      o = make_float4(d[0], d[1], d[2], 1.0f);
    }
  }
  offset[p] = o;
}

// k_reproject_moments' layout and loads, and per hit pixel with history one more 16-B load (the offset) and, where
// its w is set, three of the instance's previous transform.
__global__ void __launch_bounds__(kBlock) k_reproject_deform(DeformPass D) {
  reproject_moments_pixel<true>(D.Q, D.offset, D.prev_l);
}

// ---- host
hipError_t launch_snapshot_mesh(hipStream_t s, const ShadeTri* stri, uint32_t tris, float* snap) {
  const uint64_t n = 9ull * tris;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_snapshot_mesh, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n, stri, snap);
  return hipGetLastError();
}

hipError_t launch_aov_deform(hipStream_t s, const SceneDev& S, int32_t W, int32_t H, const HitOut* hits,
                             const float* const* snaps, float4* offset) {
  const uint64_t n = (uint64_t)W * (uint64_t)H;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_aov_deform, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (int32_t)n, hits,
                     S.inst, S.mesh, S.stri, snaps, offset);
  return hipGetLastError();
}

hipError_t launch_reproject_deform(hipStream_t s, const DeformPass& P) {
  const ReprojectPass& R = P.Q.M.R;
  if (R.W <= 0 || R.H <= 0) return hipSuccess;
  const dim3 grid((unsigned)((R.W + kVaBX - 1) / kVaBX), (unsigned)((R.H + kVaBY - 1) / kVaBY));
  hipLaunchKernelGGL(k_reproject_deform, grid, dim3(kBlock), 0, s, P);
  return hipGetLastError();
}

}  // namespace prt
