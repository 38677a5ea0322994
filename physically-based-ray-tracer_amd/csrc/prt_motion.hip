// prt_motion.hip -- temporal reprojection that follows moving instances (gfx950).
//
// k_aov_ids:          HitOut of k_primary_hits -> the first hit's instance index per pixel (a miss: 0xFFFFFFFF).
// k_reproject_motion: k_reproject (prt_temporal.hip) with the pixel's world-space hit and normal carried back by the
//                     motion matrix of its instance (prev * inverse(cur)) before the projection into the previous
//                     view, and the taps optionally compared by instance id (DESIGN.md "Moving instances" has the
//                     definition).  Every operation is a correctly rounded f32 + - * / or sqrt in a fixed order (no
//                     FMA contraction, IEEE division), so tests/motion_ref.py reproduces it bit for bit; with identity
//                     matrices every added product and sum is exact and the output is k_reproject's.
#include "prt_motion.h"
#include "prt_path.h"

namespace prt {

namespace {

constexpr int kMoBX = 32, kMoBY = 8;  // pixel block of one workgroup (kBlock = 256 threads), as k_reproject's
static_assert(kMoBX * kMoBY == kBlock, "motion reproject block");

struct M3 {
  float x, y, z;
};
__device__ __forceinline__ M3 m3(const float* a) { return M3{a[0], a[1], a[2]}; }
__device__ __forceinline__ M3 vsub(M3 a, M3 b) { return M3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float vdot(M3 a, M3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ M3 vunit(M3 n) {
  const float inv = 1.0f / sqrtf(vdot(n, n));
  return M3{n.x * inv, n.y * inv, n.z * inv};
}
// one row of the 3 x 4 matrix applied to a direction / to a point
__device__ __forceinline__ float row3(float4 a, M3 v) { return (a.x * v.x + a.y * v.y) + a.z * v.z; }
__device__ __forceinline__ float row4(float4 a, M3 v) { return row3(a, v) + a.w; }

__device__ __forceinline__ void motion_store(const ReprojectPass& P, int32_t p, float4 o) {
  if (P.out) P.out[p] = o;
  if (P.rgb8) P.rgb8[p] = (pack1(o.x) << 16) + (pack1(o.y) << 8) + pack1(o.z);
}

}  // namespace

__global__ void __launch_bounds__(kBlock) k_aov_ids(int32_t n, const HitOut* __restrict__ hits,
                                                    uint32_t* __restrict__ instance) {
  const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= n) return;
  const HitOut h = hits[p];
  instance[p] = h.t < kFar ? h.inst : 0xFFFFFFFFu;
}

// One block is 32 x 8 pixels, one thread per pixel, no LDS, as k_reproject.  The matrix is three 16-B loads indexed by
// the pixel's instance id: a wave covers 32 x 2 pixels and sees few distinct instances, so its lanes share the lines.
__global__ void __launch_bounds__(kBlock) k_reproject_motion(MotionPass M) {
  const ReprojectPass& P = M.R;
  const int32_t x = (int32_t)(blockIdx.x * kMoBX + threadIdx.x % kMoBX);
  const int32_t y = (int32_t)(blockIdx.y * kMoBY + threadIdx.x / kMoBX);
  if (x >= P.W || y >= P.H) return;
  const int32_t p = y * P.W + x;
  const float4 C = P.color[p];
  const float4 fresh = make_float4(C.x, C.y, C.z, 1.0f);
  if (!P.hist) {  // no history yet
    motion_store(P, p, fresh);
    return;
  }
  const float4 G0 = P.nd[p];
  const float Z = G0.w;
  if (!(Z < kFar)) {  // a miss
    motion_store(P, p, fresh);
    return;
  }
  const uint32_t id = M.inst[p];
  if (id >= (uint32_t)M.count) {  // an instance the caller gave no matrix for
    motion_store(P, p, fresh);
    return;
  }
  const float4* A = M.motion + 3 * (size_t)id;
  const float4 A0 = A[0], A1 = A[1], A2 = A[2];
  const float fW = (float)P.W, fH = (float)P.H;
  const float u = (float)x * (1.0f / fW), v = (float)y * (1.0f / fH);
  const M3 pos = m3(P.pos), tl = m3(P.tl), du = m3(P.du), dv = m3(P.dv);
  const M3 Pp{(tl.x + u * du.x) + v * dv.x, (tl.y + u * du.y) + v * dv.y, (tl.z + u * du.z) + v * dv.z};
  const M3 d = vsub(Pp, pos);
  const float dinv = 1.0f / sqrtf(vdot(d, d));
  const M3 D{d.x * dinv, d.y * dinv, d.z * dinv};
  const M3 X{pos.x + Z * D.x, pos.y + Z * D.y, pos.z + Z * D.z};
  const M3 Xp{row4(A0, X), row4(A1, X), row4(A2, X)};  // where the point was in the previous frame
  const M3 w = vsub(Xp, m3(P.ppos));
  const float s = vdot(w, m3(P.cuv)) / P.det;
  const float sa = vdot(w, m3(P.cv0)) / P.det;
  const float sb = vdot(w, m3(P.c0u)) / P.det;
  const float px = (sa / s) * fW, py = (sb / s) * fH;
  const float Zp = sqrtf(vdot(w, w));
  if (!(s > 0.0f && px >= -1.0f && px < fW && py >= -1.0f && py < fH)) {  // behind or off the previous screen (NaN too)
    motion_store(P, p, fresh);
    return;
  }
  const float fx = floorf(px), fy = floorf(py);
  const float ax = px - fx, ay = py - fy;
  const int32_t ix = (int32_t)fx, iy = (int32_t)fy;  // -1 .. W - 1, -1 .. H - 1
  const M3 N{G0.x, G0.y, G0.z};
  const M3 n = vunit(M3{row3(A0, N), row3(A1, N), row3(A2, N)});  // the normal as it was in the previous frame
  const float tol = P.depth_tol * Zp;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float ws = 0.0f;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int32_t qy = iy + j;
    if (qy < 0 || qy >= P.H) continue;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int32_t qx = ix + i;
      if (qx < 0 || qx >= P.W) continue;
      const int32_t q = qy * P.W + qx;
      const float4 G = P.hist_nd[q], Hq = P.hist[q];
      const float wb = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
      if (!(G.w < kFar && fabsf(G.w - Zp) <= tol && vdot(n, vunit(M3{G.x, G.y, G.z})) >= P.normal_min &&
            Hq.w >= 1.0f))
        continue;
      if (M.hist_inst && M.hist_inst[q] != id) continue;  // another instance's surface
      acc.x = acc.x + wb * Hq.x;
      acc.y = acc.y + wb * Hq.y;
      acc.z = acc.z + wb * Hq.z;
      acc.w = acc.w + wb * Hq.w;
      ws = ws + wb;
    }
  }
  if (!(ws > 1.0f / 64.0f)) {  // disoccluded: no tap of weight agrees
    motion_store(P, p, fresh);
    return;
  }
  const float hx = acc.x / ws, hy = acc.y / ws, hz = acc.z / ws, hw = acc.w / ws;
  const float len = fminf(hw + 1.0f, P.max_history);
  const float a = 1.0f / len;
  motion_store(P, p, make_float4(hx + a * (C.x - hx), hy + a * (C.y - hy), hz + a * (C.z - hz), len));
}

// ---- host
hipError_t launch_aov_ids(hipStream_t s, int32_t W, int32_t H, const HitOut* hits, uint32_t* instance) {
  const size_t n = (size_t)W * H;
  if (n == 0 || !instance) return hipSuccess;
  hipLaunchKernelGGL(k_aov_ids, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (int32_t)n, hits,
                     instance);
  return hipGetLastError();
}

hipError_t launch_reproject_motion(hipStream_t s, const MotionPass& P) {
  if (P.R.W <= 0 || P.R.H <= 0) return hipSuccess;
  const dim3 grid((unsigned)((P.R.W + kMoBX - 1) / kMoBX), (unsigned)((P.R.H + kMoBY - 1) / kMoBY));
  hipLaunchKernelGGL(k_reproject_motion, grid, dim3(kBlock), 0, s, P);
  return hipGetLastError();
}

}  // namespace prt
