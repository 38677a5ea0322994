// prt_temporal.hip -- temporal reprojection of the frame history under camera motion (gfx950).
//
// k_reproject: the first hit of every pixel is projected into the previous view, the previous output is gathered with
//              bilinear weights from the taps whose depth and normal agree, and this frame is blended in with
//              1 / history length (DESIGN.md "Temporal reprojection" has the definition).  Every operation is a
//              correctly rounded f32 + - * / or sqrt in a fixed order (no FMA contraction, IEEE division), so
//              tests/reproject_ref.py reproduces it bit for bit.
#include "prt_temporal.h"
#include "prt_path.h"

namespace prt {

constexpr int kRpBX = 32, kRpBY = 8;  // pixel block of one workgroup (kBlock = 256 threads), as the denoiser's
static_assert(kRpBX * kRpBY == kBlock, "reproject block");

struct F3 {
  float x, y, z;
};
__host__ __device__ __forceinline__ F3 f3(const float* a) { return F3{a[0], a[1], a[2]}; }
__host__ __device__ __forceinline__ F3 sub3(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ __forceinline__ F3 cross3(F3 a, F3 b) {
  return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ F3 unit3(float4 g) {
  const F3 n{g.x, g.y, g.z};
  const float inv = 1.0f / sqrtf(dot3(n, n));
  return F3{n.x * inv, n.y * inv, n.z * inv};
}

__device__ __forceinline__ void reproject_store(const ReprojectPass& P, int32_t p, float4 o) {
  if (P.out) P.out[p] = o;
  if (P.rgb8) P.rgb8[p] = (pack1(o.x) << 16) + (pack1(o.y) << 8) + pack1(o.z);
}

// One block is 32 x 8 pixels, one thread per pixel: a wave reads this frame's colour and normal_depth as two runs of
// 32 consecutive 16-B items and gathers up to eight 16-B history items around the reprojected position; neighbouring
// pixels land on neighbouring taps, so the gathers of a wave share their cache lines.  No LDS.
__global__ void __launch_bounds__(kBlock) k_reproject(ReprojectPass P) {
  const int32_t x = (int32_t)(blockIdx.x * kRpBX + threadIdx.x % kRpBX);
  const int32_t y = (int32_t)(blockIdx.y * kRpBY + threadIdx.x / kRpBX);
  if (x >= P.W || y >= P.H) return;
  const int32_t p = y * P.W + x;
  const float4 C = P.color[p];
  const float4 fresh = make_float4(C.x, C.y, C.z, 1.0f);
  if (!P.hist) {  // no history yet
    reproject_store(P, p, fresh);
    return;
  }
  const float4 G0 = P.nd[p];
  const float Z = G0.w;
  if (!(Z < kFar)) {  // a miss
    reproject_store(P, p, fresh);
    return;
  }
  const float fW = (float)P.W, fH = (float)P.H;
  const float u = (float)x * (1.0f / fW), v = (float)y * (1.0f / fH);
  const F3 pos = f3(P.pos), tl = f3(P.tl), du = f3(P.du), dv = f3(P.dv);
  const F3 Pp{(tl.x + u * du.x) + v * dv.x, (tl.y + u * du.y) + v * dv.y, (tl.z + u * du.z) + v * dv.z};
  const F3 d = sub3(Pp, pos);
  const float dinv = 1.0f / sqrtf(dot3(d, d));
  const F3 D{d.x * dinv, d.y * dinv, d.z * dinv};
  const F3 X{pos.x + Z * D.x, pos.y + Z * D.y, pos.z + Z * D.z};
  const F3 w = sub3(X, f3(P.ppos));
  const float s = dot3(w, f3(P.cuv)) / P.det;
  const float sa = dot3(w, f3(P.cv0)) / P.det;
  const float sb = dot3(w, f3(P.c0u)) / P.det;
  const float px = (sa / s) * fW, py = (sb / s) * fH;
  const float Zp = sqrtf(dot3(w, w));
  if (!(s > 0.0f && px >= -1.0f && px < fW && py >= -1.0f && py < fH)) {  // behind or off the previous screen (NaN too)
    reproject_store(P, p, fresh);
    return;
  }
  const float fx = floorf(px), fy = floorf(py);
  const float ax = px - fx, ay = py - fy;
  const int32_t ix = (int32_t)fx, iy = (int32_t)fy;  // -1 .. W - 1, -1 .. H - 1
  const F3 n = unit3(G0);
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
      if (!(G.w < kFar && fabsf(G.w - Zp) <= tol && dot3(n, unit3(G)) >= P.normal_min && Hq.w >= 1.0f)) continue;
      acc.x = acc.x + wb * Hq.x;
      acc.y = acc.y + wb * Hq.y;
      acc.z = acc.z + wb * Hq.z;
      acc.w = acc.w + wb * Hq.w;
      ws = ws + wb;
    }
  }
  if (!(ws > 1.0f / 64.0f)) {  // disoccluded: no tap of weight agrees
    reproject_store(P, p, fresh);
    return;
  }
  const float hx = acc.x / ws, hy = acc.y / ws, hz = acc.z / ws, hw = acc.w / ws;
  const float len = fminf(hw + 1.0f, P.max_history);
  const float a = 1.0f / len;
  reproject_store(P, p, make_float4(hx + a * (C.x - hx), hy + a * (C.y - hy), hz + a * (C.z - hz), len));
}

// ---- host
void make_reproject_pass(ReprojectPass& P, const prt_camera& cam, const prt_camera* prev) {
  const F3 tl = f3(cam.top_left), du = sub3(f3(cam.top_right), tl), dv = sub3(f3(cam.bottom_left), tl);
  const F3 zero{0.0f, 0.0f, 0.0f};
  F3 pp = zero, cuv = zero, cv0 = zero, c0u = zero;
  P.det = 0.0f;
  if (prev) {
    pp = f3(prev->pos);
    const F3 ptl = f3(prev->top_left);
    const F3 e0 = sub3(ptl, pp), eu = sub3(f3(prev->top_right), ptl), ev = sub3(f3(prev->bottom_left), ptl);
    cuv = cross3(eu, ev);
    cv0 = cross3(ev, e0);
    c0u = cross3(e0, eu);
    P.det = dot3(e0, cuv);
  }
  const F3 src[8] = {f3(cam.pos), tl, du, dv, pp, cuv, cv0, c0u};
  float* dst[8] = {P.pos, P.tl, P.du, P.dv, P.ppos, P.cuv, P.cv0, P.c0u};
  for (int k = 0; k < 8; k++) {
    dst[k][0] = src[k].x;
    dst[k][1] = src[k].y;
    dst[k][2] = src[k].z;
  }
}

hipError_t launch_reproject(hipStream_t s, const ReprojectPass& P) {
  if (P.W <= 0 || P.H <= 0) return hipSuccess;
  const dim3 grid((unsigned)((P.W + kRpBX - 1) / kRpBX), (unsigned)((P.H + kRpBY - 1) / kRpBY));
  hipLaunchKernelGGL(k_reproject, grid, dim3(kBlock), 0, s, P);
  return hipGetLastError();
}

}  // namespace prt
