// prt_reproject_dev.h -- the device code of one pixel of the reprojection pass that carries luminance moments, shared
// by k_reproject_moments (prt_variance.hip) and k_reproject_deform (prt_deform.hip).  Device only; include it from a
// .hip file after prt_path.h.  kDeform = false is prt_reproject_moments' definition, kDeform = true adds the
// per-pixel object-space offset of a deforming mesh to the point carried back (DESIGN.md "Variance guidance",
// "Deforming meshes").  Every operation is a correctly rounded f32 + - * / or sqrt in a fixed order.
#pragma once
#include "prt_variance.h"

namespace prt {

namespace {

constexpr int kVaBX = 32, kVaBY = 8;  // pixel block of one workgroup (kBlock = 256 threads), as the earlier passes'
static_assert(kVaBX * kVaBY == kBlock, "variance block");

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 v3(const float* a) { return V3{a[0], a[1], a[2]}; }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float vdot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 vunit(V3 n) {
  const float inv = 1.0f / sqrtf(vdot(n, n));
  return V3{n.x * inv, n.y * inv, n.z * inv};
}
__device__ __forceinline__ float row3(float4 a, V3 v) { return (a.x * v.x + a.y * v.y) + a.z * v.z; }
__device__ __forceinline__ float row4(float4 a, V3 v) { return row3(a, v) + a.w; }
__device__ __forceinline__ float dot3(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float luminance(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// The gathered history of pixel p: k_reproject_motion's body up to the division by ws, with the moments along.
// false: the pixel starts over.  h: (rgb, history length), hm: the two moments.  kDeform: offset[p] = (delta, w) is
// the pixel's object-space displacement to where its surface point was, prev_l three float4 rows per instance whose
// xyz are the previous transform's upper-left 3 x 3; with w != 0 row r of the point carried back gets
// (L_r.x * delta.x + L_r.y * delta.y) + L_r.z * delta.z added.
template <bool kDeform>
__device__ __forceinline__ bool gather_history(const MomentsPass& Q, const float4* __restrict__ offset,
                                               const float4* __restrict__ prev_l, int32_t x, int32_t y, float4 G0,
                                               uint32_t id, float4& h, float& hm1, float& hm2) {
  const MotionPass& M = Q.M;
  const ReprojectPass& P = M.R;
  const float Z = G0.w;
  const float4* A = M.motion + 3 * (size_t)id;
  const float4 A0 = A[0], A1 = A[1], A2 = A[2];
  const float fW = (float)P.W, fH = (float)P.H;
  const float u = (float)x * (1.0f / fW), v = (float)y * (1.0f / fH);
  const V3 pos = v3(P.pos), tl = v3(P.tl), du = v3(P.du), dv = v3(P.dv);
  const V3 Pp{(tl.x + u * du.x) + v * dv.x, (tl.y + u * du.y) + v * dv.y, (tl.z + u * du.z) + v * dv.z};
  const V3 d = vsub(Pp, pos);
  const float dinv = 1.0f / sqrtf(vdot(d, d));
  const V3 D{d.x * dinv, d.y * dinv, d.z * dinv};
  const V3 X{pos.x + Z * D.x, pos.y + Z * D.y, pos.z + Z * D.z};
  V3 Xp{row4(A0, X), row4(A1, X), row4(A2, X)};  // where the point was in the previous frame
  if constexpr (kDeform) {
    const float4 o = offset[y * P.W + x];
    if (o.w != 0.0f) {  // the surface point itself moved within its mesh
      const float4* L = prev_l + 3 * (size_t)id;
      const V3 dl{o.x, o.y, o.z};
      Xp = V3{Xp.x + row3(L[0], dl), Xp.y + row3(L[1], dl), Xp.z + row3(L[2], dl)};
    }
  }
  const V3 w = vsub(Xp, v3(P.ppos));
  const float s = vdot(w, v3(P.cuv)) / P.det;
  const float sa = vdot(w, v3(P.cv0)) / P.det;
  const float sb = vdot(w, v3(P.c0u)) / P.det;
  const float px = (sa / s) * fW, py = (sb / s) * fH;
  const float Zp = sqrtf(vdot(w, w));
  if (!(s > 0.0f && px >= -1.0f && px < fW && py >= -1.0f && py < fH)) return false;  // behind / off screen / NaN
  const float fx = floorf(px), fy = floorf(py);
  const float ax = px - fx, ay = py - fy;
  const int32_t ix = (int32_t)fx, iy = (int32_t)fy;  // -1 .. W - 1, -1 .. H - 1
  const V3 N{G0.x, G0.y, G0.z};
  const V3 n = vunit(V3{row3(A0, N), row3(A1, N), row3(A2, N)});  // the normal as it was in the previous frame
  const float tol = P.depth_tol * Zp;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float a1 = 0.0f, a2 = 0.0f, ws = 0.0f;
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
      if (!(G.w < kFar && fabsf(G.w - Zp) <= tol && vdot(n, vunit(V3{G.x, G.y, G.z})) >= P.normal_min &&
            Hq.w >= 1.0f))
        continue;
      if (M.hist_inst && M.hist_inst[q] != id) continue;  // another instance's surface
      const float4 Mq = Q.hist_mom[q];
      acc.x = acc.x + wb * Hq.x;
      acc.y = acc.y + wb * Hq.y;
      acc.z = acc.z + wb * Hq.z;
      acc.w = acc.w + wb * Hq.w;
      a1 = a1 + wb * Mq.x;
      a2 = a2 + wb * Mq.y;
      ws = ws + wb;
    }
  }
  if (!(ws > 1.0f / 64.0f)) return false;  // disoccluded: no tap of weight agrees
  h = make_float4(acc.x / ws, acc.y / ws, acc.z / ws, acc.w / ws);
  hm1 = a1 / ws;
  hm2 = a2 / ws;
  return true;
}

// h clamped per channel to mean +- k * sigma of the in-image pixels of the 3 x 3 neighbourhood of (x, y) in P.color
__device__ __forceinline__ void clamp_history(const ReprojectPass& P, float k, int32_t x, int32_t y, float4& h) {
  float s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f, n = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const int32_t qy = y + dy;
    if (qy < 0 || qy >= P.H) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int32_t qx = x + dx;
      if (qx < 0 || qx >= P.W) continue;
      const float4 c = P.color[qy * P.W + qx];
      s1x = s1x + c.x;
      s1y = s1y + c.y;
      s1z = s1z + c.z;
      s2x = s2x + c.x * c.x;
      s2y = s2y + c.y * c.y;
      s2z = s2z + c.z * c.z;
      n = n + 1.0f;
    }
  }
  const float mx = s1x / n, my = s1y / n, mz = s1z / n;
  const float sx = sqrtf(fmaxf(s2x / n - mx * mx, 0.0f)), sy = sqrtf(fmaxf(s2y / n - my * my, 0.0f)),
              sz = sqrtf(fmaxf(s2z / n - mz * mz, 0.0f));
  h.x = fminf(fmaxf(h.x, mx - k * sx), mx + k * sx);
  h.y = fminf(fmaxf(h.y, my - k * sy), my + k * sy);
  h.z = fminf(fmaxf(h.z, mz - k * sz), mz + k * sz);
}

// the luminance variance over the hit pixels of instance id in the 5 x 5 window of (x, y); the centre always counts
__device__ __forceinline__ float spatial_variance(const MotionPass& M, int32_t x, int32_t y, uint32_t id) {
  const ReprojectPass& P = M.R;
  float s1 = 0.0f, s2 = 0.0f, n = 0.0f;
#pragma unroll 1
  for (int dy = -2; dy <= 2; dy++) {
    const int32_t qy = y + dy;
    if (qy < 0 || qy >= P.H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int32_t qx = x + dx;
      if (qx < 0 || qx >= P.W) continue;
      const int32_t q = qy * P.W + qx;
      if (M.inst[q] != id || !(P.nd[q].w < kFar)) continue;
      const float Lq = luminance(P.color[q]);
      s1 = s1 + Lq;
      s2 = s2 + Lq * Lq;
      n = n + 1.0f;
    }
  }
  const float mu = s1 / n;
  return fmaxf(s2 / n - mu * mu, 0.0f);
}

// One pixel of the pass: one block is 32 x 8 pixels, one thread per pixel, every load straight from memory, as
// k_reproject_motion.  The clamp window sits behind a wave-uniform branch; the 5 x 5 window runs only for the lanes
// whose history is shorter than min_temporal (the disoccluded minority, and every hit pixel of a frame that starts a
// history).
template <bool kDeform>
__device__ __forceinline__ void reproject_moments_pixel(const MomentsPass& Q, const float4* __restrict__ offset,
                                                        const float4* __restrict__ prev_l) {
  const MotionPass& M = Q.M;
  const ReprojectPass& P = M.R;
  const int32_t x = (int32_t)(blockIdx.x * kVaBX + threadIdx.x % kVaBX);
  const int32_t y = (int32_t)(blockIdx.y * kVaBY + threadIdx.x / kVaBX);
  if (x >= P.W || y >= P.H) return;
  const int32_t p = y * P.W + x;
  const float4 C = P.color[p];
  const float4 G0 = P.nd[p];
  const uint32_t id = M.inst[p];
  const bool hit = G0.w < kFar;
  const float L = luminance(C);
  float4 o = make_float4(C.x, C.y, C.z, 1.0f);  // a pixel that starts over
  float m1 = L, m2 = L * L;
  float4 h;
  float hm1, hm2;
  if (P.hist && hit && id < (uint32_t)M.count && gather_history<kDeform>(Q, offset, prev_l, x, y, G0, id, h, hm1, hm2)) {
    const float len = fminf(h.w + 1.0f, P.max_history);
    const float a = 1.0f / len;
    if (Q.clamp_k > 0.0f) clamp_history(P, Q.clamp_k, x, y, h);
    o = make_float4(h.x + a * (C.x - h.x), h.y + a * (C.y - h.y), h.z + a * (C.z - h.z), len);
    m1 = hm1 + a * (L - hm1);
    m2 = hm2 + a * (L * L - hm2);
  }
  float var = 0.0f;  // a miss
  if (hit) {
    if (o.w >= Q.min_temporal)
      var = fmaxf(m2 - m1 * m1, 0.0f);
    else
      var = spatial_variance(M, x, y, id) * (Q.min_temporal / o.w);
  }
  if (P.out) P.out[p] = o;
  if (P.rgb8) P.rgb8[p] = (pack1(o.x) << 16) + (pack1(o.y) << 8) + pack1(o.z);
  Q.mom[p] = make_float4(m1, m2, var, 0.0f);
}

}  // namespace

}  // namespace prt
