// prt_variance.hip -- luminance moments carried with the frame history, and the a-trous filter they guide (gfx950).
//
// k_reproject_moments: k_reproject_motion (prt_motion.hip) with the first and second luminance moments gathered over
//                      the same taps and blended with the same factor, an optional clamp of the gathered history to the
//                      3 x 3 neighbourhood of this frame's colour, and a variance estimate: the moments' own once the
//                      history is min_temporal long, a 5 x 5 estimate over this frame's pixels of the same instance
//                      before that.  With clamp_k == 0 the colour is k_reproject_motion's bit for bit.
// k_denoise_var_prep:  k_denoise_prep, and the colour packed with its variance into one float4 (rgb, V).
// k_denoise_var:       k_denoise (prt_denoise.hip) with the colour weight's sigma scaled by the 3 x 3 pre-filtered
//                      variance of the centre pixel, and the variance filtered along with the squared weights.
// DESIGN.md "Variance guidance" has the definitions.  Every operation is a correctly rounded f32 + - * / or sqrt in a
// fixed order (no FMA contraction, IEEE division), so tests/variance_ref.py reproduces the passes bit for bit.
#include "prt_variance.h"
#include "prt_path.h"

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
// false: the pixel starts over.  h: (rgb, history length), hm: the two moments.
__device__ __forceinline__ bool gather_history(const MomentsPass& Q, int32_t x, int32_t y, float4 G0, uint32_t id,
                                               float4& h, float& hm1, float& hm2) {
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
  const V3 Xp{row4(A0, X), row4(A1, X), row4(A2, X)};  // where the point was in the previous frame
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

}  // namespace

// One block is 32 x 8 pixels, one thread per pixel, every load straight from memory, as k_reproject_motion.  The clamp
// window sits behind a wave-uniform branch; the 5 x 5 window runs only for the lanes whose history is shorter than
// min_temporal (the disoccluded minority, and every hit pixel of a frame that starts a history).
__global__ void __launch_bounds__(kBlock) k_reproject_moments(MomentsPass Q) {
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
  if (P.hist && hit && id < (uint32_t)M.count && gather_history(Q, x, y, G0, id, h, hm1, hm2)) {
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

__global__ void __launch_bounds__(kBlock) k_denoise_var_prep(int32_t n, const float4* __restrict__ normal_depth,
                                                             const float4* __restrict__ color,
                                                             const float4* __restrict__ moments,
                                                             float4* __restrict__ geo, float4* __restrict__ iv) {
  const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= n) return;
  const float4 g = normal_depth[p];
  float4 o = make_float4(0.0f, 0.0f, 0.0f, g.w);
  if (g.w < kFar) {
    const float inv = 1.0f / sqrtf(dot3(g, g));
    o = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w);
  }
  geo[p] = o;
  const float4 c = color[p];
  iv[p] = make_float4(c.x, c.y, c.z, moments[p].z);
}

namespace {

// the B3-spline kernel {1/16, 1/4, 3/8, 1/4, 1/16} at offset d = -2..2
__device__ __forceinline__ float bspline(int d) {
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

struct VaAcc {
  float r, g, b, w, v;
};

// one tap q of pixel p (q inside the image, q a hit): k_denoise's tap with the colour weight over den = sc2 * Vp, and
// the variance accumulated with the squared weight.  centre: dx == 0 && dy == 0.
__device__ __forceinline__ void var_tap(const DenoisePass& P, float den, bool centre, float hw, float dist, float4 Gp,
                                        float4 Ip, float4 Ap, float4 Gq, float4 Iq, float4 Aq, VaAcc& A) {
  float w;
  if (centre) {
    w = 0.375f * 0.375f;
  } else {
    const float dn = dot3(Gp, Gq);
    float wn = dn > 0.0f ? dn : 0.0f;  // a NaN counts as 0
    for (int k = 0; k < P.normal_power; k++) wn = wn * wn;
    const float rz = (Gq.w - Gp.w) / ((P.sigma_depth * Gp.w) * dist);
    const float wz = 1.0f / (1.0f + rz * rz);
    const float4 dc = make_float4(Iq.x - Ip.x, Iq.y - Ip.y, Iq.z - Ip.z, 0.0f);
    const float c2 = dot3(dc, dc);
    const float wc = 1.0f / (1.0f + c2 / den);
    w = (hw * wn) * wz;
    w = w * wc;
    if (P.albedo) {
      const float4 da = make_float4(Aq.x - Ap.x, Aq.y - Ap.y, Aq.z - Ap.z, 0.0f);
      w = w * (1.0f / (1.0f + dot3(da, da) / P.sa2));
    }
  }
  A.r = A.r + w * Iq.x;
  A.g = A.g + w * Iq.y;
  A.b = A.b + w * Iq.z;
  A.w = A.w + w;
  A.v = A.v + (w * w) * Iq.w;
}

__device__ __forceinline__ void var_store(const VarDenoisePass& Q, int32_t p, float r, float g, float b, float V) {
  const DenoisePass& P = Q.D;
  if (P.out) P.out[p] = make_float4(r, g, b, Q.restore ? Q.restore[p].w : V);
  if (P.rgb8) P.rgb8[p] = (pack1(r) << 16) + (pack1(g) << 8) + pack1(b);
  if (Q.variance) Q.variance[p] = V;
}

}  // namespace

// k_denoise's layout: 32 x 8 pixels per block, every tap loaded straight from memory.  The variance rides in the w of
// the colour image, so a tap stays at two or three 16-B loads; the 3 x 3 pre-filter adds nine pairs of 4-B loads per
// pixel (the neighbour's depth and variance).
__global__ void __launch_bounds__(kBlock) k_denoise_var(VarDenoisePass Q) {
  const DenoisePass& P = Q.D;
  const int32_t x = (int32_t)(blockIdx.x * kVaBX + threadIdx.x % kVaBX);
  const int32_t y = (int32_t)(blockIdx.y * kVaBY + threadIdx.x / kVaBX);
  if (x >= P.W || y >= P.H) return;
  const int32_t p = y * P.W + x;
  const float4 Gp = P.geo[p], Ip = P.color[p];
  if (!(Gp.w < kFar)) {  // a miss passes through, with its variance
    var_store(Q, p, Ip.x, Ip.y, Ip.z, Ip.w);
    return;
  }
  float gs = 0.0f, gw = 0.0f;  // the 3 x 3 Gaussian of the variance over the hits around p (the centre is one)
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const int32_t qy = y + dy;
    if (qy < 0 || qy >= P.H) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int32_t qx = x + dx;
      if (qx < 0 || qx >= P.W) continue;
      const int32_t q = qy * P.W + qx;
      if (!(P.geo[q].w < kFar)) continue;
      const float g = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
      gs = gs + g * P.color[q].w;
      gw = gw + g;
    }
  }
  const float den = P.sc2 * fmaxf(gs / gw, Q.variance_floor);
  const float4 Ap = P.albedo ? P.albedo[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int32_t s = P.step;
  VaAcc A = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (int dy = -2; dy <= 2; dy++) {
    const int32_t qy = y + s * dy;
    if (qy < 0 || qy >= P.H) continue;
    const float hy = bspline(dy);
    const int ady = dy < 0 ? -dy : dy;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int32_t qx = x + s * dx;
      if (qx < 0 || qx >= P.W) continue;
      const int32_t q = qy * P.W + qx;
      const float4 Gq = P.geo[q], Iq = P.color[q];
      const float4 Aq = P.albedo ? P.albedo[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (!(Gq.w < kFar)) continue;
      const int adx = dx < 0 ? -dx : dx;
      const float dist = (float)(s * (adx > ady ? adx : ady));
      var_tap(P, den, dx == 0 && dy == 0, hy * bspline(dx), dist, Gp, Ip, Ap, Gq, Iq, Aq, A);
    }
  }
  var_store(Q, p, A.r / A.w, A.g / A.w, A.b / A.w, A.v / (A.w * A.w));
}

// ---- host
hipError_t launch_reproject_moments(hipStream_t s, const MomentsPass& P) {
  const ReprojectPass& R = P.M.R;
  if (R.W <= 0 || R.H <= 0) return hipSuccess;
  const dim3 grid((unsigned)((R.W + kVaBX - 1) / kVaBX), (unsigned)((R.H + kVaBY - 1) / kVaBY));
  hipLaunchKernelGGL(k_reproject_moments, grid, dim3(kBlock), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_denoise_var_prep(hipStream_t s, int32_t W, int32_t H, const float4* normal_depth,
                                   const float4* color, const float4* moments, float4* geo, float4* iv) {
  const uint64_t n = (uint64_t)W * (uint64_t)H;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_denoise_var_prep, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (int32_t)n,
                     normal_depth, color, moments, geo, iv);
  return hipGetLastError();
}

hipError_t launch_denoise_var_pass(hipStream_t s, const VarDenoisePass& P) {
  if (P.D.W <= 0 || P.D.H <= 0) return hipSuccess;
  const dim3 grid((unsigned)((P.D.W + kVaBX - 1) / kVaBX), (unsigned)((P.D.H + kVaBY - 1) / kVaBY));
  hipLaunchKernelGGL(k_denoise_var, grid, dim3(kBlock), 0, s, P);
  return hipGetLastError();
}

}  // namespace prt
