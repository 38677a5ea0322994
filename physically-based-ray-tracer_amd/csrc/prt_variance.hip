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
#include "prt_reproject_dev.h"

namespace prt {

// the pixel's code: prt_reproject_dev.h (k_reproject_deform of prt_deform.hip shares it)
__global__ void __launch_bounds__(kBlock) k_reproject_moments(MomentsPass Q) {
  reproject_moments_pixel<false>(Q, nullptr, nullptr);
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
