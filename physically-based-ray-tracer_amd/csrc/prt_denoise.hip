// prt_denoise.hip -- first-hit feature buffers and the edge-avoiding a-trous filter they guide (gfx950).
//
// k_aov:          HitOut of k_primary_hits -> albedo / normal+depth with the shading kernels' hit_attributes().
// k_denoise_prep: unit normal + depth packed into one float4 per pixel, so a filter tap is two or three 16-B loads.
// k_denoise:      one a-trous iteration (DESIGN.md "Denoiser" has the definition).  Every operation is a correctly
//                 rounded f32 + - * / in a fixed order (no FMA contraction, IEEE division), so tests/denoise_ref.py
//                 reproduces it bit for bit.
#include "prt_denoise.h"
#include "prt_path.h"

namespace prt {

constexpr int kDnBX = 32, kDnBY = 8;  // pixel block of one workgroup (kBlock = 256 threads)
static_assert(kDnBX * kDnBY == kBlock, "denoise block");

__global__ void __launch_bounds__(kBlock) k_aov(SceneDev S, int32_t n, int32_t normalmapped,
                                                const HitOut* __restrict__ hits, float4* __restrict__ albedo,
                                                float4* __restrict__ normal_depth) {
  const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= n) return;
  const HitOut h = hits[p];
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 g = make_float4(0.0f, 0.0f, 0.0f, kFar);
  if (h.t < kFar) {
    const HitAttr ha = hit_attributes(S, h.inst, h.prim, h.u, h.v, normalmapped != 0);
    a = make_float4(ha.m.base.x, ha.m.base.y, ha.m.base.z, 1.0f);
    g = make_float4(ha.N.x, ha.N.y, ha.N.z, h.t);
  }
  if (albedo) albedo[p] = a;
  if (normal_depth) normal_depth[p] = g;
}

__device__ __forceinline__ float dot3(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__global__ void __launch_bounds__(kBlock) k_denoise_prep(int32_t n, const float4* __restrict__ normal_depth,
                                                         float4* __restrict__ geo) {
  const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= n) return;
  const float4 g = normal_depth[p];
  float4 o = make_float4(0.0f, 0.0f, 0.0f, g.w);
  if (g.w < kFar) {
    const float inv = 1.0f / sqrtf(dot3(g, g));
    o = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w);
  }
  geo[p] = o;
}

// the B3-spline kernel {1/16, 1/4, 3/8, 1/4, 1/16} at offset d = -2..2
__device__ __forceinline__ float bspline(int d) {
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

struct DnAcc {
  float r, g, b, w;
};

// one tap q of pixel p (q inside the image, q a hit).  centre: dx == 0 && dy == 0.
__device__ __forceinline__ void denoise_tap(const DenoisePass& P, bool centre, float hw, float dist, float4 Gp, float4 Ip,
                                            float4 Ap, float4 Gq, float4 Iq, float4 Aq, DnAcc& A) {
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
    const float wc = 1.0f / (1.0f + c2 / P.sc2);
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
}

__device__ __forceinline__ void denoise_store(const DenoisePass& P, int32_t p, float4 o) {
  if (P.out) P.out[p] = o;
  if (P.rgb8) P.rgb8[p] = (pack1(o.x) << 16) + (pack1(o.y) << 8) + pack1(o.z);
}

// One block is 32 x 8 pixels.  Every tap is loaded straight from memory: at any step a tap of the wave is two runs
// of 32 consecutive pixels, 16 B each, and the pass is bound by its arithmetic (six IEEE divisions per tap), not by
// the tap traffic -- staging the block and its halo in LDS for steps 1 and 2 measured the same time.
__global__ void __launch_bounds__(kBlock) k_denoise(DenoisePass P) {
  const int32_t x = (int32_t)(blockIdx.x * kDnBX + threadIdx.x % kDnBX);
  const int32_t y = (int32_t)(blockIdx.y * kDnBY + threadIdx.x / kDnBX);
  if (x >= P.W || y >= P.H) return;
  const int32_t p = y * P.W + x;
  const float4 Gp = P.geo[p], Ip = P.color[p];
  if (!(Gp.w < kFar)) {  // a miss passes through
    denoise_store(P, p, Ip);
    return;
  }
  const float4 Ap = P.albedo ? P.albedo[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int32_t s = P.step;
  DnAcc A = {0.0f, 0.0f, 0.0f, 0.0f};
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
      denoise_tap(P, dx == 0 && dy == 0, hy * bspline(dx), dist, Gp, Ip, Ap, Gq, Iq, Aq, A);
    }
  }
  denoise_store(P, p, make_float4(A.r / A.w, A.g / A.w, A.b / A.w, Ip.w));
}

// ---- launchers (host)
static inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

hipError_t launch_aov(hipStream_t s, const SceneDev& S, int32_t W, int32_t H, bool normalmapped, const HitOut* hits,
                      float4* albedo, float4* normal_depth) {
  const uint64_t n = (uint64_t)W * (uint64_t)H;
  if (n == 0 || (!albedo && !normal_depth)) return hipSuccess;
  hipLaunchKernelGGL(k_aov, dim3(grid_of(n)), dim3(kBlock), 0, s, S, (int32_t)n, normalmapped ? 1 : 0, hits, albedo,
                     normal_depth);
  return hipGetLastError();
}

hipError_t launch_denoise_prep(hipStream_t s, int32_t W, int32_t H, const float4* normal_depth, float4* geo) {
  const uint64_t n = (uint64_t)W * (uint64_t)H;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_denoise_prep, dim3(grid_of(n)), dim3(kBlock), 0, s, (int32_t)n, normal_depth, geo);
  return hipGetLastError();
}

hipError_t launch_denoise_pass(hipStream_t s, const DenoisePass& P) {
  if (P.W <= 0 || P.H <= 0) return hipSuccess;
  const dim3 grid((unsigned)((P.W + kDnBX - 1) / kDnBX), (unsigned)((P.H + kDnBY - 1) / kDnBY));
  hipLaunchKernelGGL(k_denoise, grid, dim3(kBlock), 0, s, P);
  return hipGetLastError();
}

}  // namespace prt
