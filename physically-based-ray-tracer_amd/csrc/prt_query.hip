// prt_query.hip -- ray queries on caller arrays (prt_query_rays / prt_query_surface) for gfx950.
//
// k_query: the persistent traversal of prt_persist.h (the engine of k_trace2) around a batch of arbitrary rays.  One
//   wave per block, MODE 2: entry g of the live range [0, total) is the closest-hit query of ray g when g < nclosest,
//   else the any-hit query of ray g - nclosest, so a call that wants both answers traces them in one launch.  The live
//   range is cut into kParts parts with one fetch counter each (fetch_some, prt_queue.h); the counters belong to the
//   context and are cleared in stream order before the launch.  A ray is read from the caller's arrays and built with
//   make_ray, as k_intersect builds it, when a lane takes it and again for every further instance it enters (the
//   engine keeps no world ray in registers).  Results are those of k_intersect / k_occluded bit for bit: the hit rule
//   does not depend on the visiting order (prt_traverse.h).
//   Never traversed: a ray with a non-finite origin or direction component, a direction whose normalisation is not
//   finite (zero length, or a squared length that underflows to zero), or a tmax that is NaN or <= 0.  load hands the
//   engine the null ray for it (the limit -1 of k_wave_init's padding entries: no box is entered at a negative limit,
//   so the lane is free again at its next step), finish writes the miss record with the tmax as given and occluded 0.
//   The engine starts a closest query as (tmax, instance 0, prim 0), which a triangle at exactly tmax in instance 0
//   beats under the tie rule; what finish finds at t >= tmax is therefore a miss (scene_closest8 reaches the same
//   with its kNoPrim start).
// k_query_surface: one thread per hit record, the shading inputs by the kernels' own hit_attributes, as k_aov.
#include "prt_launch.h"
#include "prt_path.h"
#include "prt_persist.h"
#include "prt_queue.h"

namespace prt {

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // false for NaN
}

// ray i of the caller's arrays as the engine gets it; false: never traversed (O, D, limit are then the null ray)
__device__ __forceinline__ bool query_ray(const QueryArgs& Q, uint32_t i, V3& O, V3& D, float& limit) {
  const float* o = Q.O + 3 * (size_t)i;
  const float* d = Q.D + 3 * (size_t)i;
  const float ox = o[0], oy = o[1], oz = o[2], dx = d[0], dy = d[1], dz = d[2];
  const float tm = Q.tmax ? Q.tmax[i] : kFar;
  const Ray r = make_ray(v3(ox, oy, oz), v3(dx, dy, dz));
  const bool ok = finite3(ox, oy, oz) && finite3(dx, dy, dz) && finite3(r.D.x, r.D.y, r.D.z) && tm > 0.0f;
  O = ok ? r.O : v3(0.0f, 0.0f, 0.0f);
  D = ok ? r.D : v3(0.0f, 0.0f, 1.0f);
  limit = ok ? tm : -1.0f;
  return ok;
}

template <int REFILL, int STACK, int WAVES, int TAILN, bool TLAS, bool SPILL>
__global__ void __launch_bounds__(64, WAVES) k_query(SceneDev S, QueryArgs Q) {
  __shared__ uint32_t lds_stack[2 * STACK * 64];
  __shared__ uint32_t tail_lds[tail_lds_words(TAILN)];
  const uint32_t total = Q.total, nC = Q.nclosest;
  if (blockIdx.x * 64u >= total) return;
  uint32_t part = xcc_id();
  trav8_persistent<2, STACK, REFILL, TAILN, TLAS, SPILL>(
      S, lds_stack + threadIdx.x,
      [&](uint32_t* base, uint32_t want) { return fetch_some(Q.fctr, total, part, base, want); },
      [&](uint32_t g, V3& O, V3& D, float& tmax, bool& any) -> uint32_t {
        any = g >= nC;
        const uint32_t i = any ? g - nC : g;
        (void)query_ray(Q, i, O, D, tmax);
        return i;
      },
      [&](uint32_t i, bool, V3& O, V3& D) {
        float limit;
        (void)query_ray(Q, i, O, D, limit);
      },
      [&](uint32_t i, const Hit& hit, bool any, bool occluded) {
        if (any) {
          Q.occ[i] = occluded ? 1 : 0;
          return;
        }
        const float tm = Q.tmax ? Q.tmax[i] : kFar;
        HitOut o;
        o.t = tm; o.u = 0.0f; o.v = 0.0f; o.prim = 0u; o.inst = 0u;  // the miss record
        if (hit.t > 0.0f && hit.t < tm) {
          o.t = hit.t; o.u = hit.u; o.v = hit.v; o.prim = hit.prim; o.inst = hit.inst;
        }
        Q.hits[i] = o;
      },
      []() -> bool { return false; }, Q.coop_tail ? tail_lds : nullptr, nullptr);
}

// one record per thread.  A record is a hit when its t is below the tmax its query ran under; a record that names no
// instance or primitive of the scene (not one prt_query_rays wrote) is taken as a miss, never dereferenced
__global__ void __launch_bounds__(kBlock) k_query_surface(SceneDev S, int32_t n, int32_t normalmapped,
                                                          const HitOut* __restrict__ hits,
                                                          const float* __restrict__ tmax, float4* __restrict__ albedo,
                                                          float4* __restrict__ normal_depth,
                                                          float4* __restrict__ geo_normal, float4* __restrict__ material) {
  const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= n) return;
  const HitOut h = hits[p];
  const float tm = tmax ? tmax[p] : kFar;
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = make_float4(0.0f, 0.0f, 0.0f, kFar);
  float4 gn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m0 = gn, m1 = gn;
  bool hit = h.t < tm && h.inst < (uint32_t)S.ninst;
  if (hit) hit = h.prim < S.mesh[S.inst[h.inst].mesh].tri_count;
  if (hit) {
    const HitAttr ha = hit_attributes(S, h.inst, h.prim, h.u, h.v, normalmapped != 0);
    a = make_float4(ha.m.base.x, ha.m.base.y, ha.m.base.z, 1.0f);
    g = make_float4(ha.N.x, ha.N.y, ha.N.z, h.t);
    if (geo_normal) {
      const V3 G = geometry_normal(S, h.inst, h.prim);
      gn = make_float4(G.x, G.y, G.z, 1.0f);
    }
    m0 = make_float4(ha.m.base.x, ha.m.base.y, ha.m.base.z, ha.m.metal);
    m1 = make_float4(ha.m.emis.x, ha.m.emis.y, ha.m.emis.z, ha.m.rough);
  }
  if (albedo) albedo[p] = a;
  if (normal_depth) normal_depth[p] = g;
  if (geo_normal) geo_normal[p] = gn;
  if (material) {
    material[2 * (size_t)p] = m0;
    material[2 * (size_t)p + 1] = m1;
  }
}

// ---- launchers (host).  The instantiations and their choice are launch_trace2_t's (prt_wave2.hip): by occupancy, by
// instance BVH, the 4-wave spill form for BVHs deeper than its 18 LDS groups; the grid is capped at one wave per 64
// entries.  LDS per wave: 2 x STACK x 256 B of stack + the tail slots (no prefix tables), within that file's budget
#ifndef PRT_REFILL
#define PRT_REFILL 32
#endif
template <int STACK, int WAVES, int TAILN>
static void launch_q(const LaunchCfg& c, const SceneDev& S, const QueryArgs& Q, unsigned cap) {
  static_assert(2 * STACK * 256 + 264 + 4 * 3 * TAILN <= 163840 / (4 * WAVES), "LDS over the occupancy budget");
  const unsigned grid = std::min<unsigned>(256u * 4u * WAVES / c.groups, cap);
  if (S.tlas)
    hipLaunchKernelGGL((k_query<PRT_REFILL, STACK, WAVES, TAILN, true, false>), dim3(grid), dim3(64), 0, c.stream, S, Q);
  else
    hipLaunchKernelGGL((k_query<PRT_REFILL, STACK, WAVES, TAILN, false, false>), dim3(grid), dim3(64), 0, c.stream, S, Q);
}

hipError_t launch_query(const LaunchCfg& c, const SceneDev& S, const QueryArgs& Q) {
  if (Q.total == 0) return hipSuccess;
  const unsigned cap = (unsigned)((Q.total + 63u) / 64u);
  if (S.spill) {
    // (the spill columns are indexed by the launch's own thread ids and sized for kSpillTraceBlocks waves)
    const unsigned grid = std::min<unsigned>(kSpillTraceBlocks / c.groups, cap);
    if (S.tlas)
      hipLaunchKernelGGL((k_query<32, kSpillTraceStack, 4, 32, true, true>), dim3(grid), dim3(64), 0, c.stream, S, Q);
    else
      hipLaunchKernelGGL((k_query<32, kSpillTraceStack, 4, 32, false, true>), dim3(grid), dim3(64), 0, c.stream, S, Q);
  } else if (c.occ == 7) launch_q<9, 7, 64>(c, S, Q, cap);
  else if (c.occ == 6) launch_q<11, 6, 64>(c, S, Q, cap);
  else if (c.occ == 5) launch_q<14, 5, 32>(c, S, Q, cap);
  else launch_q<18, 4, 32>(c, S, Q, cap);
  return hipGetLastError();
}

hipError_t launch_query_surface(hipStream_t s, const SceneDev& S, int32_t n, bool normalmapped, const HitOut* hits,
                                const float* tmax, float4* albedo, float4* normal_depth, float4* geo_normal,
                                float4* material) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_query_surface, dim3((unsigned)(((size_t)n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, S, n,
                     normalmapped ? 1 : 0, hits, tmax, albedo, normal_depth, geo_normal, material);
  return hipGetLastError();
}

}  // namespace prt
