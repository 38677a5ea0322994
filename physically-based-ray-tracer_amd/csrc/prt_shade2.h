// prt_shade2.h -- the shading stage of the wavefront path tracer (prt_wave2.hip): k_shade2 and what it shares with the
// misses' pass and the resolves.  A header so that the deferred-resolve forms are instantiated in a translation unit
// of their own (prt_defer.hip) and the kernels of prt_wave2.hip keep their machine code.
#pragma once
#include "prt_launch.h"
#include "prt_path.h"
#include "prt_queue.h"

namespace prt {

// The resolve of the plain pipeline (no extensions, render mode 0) and of the merged one walks all items in index
// order and takes those whose rinfo carries kRiFresh (set by the shading of the last iteration, cleared by the
// resolve), so its record loads coalesce; with extensions or a debug render mode it walks the last iteration's queue
// (k_resmiss2), which also shades that iteration's misses
constexpr uint32_t kResFresh = kRiFresh;

// the skybox lookup out of line: its correctly rounded double atan2 / acos would otherwise raise the register
// budget of the shading kernel, which looks up the sky for its misses itself
// (the three fields it reads passed by value: a SceneDev& of a kernel argument would copy the struct to scratch)
__device__ __noinline__ V3 sample_sky_call(const float* sky, int32_t w, int32_t h, V3 D) {
  SceneDev S{};
  S.sky = sky;
  S.skyw = w;
  S.skyh = h;
  return sample_sky(S, D);
}

// ---- misses of P(iter) (:159): sky radiance (or 0) into ne, before k_shade2 replaces the ray.  EXT: a ray
// that reaches the area light before any geometry ends there (ne = its MIS-weighted radiance, hit = miss).
template <bool EXT>
__device__ __forceinline__ void miss_item(const SceneDev& S, const TraceArgs& A, const WaveBufs& B, uint32_t item) {
  float4 hh = B.hit[item];
  if constexpr (EXT) {
    if (S.area) {
      const float4 o = B.ro[item], d = B.rd[item];
      const AreaLight AL = area_light(S);
      float tq, cl;
      if (area_hit(AL, v3(o.x, o.y, o.z), v3(d.x, d.y, d.z), hh.x, tq, cl)) {
        const uint32_t depth = B.info[item] & 0xFFu;
        const float pdf = depth == 0 ? kFar : B.T[(size_t)(depth - 1) * B.n + item].w;
        const V3 L = area_seen(AL, tq, cl, pdf);
        B.ne[item] = make_float4(L.x, L.y, L.z, 0.0f);
        B.hit[item] = make_float4(kFar, 0.0f, 0.0f, 0.0f);
        return;
      }
    }
  }
  if (hh.x < kFar) return;
  V3 L = v3(0.0f, 0.0f, 0.0f);
  if (A.flags & kSkybox) {
    const float4 d = B.rd[item];
    L = sample_sky_call(S.sky, S.skyw, S.skyh, v3(d.x, d.y, d.z));
  }
  B.ne[item] = make_float4(L.x, L.y, L.z, 0.0f);
}
template <bool EXT>
__global__ void __launch_bounds__(kBlock) k_miss2(SceneDev S, TraceArgs A, WaveBufs B, uint32_t iter) {
  __shared__ uint32_t pref[kNSub + 1];
  const uint32_t* q = (iter & 1) ? B.q1 : B.q0;
  const uint32_t total = load_prefix(B.ctr, iter, 0, pref);
  for (uint32_t c = blockIdx.x; c * kBlock < total; c += gridDim.x) {
    const uint32_t g = c * kBlock + threadIdx.x;
    if (g >= total) continue;
    miss_item<EXT>(S, A, B, q[map_slot(pref, g, B.qcap)]);
  }
}

// the path of `item` ends at this iteration: with AA and path 1, queue path 2's primary ray (its jitter was
// drawn at init, :61) -- returns true when a ray was set up for P(iter + 1)
__device__ __forceinline__ bool start_path2(const SceneDev& S, const TraceArgs& A, const TileMap& M,
                                            const WaveBufs& B, uint32_t item, uint32_t path) {
  if (path != 0 || !(A.flags & kAA)) return false;
  const uint32_t r = (B.base + item) % M.items;
  int32_t x, y;
  item_pixel(M, r, x, y);
  const float2 j = B.jit[item];
  const Ray r2 = primary_ray(S, (float)x + j.x, (float)y + j.y, A.W, A.H);
  B.ro[item] = make_float4(r2.O.x, r2.O.y, r2.O.z, 0.0f);
  B.rd[item] = make_float4(r2.D.x, r2.D.y, r2.D.z, 0.0f);
  B.info[item] = 1u << 8;
  return true;
}

// the sub-path of `item` ends at this iteration (EXT): continue with the refraction ray of the deepest
// dielectric node whose reflection subtree this was (the reference's depth-first recursion order,
// Core/Renderer.cpp:346 before :358) -- returns true when a ray was set up for P(iter + 1)
__device__ __forceinline__ bool diel_next(const WaveBufs& B, uint32_t item, uint32_t depth, uint32_t path) {
  uint32_t ds = B.dst[item];
  const uint32_t pend = ds & ~(ds >> 8) & ~(ds >> 24) & 0xFFu & ((1u << depth) - 1u);
  if (!pend) return false;
  const uint32_t k = 31u - (uint32_t)__builtin_clz(pend);
  const float4 o = B.dro[(size_t)k * B.n + item], d = B.drd[(size_t)k * B.n + item];
  B.ro[item] = make_float4(o.x, o.y, o.z, 0.0f);
  B.rd[item] = make_float4(d.x, d.y, d.z, 0.0f);
  B.info[item] = (k + 1u) | (path << 8);
  B.dst[item] = ds | (1u << (8 + k));
  return true;
}

// ---- the light-visibility record (WaveBufs::lvis; header comment).  An entry is 8 bytes, byte l for light l
// (x: point lights 0-3, y: kLightDir, kLightSpot): 0 unknown, 1 occluded, 2 unoccluded.  Ray k of an item of
// `kind` goes to light k (kind 0) or to the kind's one light (k = 0).
static_assert(kBlock <= 256, "block_append_skip packs two counts of up to 4 x kBlock into one word");
// the bytes of this kind's lights, ray k's in byte k -> ask: bit 8k set where ray k's answer is unknown (it is
// queued); vis0: byte k = 1 where it is known unoccluded (the visibility word the traversal would have left)
__device__ __forceinline__ void lvis_split(uint2 e, int kind, uint32_t& ask, uint32_t& vis0) {
  const uint32_t w = kind == 0 ? e.x : ((kind == 2 ? e.y >> 8 : e.y) & 0xFFu);
  const uint32_t rays = kind == 0 ? 0x01010101u : 1u;
  vis0 = (w >> 1) & rays;
  ask = ~(w | (w >> 1)) & rays;
}
// what the asked rays of a kRiLearn item found (its visibility word after the traversal; the bytes of rays that
// were not asked hold what the record already said) -> the record.  Plain stores: every frame of a pixel that
// learns writes the same values, and an item of kind 0 writes all four point-light bytes, as one word.
__device__ __forceinline__ void lvis_learn(const WaveBufs& B, uint32_t item, uint32_t ri) {
  const uint32_t kind = (ri >> 20) & 3u, vw = B.vis[item];
  uint2* e = B.lvis + (B.base + item) % B.pitems;
  if (kind == 0) e->x = 0x01010101u + (vw & 0x01010101u);
  else reinterpret_cast<uint8_t*>(e)[kind == 2 ? 5 : 4] = (uint8_t)(1u + (vw & 1u));
}
// the context's running total of shadow rays answered from the record (prt_shadow_reuse): 8 bytes behind the ray
// totals in the diagnostics buffer
__device__ __forceinline__ unsigned long long* lvis_total(const SceneDev& S) {
  return reinterpret_cast<unsigned long long*>(S.diag + 8);
}
// ... and of the dead shadow rays that were counted instead of queued (prt_shadow_dead): the 8 bytes behind that
__device__ __forceinline__ unsigned long long* dead_total(const SceneDev& S) {
  return reinterpret_cast<unsigned long long*>(S.diag + 10);
}
// the light-class shadow-queue entries of an item, rebuilt from its light class and its live mask (nee_live) in
// compact slots from s0 on: ray k of kind 0 goes to point light k, the other kinds have ray 0 alone; vi = the index
// of the item's visibility word
__device__ __forceinline__ void queue_live(uint32_t* shq, uint32_t s0, int kind, uint32_t live, uint32_t vi) {
  const uint32_t l0 = kind == 0 ? 0u : (kind == 2 ? kLightSpot : kLightDir);
#pragma unroll
  for (uint32_t k = 0; k < 4; k++)
    if (live & (1u << k)) shq[s0 + (uint32_t)__popc(live & ((1u << k) - 1u))] = ((l0 + k) << 29) | (4u * vi + k);
}

// ---- shading of P(iter): NEE set-up -> S(iter), BRDF sample or path-2 start -> P(iter + 1)
// k_shade2's parameter list as the kernarg segment holds it (explicit arguments in order, each at its natural
// alignment, as C lays out these members)
struct Shade2Args {
  SceneDev S;
  TraceArgs A;
  TileMap M;
  WaveBufs B;
  uint32_t iter;
};
typedef const __attribute__((address_space(4))) Shade2Args* Shade2ArgsPtr;
// EXT (area light, dielectrics): held to 3 waves/SIMD (168 VGPRs, no spills; unbounded it took 175 and ran 2
// waves: C5 frame 135.7 -> 132.4 ms).  The plain form runs 4 waves at its natural 125 VGPRs (forcing 5 spilled
// and was 2 % slower).
// I0 (plain form): iteration 0 of a pass with pmode kPrimReuse and a light-visibility record (B.lvis), an
// instantiation of its own so that the shading of every other launch carries nothing for it
// DEFER (plain form): a pass with a deferred resolve (prt_defer.hip k_shade2d / k_resolve_pass).  The host hands the
// launch the record plane of its iteration in rinfo / ne / nb / nk / vis / T, so the one index that differs is the
// throughput's: the plane holds one entry per item, not one per depth.
// The body (prt_shade2_body.inc) is shared by k_shade2 (below) and k_shade2d, whose parameter lists are the same
// (Shade2Args)
template <bool EXT, bool I0 = false>
__global__ void __launch_bounds__(kBlock, EXT ? 3 : (I0 ? 4 : 1)) k_shade2(SceneDev S, TraceArgs A, TileMap M, WaveBufs B, uint32_t iter) {
  constexpr bool DEFER = false;
#include "prt_shade2_body.inc"
}

}  // namespace prt
