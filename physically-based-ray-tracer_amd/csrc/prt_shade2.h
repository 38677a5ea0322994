// prt_shade2.h -- what the wavefront pipelines (prt_wave2.hip, prt_defer.hip) share on the device, stated once:
//   shade_miss / shade_hit      the shading of one path segment: every shading kernel (k_shade2, k_shade2d, both
//                               passes of k_shade2m) calls them with its own record index, throughput index and ray
//   shade2_body                 the chunk loop of k_shade2 and k_shade2d around them
//   resolve_segment, vis_mask   the resolve of one segment (the deferred pass's resolve_path; the per-iteration
//                               resolve_item keeps the expressions written out, for speed, and shares vis_mask)
//   pixel_value, finish_path    the end of a path: AA average, gamma, frame write
// and k_miss2 and the light-visibility record's helpers.  A header so that the deferred-resolve forms are instantiated
// in a translation unit of their own (prt_defer.hip).
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

// ---- a segment that misses (:159): the sky radiance (or 0) ends the path, into ne of record e.  rd: the ray's
// direction where the caller keeps it (a register, or the item's entry of rd, then loaded only under kSkybox)
__device__ __forceinline__ V3 miss_radiance(const SceneDev& S, uint32_t fl, const float4& rd) {
  V3 L = v3(0.0f, 0.0f, 0.0f);
  if (fl & kSkybox) {
    const float4 d = rd;
    L = sample_sky_call(S.sky, S.skyw, S.skyh, v3(d.x, d.y, d.z));
  }
  return L;
}
__device__ __forceinline__ void shade_miss(const SceneDev& S, const WaveBufs& B, uint32_t fl, size_t e,
                                           const float4& rd) {
  const V3 L = miss_radiance(S, fl, rd);
  B.ne[e] = make_float4(L.x, L.y, L.z, 0.0f);
}

// ---- misses of P(iter) in a pass of their own (extensions, debug modes), before k_shade2 replaces the ray.  EXT: a
// ray that reaches the area light before any geometry ends there (ne = its MIS-weighted radiance, hit = miss).
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
  shade_miss(S, B, A.flags, item, B.rd[item]);
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

// ---- the light-visibility record (WaveBufs::lvis; prt_wave2.hip's header comment).  An entry is 8 bytes, byte l for
// light l (x: point lights 0-3, y: kLightDir, kLightSpot): 0 unknown, 1 occluded, 2 unoccluded.  Ray k of an item of
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

// ---- a segment that hits: hit attributes, NEE set-up, BRDF sample -> the segment's record and the item's next ray.
//   e          the segment's record (hp / ne / nb / nk / vis): the item, or path x n + item in the merged pipeline
//   ti         its entry of the throughput planes T (EXT: of dro / drd too, which lie alike)
//   ro, rd     the ray, where the caller keeps it: a register, or the item's entries of the ray buffers -- read once
//              on entry, before the next ray overwrites them
//   hh         its hit; kind, nr: the light class drawn for it (nee_kind) and that class's number of shadow rays, > 0
//   q          what the light-visibility record says about the segment's rays (Asked, below)
//   shq        the block's part of the shadow queue
// Returns a ShadedHit.
// Asked: cached = the record answers for this segment (iteration 0 of a kPrimReuse pass, path 1): shade_hit queues the
// rays of `ask` (lvis_split; bit 8k = ray k) itself, in compact slots from s0 on, and the visibility word starts as
// vis0.  Not cached (the default): the rest is 0 and the rays to queue come back in ShadedHit::live
struct Asked {
  bool cached = false;
  uint32_t ask = 0, vis0 = 0, s0 = 0;
  bool rec = false;  // (cached) a primary-surface record form (below): hp is stored only where a ray is queued
};
struct ShadedHit {
  uint32_t rinfo;  // the segment's rinfo bits: status << 16 (kStNeeEnd or kStNeeCont) and kRiEmissive
  uint32_t live;   // (not cached) the light-class shadow rays to queue behind the NEE block (queue_live), bit k = ray k
  bool area_ray;   // (EXT) the area light's shadow ray is stored in ao / ad / na, for the caller to queue
  // the path goes on: ro / rd / info of the item hold the next ray
  __device__ bool cont() const { return ((rinfo >> 16) & 3u) == kStNeeCont; }
};
// The surface of a hit: the hit point and the hit attributes.  shade_hit computes it from the ray and the hit; the
// primary-surface record keeps the one of a fixed path-1 primary hit (surf_store / surf_load)
struct Surface {
  V3 I;
  HitAttr ha;
};
// the emissive term of a hit (:196); all +0 unless the mesh has an emission texture
__device__ __forceinline__ V3 emission_of(const Material& m) {
  return v3(0.0f, 0.0f, 0.0f) + v3(1.0f, 1.0f, 1.0f) * m.emis;
}
// ---- the primary-surface record (SurfBufs, prt_launch.h; prt_surface.hip): entry r, three 16-byte words.
//   n4  hit: N, t with the "emissive" bit in its sign (a hit's t is >= 0);  miss: the sky radiance (or 0), t >= kFar
//   b4  m.base, m.rough           i4  I, m.metal           e4  m.emis, where the emissive bit is set
// The instance's material kind is not kept: the plain pipeline reads none of it behind hit_attributes (which has folded
// a mirror into metal and rough already); only the extensions' shading does, and it has no record.
__device__ __forceinline__ float surf_t(const float4& sn) { return __uint_as_float(__float_as_uint(sn.w) & 0x7FFFFFFFu); }
__device__ __forceinline__ void surf_store(const SurfBufs& R, uint32_t r, const V3 I, const HitAttr& ha, float t) {
  const Material& m = ha.m;
  const V3 em = emission_of(m);
  const bool emissive = (em.x != 0.0f || em.y != 0.0f || em.z != 0.0f) && R.e4;
  R.n4[r] = make_float4(ha.N.x, ha.N.y, ha.N.z,
                        __uint_as_float(__float_as_uint(t) | (emissive ? 0x80000000u : 0u)));
  R.b4[r] = make_float4(m.base.x, m.base.y, m.base.z, m.rough);
  R.i4[r] = make_float4(I.x, I.y, I.z, m.metal);
  if (emissive) R.e4[r] = make_float4(m.emis.x, m.emis.y, m.emis.z, 0.0f);
}
// sn, sb, si: the entry's words as the prefetch loaded them
__device__ __forceinline__ Surface surf_load(const SurfBufs& R, uint32_t r, const float4& sn, const float4& sb,
                                             const float4& si) {
  Surface sf;
  sf.I = v3(si.x, si.y, si.z);
  sf.ha.N = v3(sn.x, sn.y, sn.z);
  sf.ha.m.base = v3(sb.x, sb.y, sb.z);
  sf.ha.m.rough = sb.w;
  sf.ha.m.metal = si.w;
  sf.ha.m.emis = v3(0.0f, 0.0f, 0.0f);
  if (__float_as_uint(sn.w) & 0x80000000u) {
    const float4 e = R.e4[r];
    sf.ha.m.emis = v3(e.x, e.y, e.z);
  }
  sf.ha.kind = kMatTextured;
  return sf;
}
// SURF (the forms under the primary-surface record, k_shade2s): kSurfFill also stores the surface it computed into
// entry r of R; kSurfRead enters behind the attributes, with the surface `in` that surf_load rebuilt from the record
template <bool EXT, int SURF = kSurfNone>
__device__ __forceinline__ ShadedHit shade_hit(const SceneDev& S, const TraceArgs& A, const WaveBufs& B, uint32_t item,
                                               size_t e, size_t ti, const float4& ro, const float4& rd, float4 hh,
                                               int kind, uint32_t nr, uint32_t info, uint32_t& seed, Asked q,
                                               uint32_t* shq, const SurfBufs R = {}, uint32_t r = 0,
                                               const Surface* in = nullptr) {
  const bool cached = q.cached;
  const uint32_t ask = q.ask, vis0 = q.vis0, s0 = q.s0;
  uint32_t live = 0;
  bool area_ray = false;
  const uint32_t fl = A.flags;
  const uint32_t depth = info & 0xFFu, path = (info >> 8) & 1u;
  const float4 o = ro, d = rd;
  const V3 D = v3(d.x, d.y, d.z);
  const uint32_t pk = __float_as_uint(hh.w);
  V3 I;
  HitAttr ha;
  if constexpr (SURF == kSurfRead) {
    I = in->I;
    ha = in->ha;
  } else {
    I = v3(o.x, o.y, o.z) + hh.x * D;                                                        // tiny_bvh.h:586
    ha = hit_attributes(S, hit_inst(S, pk), hit_prim(S, pk), hh.y, hh.z, (fl & kNormalMap) != 0);
  }
  if constexpr (SURF == kSurfFill) surf_store(R, r, I, ha, hh.x);
  const V3 V = -D;
  float4 nk;
  const V3 brdf = nee_lights(S, fl, kind, I, V, ha.N, ha.m, seed, nk, [&](int k, uint32_t light) {
    if (cached && (ask & (1u << (8 * k))))  // compact slots: the asked rays below k come first
      shq[s0 + (uint32_t)__popc(ask & ((1u << (8 * k)) - 1u))] = (light << 29) | (4u * (uint32_t)e + (uint32_t)k);
  });
  // dead rays: counted, not queued; their visibility bytes keep the "occluded" 0 stored below
  if (!cached) live = B.dead ? nee_live(S, fl, kind, nk, brdf, B.dead > 1u) : (1u << nr) - 1u;
  // a shadow ray is queued as (light, visibility index) with the segment's hit point I stored once: the traversal
  // kernel rebuilds it (shadow_of, the only reader: a segment that queues no light-class ray needs none)
  if ((cached && (!q.rec || ask)) || live) B.hp[e] = make_float4(I.x, I.y, I.z, 0.0f);
  uint32_t emissive = 0;
  const V3 em = emission_of(ha.m);                                                           // :196
  if (em.x != 0.0f || em.y != 0.0f || em.z != 0.0f) {  // otherwise em is +0 and the resolve rebuilds it
    B.ne[e] = make_float4(em.x, em.y, em.z, 0.0f);
    emissive = kRiEmissive;
  }
  B.nb[e] = make_float4(brdf.x, brdf.y, brdf.z, 0.0f);
  B.nk[e] = nk;
  B.vis[e] = vis0;
  uint32_t status = kStNeeEnd;
  if constexpr (EXT) {
    // area-light sample (2 draws after the light-class NEE draws) at lit, non-delta, non-dielectric hits
    reinterpret_cast<uint8_t*>(B.vis)[4 * (size_t)B.n + item] = 0;
    if (S.area && (fl & kLighted) && ha.kind != kMatDielectric && !delta_lobe(ha.m)) {
      const float xi1 = random_float(seed), xi2 = random_float(seed);
      Ray sr;
      float tmax;
      V3 fa;
      if (area_nee(area_light(S), I, ha.N, V, ha.m, xi1, xi2, (int)depth == A.bounces - 1, sr, tmax, fa)) {
        area_ray = true;
        B.ao[item] = make_float4(sr.O.x, sr.O.y, sr.O.z, tmax);
        B.ad[item] = make_float4(sr.D.x, sr.D.y, sr.D.z, 0.0f);
        B.na[item] = make_float4(fa.x, fa.y, fa.z, 0.0f);
      }
    }
  }
  if ((int)depth != A.bounces - 1) {                                                         // :329
    if (EXT && ha.kind == kMatDielectric) {                                                  // :331-372
      const Dielectric dl = dielectric_split(I, D, ha.N);
      B.dro[ti] = make_float4(dl.refr.O.x, dl.refr.O.y, dl.refr.O.z, dl.fresnel);
      B.drd[ti] = make_float4(dl.refr.D.x, dl.refr.D.y, dl.refr.D.z, 0.0f);
      B.T[ti] = make_float4(0.0f, 0.0f, 0.0f, kFar);  // w: the continuation is not BRDF-sampled
      const uint32_t bit = 1u << depth, keep = ~(0x01010101u << depth);
      B.dst[item] = (B.dst[item] & keep) | bit | (dl.has_refr ? 0u : (bit << 24));
      status = kStNeeCont;
      B.ro[item] = make_float4(dl.refl.O.x, dl.refl.O.y, dl.refl.O.z, 0.0f);
      B.rd[item] = make_float4(dl.refl.D.x, dl.refl.D.y, dl.refl.D.z, 0.0f);
      B.info[item] = (depth + 1u) | (path << 8);
    } else {
      V3 dir, thr;
      float bp = 2.0f;
      if (sample_bounce(ha.m, V, ha.N, seed, dir, thr, EXT ? &bp : nullptr)) {               // :376-399
        status = kStNeeCont;
        float pdf = 0.0f;
        if constexpr (EXT)  // MIS density of the sampled direction (kFar: delta lobe or no light sampling)
          pdf = (bp > 1.0f || !S.area || !(fl & kLighted)) ? kFar : brdf_pdf(ha.m, ha.N, V, dir, bp);
        B.T[ti] = make_float4(thr.x, thr.y, thr.z, pdf);
        const Ray nr2 = make_ray(I + dir * kEpsilon, dir);                                   // :404
        B.ro[item] = make_float4(nr2.O.x, nr2.O.y, nr2.O.z, 0.0f);
        B.rd[item] = make_float4(nr2.D.x, nr2.D.y, nr2.D.z, 0.0f);
        B.info[item] = (depth + 1u) | (path << 8);
      }
    }
  }
  B.seed[item] = seed;
  return {(status << 16) | emissive, live, area_ray};
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
// The body of k_shade2<EXT, I0> (below) and k_shade2d<I0> (prt_defer.hip), whose parameter lists are the same
// (Shade2Args): the chunk loop, its prefetch and its queue appends around shade_miss / shade_hit.
// EXT (area light, dielectrics): the misses are shaded by k_miss2 / k_resmiss2.
// I0 (plain form): iteration 0 of a pass with pmode kPrimReuse and a light-visibility record (B.lvis), an
// instantiation of its own so that the shading of every other launch carries nothing for it
// DEFER (plain form): a pass with a deferred resolve (prt_defer.hip k_shade2d / k_resolve_pass).  The host hands the
// launch the record plane of its iteration in rinfo / ne / nb / nk / vis / T, so the one index that differs is the
// throughput's: the plane holds one entry per item, not one per depth.
// SURF (I0 forms; prt_surface.hip k_shade2s): kSurfFill stores each item's surface (or its sky radiance) into the
// primary-surface record R as it shades it, kSurfRead shades from the record: its prefetch loads the entry and never
// touches phit, the ShadeTri records, the texels, the sRGB table, the sky or the descriptors.  The stored values are
// the ones the fill form just used, so both forms run the rest of shade_hit on the same bits.
// kSurfInit: kSurfRead without a k_wave_init in front of it.  It walks the pass's items by index as k_wave_init does
// (item_pixel, the `out` entry and rinfo 0 of an entry without a pixel), computes the seed, the jitter and the
// primary ray with k_wave_init's own functions, writes seed, jit, s1 and rinfo itself and counts the items into P(0)'s
// counters; q0, info, ro and rd of the wave init are neither written nor read
template <bool EXT, bool I0, bool DEFER, int SURF = kSurfNone>
__device__ __forceinline__ void shade2_body(const SceneDev& S, const TraceArgs& A, const TileMap& M, const WaveBufs& B,
                                            uint32_t iter, const SurfBufs R = {}, float4* __restrict__ out = nullptr) {
  constexpr bool kRead = SURF == kSurfRead || SURF == kSurfInit;
  static_assert(!(EXT && I0), "the light-visibility record belongs to the plain pipelines");
  static_assert(!(EXT && DEFER), "the deferred resolve belongs to the plain pipeline");
  static_assert(SURF == kSurfNone || I0, "the primary-surface record rides on the light-visibility record");
  const Shade2ArgsPtr args = (Shade2ArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  // fail the call if the Shade2Args layout does not match this compiler's, or the block is not kBlock threads.  The
  // block-size test also makes blockDim.x a constant for the appends below: read anew inside the chunk loop (a vector
  // load of the dispatch's group size) it made the I0 forms wait for their prefetch loads, 2 % of the launch
  if (args->iter != iter || args->B.n != B.n || blockDim.x != kBlock) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(S.diag + 1, 1u);
    return;
  }
  __shared__ uint32_t pref[kNSub + 1];
  __shared__ uint32_t sm[8];
  const uint32_t* q = (iter & 1) ? B.q1 : B.q0;
  uint32_t* qn = (iter & 1) ? B.q0 : B.q1;
  const uint32_t sub = blockIdx.x % kNSub;
  uint32_t* shcnt = qcounter(B.ctr, iter, 1, sub);
  uint32_t* ncnt = qcounter(B.ctr, iter + 1, 0, sub);
  uint32_t* shq = B.shq + (size_t)sub * B.scap;
  uint32_t total_;
  if constexpr (SURF == kSurfInit) total_ = B.n;
  else total_ = load_prefix(B.ctr, iter, 0, pref);
  const uint32_t total = total_;
  const uint32_t fl = A.flags;
  // software pipeline over the grid-stride chunks: the next chunk's item, info, hit and seed are loaded while this
  // chunk's item is shaded
  uint32_t item_n = 0, info_n = 0, seed_n = 0;
  float4 hh_n = make_float4(kFar, 0.0f, 0.0f, 0.0f);
  float4 ro_n = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rd_n = ro_n;  // (plain form: the ray too)
  uint2 lv_n = make_uint2(0u, 0u);                                 // (I0: the entry's light-visibility bytes)
  float4 sn_n = ro_n, sb_n = ro_n, si_n = ro_n;                    // (kSurfRead: the entry's three record words)
  auto prefetch = [&](uint32_t cc) {
    const uint32_t gg = cc * kBlock + threadIdx.x;
    if (gg < total) {
      if constexpr (SURF == kSurfInit) {  // item gg itself: the record and the light visibility of its entry
        const uint32_t r = (B.base + gg) % B.pitems;
        item_n = gg;
        sn_n = R.n4[r]; sb_n = R.b4[r]; si_n = R.i4[r];
        lv_n = B.lvis[r];
        return;
      }
      item_n = q[map_slot(pref, gg, B.qcap)];
      info_n = B.info[item_n];
      if constexpr (SURF == kSurfRead) {  // the record in place of the hit; of the ray, the direction alone
        const uint32_t r = (B.base + item_n) % B.pitems;
        sn_n = R.n4[r]; sb_n = R.b4[r]; si_n = R.i4[r];
        lv_n = B.lvis[r];
        seed_n = B.seed[item_n];
        rd_n = B.rd[item_n];
        return;
      }
      // iteration 0 with primary-hit reuse (plain form only): the hit of the pixel's fixed path-1 primary ray
      hh_n = (!EXT && iter == 0 && B.pmode != kPrimTrace) ? B.phit[(B.base + item_n) % B.pitems] : B.hit[item_n];
      if constexpr (I0) lv_n = B.lvis[(B.base + item_n) % B.pitems];
      seed_n = B.seed[item_n];
      if (!EXT) { ro_n = B.ro[item_n]; rd_n = B.rd[item_n]; }
    }
  };
  prefetch(blockIdx.x);
  uint32_t init_count = 0;  // (kSurfInit) the items this wave found a pixel for
  for (uint32_t c = blockIdx.x; c * kBlock < total; c += gridDim.x) {
    const float4 ro_c = ro_n, rd_c = rd_n;
    // The scene and buffer descriptors are read from the kernarg segment inside each chunk (scalar loads, scalar
    // cache) instead of being held in SGPRs across the loop: their ~90 live words spilled to VGPR lanes (378
    // v_readlane in the loop) when hoisted.  The empty asm hides the pointer's loop invariance.
    Shade2ArgsPtr ka = args;
    asm volatile("" : "+s"(ka));
    const SceneDev& Sc = *(const SceneDev*)&ka->S;
    const WaveBufs& Bc = *(const WaveBufs*)&ka->B;
    const uint32_t g = c * kBlock + threadIdx.x;
    uint32_t item = 0, info = 0, seed = 0, nr = 0;
    Asked q;  // (I0) the rays to queue, the visibility word's initial value, their slots
    q.cached = I0;
    int kind = 0;
    float4 hh = make_float4(kFar, 0.0f, 0.0f, 0.0f);
    // (kSurfInit) k_wave_init's work for item g: its pixel, seed, jitter and primary ray direction
    bool init_valid = false;
    uint32_t init_seed_ = 0;
    float4 init_rd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (SURF == kSurfInit) {
      if (g < total) {
        const uint32_t gi = Bc.base + g;  // item index within the call
        const uint32_t f = gi / M.items, r = gi % M.items;
        int32_t x, y;
        init_valid = item_pixel(M, r, x, y);
        if (init_valid) {
          const uint32_t p = (uint32_t)(y * A.W + x);
          init_seed_ = init_seed(A.seed + p + (uint32_t)A.W * (uint32_t)A.H * (A.frame_index + f));
          float jx = 0.0f, jy = 0.0f;
          if (A.flags & kAA) { jx = random_float(init_seed_); jy = random_float(init_seed_); }  // :61
          const Ray r1 = primary_ray(Sc, (float)x, (float)y, A.W, A.H);
          init_rd = make_float4(r1.D.x, r1.D.y, r1.D.z, 0.0f);
          Bc.jit[g] = make_float2(jx, jy);
        } else {
          out[g] = make_float4(0.0f, 0.0f, 0.0f, kFar);
          Bc.rinfo[g] = 0u;
        }
      }
      init_count += (uint32_t)__popcll(__ballot(init_valid));
    }
    const float4 rd_s = SURF == kSurfInit ? init_rd : rd_c;
    const bool active = SURF == kSurfInit ? init_valid : g < total;
    const float4 sn = sn_n, sb = sb_n, si = si_n;
    if (active) {
      item = item_n; info = info_n; hh = hh_n;
      if constexpr (kRead) hh.x = surf_t(sn);
      const uint32_t sd = SURF == kSurfInit ? init_seed_ : seed_n;
      const uint2 lv = lv_n;
      if constexpr (SURF == kSurfInit) Bc.s1[item] = make_float4(0.0f, 0.0f, 0.0f, hh.x);
      else if ((info & 0x1FFu) == 0) Bc.s1[item].w = hh.x;                                   // r1.hit.t
      if constexpr (kRead) {
        if (hh.x >= kFar) {
          Bc.ne[item] = make_float4(sn.x, sn.y, sn.z, 0.0f);
          if constexpr (SURF == kSurfInit) Bc.seed[item] = sd;  // (a hit's seed is stored by shade_hit)
        }
      } else if constexpr (SURF == kSurfFill) {
        if (hh.x >= kFar) {
          const V3 L = miss_radiance(Sc, fl, rd_c);
          Bc.ne[item] = make_float4(L.x, L.y, L.z, 0.0f);
          R.n4[(Bc.base + item) % Bc.pitems] = make_float4(L.x, L.y, L.z, hh.x);
        }
      } else {
        if (!EXT && hh.x >= kFar) shade_miss(Sc, Bc, fl, item, rd_c);
      }
      if (hh.x < kFar) {
        seed = sd;
        kind = nee_kind(fl, seed);                                                           // :198-214
        nr = (uint32_t)nee_rays(kind);
        if constexpr (I0) lvis_split(lv, kind, q.ask, q.vis0);
      }
    }
    prefetch(c + gridDim.x);
    // the block's shadow-ray slots, one atomic (I0: of the rays whose answer is not known yet; the known ones are
    // counted, not queued).  Every other form appends behind the NEE block, once it knows which rays are live
    if constexpr (I0)
      q.s0 = block_append_skip(shcnt, (uint32_t)__popc(q.ask), qcounter(B.ctr, B.lslot, 1, sub), lvis_total(S),
                               nr - (uint32_t)__popc(q.ask), sm);
    const uint32_t depth = info & 0xFFu, path = (info >> 8) & 1u;
    ShadedHit h = {kStMiss << 16, 0u, false};
    if constexpr (SURF != kSurfNone) {
      q.rec = true;
      if (nr) {
        const uint32_t r = (Bc.base + item) % Bc.pitems;
        Surface sf;
        if constexpr (kRead) sf = surf_load(R, r, sn, sb, si);
        h = shade_hit<EXT, kRead ? kSurfRead : SURF>(Sc, A, Bc, item, item,
                                                     DEFER ? (size_t)item : (size_t)depth * Bc.n + item, ro_c, rd_s, hh,
                                                     kind, nr, info, seed, q, shq, R, r, &sf);
      }
    } else if (nr)
      h = shade_hit<EXT>(Sc, A, Bc, item, item, DEFER ? (size_t)item : (size_t)depth * Bc.n + item,
                         EXT ? Bc.ro[item] : ro_c, EXT ? Bc.rd[item] : rd_c, hh, kind, nr, info, seed, q, shq);
    if constexpr (!I0) {  // only the mask lived across the NEE block: the live rays' slots, the dead ones counted
      const uint32_t nl = (uint32_t)__popc(h.live);
      const uint32_t s0 = block_append_skip(shcnt, nl, qcounter(B.ctr, B.lslot, 1, sub), dead_total(S), nr - nl, sm);
      queue_live(shq, s0, kind, h.live, item);
    }
    if constexpr (EXT) {  // the area-light shadow rays of the block, one more append
      const uint32_t a0 = block_append(shcnt, h.area_ray ? 1u : 0u, sm);
      if (h.area_ray) shq[a0] = (kLightArea << 29) | item;
    }
    bool next = h.cont();
    if (active) {
      if (!next) {
        if (EXT && Sc.has_diel) next = diel_next(Bc, item, depth, path);
        if (!next) next = start_path2(Sc, A, M, Bc, item, path);
      }
      Bc.rinfo[item] = depth | (path << 8) | h.rinfo | ((uint32_t)kind << 20) | (next ? kRiQueued : 0u) |
                       (EXT ? 0u : kResFresh) | ((I0 && q.ask) ? kRiLearn : 0u);
    }
    const uint32_t slot = block_append(ncnt, next ? 1u : 0u, sm);
    if (next) qn[sub * Bc.qcap + slot] = item;
  }
  // (kSurfInit) P(0)'s count, which k_wave_init's appends would have produced: the ray totals are the queue counters
  if constexpr (SURF == kSurfInit) {
    if (lane_id() == 0 && init_count) atomicAdd(qcounter(B.ctr, 0, 0, sub), init_count);
  }
}
// EXT: held to 3 waves/SIMD (168 VGPRs, no spills; unbounded it took 175 and ran 2 waves: C5 frame 135.7 ->
// 132.4 ms).  The plain form runs 4 waves at its natural 125 VGPRs (forcing 5 spilled and was 2 % slower).
template <bool EXT, bool I0 = false>
__global__ void __launch_bounds__(kBlock, EXT ? 3 : (I0 ? 4 : 1)) k_shade2(SceneDev S, TraceArgs A, TileMap M, WaveBufs B, uint32_t iter) {
  shade2_body<EXT, I0, false>(S, A, M, B, iter);
}

// ---- the resolve of one segment.  The four visibility bytes of a segment's light-class rays (1 = unoccluded,
// written by k_trace2) -> bit k = ray k
__device__ __forceinline__ uint32_t vis_mask(uint32_t vw) {
  return ((vw & 0xFFu) ? 1u : 0u) | ((vw & 0xFF00u) ? 2u : 0u) | ((vw & 0xFF0000u) ? 4u : 0u) |
         ((vw & 0xFF000000u) ? 8u : 0u);
}
// one segment's value from its record e (ri = its rinfo): ne (a miss's or a debug mode's end value, or a hit's
// emissive term, stored only where kRiEmissive) through nee_resolve.  (resolve_item keeps a copy: prt_wave2.hip)
__device__ __forceinline__ V3 resolve_segment(const SceneDev& S, const WaveBufs& B, size_t e, uint32_t ri, uint32_t fl) {
  const uint32_t status = (ri >> 16) & 3u, kind = (ri >> 20) & 3u;
  const bool nee = status == kStNeeEnd || status == kStNeeCont;
  const float4 ne = (!nee || (ri & kRiEmissive)) ? B.ne[e] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  V3 L = v3(ne.x, ne.y, ne.z);
  if (nee) {
    const float4 nb = B.nb[e], nk = B.nk[e];
    L = nee_resolve(S, (int)kind, vis_mask(B.vis[e]), L, v3(nb.x, nb.y, nb.z), nk, fl);
  }
  return L;
}

// ---- the end of a path.  A pixel's value from its two paths' radiances (a is not used without AA)
__device__ __forceinline__ V3 pixel_value(V3 a, V3 b, uint32_t fl) {
  V3 res = (fl & kAA) ? 0.5f * (a + b) : b;                                                  // :65
  if (fl & kGamma) res = v3(sqrtf(res.x), sqrtf(res.y), sqrtf(res.z));                      // :73-79
  return res;
}
// a path of `item` ended with radiance L: path 1 under AA keeps it in s1 (path 2 follows); otherwise the frame write
__device__ __forceinline__ void finish_path(const WaveBufs& B, uint32_t item, uint32_t path, V3 L, uint32_t fl,
                                            float4* __restrict__ out) {
  const float4 s1 = B.s1[item];
  if (path == 0 && (fl & kAA)) {
    B.s1[item] = make_float4(L.x, L.y, L.z, s1.w);
  } else {
    const V3 res = pixel_value(v3(s1.x, s1.y, s1.z), L, fl);
    out[item] = make_float4(res.x, res.y, res.z, s1.w);
  }
}

}  // namespace prt
