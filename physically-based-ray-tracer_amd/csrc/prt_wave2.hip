// prt_wave2.hip -- the merged-trace wavefront path tracer for gfx950.
//
// The reference's recursive per-pixel Renderer::Trace (Core/Renderer.cpp:150-406) is re-cut into stages over
// queues of live work items.  One item = one pixel x reference frame; it traces its AA path pair
// sequentially, so the canonical RNG stream of SURVEY Appendix B is preserved.  All per-item state is SoA in
// HBM.  Queues are split into kNSub sub-queues, each with its own counter on its own 128-B line; appends are
// block-aggregated (one atomic per block), consumers read the kNSub counts into an LDS prefix table.
//
// Every random number of a path is drawn in the shading stage, so the shading
// of iteration i already knows the ray of iteration i+1 (the sampled bounce, or the AA path-2 primary
// ray when path 1 ends) and queues it at once.  The closest-hit rays of iteration i+1 and the shadow
// rays of iteration i are then traced by ONE persistent launch, and the NEE resolve of iteration i
// (which needs those shadow results) runs after it:
//
//   k_wave_init                                   P(0) = primary rays r1
//   for i = 0 .. iters:
//     k_trace2(i)    closest hits of P(i)  +  any hits of S(i-1)         (one launch, mixed lanes; P(0): the
//                    primary-hit reuse below)
//     k_res2d(i)     the items of P(i-1) (rinfo kRiFresh), walked in index order: NEE result of iteration i-1,
//                    (result, throughput) stack, path end, frame write.  With the extensions or a debug render mode
//                    k_resmiss2(i) walks the queue P(i-1) instead and also shades, for the items k_shade2(i-1)
//                    queued into P(i) (a subset of P(i-1)), this iteration's misses (i = 0: k_miss2 over P(0))
//     k_shade2(i)    the sky radiance of the misses (no extensions), hit attributes, NEE set-up -> S(i), BRDF
//                    sample or path-2 start -> P(i+1)
// Which instantiation each stage of launch i is, for each of the five pipelines, is wave_schedule (prt_plan.h); which
// pipeline a call takes is plan_render there.  launch_wave2_iter below only launches what they name.
// What the pipelines compute per path segment is stated once, in prt_shade2.h: every shading kernel (k_shade2 and
// k_shade2d through shade2_body, both passes of k_shade2m) shades a segment with shade_miss / shade_hit, and every
// resolve ends a path with pixel_value.  The kernels differ in their chunk loops, prefetches and queue appends, and in
// the record index, throughput index and ray they hand those functions.  A segment's resolve stands twice, the one
// exception: resolve_segment for k_resolve_pass, and written out in resolve_item below, for speed (reason there).
//
// Hazards (all kernels on one stream): P(i+1) reuses P(i-1)'s buffer after the resolve (i) read it;
// S(i) reuses S(i-1)'s buffer after k_trace2(i) read it; the resolve (i) reads ne/nb/nk/vis/R/T of an item for
// iteration i-1 before it (misses) or k_shade2(i) (hits) overwrites them; rinfo keeps iteration i-1's status
// (and whether the item was queued) while info already holds the state of the queued next ray.
//
// Deferred resolve (Pipeline::PlainDeferred; prt_defer.hip).  Nothing downstream needs a path's radiance before
// k_accumulate, and an item is shaded in consecutive iterations from 0, so a pass whose record planes fit the budget
// (prt_plan.h plan_render) launches no k_res2d: the host hands k_shade2d(i) plane i of rinfo / ne / nb / nk / vis / T
// (throughput per iteration, not per depth) and k_trace2(i) the vis of plane i - 1, and one
// k_resolve_pass behind the last traversal launch walks every item's planes bottom-up.  R is not used; the hazards on
// ne / nb / nk / vis / T above are gone with the shared record; k_trace2 is the same kernel with another pointer.
//
// Primary-hit reuse (the plain and merged pipelines; WaveBufs::phit / pmode).  Path 1 of
// a pixel starts at the pixel centre (only path 2 is jittered, :61), so its primary ray is the same in every
// reference frame of a call and in every later call while camera, tile map, scene and instances stay put.  Its
// hit is kept in phit, one record per tile-map entry, and P(0) itself is never traced:
//   kPrimDense  (the host's stamp of phit is stale) k_trace2(0) traces the entries of the pass's first frame in
//               index order, once each, and writes phit; k_wave_init gave the padding entries a null ray
//   kPrimReuse  (stamp current) k_trace2(0) traces only the merged pipeline's path-2 primaries; the plain
//               pipeline does not launch it
// and the shading of iteration 0 takes an item's hit from phit[(base + item) % pitems] instead of hit[item].
// k_wave_init still queues every item into P(0) (the shading consumes it; the ray totals are the queue counters);
// hit is written and read from iteration 1 on.  Writer of phit: k_trace2(0) of a dense pass; readers: the shading
// kernels at iteration 0 of that pass and of every later pass and call on the same wavefront state.  Each state
// (the context's own, one per further frame in flight) owns its copy and its stamp and runs its calls on one
// stream at a time, so writer and readers are ordered by that stream and chains never share a copy.
//
// Light-visibility record (WaveBufs::lvis, next to phit and indexed like it; the same pipelines).  The shading of
// iteration 0 builds every NEE shadow ray of path 1 from the fixed primary hit point and a light position alone
// (light_ray); the RNG only picks which light class an item asks about.  So for a tile-map entry and a light the
// any-hit answer of S(0) repeats while phit and the light positions stay put.  The record holds it: 8 bytes per
// entry, byte l for light l (0-3 point, kLightDir, kLightSpot): 0 unknown, 1 occluded, 2 unoccluded.  Only passes
// with pmode kPrimReuse use and fill it (B.lvis is null otherwise: a dense pass, or a camera that moves every call,
// pays nothing), through instantiations of their own, so the kernels of every other launch are what they were:
//   k_shade2<false, true> / k_shade2m<true> (iteration 0; the merged form's pass 0): reads the entry in the
//               prefetch; queues, in compact slots, only the rays of the item's light class whose byte is 0; starts
//               vis[item] with byte k = 1 for the rays known unoccluded; sets kRiLearn in rinfo if it queued any.
//               nk, nb, hp and every RNG draw stay as they are.  The rays not queued are counted into the shadow
//               counter of iteration iters + 1 (B.lslot), which no kernel prefixes and k_accumulate, read_stats and
//               the multi-pass carry sum, so the ray totals still count every shadow ray the reference casts; and
//               into the context's running total (prt_shadow_reuse)
//   k_trace2(1) traces the shorter S(0); it is not changed
//   k_res2d<true> / k_res2md<true> (launch 1; slot 0): for a kRiLearn item, writes what vis[item] now says into the
//               bytes of the item's light class (lvis_learn)
// There is no extra pass and no recomputed hit point: the record is learned from the very rays the frames trace.
// Writer: the resolve of launch 1; reader: the shading of iteration 0 of a later pass or call on the same state (all
// frames of a pass shade before its resolve runs, so a pass never reads what it writes).  Two frames of a pixel may
// store the same bytes in one launch, always with the same values (the pattern of vis8).  Each wavefront state owns
// its record; the host clears it (hipMemsetAsync on the state's stream, before k_wave_init) when a dense pass has
// rewritten phit since it was learned or the light positions differ (prt_api_render.cpp enqueue_render_body).
//
// Dead shadow rays (every shading form but the two under the record above; B.dead, the PRT_DEAD_SHADOW level).  A
// light-class shadow ray is dead when its visibility answer is multiplied by exactly zero: PRT_FLAG_LIGHTED is off,
// or every channel of nee_contrib compares equal to zero (prt_path.h nee_live: the cosine clamped to 0, a hit outside
// the spot's cone, a black light), or (level 2) the item's one BRDF value is zero in every channel while every ray's
// contribution is bounded: the shading normal faces away from the viewer, or from the light the BRDF was evaluated for
// (the point-light class multiplies all four rays by the BRDF of the one drawn light), so every ray of the item is
// moot.  The reference traces such rays; their answer cannot change a bit of the result.  Levels (read per call,
// wave-uniform): PRT_DEAD_SHADOW=0 traces everything, 1 applies the contribution rule alone, unset or anything else
// applies both.
// The shading runs its NEE block first and appends the block's shadow-ray slots behind it: only the live rays are
// queued, in compact slots, their entries rebuilt from the item's light class and its live mask (queue_live); the
// dead ones are counted into the shadow counter of iteration iters + 1 (B.lslot, as the rays the record answers) and
// into the context's running total (prt_shadow_dead), and their visibility bytes keep the "occluded" 0 the shading
// stores, so the resolve kernels and k_trace2 are what they were.  An item with no live ray stores no hp.  Nothing is
// kept between calls: deadness depends on the spot direction, the colours and the flags, which do not invalidate
// the record, and so the rays under the record (iteration 0 of a kPrimReuse pass) are asked, learned and counted as
// before.  The area light's ray (EXT) is queued as ever.
#include <cstdio>

#include "prt_launch.h"
#include "prt_path.h"
#include "prt_persist.h"
#include "prt_queue.h"

namespace prt {

#ifdef PRT_LANE_STATS  // diagnostic build: prt_persist.h lane counters, one 32-counter row per traversal launch
__device__ unsigned long long g_lane_stats[(kMaxIters + 2) * 32];
void lane_stats_dump() {
  static unsigned long long h[(kMaxIters + 2) * 32];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lane_stats), sizeof(h)) != hipSuccess) return;
  for (int i = 0; i < kMaxIters + 2; i++) {
    const unsigned long long* r = h + 32 * i;
    if (!r[31]) continue;
    std::fprintf(stderr, "prt: lanestats %d", i);
    for (int k = 0; k < 32; k++) std::fprintf(stderr, " %llu", r[k]);
    std::fprintf(stderr, "\n");
  }
  static const unsigned long long z[(kMaxIters + 2) * 32] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lane_stats), z, sizeof(z));
}
#endif

// the merged pipeline's queue of path-2 primaries: the counters of iteration iters + 1 (kind 0), never a path queue
__device__ __forceinline__ uint32_t q2_iter(const TraceArgs& A) { return 2u * (uint32_t)A.bounces; }

// ---- init: items -> primary rays, appended to queue 0 (sub-queue = block % kNSub).  Merged pipeline (B.merge):
// the AA path-2 primary ray too (its jitter is drawn here, :61), into ro2 / rd2 and the path-2 queue Q2 (shq)
__global__ void __launch_bounds__(kBlock) k_wave_init(SceneDev S, TraceArgs A, TileMap M, WaveBufs B,
                                                      float4* __restrict__ out) {
  __shared__ uint32_t sm[8];
  const uint32_t sub = blockIdx.x % kNSub;
  uint32_t* cnt = qcounter(B.ctr, 0, 0, sub);
  uint32_t* cnt2 = qcounter(B.ctr, q2_iter(A), 0, sub);
  for (uint32_t c = blockIdx.x; c * kBlock < B.n; c += gridDim.x) {
    const uint32_t i = c * kBlock + threadIdx.x;
    bool enq = false;
    if (i < B.n) {
      const uint32_t gi = B.base + i;  // item index within the call (batches cover consecutive ranges)
      const uint32_t f = gi / M.items, r = gi % M.items;
      int32_t x, y;
      const bool valid = item_pixel(M, r, x, y);
      if (valid && A.bounces > 0) {
        const uint32_t p = (uint32_t)(y * A.W + x);
        uint32_t seed = init_seed(A.seed + p + (uint32_t)A.W * (uint32_t)A.H * (A.frame_index + f));
        float jx = 0.0f, jy = 0.0f;
        if (A.flags & kAA) { jx = random_float(seed); jy = random_float(seed); }         // :61
        const Ray r1 = primary_ray(S, (float)x, (float)y, A.W, A.H);
        B.seed[i] = seed;
        B.jit[i] = make_float2(jx, jy);
        B.ro[i] = make_float4(r1.O.x, r1.O.y, r1.O.z, 0.0f);
        B.rd[i] = make_float4(r1.D.x, r1.D.y, r1.D.z, 0.0f);
        B.info[i] = 0u;
        B.s1[i] = make_float4(0.0f, 0.0f, 0.0f, kFar);
        if (B.merge) {
          const Ray r2 = primary_ray(S, (float)x + jx, (float)y + jy, A.W, A.H);
          B.ro2[i] = make_float4(r2.O.x, r2.O.y, r2.O.z, 0.0f);
          B.rd2[i] = make_float4(r2.D.x, r2.D.y, r2.D.z, 0.0f);
          B.rinfo[B.n + i] = 0u;
        }
        B.rinfo[i] = 0u;
        enq = true;
      } else {
        out[i] = make_float4(0.0f, 0.0f, 0.0f, kFar);  // bounces == 0: Trace returns 0, t1 stays BVH_FAR
        // dense primary pass: a padding entry of the tile map (no pixel) holds the null ray (rd.w < 0), which
        // k_trace2 turns into a query that ends at once and writes nothing
        if (B.pmode == kPrimDense && gi < B.pitems) {
          B.ro[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          B.rd[i] = make_float4(0.0f, 0.0f, 1.0f, -1.0f);
        }
        if (B.merge) B.rinfo[B.n + i] = 0u;
        B.rinfo[i] = 0u;
      }
    }
    const uint32_t slot = block_append(cnt, enq ? 1u : 0u, sm);
    if (enq) B.q0[sub * B.qcap + slot] = i;
    if (B.merge) {
      const uint32_t s2 = block_append(cnt2, enq ? 1u : 0u, sm);
      if (enq) B.shq[sub * B.scap + s2] = i;
    }
  }
}

// ---- a shadow-queue entry (light << 29 | index) -> its world ray: rebuilt by light_ray from the item's hit point
// (hp, one per item for its up to four light-class rays) exactly as the shading kernel's NEE built it; the area
// light's rays (EXT, light kLightArea, index = item) are stored whole in ao / ad
constexpr uint32_t kShIndexMask = (1u << 29) - 1u;
__device__ __forceinline__ void shadow_of(const SceneDev& S, const WaveBufs& B, uint32_t code, V3& O, V3& D,
                                          float& tmax) {
  const uint32_t light = code >> 29;
  if (light == kLightArea) {
    const float4 o = B.ao[code & kShIndexMask], d = B.ad[code & kShIndexMask];
    O = v3(o.x, o.y, o.z);
    D = v3(d.x, d.y, d.z);
    tmax = o.w;
    return;
  }
  const float4 I = B.hp[(code & kShIndexMask) >> 2];
  Ray r;
  V3 L;
  float dl;
  light_ray(S, light, v3(I.x, I.y, I.z), r, tmax, L, dl);
  O = r.O;
  D = r.D;
}
// the visibility byte of a shadow-queue entry: 4 x item + k, or 4n + item for the area light's ray
__device__ __forceinline__ uint32_t shadow_vis(const WaveBufs& B, uint32_t code) {
  return (code >> 29) == kLightArea ? 4u * B.n + (code & kShIndexMask) : (code & kShIndexMask);
}

// ---- one traversal launch: closest hits of P(iter) (iter < iters) + any hits of S(iter - 1) (iter > 0)
// DENSE: the dense primary pass (iteration 0 of a pass with pmode kPrimDense), an instantiation of its own so
// that the loop of every other launch carries no state for it
template <int REFILL, int STACK, int WAVES, int TAILN, bool TLAS, bool SPILL = false, bool DENSE = false>
__global__ void __launch_bounds__(64, WAVES) k_trace2(SceneDev S, WaveBufs B, uint32_t iter, uint32_t iters) {
  __shared__ uint32_t lds_stack[2 * STACK * 64];
  __shared__ uint32_t prefP[kNSub + 1], prefS[kNSub + 1];
  __shared__ uint32_t tail_lds[tail_lds_words(TAILN)];
  uint8_t* vis8 = reinterpret_cast<uint8_t*>(B.vis);
  const uint32_t* q = (iter & 1) ? B.q1 : B.q0;
  // iteration 0 with primary-hit reuse: P(0) is not traced.  Dense pass: the first segment is the pitems entries
  // of the pass's first frame in index order (slot g = item g = record g; base is 0), closest hits -> phit;
  // kPrimReuse: phit is current and the segment is empty
  constexpr bool dense = DENSE;
  const uint32_t nP = DENSE ? B.pitems
                            : (iter < iters && !(iter == 0 && B.pmode == kPrimReuse) ? load_prefix(B.ctr, iter, 0, prefP)
                                                                                     : 0u);
  // merged pipeline, iteration 0: the second segment is the path-2 primaries (Q2, in shq; closest hits -> hit2)
  const bool q2 = iter == 0 && B.merge;
  const uint32_t nS = iter > 0 ? load_prefix(B.ctr, iter - 1, 1, prefS)
                               : (q2 ? load_prefix(B.ctr, iters + 1, 0, prefS) : 0u);
  const uint32_t total = nP + nS;
  if (blockIdx.x * 64u >= total) return;
  uint32_t* fctr = fetch_counters(B.ctr, iter, 0);
  uint32_t* dflag = fetch_counters(B.ctr, iter, 1);  // set once some wave found the queue empty (cleared per call)
  uint32_t part = xcc_id();
  // timeline diagnostic (s_memrealtime, one record per wave: start, first empty fetch, exit)
  unsigned long long* tl = B.tl ? B.tl + ((size_t)iter * kTlWaves + blockIdx.x) * 4 : nullptr;
  bool seen_drain = false;
  if (tl && threadIdx.x == 0) tl[0] = __builtin_amdgcn_s_memrealtime();
  trav8_persistent<2, STACK, REFILL, TAILN, TLAS, SPILL>(
      S, lds_stack + threadIdx.x,
      [&](uint32_t* base, uint32_t want) {
        const uint32_t got = fetch_some(fctr, total, part, base, want);
#ifdef PRT_DRAIN_POLL  // A/B: the first empty fetch of a wave tells the other waves
        if (got == 0 && !seen_drain && threadIdx.x == 0)
          __hip_atomic_store(dflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        if (tl && got == 0 && !seen_drain) {
          seen_drain = true;
          if (threadIdx.x == 0) tl[1] = __builtin_amdgcn_s_memrealtime();
        }
        return got;
      },
      [&](uint32_t g, V3& O, V3& D, float& tmax, bool& any) -> uint32_t {
        float4 o, d;
        uint32_t h;
        if (g < nP) {
          h = dense ? g : q[map_slot(prefP, g, B.qcap)];
          o = B.ro[h];
          d = B.rd[h];
          // (dense: k_wave_init's null ray of a padding entry; no box is entered at a negative limit)
          tmax = (dense && d.w < 0.0f) ? -1.0f : kFar;
          any = false;
        } else if (q2) {  // a path-2 primary ray: handle = item | 1 << 31
          h = B.shq[map_slot(prefS, g - nP, B.scap)];
          o = B.ro2[h];
          d = B.rd2[h];
          tmax = kFar;
          any = false;
          h |= 0x80000000u;
        } else {
          h = map_slot(prefS, g - nP, B.scap);
          any = true;
          shadow_of(S, B, B.shq[h], O, D, tmax);
          return h;
        }
        O = v3(o.x, o.y, o.z);
        D = v3(d.x, d.y, d.z);
        return h;
      },
      [&](uint32_t h, bool any, V3& O, V3& D) {
        if (any) {
          float tmax;
          shadow_of(S, B, B.shq[h], O, D, tmax);
          return;
        }
        const bool p2 = (h & 0x80000000u) != 0u;
        const float4 o = p2 ? B.ro2[h & 0x7FFFFFFFu] : B.ro[h], d = p2 ? B.rd2[h & 0x7FFFFFFFu] : B.rd[h];
        O = v3(o.x, o.y, o.z);
        D = v3(d.x, d.y, d.z);
      },
      [&](uint32_t h, const Hit& hit, bool any, bool occluded) {
        if (any) {
          if (!occluded) vis8[shadow_vis(B, B.shq[h])] = 1;
        } else {
          const float4 rec = make_float4(hit.t, hit.u, hit.v, __uint_as_float(pack_hit(S, hit.prim, hit.inst)));
          if (h & 0x80000000u) B.hit2[h & 0x7FFFFFFFu] = rec;
          else if (!dense) B.hit[h] = rec;
          else if (hit.t >= 0.0f) B.phit[h] = rec;  // (a padding entry's null query keeps t = -1)
        }
      },
      [&]() -> bool { return __hip_atomic_load(dflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u; },
#ifdef PRT_LANE_STATS
      B.coop_tail ? tail_lds : nullptr, g_lane_stats + 32 * iter);
#else
      B.coop_tail ? tail_lds : nullptr, tl ? tl + 3 : nullptr);
#endif
  if (tl && threadIdx.x == 0) tl[2] = __builtin_amdgcn_s_memrealtime();
}

}  // namespace prt
#include "prt_shade2.h"  // k_miss2, k_shade2; the shading and the resolve of one segment, the end of a path
namespace prt {

// ---- merged pipeline (B.merge: AA, render mode 0, no extensions).  Shading of P(iter) by k_shade2<false>'s
// shade_miss / shade_hit, each path's records (hit point, NEE record, status, (result, throughput) stack) in its own
// slot (slot = path, at slot * n + item), and where path 1 ends its item shades path 2's first segment at once (pass
// 1: the same two functions on slot 1, with the ray from ro2 / rd2), from the primary hit
// k_trace2(0) traced next to path 1's: the RNG stream continues from path 1's last draw exactly as if path 2's
// primary ray had been traced after path 1 ended, so the result is the same bit for bit and
// a frame needs one wavefront iteration (a traversal, a shading and a resolve launch) fewer.
// I0: iteration 0 of a pass with pmode kPrimReuse and a light-visibility record, as k_shade2's; pass 0 of every
// item is then path 1 at depth 0 (pass 1, path 2's first segment, asks for all its rays as ever)
template <bool I0>
__global__ void __launch_bounds__(kBlock, I0 ? 4 : 1) k_shade2m(SceneDev S, TraceArgs A, TileMap M, WaveBufs B, uint32_t iter) {
  const Shade2ArgsPtr args = (Shade2ArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  // the Shade2Args layout does not match this compiler's, or the block is not kBlock threads (shade2_body): fail
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
  const uint32_t total = load_prefix(B.ctr, iter, 0, pref);
  const uint32_t fl = A.flags;
  const uint32_t levels = (uint32_t)max(1, A.bounces - 1);
  uint32_t item_n = 0, info_n = 0, seed_n = 0;
  float4 hh_n = make_float4(kFar, 0.0f, 0.0f, 0.0f);
  uint2 lv_n = make_uint2(0u, 0u);
  auto prefetch = [&](uint32_t cc) {
    const uint32_t gg = cc * kBlock + threadIdx.x;
    if (gg < total) {
      item_n = q[map_slot(pref, gg, B.qcap)];
      info_n = B.info[item_n];
      // iteration 0 with primary-hit reuse: every item of P(0) is path 1 at depth 0, its hit is in phit
      hh_n = (iter == 0 && B.pmode != kPrimTrace) ? B.phit[(B.base + item_n) % B.pitems] : B.hit[item_n];
      if constexpr (I0) lv_n = B.lvis[(B.base + item_n) % B.pitems];
      seed_n = B.seed[item_n];
    }
  };
  prefetch(blockIdx.x);
  for (uint32_t c = blockIdx.x; c * kBlock < total; c += gridDim.x) {
    Shade2ArgsPtr ka = args;  // descriptors from the kernarg segment per chunk (shade2_body)
    asm volatile("" : "+s"(ka));
    const SceneDev& Sc = *(const SceneDev*)&ka->S;
    const WaveBufs& Bc = *(const WaveBufs*)&ka->B;
    const uint32_t g = c * kBlock + threadIdx.x;
    const bool active = g < total;
    uint32_t item = 0, info = 0, seed = 0;
    float4 hh = make_float4(kFar, 0.0f, 0.0f, 0.0f);
    if (active) { item = item_n; info = info_n; hh = hh_n; seed = seed_n; }
    const uint2 lv = lv_n;
    prefetch(c + gridDim.x);
    bool next = false, need2 = false;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
      const bool act = pass == 0 ? active : need2;
      if (pass == 1 && act) { info = 1u << 8; hh = Bc.hit2[item]; }          // path 2, depth 0: its primary hit
      const uint32_t depth = info & 0xFFu, path = (info >> 8) & 1u;
      const size_t sn = (size_t)path * Bc.n + item;                         // this path's record slot
      const float4* rop = pass ? Bc.ro2 : Bc.ro;
      const float4* rdp = pass ? Bc.rd2 : Bc.rd;
      int kind = 0;
      uint32_t nr = 0;
      Asked q;  // (I0, pass 0) the rays to queue, the visibility word's start, their slots
      q.cached = I0 && pass == 0;
      if (act) {
        if ((info & 0x1FFu) == 0) Bc.s1[item].w = hh.x;                                     // r1.hit.t
        if (hh.x >= kFar) {
          shade_miss(Sc, Bc, fl, sn, rdp[item]);
        } else {
          kind = nee_kind(fl, seed);                                                        // :198-214
          nr = (uint32_t)nee_rays(kind);
          if (q.cached) lvis_split(lv, kind, q.ask, q.vis0);
        }
      }
      // the block's shadow-ray slots, one atomic per pass (I0, pass 0: of the rays not known yet; else behind the NEE
      // block, of the live rays), as shade2_body's
      if (q.cached)
        q.s0 = block_append_skip(shcnt, (uint32_t)__popc(q.ask), qcounter(B.ctr, B.lslot, 1, sub), lvis_total(S),
                                 nr - (uint32_t)__popc(q.ask), sm);
      ShadedHit h = {kStMiss << 16, 0u, false};
      if (nr)
        h = shade_hit<false>(Sc, A, Bc, item, sn, ((size_t)path * levels + depth) * Bc.n + item, rop[item], rdp[item],
                             hh, kind, nr, info, seed, q, shq);
      if (h.cont()) next = true;
      if (!q.cached) {  // the live rays' slots; the dead ones counted
        const uint32_t nl = (uint32_t)__popc(h.live);
        const uint32_t s0 = block_append_skip(shcnt, nl, qcounter(B.ctr, B.lslot, 1, sub), dead_total(S), nr - nl, sm);
        queue_live(shq, s0, kind, h.live, (uint32_t)sn);
      }
      if (act) {
        Bc.rinfo[sn] = depth | (path << 8) | h.rinfo | ((uint32_t)kind << 20) | kRiFresh | (q.ask ? kRiLearn : 0u);
        need2 = pass == 0 && path == 0 && !h.cont() && (fl & kAA);
      }
    }
    const uint32_t slot = block_append(ncnt, next ? 1u : 0u, sm);
    if (next) qn[sub * Bc.qcap + slot] = item;
  }
}

// ---- debug render modes (:170-194): the hit's debug colour (or the sky) ends the path
__global__ void __launch_bounds__(kBlock) k_shade2_debug(SceneDev S, TraceArgs A, TileMap M, WaveBufs B,
                                                         uint32_t iter) {
  __shared__ uint32_t pref[kNSub + 1];
  __shared__ uint32_t sm[8];
  const uint32_t* q = (iter & 1) ? B.q1 : B.q0;
  uint32_t* qn = (iter & 1) ? B.q0 : B.q1;
  const uint32_t sub = blockIdx.x % kNSub;
  uint32_t* ncnt = qcounter(B.ctr, iter + 1, 0, sub);
  const uint32_t total = load_prefix(B.ctr, iter, 0, pref);
  for (uint32_t c = blockIdx.x; c * kBlock < total; c += gridDim.x) {
    const uint32_t g = c * kBlock + threadIdx.x;
    bool next = false;
    uint32_t item = 0;
    if (g < total) {
      item = q[map_slot(pref, g, B.qcap)];
      const uint32_t info = B.info[item];
      const float4 hh = B.hit[item];
      if ((info & 0x1FFu) == 0) B.s1[item].w = hh.x;
      if (hh.x < kFar) {  // misses keep k_miss2's sky value
        const uint32_t pk = __float_as_uint(hh.w);
        const HitAttr ha = hit_attributes(S, hit_inst(S, pk), hit_prim(S, pk), hh.y, hh.z, (A.flags & kNormalMap) != 0);
        const V3 L = debug_view(S, A.mode, ha, hit_inst(S, pk), hit_prim(S, pk));
        B.ne[item] = make_float4(L.x, L.y, L.z, 0.0f);
      }
      next = start_path2(S, A, M, B, item, (info >> 8) & 1u);
      B.rinfo[item] = (info & 0x1FFu) | (next ? kRiQueued : 0u);  // kStEndValue
    }
    const uint32_t slot = block_append(ncnt, next ? 1u : 0u, sm);
    if (next) qn[sub * B.qcap + slot] = item;
  }
}

// ---- NEE resolve of P(iter) (after k_trace2(iter + 1) traced S(iter)), stack, path end, frame write.
// ri: the rinfo of the segment's record e, a segment of `path`; sb: the first level of that path's (result, throughput)
// stack in R / T.  Plain and extensions pipelines: e = item, sb = 0; merged: e = path x n + item, sb = path x levels.
// path is bit 8 of ri; it is an argument all the same so that k_res2md's two calls, which know it, hand in a constant
// and each keeps only its side of the path end (taken from ri there, k_res2md<false> ran 3 us of 36 slower)
template <bool EXT>
__device__ __forceinline__ void resolve_item(const SceneDev& S, const TraceArgs& A, const WaveBufs& B, uint32_t item,
                                             uint32_t path, uint32_t ri, size_t e, uint32_t sb,
                                             float4* __restrict__ out) {
  const uint32_t fl = A.flags;
  const uint32_t depth = ri & 0xFFu, status = (ri >> 16) & 3u;
  // resolve_segment's expressions (prt_shade2.h) written out, the exception to "one resolve": the extensions' term and
  // the stack store sit inside the NEE branch, and built from resolve_segment or from halves of it k_res2md<false> ran
  // 6 % and k_res2d 2 % slower than this form (profiles/shade_resolve_ab.txt)
  const uint32_t kind = (ri >> 20) & 3u;
  const bool nee = status == kStNeeEnd || status == kStNeeCont;
  const float4 ne = (!nee || (ri & kRiEmissive)) ? B.ne[e] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  V3 L = v3(ne.x, ne.y, ne.z);
  if (nee) {
    const float4 nb = B.nb[e], nk = B.nk[e];
    V3 result = nee_resolve(S, (int)kind, vis_mask(B.vis[e]), L, v3(nb.x, nb.y, nb.z), nk, fl);
    if constexpr (EXT) {
      if (reinterpret_cast<const uint8_t*>(B.vis)[4 * (size_t)B.n + item]) {  // area light unoccluded
        const float4 a = B.na[item];
        result = result + v3(a.x, a.y, a.z);
      }
    }
    if (status == kStNeeCont) {  // the path goes on: result joins the stack
      B.R[(size_t)(sb + depth) * B.n + item] = make_float4(result.x, result.y, result.z, 0.0f);
      return;
    }
    L = result;
  }
  if constexpr (EXT) {
    // unwind through dielectric nodes: the end of a reflection subtree parks its radiance in T[level] and
    // stops (the refraction subtree is already queued); the end of a refraction subtree combines (:369)
    uint32_t ds = S.has_diel ? B.dst[item] : 0u;
    bool parked = false;
    for (int k = (int)depth - 1; k >= 0; k--) {
      const size_t ek = (size_t)(sb + (uint32_t)k) * B.n + item;
      const uint32_t bit = 1u << k;
      if (ds & bit) {
        const float F = B.dro[ek].w;
        if (ds & (bit << 24)) {
          L = dielectric_combine(F, L, v3(0.0f, 0.0f, 0.0f));
        } else if (!(ds & (bit << 16))) {
          B.T[ek] = make_float4(L.x, L.y, L.z, kFar);
          ds |= bit << 16;
          parked = true;
          break;
        } else {
          const float4 Lr = B.T[ek];
          L = dielectric_combine(F, v3(Lr.x, Lr.y, Lr.z), L);
        }
        ds &= ~(0x01010101u << k);
        continue;
      }
      const float4 Rk = B.R[ek], Tk = B.T[ek];
      L = v3(Rk.x, Rk.y, Rk.z) + L * v3(Tk.x, Tk.y, Tk.z);
    }
    if (S.has_diel) B.dst[item] = ds;
    if (parked) return;
  } else {
    for (int k = (int)depth - 1; k >= 0; k--) {                                            // result + Trace(..) * throughput
      const size_t ek = (size_t)(sb + (uint32_t)k) * B.n + item;
      const float4 Rk = B.R[ek], Tk = B.T[ek];
      L = v3(Rk.x, Rk.y, Rk.z) + L * v3(Tk.x, Tk.y, Tk.z);
    }
  }
  finish_path(B, item, path, L, fl, out);
}
// ---- resolve of P(iter - 1) and the misses of P(iter) in one pass over P(iter - 1): P(iter) is the subset
// k_shade2(iter - 1) queued (rinfo bit kRiQueued), so each of its items is visited once, resolved first (it
// reads ne / T of iteration iter - 1) and then given its sky value (ne of iteration iter), the order of the
// separate kernels
template <bool EXT>
__global__ void __launch_bounds__(kBlock) k_resmiss2(SceneDev S, TraceArgs A, WaveBufs B, uint32_t iter,
                                                     uint32_t iters, uint32_t misses, float4* __restrict__ out) {
  __shared__ uint32_t pref[kNSub + 1];
  const uint32_t* q = ((iter - 1) & 1) ? B.q1 : B.q0;
  const uint32_t total = load_prefix(B.ctr, iter - 1, 0, pref);
  // software pipeline over the grid-stride chunks: the next chunk's item and rinfo are loaded while this
  // chunk's item is resolved
  uint32_t item_n = 0, ri_n = 0;
  auto prefetch = [&](uint32_t cc) {
    const uint32_t gg = cc * kBlock + threadIdx.x;
    if (gg < total) {
      item_n = q[map_slot(pref, gg, B.qcap)];
      ri_n = B.rinfo[item_n];
    }
  };
  prefetch(blockIdx.x);
  for (uint32_t c = blockIdx.x; c * kBlock < total; c += gridDim.x) {
    const uint32_t g = c * kBlock + threadIdx.x;
    const uint32_t item = item_n, ri = ri_n;
    prefetch(c + gridDim.x);
    if (g >= total) continue;
    resolve_item<EXT>(S, A, B, item, (ri >> 8) & 1u, ri, item, 0u, out);
    if (misses && iter < iters && (ri & kRiQueued)) miss_item<EXT>(S, A, B, item);
  }
}

// dense resolve (plain pipeline, no extensions, render mode 0): every item in index order, the next item's rinfo
// loaded while this one is resolved.  LEARN: the resolve of launch 1 in a pass whose iteration 0 used the
// light-visibility record (an instantiation of its own, like the shading's): it also records what the queued
// shadow rays of the kRiLearn items found
template <bool LEARN>
__global__ void __launch_bounds__(kBlock) k_res2d(SceneDev S, TraceArgs A, WaveBufs B, float4* __restrict__ out) {
  const uint32_t stride = gridDim.x * kBlock;
  uint32_t item = blockIdx.x * kBlock + threadIdx.x;
  uint32_t ri_n = item < B.n ? B.rinfo[item] : 0u;
  for (; item < B.n; item += stride) {
    const uint32_t ri = ri_n;
    if (item + stride < B.n) ri_n = B.rinfo[item + stride];
    if (!(ri & kRiFresh)) continue;
    resolve_item<false>(S, A, B, item, (ri >> 8) & 1u, ri, item, 0u, out);
    if constexpr (LEARN) {
      if (ri & kRiLearn) lvis_learn(B, item, ri);
    }
    B.rinfo[item] = ri & ~(kRiFresh | kRiLearn);
  }
}

// ---- merged pipeline: the resolve of P(iter - 1) per record slot (path 1's, then path 2's), each with its own stack
template <bool LEARN>  // (as k_res2d's; slot 0 is path 1)
__global__ void __launch_bounds__(kBlock) k_res2md(SceneDev S, TraceArgs A, WaveBufs B, float4* __restrict__ out) {
  const uint32_t levels = (uint32_t)max(1, A.bounces - 1);  // of each path's (result, throughput) stack
  const uint32_t stride = gridDim.x * kBlock;
  uint32_t item = blockIdx.x * kBlock + threadIdx.x;
  uint32_t r0_n = 0, r1_n = 0;
  if (item < B.n) { r0_n = B.rinfo[item]; r1_n = B.rinfo[B.n + item]; }
  for (; item < B.n; item += stride) {
    const uint32_t r0 = r0_n, r1 = r1_n;
    if (item + stride < B.n) { r0_n = B.rinfo[item + stride]; r1_n = B.rinfo[B.n + item + stride]; }
    if (r0 & kRiFresh) {
      resolve_item<false>(S, A, B, item, 0u, r0, item, 0u, out);
      if constexpr (LEARN) {
        if (r0 & kRiLearn) lvis_learn(B, item, r0);
      }
      B.rinfo[item] = r0 & ~(kRiFresh | kRiLearn);
    }
    if (r1 & kRiFresh) {
      resolve_item<false>(S, A, B, item, 1u, r1, (size_t)B.n + item, levels, out);
      B.rinfo[B.n + item] = r1 & ~kRiFresh;
    }
  }
}

// LDS per wave (one block): 2 x STACK x 256 B of stack + 264 B of prefix tables + the tail slots, within
// 160 KB / (4 x WAVES) blocks per CU
#ifndef PRT_REFILL
#define PRT_REFILL 32  // idle lanes before a wave refills from the queue (A/B builds: -DPRT_REFILL=16 ...)
#endif
template <int STACK, int WAVES, int TAILN, bool DENSE>
void launch_t2(const LaunchCfg& c, const SceneDev& S, const WaveBufs& B, uint32_t it, uint32_t iters) {
  static_assert(2 * STACK * 256 + 264 + 4 * 3 * TAILN <= 163840 / (4 * WAVES), "LDS over the occupancy budget");
  if (S.tlas)
    hipLaunchKernelGGL((k_trace2<PRT_REFILL, STACK, WAVES, TAILN, true, false, DENSE>),
                       dim3(256u * 4u * WAVES / c.groups), dim3(64), 0, c.stream, S, B, it, iters);
  else
    hipLaunchKernelGGL((k_trace2<PRT_REFILL, STACK, WAVES, TAILN, false, false, DENSE>),
                       dim3(256u * 4u * WAVES / c.groups), dim3(64), 0, c.stream, S, B, it, iters);
}
// persistent traversal occupancy (waves/SIMD) -> LDS stack groups per lane; a BVH deeper than the 18 LDS
// groups at 4 waves/SIMD hold runs the 4-wave form with the HBM spill columns (S.spill)
// DENSE: the dense primary pass of iteration 0 (Kernel::Trace2Dense), an instantiation of its own
template <bool DENSE>
static void launch_trace2_t(const LaunchCfg& c, const SceneDev& S, const WaveBufs& B, uint32_t it, uint32_t iters) {
  if (S.spill) {
    if (S.tlas)
      hipLaunchKernelGGL((k_trace2<32, 18, 4, 32, true, true, DENSE>), dim3(kSpillTraceBlocks / c.groups), dim3(64), 0,
                         c.stream, S, B, it, iters);
    else
      hipLaunchKernelGGL((k_trace2<32, 18, 4, 32, false, true, DENSE>), dim3(kSpillTraceBlocks / c.groups), dim3(64), 0,
                         c.stream, S, B, it, iters);
  } else if (c.occ == 7) launch_t2<9, 7, 64, DENSE>(c, S, B, it, iters);
  else if (c.occ == 6) launch_t2<11, 6, 64, DENSE>(c, S, B, it, iters);
  else if (c.occ == 5) launch_t2<14, 5, 32, DENSE>(c, S, B, it, iters);
  else launch_t2<18, 4, 32, DENSE>(c, S, B, it, iters);
}

// producer grids (the kernels that append to the sub-queues: k_wave_init, the shading kernels): a multiple of kNSub,
// so that block b appends to sub-queue b % kNSub exactly the chunks c == b (mod kNSub) it consumes -- the bound
// wave_layout sizes each sub-queue by (qcap).  1/groups of the resident blocks, rounded down to that multiple
__host__ inline unsigned producer_blocks(const LaunchCfg& c) {
  const unsigned g = 256u * 4u / c.groups;
  return g < kNSub ? kNSub : g - g % kNSub;
}

// launch `it` of a pass: trace P(it) + S(it - 1), resolve P(it - 1), miss + shade P(it), by the kernels wave_schedule
// (prt_plan.h) names for the plan's pipeline
hipError_t launch_wave2_iter(const LaunchCfg& c, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                             const WaveBufs& B, float4* out, WaveTimers* tm, const WavePlan& P, bool lrec,
                             uint32_t it, int surf, const SurfBufs* R) {
  if (B.n == 0) return hipSuccess;
  const unsigned gprod = producer_blocks(c);
  // k_shade2 over 4x the resident blocks when a call holds >= 2^21 items: the extra blocks queue behind the
  // resident ones and even out the kernel's end (C4 frame -1 to -2 %); below that the extra launch width costs
  // more than it evens out (world-8 shares). PRT_SHADE_GRID overrides (A/B runs).
#ifndef PRT_SHADE_GRID
  const unsigned gshade = B.n >= (1u << 21) ? 4u * gprod : gprod;
#else
  // the sub-queue bound of wave_layout (qcap) holds only when block b appends to sub-queue b % kNSub for
  // chunks c == b (mod kNSub), i.e. for grids that are multiples of kNSub
  static_assert(PRT_SHADE_GRID % kNSub == 0, "PRT_SHADE_GRID must be a multiple of kNSub");
  const unsigned gshade = PRT_SHADE_GRID;
#endif
  const uint32_t iters = P.iters;
  const Schedule k = wave_schedule(P.pipeline, lrec, B.pmode, it, iters, surf);
  if (tm) (void)hipEventRecord(tm->ev[4 * it + 0], c.stream);
  // deferred resolve (prt_defer.hip): B's record pointers are plane 0.  This launch's shading gets plane `it`; its
  // traversal gets vis of plane it - 1, whose bytes the shadow entries of S(it - 1) index (shadow_vis)
  WaveBufs Bt = B, Bs = B;
  if (P.defer()) {
    if (it > 0) Bt.vis = B.vis + (size_t)(it - 1u) * B.n;
    const size_t o = (size_t)it * B.n;
    Bs.rinfo += o; Bs.ne += o; Bs.nb += o; Bs.nk += o; Bs.vis += o; Bs.T += o;
  }
  // a launch with nothing to trace (Kernel::None) still records its two timer events, back to back (read_stats reads a
  // pair per iteration; the launch shows as ~0 ms and leaves no PRT_DEBUG_QUEUES timeline record)
  if (k.trace == Kernel::Trace2Dense) launch_trace2_t<true>(c, S, Bt, it, iters);
  else if (k.trace == Kernel::Trace2) launch_trace2_t<false>(c, S, Bt, it, iters);
  if (tm) (void)hipEventRecord(tm->ev[4 * it + 1], c.stream);
#ifndef PRT_RES_GRID
  const unsigned gres = gprod;
#else
  const unsigned gres = PRT_RES_GRID;  // A/B
#endif
  // the dense resolves over 2x the resident producer blocks (8 waves/SIMD), at most one chunk per block
  const unsigned gdense = std::min<unsigned>(2u * gprod, (B.n + kBlock - 1) / kBlock);
  // (the cases stand in the order this file has always first named the instantiations in: that order places them in
  // the code object, and their machine code holds offsets relative to that place)
#define PRT_LAUNCH(kernel, grid, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, c.stream, __VA_ARGS__)
  switch (k.resolve) {
    case Kernel::Res2mdLearn: PRT_LAUNCH(k_res2md<true>, gdense, S, A, B, out); break;
    case Kernel::Res2md: PRT_LAUNCH(k_res2md<false>, gdense, S, A, B, out); break;
    case Kernel::Res2dLearn: PRT_LAUNCH(k_res2d<true>, gdense, S, A, B, out); break;
    case Kernel::Res2d: PRT_LAUNCH(k_res2d<false>, gdense, S, A, B, out); break;
    case Kernel::ResolvePassLearn: launch_resolve_pass(c.stream, gdense, S, A, B, iters, out, true); break;
    case Kernel::ResolvePass: launch_resolve_pass(c.stream, gdense, S, A, B, iters, out, false); break;
    // the misses' sky radiance in a pass of their own (misses = 1), from launch 1 on behind the resolve of P(it - 1)
    case Kernel::ResMiss2Ext: PRT_LAUNCH(k_resmiss2<true>, gres, S, A, B, it, iters, 1u, out); break;
    case Kernel::ResMiss2: PRT_LAUNCH(k_resmiss2<false>, gres, S, A, B, it, iters, 1u, out); break;
    case Kernel::Miss2Ext: PRT_LAUNCH(k_miss2<true>, gprod, S, A, B, it); break;
    case Kernel::Miss2: PRT_LAUNCH(k_miss2<false>, gprod, S, A, B, it); break;
    default: assert(k.resolve == Kernel::None);
  }
  switch (k.shade) {
    case Kernel::Shade2mLearn: PRT_LAUNCH(k_shade2m<true>, gshade, S, A, M, B, it); break;
    case Kernel::Shade2m: PRT_LAUNCH(k_shade2m<false>, gshade, S, A, M, B, it); break;
    case Kernel::Shade2Debug: PRT_LAUNCH(k_shade2_debug, gprod, S, A, M, B, it); break;
    case Kernel::Shade2Ext: PRT_LAUNCH(k_shade2<true>, gshade, S, A, M, B, it); break;
    case Kernel::Shade2dLearn: launch_shade2d(c.stream, gshade, S, A, M, Bs, it, true); break;
    case Kernel::Shade2d: launch_shade2d(c.stream, gshade, S, A, M, Bs, it, false); break;
    case Kernel::Shade2Learn: PRT_LAUNCH((k_shade2<false, true>), gshade, S, A, M, B, it); break;
    case Kernel::Shade2: PRT_LAUNCH(k_shade2<false>, gshade, S, A, M, B, it); break;
    // iteration 0 under the primary-surface record (prt_surface.hip)
    case Kernel::Shade2sdFill: launch_shade2s(c.stream, gshade, S, A, M, Bs, it, true, kSurfFill, *R, out); break;
    case Kernel::Shade2sdRead: launch_shade2s(c.stream, gshade, S, A, M, Bs, it, true, kSurfRead, *R, out); break;
    case Kernel::Shade2sdInit: launch_shade2s(c.stream, gshade, S, A, M, Bs, it, true, kSurfInit, *R, out); break;
    case Kernel::Shade2sFill: launch_shade2s(c.stream, gshade, S, A, M, B, it, false, kSurfFill, *R, out); break;
    case Kernel::Shade2sRead: launch_shade2s(c.stream, gshade, S, A, M, B, it, false, kSurfRead, *R, out); break;
    default: assert(k.shade == Kernel::None);
  }
#undef PRT_LAUNCH
  if (tm) tm->iters = iters + 1;
  return hipGetLastError();
}

hipError_t launch_wave_init(const LaunchCfg& c, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                            const WaveBufs& B, float4* out) {
  hipLaunchKernelGGL(k_wave_init, dim3(producer_blocks(c)), dim3(kBlock), 0, c.stream, S, A, M, B, out);
  return hipGetLastError();
}

}  // namespace prt
