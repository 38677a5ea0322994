// prt_launch.h -- the host-side launchers of the kernel files (prt_render.hip, prt_wave2.hip, prt_defer.hip) and the
// argument structs they share with the host code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "prt_kernels.h"
#include "prt_plan.h"
#include "prt_post.h"
#include "prt_traverse8.h"

namespace prt {

struct Counters {
  unsigned long long segments, shadow;
};
struct HitOut {
  float t, u, v;
  uint32_t prim, inst;
};
struct LaunchCfg {
  hipStream_t stream;
  int occ;     // persistent traversal waves/SIMD: 7 / 6 / 5 / 4 (9 / 11 / 14 / 18 LDS stack groups)
  uint32_t groups = 1;  // grid divisor: every wavefront grid is 1/groups of the resident blocks (frames in flight:
                        // the chains' persistent launches co-reside on the SIMDs, prt_api_render.cpp enqueue_render)
};

// wavefront pipeline buffers (SoA over n work items; R/T hold (bounces-1) x n entries; layout: prt_plan.h)
struct WaveBufs {
  uint32_t n;       // items of this call
  uint32_t base;    // first item of the state arrays within the call (0)
  uint32_t qcap;    // capacity of one path sub-queue  (multiple of 256)
  uint32_t scap;    // capacity of one shadow sub-queue (4 x qcap)
  uint32_t* seed;
  uint32_t* info;   // depth | path << 8 | status << 16 | nee kind << 20
  uint32_t* rinfo;  // what the resolve of the next launch finishes (depth | path << 8 | status << 16 | kind << 20)
  float4* ro;
  float4* rd;
  float4* R;
  float4* T;
  float4* s1;       // path-1 radiance, w = r1.hit.t
  float2* jit;
  float4* hit;      // t, u, v, bits(prim | inst << 26)
  float4* ne;       // emissive (or the path's end value)
  float4* nb;       // NEE BRDF value
  float4* nk;       // NEE factors the shadow rays' contributions are rebuilt from (prt_path.h nee_lights)
  uint32_t* vis;    // 4 visibility bytes per item
  uint32_t* q0;
  uint32_t* q1;
  uint32_t* shq;    // shadow queue: light << 29 | visibility index (prt_wave2.hip shadow_of)
  float4* hp;       // the hit point I of the item's last shading (its shadow rays' origin before the offset)
  uint32_t* ctr;    // [iteration][path|shadow][sub-queue] counters, kCtrStride apart
  // extensions (area light / dielectric instances; Pipeline::Ext only): vis holds 5 x n bytes, the area
  // light's shadow ray writes byte 4 * n + item
  float4* na;       // area-light NEE contribution before visibility
  uint32_t* dst;    // dielectric DFS state: bits 0-7 dielectric level, 8-15 refraction started,
                    // 16-23 reflected radiance stored (in T[level]), 24-31 no refraction (k <= 0)
  float4* dro;      // per level: refraction ray origin, fresnel
  float4* drd;      // per level: refraction ray direction
  float4* ao;       // the area light's shadow ray per item: origin, tmax (its NEE sample is random: stored whole)
  float4* ad;       // ... direction
  unsigned long long* tl;  // PRT_DEBUG_QUEUES: [launch][wave] {start, first empty fetch, exit, -}
  int32_t coop_tail;       // cooperative traversal tail (prt_persist.h)
  int32_t merge;           // path-2 merge (prt_wave2.hip): the AA path-2 primaries traced with path 1's, and
                           // each path's NEE record / (result, throughput) stack in its own slot (slot p at p * n)
  float4* ro2;             // merge: the path-2 primary ray (k_wave_init), traced by k_trace2(0) ...
  float4* rd2;
  float4* hit2;            // ... into hit2; shaded by k_shade2 right after path 1 ends
  // primary-hit reuse (prt_wave2.hip): the hit record of every tile-map entry's path-1 primary ray (the pixel
  // centre: the same ray in every reference frame while camera, tile map, scene and instances stay put)
  float4* phit;            // pitems records, entry r = (base + item) % pitems; one copy per wavefront state
  uint32_t pitems;         // entries of the call's tile map (TileMap::items)
  int32_t pmode;           // kPrimTrace: every item's primary ray is traced into hit (no reuse);
                           // kPrimDense: launch 0 traces the pitems rays of the pass's first frame into phit;
                           // kPrimReuse: phit is current, launch 0 traces no path-1 primary
  // light-visibility record (prt_wave2.hip): per tile-map entry, indexed like phit, what the shadow rays from the
  // entry's fixed primary hit towards the six light-class lights found (8 bytes: byte l for light l; 0 unknown,
  // 1 occluded, 2 unoccluded).  Null unless the pass runs with kPrimReuse and the record belongs to phit and to
  // the lights' positions (prt_api_render.cpp); one copy per wavefront state
  uint2* lvis;
  uint32_t lslot;          // the iteration whose shadow counter counts the shadow rays not queued (iters + 1): those
                           // answered from lvis and the dead ones
  uint32_t dead;           // dead shadow rays (prt_wave2.hip), the PRT_DEAD_SHADOW level: 0 trace them all, 1 skip those
                           // whose contribution is zero, 2 (default) also those a zero BRDF value multiplies.  In the
                           // struct's tail padding: the kernel arguments behind a WaveBufs stay where they were
};
static_assert(sizeof(WaveBufs) % 8 == 0 && offsetof(WaveBufs, dead) + 4 == sizeof(WaveBufs),
              "dead fills WaveBufs' tail padding");
// primary-surface record (prt_shade2.h surf_store; prt_surface.hip): per tile-map entry, indexed like phit and lvis,
// what the shading of iteration 0 needs of the entry's fixed path-1 primary hit in place of hit_attributes, the hit
// point and the sky lookup.  SoA planes of 16-byte words, one copy per wavefront state.  A kernel argument of its own
// behind the k_shade2s forms' Shade2Args, so that WaveBufs and every other kernel's arguments stay where they are
struct SurfBufs {
  float4* n4;  // hit: N, t (sign bit: emissive); miss: the sky radiance (or 0), t >= kFar
  float4* b4;  // m.base, m.rough
  float4* i4;  // I, m.metal
  float4* e4;  // m.emis of the entries whose emissive bit is set; null unless some mesh has an emission texture
};
#ifdef PRT_LANE_STATS
void lane_stats_dump();  // diagnostic build: prints and clears the traversal lane counters (prt_wave2.hip)
#endif
constexpr int kTlWaves = 256 * 4 * 8;  // timeline records per traversal launch (max persistent grid)
struct WaveTimers {
  hipEvent_t ev[4 * (kMaxIters + 1)];
  uint32_t iters;
};

hipError_t launch_wave_init(const LaunchCfg& c, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                            const WaveBufs& B, float4* out);
// launch `it` (0..iters) of a pass after launch_wave_init (prt_wave2.hip): one traversal launch for P(it) closest +
// S(it-1) any-hit, then resolve / miss / shade -- the kernels wave_schedule (prt_plan.h) names for the plan's pipeline.
// lrec: the pass runs with kPrimReuse and holds a light-visibility record (B.lvis).
// Pipeline::PlainDeferred: the pass's resolve is one launch behind the last traversal (prt_defer.hip k_resolve_pass).
// B's rinfo / ne / nb / nk / vis / T then point at plane 0 of `iters` record planes of B.n entries each (plane i at
// i * B.n); B.R is not used
// surf: the pass's iteration 0 fills (kSurfFill) or reads (kSurfRead) the primary-surface record R (prt_surface.hip)
hipError_t launch_wave2_iter(const LaunchCfg& c, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                             const WaveBufs& B, float4* out, WaveTimers* tm, const WavePlan& P, bool lrec,
                             uint32_t it, int surf = kSurfNone, const SurfBufs* R = nullptr);
// ... whose shading (into the record plane B points at) and resolve launches prt_defer.hip holds
void launch_shade2d(hipStream_t s, unsigned grid, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                    const WaveBufs& B, uint32_t it, bool i0);
// iteration 0 of a kPrimReuse pass under the primary-surface record (prt_surface.hip k_shade2s): defer as
// launch_shade2d's plane, surf kSurfFill, kSurfRead or (deferred) kSurfInit; out: the pass's frame buffer (kSurfInit
// writes the entries without a pixel, as k_wave_init does)
void launch_shade2s(hipStream_t s, unsigned grid, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                    const WaveBufs& B, uint32_t it, bool defer, int surf, const SurfBufs& R, float4* out);
void launch_resolve_pass(hipStream_t s, unsigned grid, const SceneDev& S, const TraceArgs& A, const WaveBufs& B,
                         uint32_t iters, float4* out, bool learn);
// zero na words at a and nb words at b (one dispatch)
hipError_t launch_clear2(const LaunchCfg& c, uint32_t* a, uint32_t na, uint32_t* b, uint32_t nb);
// acc_prev (nullable): the accumulator state before the last frame of the call (screen-pass input);
// totals (nullable): running ray totals, incremented by the queue counters ctr of the pass's `iters` iterations
hipError_t launch_accumulate(const LaunchCfg& c, const TileMap& M, int32_t frames, uint32_t flags, const float4* fr,
                             float4* acc, int32_t* nsamp, float* dist, float4* avg, uint32_t* rgb8, float4* tiles,
                             float4* acc_prev, const uint32_t* ctr, uint32_t iters, Counters* totals);
// post-processed RGB8 of the whole image (Core/Renderer.cpp:107-133)
hipError_t launch_postfx(const LaunchCfg& c, const PostDev& P, const float4* acc_new, const float4* acc_old,
                         const int32_t* nsamp, const float4* avg, uint32_t* rgb8);
hipError_t launch_untile(const LaunchCfg& c, int32_t W, int32_t H, int32_t ts, int32_t world, uint32_t per_rank,
                         const float4* gathered, float4* avg, uint32_t* rgb8, const PostDev* post);
struct InstSrc;
// persistent traversal grid when the stacks spill to HBM (4 waves/SIMD: 256 CUs x 4 SIMDs x 4), and the LDS
// stack levels of that form and of the one-ray query kernels (prt_traverse8.h kQueryStack)
constexpr uint32_t kSpillTraceBlocks = 256u * 4u * 4u;
constexpr int kSpillTraceStack = 18;
// device refit of the instances (prt_refit.h)
hipError_t launch_refit(hipStream_t s, const InstSrc* src, int32_t n, InstDev* out);
// the stream waits until *flag (coherent pinned host memory, device address) is nonzero; after `seconds` it stops
// waiting and sets *err (prt_render.hip k_wait_host)
hipError_t launch_wait_host(hipStream_t s, uint32_t* flag, uint32_t* err, double seconds);
// prt_rebuild_instances (prt_tlas_build.hip; the definitions: prt_tlas_build.h).  launch_tlas_prims: the device
// builder's input, three float4 per instance, from the boxes of the records inst[0 .. n).  launch_tlas_finish: the
// builder's tree nodes[0 .. n_nodes) over the records tris[0 .. n_tris), whose level d is [level_ends[d - 1],
// level_ends[d]) (host array), as an instance BVH into dst / dst_slot (80 and 32 bytes per node; neither may overlap
// nodes), each level in its canonical order: the same tree gives the same bytes wherever the builder's atomic counters
// placed its nodes.  The levels stay where they are.  order_scratch: 12 bytes per node
struct TriMT;
hipError_t launch_tlas_prims(hipStream_t s, const InstDev* inst, int32_t n, float4* fat);
hipError_t launch_tlas_finish(hipStream_t s, const Node8* nodes, const TriMT* tris, uint32_t n_tris, uint32_t n_nodes,
                              uint32_t ninst, const uint32_t* level_ends, size_t levels, uint32_t* order_scratch,
                              Node8* dst, uint32_t* dst_slot);
hipError_t launch_primary_hits(const LaunchCfg& c, const SceneDev& S, const TileMap& M, HitOut* out, Counters* cnt);
hipError_t launch_intersect(const LaunchCfg& c, const SceneDev& S, int32_t n, const float* O, const float* D,
                            const float* tmax, HitOut* out);
hipError_t launch_occluded(const LaunchCfg& c, const SceneDev& S, int32_t n, const float* O, const float* D,
                           const float* tmax, int32_t* out);
// prt_query_rays (prt_query.hip k_query): n rays in the caller's arrays (device memory; tmax nullable = kFar each), the
// closest hits into hits and / or the any-hit answers into occ (each nullable).  The live range of the persistent
// launch is [0, total): nclosest closest-hit entries (n or 0), then the any-hit entries.  fctr: kParts fetch counters,
// kCtrStride words apart, zero at launch
struct QueryArgs {
  const float* O;
  const float* D;
  const float* tmax;
  HitOut* hits;
  int32_t* occ;
  uint32_t* fctr;
  uint32_t nclosest, total;
  int32_t coop_tail;  // cooperative traversal tail (prt_persist.h), the context's tunable as the render's
};
hipError_t launch_query(const LaunchCfg& c, const SceneDev& S, const QueryArgs& Q);
// prt_query_surface (k_query_surface): the shading inputs at n hit records; a record is a hit when t < tmax (nullable =
// kFar).  Every output nullable: albedo / normal_depth as launch_aov's, the geometry normal (w = 1), and the material as
// two float4 per record (base rgb, metalness | emissive rgb, roughness); misses get the zeros include/prt.h defines
hipError_t launch_query_surface(hipStream_t s, const SceneDev& S, int32_t n, bool normalmapped, const HitOut* hits,
                                const float* tmax, float4* albedo, float4* normal_depth, float4* geo_normal,
                                float4* material);
// prt_brdf_probe: n records of 24 floats in, 8 out (include/prt.h PRT_PROBE_*)
hipError_t launch_brdf_probe(hipStream_t s, int32_t op, int32_t n, const float* in, float* out);

}  // namespace prt
