// prt_plan.h -- what a render call decides before it launches anything: the environment switches (Tunables), the
// wavefront pipeline and pass split of the call (WavePlan, plan_render), the kernels of each launch of a pass
// (wave_schedule) and the byte layout of the wavefront buffer and of the record planes.  Plain C++, no HIP: the host
// code (prt_api_render.cpp, prt_wave2.hip launch_wave2_iter) and tests/cpp/plan_check.cpp compile the same text.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/prt.h"

namespace prt {

constexpr uint32_t kNSub = 32;       // sub-queues per queue (one append counter each)
constexpr uint32_t kCtrStride = 32;  // words between counters (each on its own 128-B line)
constexpr uint32_t kParts = 8;  // XCD parts of a traversal launch's live range, one fetch counter each (prt_queue.h)
constexpr int kMaxIters = 128;  // wavefront iterations per call: bounces <= 64 (AA) / 6 with dielectrics (AA)
// WaveBufs::pmode
enum : int32_t { kPrimTrace = 0, kPrimDense = 1, kPrimReuse = 2 };
// what iteration 0 of a pass does with the primary-surface record (prt_launch.h SurfBufs): nothing, store, shade from
// it, shade from it and do the wave init's work itself (the pass then launches no k_wave_init)
enum : int { kSurfNone = 0, kSurfFill = 1, kSurfRead = 2, kSurfInit = 3 };

// A call's work items (pixels x reference frames) index the shadow-queue entries as 4 x item + k in 29 bits
// (prt_wave2.hip kShIndexMask; the light class takes the top 3), so one pass holds at most 2^27 items; the merged
// pipeline's entries index 4 x (slot x n + item) + k: at most 2^26 items per pass
constexpr uint64_t kMaxPassItems = 1ull << 27;
constexpr uint64_t kMaxMergedPassItems = 1ull << 26;

// ---- the environment switches of a render call, each read on every call (A/B runs and tests flip them between calls)
inline bool debug_queues_on() { return std::getenv("PRT_DEBUG_QUEUES") != nullptr; }
struct Tunables {
  int32_t merge = -1;              // PRT_MERGE: 0 / 1 forces the merged pipeline off / on (-1: unset, by size)
  bool defer = true;               // PRT_DEFER_RESOLVE=0 switches the deferred resolve off
  uint64_t defer_budget = 4096ull << 20;  // PRT_DEFER_BUDGET_MB (MiB), in bytes: the record planes a pass may take
  bool primary_reuse = true;       // PRT_PRIMARY_REUSE=0: every item's primary ray traced every frame
  bool shadow_reuse = true;        // PRT_SHADOW_REUSE=0: no light-visibility record
  bool surface_reuse = true;       // PRT_SURFACE_REUSE=0: no primary-surface record
  bool init_fold = true;           // PRT_INIT_FOLD=0: a pass that shades from that record still launches k_wave_init
  uint32_t dead_shadow = 2;        // PRT_DEAD_SHADOW: 0 traces every shadow ray, 1 skips those whose own contribution
                                   // is zero, unset or anything else (2) also those a zero BRDF value multiplies
  uint64_t max_items = 0;          // PRT_MAX_ITEMS: a smaller pass size, at least 1 (0: unset)
  bool coop_tail = true;           // PRT_TAIL=0 switches the cooperative traversal tail off (prt_persist.h)
  bool debug_queues = false;       // PRT_DEBUG_QUEUES: stats calls record the launch timeline
  int32_t fail_rank = -1;          // PRT_FAIL_RENDER=<rank>: that shard's render fails before anything is enqueued
  bool fail_all = false;           // ... "all": every context's
};
inline Tunables read_tunables() {
  Tunables t;
  auto off = [](const char* name) {  // set, and 0
    const char* e = std::getenv(name);
    return e && std::atoi(e) == 0;
  };
  if (const char* e = std::getenv("PRT_MERGE")) t.merge = std::atoi(e) != 0 ? 1 : 0;
  t.defer = !off("PRT_DEFER_RESOLVE");
  if (const char* e = std::getenv("PRT_DEFER_BUDGET_MB")) t.defer_budget = std::strtoull(e, nullptr, 10) << 20;
  t.primary_reuse = !off("PRT_PRIMARY_REUSE");
  t.shadow_reuse = !off("PRT_SHADOW_REUSE");
  t.surface_reuse = !off("PRT_SURFACE_REUSE");
  t.init_fold = !off("PRT_INIT_FOLD");
  if (const char* e = std::getenv("PRT_DEAD_SHADOW")) {
    const int v = std::atoi(e);
    t.dead_shadow = v == 0 ? 0u : (v == 1 ? 1u : 2u);
  }
  if (const char* e = std::getenv("PRT_MAX_ITEMS")) t.max_items = std::max<uint64_t>(std::strtoull(e, nullptr, 10), 1);
  t.coop_tail = !off("PRT_TAIL");
  t.debug_queues = debug_queues_on();
  if (const char* e = std::getenv("PRT_FAIL_RENDER"); e && *e) {
    t.fail_all = std::strcmp(e, "all") == 0;
    t.fail_rank = std::max(std::atoi(e), -1);
  }
  return t;
}

// ---- byte layouts: every array on a 256-byte boundary, in the order of its list.  The offsets decide which HBM
// channels the SoA streams start on, so the order is part of the measured behaviour
constexpr size_t round256(size_t bytes) { return (bytes + 255) & ~size_t(255); }

// queue counters [iter][path|shadow][kNSub] + traversal fetch counters [iter][path|shadow][8 parts]
constexpr size_t kCtrWords = (size_t)(kMaxIters + 2) * 2 * (kNSub + kParts) * kCtrStride;
// shadow-queue entries one shading launch may append per item: <= 4 light-class + 1 area-light ray; the merged
// pipeline (no extensions) shades path 1's last segment and path 2's first in the same launch, 4 + 4
constexpr uint32_t shadow_per_item(bool merge) { return merge ? 8u : 5u; }

// The wavefront buffer of n items and `levels` (result, throughput) stack levels: X(WaveBufs member, bytes per
// element, elements, present-if), over n, ns (record slots: 2 n merged), levels, qn / sn (path / shadow queue
// entries), merge, ext and needR.  An absent array takes no bytes and its pointer is null
#define PRT_WAVE_ARRAYS(X)                                                                                      \
  X(seed, 4, n, true) X(info, 4, n, true) X(rinfo, 4, ns, true) X(ro, 16, n, true) X(rd, 16, n, true)          \
  X(R, 16, ns * levels, needR) X(T, 16, ns * levels, true) X(s1, 16, n, true) X(jit, 8, n, true)               \
  X(hit, 16, n, true) X(ne, 16, ns, true) X(nb, 16, ns, true) X(nk, 16, ns, true)                              \
  X(vis, 1, (merge ? 8 : 5) * n, true) X(q0, 4, qn, true) X(q1, 4, qn, true) X(shq, 4, sn, true)               \
  X(hp, 16, ns, true) X(ctr, 4, kCtrWords, true)                                                               \
  X(ro2, 16, n, merge) X(rd2, 16, n, merge) X(hit2, 16, n, merge)                                              \
  X(na, 16, n, ext) X(dst, 4, n, ext) X(dro, 16, n * levels, ext) X(drd, 16, n * levels, ext)                  \
  X(ao, 16, n, ext) X(ad, 16, n, ext)
// The record planes of a deferred pass (n items, `iters` iterations; plane i of an array lies i * n entries behind
// plane 0): X(WaveBufs member, bytes per element)
#define PRT_PLANE_ARRAYS(X) X(rinfo, 4) X(vis, 4) X(ne, 16) X(nb, 16) X(nk, 16) X(T, 16)

#define PRT_LAYOUT_ID(m, ...) kW_##m,
enum WaveArray : int { PRT_WAVE_ARRAYS(PRT_LAYOUT_ID) kWaveArrays };
#undef PRT_LAYOUT_ID
#define PRT_LAYOUT_ID(m, ...) kP_##m,
enum PlaneArray : int { PRT_PLANE_ARRAYS(PRT_LAYOUT_ID) kPlaneArrays };
#undef PRT_LAYOUT_ID

struct WaveLayout {
  uint32_t levels, qcap, scap;  // stack levels; capacity of one path / shadow sub-queue
  bool has[kWaveArrays];
  size_t off[kWaveArrays];      // (0 for an absent array)
  size_t bytes;
};
// needR: the pass resolves per iteration (every pipeline but the plain one with a deferred resolve) and stacks results
inline WaveLayout wave_layout(uint32_t n_items, int bounces, bool ext, bool merge, bool needR) {
  WaveLayout L{};
  L.levels = (uint32_t)std::max(1, bounces - 1);
  // sub-queue t receives the 256-entry chunks c == t (mod kNSub): at most ceil(ceil(n/256)/kNSub) of them
  L.qcap = 256u * (((n_items + 255u) / 256u + kNSub - 1) / kNSub);
  L.scap = shadow_per_item(merge) * L.qcap;
  // merge: two record slots (path 1, path 2) per item for the NEE record, hit point, status and stack
  const size_t n = n_items, ns = merge ? 2 * n : n, levels = L.levels;
  const size_t qn = (size_t)kNSub * L.qcap, sn = shadow_per_item(merge) * qn;
#define PRT_LAYOUT_TAKE(m, eb, count, cond)                         \
  L.has[kW_##m] = (cond);                                           \
  L.off[kW_##m] = (cond) ? L.bytes : 0;                             \
  if (cond) L.bytes += round256((size_t)(eb) * (size_t)(count));
  PRT_WAVE_ARRAYS(PRT_LAYOUT_TAKE)
#undef PRT_LAYOUT_TAKE
  return L;
}

struct PlaneLayout {
  size_t off[kPlaneArrays];
  size_t bytes;
};
inline PlaneLayout plane_layout(uint32_t n, uint32_t iters) {
  PlaneLayout L{};
#define PRT_LAYOUT_TAKE(m, eb)  \
  L.off[kP_##m] = L.bytes;      \
  L.bytes += round256((size_t)(eb) * n * iters);
  PRT_PLANE_ARRAYS(PRT_LAYOUT_TAKE)
#undef PRT_LAYOUT_TAKE
  return L;
}

// ---- the plan of a call
// wavefront iterations of one call: one per path segment, paths x bounces; with dielectric instances a path
// is a binary tree walked depth first (one segment per iteration), at most 2^bounces - 1 segments per path
inline uint32_t wave_iters(bool dielectric, int bounces, uint32_t flags, bool merge) {
  const uint32_t paths = (flags & PRT_FLAG_AA) ? 2u : 1u;  // two camera paths per reference frame
  // merged: path 2's first segment is shaded in the iteration path 1 ends in (its primary hit traced up front)
  if (merge && paths == 2 && bounces > 0) return 2u * (uint32_t)bounces - 1u;
  if (!dielectric) return paths * (uint32_t)bounces;
  return bounces > 8 ? 0xFFFFFFFFu : paths * ((1u << bounces) - 1u);  // dst holds 4 bits per level for 8 levels
}

// The five wavefront pipelines (the kernels of each: wave_schedule):
//   Plain          render mode 0 without extensions; the misses' sky radiance by the shading itself
//   PlainDeferred  ... whose passes resolve once, behind their last traversal (prt_defer.hip), from record planes the
//                  shading of each iteration fills: rinfo, ne, nb, nk, vis and T, 72 bytes per item and iteration.  A
//                  call defers when the planes of its largest pass fit Tunables::defer_budget per wavefront state
//                  (4096 MiB by default: the bench's 1920x1080 x 2 frames x 8 iterations take 2279)
//   Merged         AA frames of render mode 0 without extensions, in calls small enough that their traversal launches
//                  are bound by their slowest rays (one launch fewer per frame: world-8 share of C4 1.83-1.87 ->
//                  1.74-1.77 ms), not by throughput (the path-2 first segments shaded in partly filled waves cost a
//                  full C4 frame 1.5 %): up to 2^21 items per call, unless Tunables::merge forces it
//   Ext            render mode 0 with an area light or dielectric instances: the EXT shading, the misses in a pass
//                  of their own (the area light can turn a hit into a miss first)
//   Debug          render modes 1-6
enum class Pipeline { Plain, PlainDeferred, Merged, Ext, Debug };
struct WavePlan {
  Pipeline pipeline = Pipeline::Plain;
  uint32_t iters = 0;     // wavefront iterations of a pass (launches 0..iters)
  // the pass split: work items are pixels x reference frames (≈ 390 B of wavefront state each); a call of more than
  // kMaxPassItems (≈ 52 GB of state), or Tunables::max_items, runs its F frames in npass passes of up to fmax frames
  // (at least one: a frame is never split), the first (largest) of F0; per: items of one frame
  int32_t F = 0, fmax = 1, npass = 1, F0 = 0;
  uint64_t per = 0;
  // Primary-hit reuse (prt_wave2.hip): the pipelines without extensions in render mode 0.  With an area light or
  // dielectrics the misses' pass rewrites hit[item] per item, and the debug modes shade from it: those keep tracing
  // P(0).  The light-visibility record rides on it: wherever it applies, unless switched off alone
  bool preuse = false, lreuse = false;
  // The primary-surface record rides on both, in the plain pipeline (deferred or not): iteration 0 of a kPrimReuse
  // pass that holds a light-visibility record fills it, or shades from it once it is valid (surface_form)
  bool sreuse = false;
  bool ifold = false;     // ... and a deferred pass that reads it folds the wave init into iteration 0 (kSurfInit)
  uint32_t dead = 2;      // dead shadow rays (prt_wave2.hip nee_live): Tunables::dead_shadow
  bool coop_tail = true;
  bool timeline = false;  // Tunables::debug_queues
  bool ext() const { return pipeline == Pipeline::Ext; }
  bool merge() const { return pipeline == Pipeline::Merged; }
  bool defer() const { return pipeline == Pipeline::PlainDeferred; }
  uint32_t items0() const { return (uint32_t)(per * (uint64_t)F0); }  // items of the first pass
};

// The plan of a call of `spp` samples over `per` items per frame, or an error code (include/prt.h) and its text.
// Pure: the same arguments give the same plan
inline int plan_render(int32_t render_mode, uint32_t flags, int32_t bounces, int32_t spp, uint64_t per, bool area,
                       bool diel, const Tunables& t, WavePlan& P, const char*& err) {
  P = WavePlan{};
  if (per > kMaxPassItems) {
    err = "more than 2^27 pixels in one frame of one shard";
    return PRT_ERR_UNSUPPORTED;
  }
  const bool aa = (flags & PRT_FLAG_AA) != 0;
  const int32_t F = aa ? spp / 2 : spp;
  const bool mode0 = render_mode == 0;
  const bool ext = (area || diel) && mode0;
  const bool plain = !ext && mode0 && bounces > 0;  // what merging, deferring and primary-hit reuse all need
  bool merge = plain && aa && per <= kMaxMergedPassItems;
  if (t.merge >= 0) merge = merge && t.merge != 0;
  else merge = merge && per * (uint64_t)F <= (1ull << 21);
  const uint64_t pass_cap = merge ? kMaxMergedPassItems : kMaxPassItems;
  const uint64_t max_items = t.max_items ? std::min(t.max_items, pass_cap) : pass_cap;
  P.F = F;
  P.per = per;
  P.fmax = (int32_t)std::max<uint64_t>(1, max_items / std::max<uint64_t>(per, 1));
  P.npass = F > P.fmax ? (F + P.fmax - 1) / P.fmax : 1;
  P.F0 = std::min(F, P.fmax);
  P.iters = wave_iters(diel, bounces, flags, merge);
  if (P.iters > (uint32_t)kMaxIters) {
    err = diel ? "dielectric path trees exceed the wavefront iteration limit (lower bounces)"
               : "too many wavefront iterations";
    return PRT_ERR_UNSUPPORTED;
  }
  // deferred: sized for the first (largest) pass; later passes hold no more items
  const bool defer = plain && !merge && P.items0() != 0 && t.defer &&
                     plane_layout(P.items0(), P.iters).bytes <= t.defer_budget;
  P.pipeline = merge ? Pipeline::Merged : !mode0 ? Pipeline::Debug : ext ? Pipeline::Ext
               : defer ? Pipeline::PlainDeferred : Pipeline::Plain;
  P.preuse = plain && t.primary_reuse && per > 0 && F > 0;
  P.lreuse = P.preuse && t.shadow_reuse;
  P.sreuse = P.lreuse && !merge && t.surface_reuse;
  P.ifold = P.sreuse && defer && t.init_fold;
  P.dead = t.dead_shadow;
  P.coop_tail = t.coop_tail;
  P.timeline = t.debug_queues;
  return PRT_OK;
}

// ---- the kernels of launch `it` (0..iters) of a pass: one value per instantiation launch_wave2_iter can launch
// (prt_wave2.hip; the Shade2d / ResolvePass forms: prt_defer.hip).  Learn: the forms that use (shading of iteration 0)
// and fill (the resolve of launch 1, or of a deferred pass) the light-visibility record
enum class Kernel {
  None,
  Trace2, Trace2Dense,                                        // k_trace2, its dense primary pass (launch_trace2)
  Res2d, Res2dLearn, Res2md, Res2mdLearn,                     // k_res2d<L>, k_res2md<L>
  ResolvePass, ResolvePassLearn,                              // k_resolve_pass<L>
  Miss2, Miss2Ext, ResMiss2, ResMiss2Ext,                     // k_miss2<EXT>, k_resmiss2<EXT> (misses = 1)
  Shade2, Shade2Learn, Shade2Ext, Shade2Debug,                // k_shade2<false, L>, k_shade2<true>, k_shade2_debug
  Shade2d, Shade2dLearn, Shade2m, Shade2mLearn,               // k_shade2d<L>, k_shade2m<L>
  Shade2sFill, Shade2sRead, Shade2sdFill, Shade2sdRead,       // k_shade2s<DEFER, SURF> (prt_surface.hip)
  Shade2sdInit,                                               // k_shade2s<true, kSurfInit>
  WaveInit,                                                   // k_wave_init (pass_init)
};
struct Schedule {
  Kernel trace, resolve, shade;
};
// What a pass's iteration 0 does with the primary-surface record: lrec as wave_schedule's, valid: the state's record
// belongs to its primary hits, the shading epoch and the call's normal-map and skybox flags (prt_api_render.cpp)
inline int surface_form(const WavePlan& P, bool lrec, bool valid) {
  if (!P.sreuse || !lrec) return kSurfNone;
  return valid ? (P.ifold ? kSurfInit : kSurfRead) : kSurfFill;
}
// the kernel in front of launch 0 of a pass: k_wave_init, unless iteration 0 does its work (kSurfInit: q0 is then
// neither written nor read, and the shading counts the items into P(0)'s counters itself)
inline Kernel pass_init(int surf) { return surf == kSurfInit ? Kernel::None : Kernel::WaveInit; }
// lrec: the pass runs with kPrimReuse and holds a light-visibility record.  The extension and debug pipelines always
// trace their primaries (kPrimTrace) and hold no record
// surf: surface_form's answer for the pass (the plain pipelines, with lrec)
inline Schedule wave_schedule(Pipeline p, bool lrec, int32_t pmode, uint32_t it, uint32_t iters, int surf = kSurfNone) {
  const bool plainish = p == Pipeline::Plain || p == Pipeline::PlainDeferred;
  assert(!lrec || pmode == kPrimReuse);
  assert(surf == kSurfNone || (lrec && plainish));
  assert(surf != kSurfInit || p == Pipeline::PlainDeferred);
  assert((plainish || p == Pipeline::Merged) || (pmode == kPrimTrace && !lrec));
  const bool learn_res = lrec && it == 1, learn_shade = lrec && it == 0;
  Schedule s{Kernel::Trace2, Kernel::None, Kernel::None};
  // launch 0 of a kPrimReuse pass has no path-1 primary to trace: nothing at all in the plain pipelines (no shadow
  // rays yet), the path-2 primaries in the merged one
  if (it == 0 && pmode == kPrimDense) s.trace = Kernel::Trace2Dense;
  else if (it == 0 && pmode == kPrimReuse && plainish) s.trace = Kernel::None;
  switch (p) {
    case Pipeline::Plain:
      if (it > 0) s.resolve = learn_res ? Kernel::Res2dLearn : Kernel::Res2d;
      s.shade = learn_shade ? Kernel::Shade2Learn : Kernel::Shade2;
      if (learn_shade && surf != kSurfNone) s.shade = surf == kSurfRead ? Kernel::Shade2sRead : Kernel::Shade2sFill;
      break;
    case Pipeline::PlainDeferred:  // one resolve per pass, behind the last traversal launch
      if (it == iters) s.resolve = lrec ? Kernel::ResolvePassLearn : Kernel::ResolvePass;
      s.shade = learn_shade ? Kernel::Shade2dLearn : Kernel::Shade2d;
      if (learn_shade && surf != kSurfNone)
        s.shade = surf == kSurfInit ? Kernel::Shade2sdInit : surf == kSurfRead ? Kernel::Shade2sdRead : Kernel::Shade2sdFill;
      break;
    case Pipeline::Merged:
      if (it > 0) s.resolve = learn_res ? Kernel::Res2mdLearn : Kernel::Res2md;
      s.shade = learn_shade ? Kernel::Shade2mLearn : Kernel::Shade2m;
      break;
    case Pipeline::Ext:  // the misses of P(it), behind the resolve of P(it - 1) from launch 1 on
      s.resolve = it > 0 ? Kernel::ResMiss2Ext : Kernel::Miss2Ext;
      s.shade = Kernel::Shade2Ext;
      break;
    case Pipeline::Debug:
      s.resolve = it > 0 ? Kernel::ResMiss2 : Kernel::Miss2;
      s.shade = Kernel::Shade2Debug;
      break;
  }
  if (it >= iters) s.shade = Kernel::None;
  return s;
}

}  // namespace prt
