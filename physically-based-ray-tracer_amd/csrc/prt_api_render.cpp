// prt_api_render.cpp -- the render path of the C ABI (include/prt.h): a call's plan (prt_plan.h), its wavefront
// state, the enqueue of its passes, frames in flight, stats and the sharded frame; prt_render, prt_render_tiles,
// prt_untile, the ray-total readers and the accumulation checkpoints.  The scene side is prt_api.cpp,
// its meshes prt_api_mesh.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "prt_ctx.h"

using namespace prt;
using namespace prt::host;

namespace {

int check_params(const prt_render_params* p) {
  if (!p) return fail(PRT_ERR_INVALID_ARGUMENT, "params is NULL");
  if (p->width <= 0 || p->height <= 0 || p->width > 16384 || p->height > 16384)
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad resolution");
  if (p->spp < 0) return fail(PRT_ERR_INVALID_ARGUMENT, "spp < 0");
  if ((p->flags & PRT_FLAG_AA) && (p->spp % 2) != 0)
    return fail(PRT_ERR_INVALID_ARGUMENT, "with PRT_FLAG_AA spp must be even (2 paths per reference frame)");
  if (p->bounces < 0 || p->bounces > 16) return fail(PRT_ERR_INVALID_ARGUMENT, "bounces must be in [0,16]");
  if (p->render_mode < 0 || p->render_mode > 6) return fail(PRT_ERR_INVALID_ARGUMENT, "bad render_mode");
  return PRT_OK;
}

int ensure_state(prt_ctx* c, int32_t W, int32_t H) {
  if (c->accW == W && c->accH == H && c->acc.p) return PRT_OK;
  if (c->acc.p) {  // a new image size: the frames still queued (or in flight) read the old state
    const int rc = drain(c);
    if (rc) return rc;
  }
  const size_t n = (size_t)W * H;
  HIP_TRY(c->acc.ensure(n * 16));
  HIP_TRY(c->nsamp.ensure(n * 4));
  HIP_TRY(c->dist.ensure(n * 4));
  HIP_TRY(hipMemsetAsync(c->acc.p, 0, n * 16, c->stream));
  HIP_TRY(hipMemsetAsync(c->nsamp.p, 0, n * 4, c->stream));
  std::vector<float> d(n, -1.0f);  // Core/Renderer.h:62 (distances = -1 -> first frame resets)
  HIP_TRY(hipMemcpyAsync(c->dist.p, d.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->accW = W;
  c->accH = H;
  return PRT_OK;
}

// wavefront buffers sized for n items and (bounces-1) (result, throughput) stack levels, laid out by wave_layout
// (prt_plan.h).  needR: the pass resolves per iteration and stacks results
int ensure_wave(WaveState& ws, uint32_t n, int bounces, bool ext, bool merge, bool needR) {
  const WaveLayout L = wave_layout(n, bounces, ext, merge, needR);
  WaveBufs& W = ws.wb;
  W.n = n;  // (an allocation kept: capacity stays; the SoA strides (R/T: depth * n + item) follow the current n)
  W.qcap = L.qcap;
  W.scap = L.scap;
  W.merge = merge ? 1 : 0;
  if (ws.n >= n && ws.levels >= L.levels && (ws.ext || !ext) && (ws.merge || !merge) && (ws.hasR || !needR) &&
      ws.wave.p)
    return PRT_OK;
  HIP_TRY(ws.wave.ensure(L.bytes));
  char* b = ws.wave.as<char>();
  W.base = 0;
#define PRT_POINT(m, ...) W.m = L.has[kW_##m] ? reinterpret_cast<decltype(W.m)>(b + L.off[kW_##m]) : nullptr;
  PRT_WAVE_ARRAYS(PRT_POINT)
#undef PRT_POINT
  ws.n = n;
  ws.levels = L.levels;
  ws.ext = ext;
  ws.merge = merge;
  ws.hasR = needR;
  return PRT_OK;
}

// deferred resolve: the record pointers of W -> plane 0 of the planes laid out for n items and `iters` iterations
// (plane_layout, prt_plan.h)
void point_planes(WaveBufs& W, const DevBuf& planes, uint32_t n, uint32_t iters) {
  const PlaneLayout L = plane_layout(n, iters);
  char* b = planes.as<char>();
#define PRT_POINT(m, ...) W.m = reinterpret_cast<decltype(W.m)>(b + L.off[kP_##m]);
  PRT_PLANE_ARRAYS(PRT_POINT)
#undef PRT_POINT
  W.R = nullptr;
}

// the context's running ray totals (prt_ray_totals): bytes 16-31 of the diag buffer, zeroed at prt_create
Counters* ray_totals_dev(prt_ctx* c) { return reinterpret_cast<Counters*>(c->diag.as<char>() + 16); }

// k_shade2 reads its arguments through the kernarg segment (prt_shade2.h Shade2Args) and flags diag[1] when the
// layout it assumes is not the compiler's (it then shades nothing).  Checked once per context, after its first
// render (one host wait), so stats-less frame loops fail loudly too; prt_ray_totals re-checks it
int check_layout_once(prt_ctx* c, hipStream_t st) {
  if (c->layout_checked) return PRT_OK;
  uint32_t v[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(v, c->diag.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (v[1] != 0) return fail(PRT_ERR_HIP, "k_shade2: kernel-argument layout check failed (Shade2Args)");
  c->layout_checked = true;
  return PRT_OK;
}

// the wavefront state and frame buffer of a call: slot 0 of the frames in flight and a call in the context stream's
// order share the context's own (they never overlap: the latter joins the flights first)
WaveState& flight_ws(prt_ctx* c, Flight* fl) { return (fl && fl != &c->fl[0]) ? fl->ws : c->ws; }
DevBuf& flight_frames(prt_ctx* c, Flight* fl) { return (fl && fl != &c->fl[0]) ? fl->frames : c->frames; }

// everything a render needs that can fail: validation and every allocation.  prepare_render enqueues no
// rendering work (ensure_state's first-use clears aside), so a failure leaves the accumulation state as it was
// and a sharded frame can still post its gather (render_sharded)
struct RenderPlan {
  SceneDev S;
  TraceArgs A;
  WavePlan plan;  // the pipeline, the pass split and the switches of the call (prt_plan.h plan_render)
};

// the key of the primary hits a call with scene S and tile map M would trace
PrimKey prim_key(const prt_ctx* c, const SceneDev& S, const TileMap& M) {
  PrimKey k;
  std::memset(&k, 0, sizeof(k));
  std::memcpy(k.cam, S.cam, sizeof(k.cam));
  std::memcpy(k.basis, S.basis, sizeof(k.basis));
  k.pan_b = S.pan_b; k.pan_d = S.pan_d; k.panini = S.panini;
  k.W = M.W; k.H = M.H; k.ts = M.ts; k.rank = M.rank; k.world = M.world;
  k.scene_epoch = c->scene_epoch;
  k.inst_epoch = c->inst_epoch;
  return k;
}

// some mesh has an emission texture: the primary-surface record needs its emission plane
bool surf_emissive(const prt_ctx* c) {
  for (const MeshDev& m : c->mesh_host)
    if (m.tex[3] >= 0) return true;
  return false;
}

int prepare_render(prt_ctx* c, const prt_render_params* p, const TileMap& M, int32_t rank, RenderPlan& R,
                   Flight* fl = nullptr) {
  SceneDev& S = R.S;
  const Tunables tun = read_tunables();  // the environment switches, once per call
  // fault injection (tests of the sharded error paths): PRT_FAIL_RENDER=<rank> makes that shard's render fail here,
  // before anything is enqueued ("all": every context)
  if (tun.fail_all || tun.fail_rank == rank)
    return fail(PRT_ERR_HIP, "injected render failure (PRT_FAIL_RENDER) on shard " + std::to_string(rank));
  int rc = scene_ready(c, S);
  if (rc) return rc;
  if (!c->have_camera) return fail(PRT_ERR_NOT_READY, "no camera: call prt_set_camera");
  if (!c->have_lights) return fail(PRT_ERR_NOT_READY, "no lights: call prt_set_lights");
  if (!depth_ok(c)) return fail(PRT_ERR_UNSUPPORTED, "BVH deeper than 64 levels");
  // the call's pipeline and passes, each pass folded into the accumulation state in order (the reference's frame
  // sequence); one frame (of this shard) may hold at most 2^27 pixels
  WavePlan& P = R.plan;
  const char* why = "";
  rc = plan_render(p->render_mode, p->flags, p->bounces, p->spp, (uint64_t)M.items, S.area != 0, S.has_diel != 0,
                   tun, P, why);
  if (rc) return fail(rc, why);
  rc = ensure_spill(c, S, 0);
  if (rc) return rc;
  rc = ensure_state(c, p->width, p->height);
  if (rc) return rc;
  DevBuf& frames = flight_frames(c, fl);
  HIP_TRY(frames.ensure(sizeof(float4) * (size_t)std::max<uint32_t>(P.items0(), 1)));
  TraceArgs& A = R.A;
  A.W = p->width; A.H = p->height; A.bounces = p->bounces; A.flags = p->flags; A.mode = p->render_mode;
  A.frame_index = p->frame_index; A.seed = p->seed; A.frames = P.F0;
  // sized for the first (largest) pass; later passes hold no more items
  WaveState& ws = flight_ws(c, fl);
  rc = ensure_wave(ws, P.items0(), p->bounces, P.ext(), P.merge(), !P.defer());
  if (rc) return rc;
  if (P.defer()) HIP_TRY(ws.planes.ensure(plane_layout(P.items0(), P.iters).bytes));
  if (P.preuse) {  // this chain's copy of the primary hits; a new allocation holds nothing yet
    const void* before = ws.phit.p;
    HIP_TRY(ws.phit.ensure(sizeof(float4) * (size_t)P.per));
    if (ws.phit.p != before) ws.pvalid = false;
  }
  if (P.lreuse) {  // and of the light-visibility record
    const void* lbefore = ws.lvis.p;
    HIP_TRY(ws.lvis.ensure(sizeof(uint2) * (size_t)P.per));
    if (ws.lvis.p != lbefore) ws.lvalid = false;
  }
  if (P.sreuse) {  // and of the primary-surface record: three 16-byte words per entry, the emission plane if needed
    const void* sbefore = ws.surf.p;
    const void* ebefore = ws.surf_e.p;
    HIP_TRY(ws.surf.ensure(3 * round256(sizeof(float4) * (size_t)P.per)));
    if (surf_emissive(c)) HIP_TRY(ws.surf_e.ensure(sizeof(float4) * (size_t)P.per));
    if (ws.surf.p != sbefore || ws.surf_e.p != ebefore) ws.svalid = false;
  }
  return PRT_OK;
}

// the shared trace + accumulate sequence for prt_render / prt_render_tiles, after prepare_render: enqueues the
// render on the context stream; want_stats: per-launch timers + read_stats() afterwards
// fl: a frame in flight (its stream, wavefront state and frame buffer; the accumulation first waits for acc_after,
// the previous call's last work), else the context stream and state
int enqueue_render_body(prt_ctx* c, const prt_render_params* p, const TileMap& M, RenderPlan& R, float4* avg_dev,
                        uint32_t* rgb8_dev, float4* tiles_dev, bool want_stats, Flight* fl, hipEvent_t acc_after);
// one call's frames on the flight's stream (or the context stream), then the mark of its read of the instance state
int enqueue_render(prt_ctx* c, const prt_render_params* p, const TileMap& M, RenderPlan& R, float4* avg_dev,
                   uint32_t* rgb8_dev, float4* tiles_dev, bool want_stats, Flight* fl = nullptr,
                   hipEvent_t acc_after = nullptr) {
  const int rc = enqueue_render_body(c, p, M, R, avg_dev, rgb8_dev, tiles_dev, want_stats, fl, acc_after);
  const int urc = record_inst_use(c, fl ? fl->stream : c->stream);
  return rc ? rc : urc;
}
int enqueue_render_body(prt_ctx* c, const prt_render_params* p, const TileMap& M, RenderPlan& R, float4* avg_dev,
                        uint32_t* rgb8_dev, float4* tiles_dev, bool want_stats, Flight* fl, hipEvent_t acc_after) {
  SceneDev& S = R.S;
  TraceArgs& A = R.A;
  const WavePlan& P = R.plan;
  const int32_t F = P.F, fmax = P.fmax, npass = P.npass;
  const uint64_t per = P.per;
  const uint32_t iters = P.iters;
  int rc = PRT_OK;
  const hipStream_t st = fl ? fl->stream : c->stream;
  WaveState& ws0 = flight_ws(c, fl);
  LaunchCfg L{st, occ_for(c), 1};
  // frames in flight: from 4 frames in flight on, each chain's wavefront grids are a fraction of the resident blocks,
  // so the chains' persistent traversal launches co-reside instead of taking the whole GPU in turns: a third for
  // calls of up to 2^20 items (C4 world-8 share 1.101-1.109 ms with half grids, 1.055-1.062 with a third, 1.079-1.085
  // with a quarter, 1.32 with an eighth; world 4: 1.940-1.949 / 1.878-1.907 / 1.945-1.953 ms), half above (world 2:
  // 3.56-3.57 ms with half grids, 3.72-3.74 with a quarter) -- profiles/r06_ab_flight_grids.txt
#ifdef PRT_FLIGHT_GW  // (A/B builds only)
  const uint32_t Gw = (fl && c->inflight >= 4) ? (uint32_t)PRT_FLIGHT_GW : 1u;
#else
  const uint32_t Gw = (fl && c->inflight >= 4) ? (per * (uint64_t)P.F0 <= (1ull << 20) ? 3u : 2u) : 1u;
#endif
  const LaunchCfg Lw{st, L.occ, Gw};  // the wavefront chain's launches
  // the call's own events (prt_stats ms / ms_trace) only with stats: each record is a gap between kernels
  if (want_stats) HIP_TRY(hipEventRecord(c->ev[0], st));
  // per-launch traversal timers (HIP events around every k_trace launch) with stats (one-pass calls): each event
  // record costs a few us between kernels, so only the stats calls carry them
  const bool timers = want_stats && npass == 1;
  unsigned long long* tl = nullptr;
  if (want_stats && P.timeline) {
    const size_t tlb = 32ull * kTlWaves * (kMaxIters + 2);
    HIP_TRY(c->tl.ensure(tlb));
    HIP_TRY(hipMemsetAsync(c->tl.p, 0, tlb, st));
    tl = c->tl.as<unsigned long long>();
  }
  c->carry_segments = c->carry_shadow = 0;
  const bool post = c->pfx.enabled && !tiles_dev && rgb8_dev && F > 0;
  for (int32_t pass = 0; pass < npass; pass++) {
    const int32_t f0 = pass * fmax, Fb = npass == 1 ? F : std::min(fmax, F - f0);
    const bool last = pass == npass - 1;
    A.frame_index = p->frame_index + f0;
    A.frames = Fb;
    const uint64_t nb = per * (uint64_t)Fb;  // this pass's items
    float4* frames = flight_frames(c, fl).as<float4>();
    // (no allocation: prepare_render sized it for pass 0)
    rc = ensure_wave(ws0, (uint32_t)nb, p->bounces, P.ext(), P.merge(), !P.defer());
    if (rc) return rc;
    ws0.wb.base = 0;
    ws0.wb.coop_tail = P.coop_tail ? 1 : 0;
    ws0.wb.tl = tl;
    // primary-hit reuse: a stale stamp makes this pass's launch 0 the dense pass over its first frame (base is 0:
    // items [0, per)), which fills this chain's phit; the later passes of the call and the later calls on this
    // state reuse it until the key changes.  The stamp is set when the dense pass is enqueued: everything that
    // reads phit afterwards follows it on this state's stream
    ws0.wb.phit = ws0.phit.as<float4>();
    ws0.wb.pitems = (uint32_t)per;
    ws0.wb.pmode = kPrimTrace;
    ws0.wb.lvis = nullptr;
    ws0.wb.lslot = iters + 1;
    ws0.wb.dead = P.dead;
    if (P.preuse && nb > 0) {
      const PrimKey key = prim_key(c, S, M);
      const uint64_t px = tile_image_pixels(M);  // the tile map's entries that have a pixel (and a ray)
      if (ws0.pvalid && std::memcmp(&ws0.pkey, &key, sizeof(key)) == 0) {
        ws0.wb.pmode = kPrimReuse;
        c->prim_reused += px * (uint64_t)Fb;
        // the light-visibility record: used and filled by kPrimReuse passes only (a camera that moves every call
        // pays nothing).  One learned on other primary hits (a dense pass since) or under other light positions
        // is cleared, on this state's stream, before the pass reads it
        if (P.lreuse) {
          float lp[18];
          std::memcpy(lp, S.ppos, sizeof(S.ppos));
          std::memcpy(lp + 12, S.dpos, sizeof(S.dpos));
          std::memcpy(lp + 15, S.spos, sizeof(S.spos));
          if (!(ws0.lvalid && ws0.lgen == ws0.pgen && std::memcmp(lp, ws0.lpos, sizeof(lp)) == 0)) {
            ws0.lvalid = false;
            HIP_TRY(hipMemsetAsync(ws0.lvis.p, 0, sizeof(uint2) * (size_t)per, st));
            ws0.lgen = ws0.pgen;
            std::memcpy(ws0.lpos, lp, sizeof(lp));
            ws0.lvalid = true;
          }
          ws0.wb.lvis = ws0.lvis.as<uint2>();
        }
      } else {
        ws0.wb.pmode = kPrimDense;
        ws0.pgen++;
        ws0.pkey = key;
        ws0.pvalid = false;  // (until the pass is enqueued: a failed enqueue leaves the stamp stale)
        c->prim_traced += px;
        c->prim_reused += px * (uint64_t)(Fb - 1);
      }
    }
    {  // the queue counters and the fetch counters of the iterations this call uses (kMaxIters is the capacity)
      const size_t qw = (size_t)(iters + 2) * 2 * kNSub * kCtrStride;
      const size_t fbase = (size_t)(kMaxIters + 2) * 2 * kNSub * kCtrStride;
      const size_t fw = (size_t)(iters + 2) * 2 * kParts * kCtrStride;
      HIP_TRY(launch_clear2(Lw, ws0.wb.ctr, (uint32_t)qw, ws0.wb.ctr + fbase, (uint32_t)fw));
    }
    if (P.ext() && S.has_diel) HIP_TRY(hipMemsetAsync(ws0.wb.dst, 0, 4ull * ws0.wb.n, st));
    // deferred resolve: the launches get the record planes (laid out for this pass's items) in place of the state's
    // per-item records; k_wave_init clears the status words of plane 0
    WaveBufs wb = ws0.wb;
    if (P.defer()) point_planes(wb, ws0.planes, (uint32_t)nb, iters);
    const bool lrec = wb.pmode == kPrimReuse && wb.lvis != nullptr;  // the pass uses and fills the record
    // the primary-surface record: valid for the primary hits it was filled on, the shading epoch, the two flags its
    // values depend on and the presence of the emission plane.  A stale one is refilled by this pass's iteration 0
    // (every entry is rewritten: no clearing) and stamped once the pass is enqueued, in stream order as phit's stamp
    const uint32_t sfl = p->flags & (PRT_FLAG_NORMALMAP | PRT_FLAG_SKYBOX);
    const bool semis = surf_emissive(c);
    const int surf = surface_form(P, lrec, ws0.svalid && ws0.sgen == ws0.pgen && ws0.sepoch == c->shade_epoch &&
                                               ws0.sflags == sfl && ws0.semis == semis);
    SurfBufs sb{};
    if (surf != kSurfNone) {
      const size_t plane = round256(sizeof(float4) * (size_t)per);
      sb.n4 = reinterpret_cast<float4*>(ws0.surf.as<char>());
      sb.b4 = reinterpret_cast<float4*>(ws0.surf.as<char>() + plane);
      sb.i4 = reinterpret_cast<float4*>(ws0.surf.as<char>() + 2 * plane);
      sb.e4 = semis ? ws0.surf_e.as<float4>() : nullptr;
      if (surf == kSurfFill) ws0.svalid = false;  // (until the pass is enqueued)
      else c->surf_reused += tile_image_pixels(M) * (uint64_t)Fb;
    }
    // (a pass whose iteration 0 reads the record with the init folded in launches no k_wave_init: prt_plan.h pass_init)
    if (pass_init(surf) == Kernel::WaveInit) HIP_TRY(launch_wave_init(Lw, S, A, M, wb, frames));
    for (uint32_t it = 0; it <= iters; it++)
      HIP_TRY(launch_wave2_iter(Lw, S, A, M, wb, frames, timers ? &c->wt : nullptr, P, lrec, it, surf, &sb));
    if (ws0.wb.pmode == kPrimDense) ws0.pvalid = true;
    if (surf == kSurfFill) {
      ws0.sgen = ws0.pgen;
      ws0.sepoch = c->shade_epoch;
      ws0.sflags = sfl;
      ws0.semis = semis;
      ws0.svalid = true;
    }
    if (last && want_stats) HIP_TRY(hipEventRecord(c->ev[1], st));
    // post-processing (single-GPU image): the screen pass needs the average and, for the aberration, the
    // accumulator before the last frame
    float4* acc_prev = nullptr;
    if (post && last) {
      const size_t np = (size_t)p->width * p->height;
      if (!avg_dev) { HIP_TRY(c->avg.ensure(np * 16)); avg_dev = c->avg.as<float4>(); }
      if (c->pfx.aberration != 0) { HIP_TRY(c->accprev.ensure(np * 16)); acc_prev = c->accprev.as<float4>(); }
    }
    // frames in flight: the accumulation state (and outputs, ray totals) are updated in call order
    if (acc_after) HIP_TRY(hipStreamWaitEvent(st, acc_after, 0));
    HIP_TRY(launch_accumulate(L, M, Fb, p->flags, frames, c->acc.as<float4>(), c->nsamp.as<int32_t>(),
                              c->dist.as<float>(), avg_dev, post ? nullptr : rgb8_dev, tiles_dev, acc_prev,
                              ws0.wb.ctr, iters, ray_totals_dev(c)));
    if (post && last) {
      // with !accumulates the accumulator held this frame's value until the end-of-frame memset
      const float4* acc_new = (p->flags & PRT_FLAG_ACCUMULATE) ? c->acc.as<float4>() : avg_dev;
      HIP_TRY(launch_postfx(L, post_params(c, p->width, p->height), acc_new, acc_prev, c->nsamp.as<int32_t>(),
                            avg_dev, rgb8_dev));
    }
    if (want_stats && !last) {  // this pass's ray counts, before the next pass clears the counters
      std::vector<uint32_t> ctr((size_t)(iters + 2) * 2 * kNSub * kCtrStride);
      HIP_TRY(hipMemcpyAsync(ctr.data(), ws0.wb.ctr, 4 * ctr.size(), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (uint32_t k = 0; k < iters + 2; k++)  // (+2: the merged path-2 primaries are counted at iters + 1)
        for (uint32_t s2 = 0; s2 < kNSub; s2++) {
          c->carry_segments += ctr[((k * 2 + 0) * kNSub + s2) * kCtrStride];
          c->carry_shadow += ctr[((k * 2 + 1) * kNSub + s2) * kCtrStride];
        }
    }
  }
  if (want_stats) HIP_TRY(hipEventRecord(c->ev[2], st));
  c->last_iters = iters;
  c->last_defer = P.defer();
  c->last_timers = timers;
  c->last_paths = tile_image_pixels(M) * (uint64_t)F * ((p->flags & PRT_FLAG_AA) ? 2u : 1u);
  return check_layout_once(c, st);
}

// frames in flight: the slot the next call takes (calls with stats or host outputs run in the context stream's
// order instead)
Flight* flight_for(prt_ctx* c, bool sync) {
  return (c->inflight > 1 && !sync && c->sh_kind != 2) ? &c->fl[c->next_fl] : nullptr;
}
// the call of slot f is enqueued: its stream forked from the context stream (fork_flight) before its first work;
// land_flight then joins the call inflight - 1 back into the context stream (its outputs are complete in the
// caller's order from now on), so up to `inflight` calls overlap
int fork_flight(prt_ctx* c, Flight& f) {
  HIP_TRY(hipEventRecord(c->fl_fork, c->stream));
  HIP_TRY(hipStreamWaitEvent(f.stream, c->fl_fork, 0));
  return PRT_OK;
}
int land_flight(prt_ctx* c, Flight& f) {
  HIP_TRY(hipEventRecord(f.done, f.stream));
  const int32_t s = (int32_t)(&f - c->fl), nxt = (s + 1) % c->inflight;
  Flight& o = c->fl[nxt];  // the call inflight - 1 back, whose slot the next call takes
  if (o.pending) {
    HIP_TRY(hipStreamWaitEvent(c->stream, o.done, 0));
    o.pending = false;
  }
  f.pending = true;
  c->last_fl = s;
  c->next_fl = nxt;
  return PRT_OK;
}
// the event the next call's accumulation waits for: the last call still in flight (none: the context stream orders)
hipEvent_t flight_after(const prt_ctx* c) { return c->last_fl >= 0 ? c->fl[c->last_fl].done : nullptr; }

int run_render(prt_ctx* c, const prt_render_params* p, const TileMap& M, float4* avg_dev, uint32_t* rgb8_dev,
               float4* tiles_dev, bool want_stats, int32_t rank = 0, bool sync = true) {
  Flight* f = flight_for(c, want_stats || sync);
  int rc = f ? PRT_OK : join_flights(c);
  if (rc) return rc;
  RenderPlan R;
  rc = prepare_render(c, p, M, rank, R, f);
  if (rc) return rc;
  if (!f) return enqueue_render(c, p, M, R, avg_dev, rgb8_dev, tiles_dev, want_stats);
  rc = fork_flight(c, *f);
  if (rc) return rc;
  rc = enqueue_render(c, p, M, R, avg_dev, rgb8_dev, tiles_dev, false, f, flight_after(c));
  const int lrc = land_flight(c, *f);  // a failed call's partial work joins the context stream too
  if (rc) {
    const std::string why = last_error();
    (void)join_flights(c);
    return fail(rc, why);
  }
  return lrc;
}

}  // namespace

// the context's traversal stack overflow count (SceneDev::diag[0]); waits for the context stream.  diag[1] != 0:
// a kernel found its kernarg layout assumption broken (prt_shade2.h Shade2Args) and did no work; diag[2] != 0: the
// stream's wait for a worker build of the instance BVH timed out (k_wait_host)
uint64_t prt::host::diag_overflows(prt_ctx* c, bool* layout_ok, bool* wait_ok) {
  uint32_t v[3] = {0, 0, 0};
  if (hipMemcpyAsync(v, c->diag.p, 12, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return ~0ull;  // unreadable counts as overflowed: never report a clean run that was not checked
  if (layout_ok) *layout_ok = v[1] == 0;
  if (wait_ok) *wait_ok = v[2] == 0;
  return v[0];
}

namespace {

// waits for the last render of run_render(..., want_stats = true) and fills its stats
int read_stats(prt_ctx* c, prt_stats* stats) {
#ifdef PRT_LANE_STATS
  HIP_TRY(hipStreamSynchronize(c->stream));
  lane_stats_dump();
#endif
  const uint32_t iters = c->last_iters;
  const bool timers = c->last_timers;
  {
    std::memset(stats, 0, sizeof(*stats));
    // per-launch traversal times summed over every launch
    const bool dump = debug_queues_on();
    // the queue counters of the iterations this render used (the whole array with the queue dump)
    std::vector<uint32_t> ctr(dump ? kCtrWords : (size_t)(iters + 2) * 2 * kNSub * kCtrStride);
    HIP_TRY(hipMemcpyAsync(ctr.data(), c->ws.wb.ctr, 4 * ctr.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const WaveTimers& wt = c->wt;
    for (uint32_t k = 0; k <= iters + 1; k++) {  // iteration iters + 1: the merged path-2 primaries (Q2)
      uint64_t qs = 0, qa = 0;
      for (uint32_t s = 0; s < kNSub; s++) {
        qs += ctr[((k * 2 + 0) * kNSub + s) * kCtrStride];
        qa += ctr[((k * 2 + 1) * kNSub + s) * kCtrStride];
      }
      stats->segments += qs;
      stats->shadow_rays += qa;
      float a = 0;
      if (timers && k <= iters) HIP_TRY(hipEventElapsedTime(&a, wt.ev[4 * k + 0], wt.ev[4 * k + 1]));
      stats->ms_closest += a;  // one merged trace launch per iteration plus the final shadow-only one
      if (dump && k < iters)
        std::fprintf(stderr, "prt: iteration %u: %llu closest rays, %llu shadow rays; trace launch %.3f ms\n", k,
                     (unsigned long long)qs, (unsigned long long)qa, a);
    }
    if (dump && c->ws.wb.tl) {  // launch timeline: start -> queue drained -> last wave out (us)
      std::vector<unsigned long long> t(4ull * kTlWaves * (kMaxIters + 2));
      HIP_TRY(hipMemcpy(t.data(), c->tl.p, 8 * t.size(), hipMemcpyDeviceToHost));
      for (uint32_t k = 0; k <= iters; k++) {
        unsigned long long s0 = ~0ull, d0 = ~0ull;
        std::vector<double> ex;
        for (int w = 0; w < kTlWaves; w++) {
          const unsigned long long* r = t.data() + 4 * ((size_t)k * kTlWaves + w);
          if (!r[0]) continue;
          s0 = std::min(s0, r[0]);
          if (r[1]) d0 = std::min(d0, r[1]);
        }
        if (s0 == ~0ull || d0 == ~0ull) continue;
        for (int w = 0; w < kTlWaves; w++) {
          const unsigned long long* r = t.data() + 4 * ((size_t)k * kTlWaves + w);
          if (r[0] && r[2]) ex.push_back(((double)r[2] - (double)d0) / 100.0);
        }
        std::sort(ex.begin(), ex.end());
        auto q = [&](double pp) { return ex.empty() ? 0.0 : ex[std::min(ex.size() - 1, (size_t)(pp * ex.size()))]; };
        std::fprintf(stderr, "prt: trace %u: %zu waves, queue empty after %.1f us; waves out at +%.1f / +%.1f / "
                     "+%.1f / +%.1f us (50/90/99/100 %%)\n", k, ex.size(), (d0 - s0) / 100.0, q(0.5), q(0.9),
                     q(0.99), ex.empty() ? 0.0 : ex.back());
        // diagnostic builds (PRT_TAIL_STATS): where the waves that left last (top 5 %) spent the time after the
        // queue emptied: main loop until their tail entry, then the cooperative tail
        struct Late { double out, entry, tail; unsigned owners, iters; };
        std::vector<Late> late;
        for (int w = 0; w < kTlWaves; w++) {
          const unsigned long long* r = t.data() + 4 * ((size_t)k * kTlWaves + w);
          if (!r[0] || !r[2] || !r[3]) continue;
          unsigned long long e = (r[2] & ~0xFFFFFFFFull) | (r[3] >> 32);
          if (e > r[2]) e -= 1ull << 32;
          late.push_back({((double)r[2] - (double)d0) / 100.0, ((double)e - (double)d0) / 100.0,
                          ((double)r[2] - (double)e) / 100.0, (unsigned)(r[3] & 0xFF),
                          (unsigned)((r[3] >> 8) & 0xFFFFFF)});
        }
        if (!late.empty()) {
          std::sort(late.begin(), late.end(), [](const Late& a, const Late& b) { return a.out < b.out; });
          for (size_t lo : {(size_t)0, late.size() * 95 / 100}) {
            auto med = [&](auto f) {
              std::vector<double> v;
              for (size_t i = lo; i < late.size(); i++) v.push_back(f(late[i]));
              std::sort(v.begin(), v.end());
              return v[v.size() / 2];
            };
            std::fprintf(stderr, "prt:   tail %s: entry +%.1f us after the queue emptied, %.1f us in the tail, %.0f "
                         "owners, %.0f tail iterations (medians over %zu waves)\n", lo ? "last 5%" : "all",
                         med([](const Late& l) { return l.entry; }), med([](const Late& l) { return l.tail; }),
                         med([](const Late& l) { return (double)l.owners; }),
                         med([](const Late& l) { return (double)l.iters; }), late.size() - lo);
          }
        }
      }
    }
    bool layout_ok = true, wait_ok = true;
    stats->stack_overflows = diag_overflows(c, &layout_ok, &wait_ok);
    if (!layout_ok) return fail(PRT_ERR_HIP, "k_shade2: kernel-argument layout check failed (Shade2Args)");
    if (!wait_ok) return fail(PRT_ERR_HIP, "the stream's wait for an instance-BVH build timed out");
    stats->segments += c->carry_segments;  // earlier passes of a call above 2^30 work items
    stats->shadow_rays += c->carry_shadow;
    stats->pipeline = c->last_defer ? 3 : 2;
    stats->iterations = (int32_t)(iters + 1);  // traversal launches
    stats->batches = 1;
    stats->ranks = 1;
    float ms = 0, ms_trace = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms_trace, c->ev[0], c->ev[1]));
    stats->paths = c->last_paths;
    stats->ms = ms;
    stats->ms_trace = ms_trace;
  }
  return PRT_OK;
}

// A rank whose part of a frame failed still posts its part of the frame's ncclGather (zeros), so its peers are
// never left blocked in the collective.  The send buffer is the tile buffer, or (if that could not be allocated)
// any context buffer large enough; root's receive buffer likewise.  With no such buffer the rank aborts its
// communicator: the peers' collective then fails through RCCL instead of completing.
void post_zero_gather(prt_ctx* c, size_t per) {
  const std::string why = last_error();  // the error being reported
  const Rccl* R = rccl(nullptr);
  if (!R || !c->comm) return;
  (void)hipSetDevice(c->device);
  (void)hipGetLastError();
  const bool root = c->sh_rank == 0;
  const size_t sb = per * sizeof(float4), rb = (size_t)c->sh_world * sb;
  auto pick = [&](DevBuf& pref, size_t bytes, DevBuf* avoid) -> void* {
    if (pref.bytes >= bytes || pref.ensure(bytes) == hipSuccess) return pref.p;
    for (DevBuf* b : {&c->ws.wave, &c->frames, &c->shtiles, &c->gathered, &c->avg})
      if (b != avoid && b->bytes >= bytes) return b->p;
    return nullptr;
  };
  void* send = pick(c->shtiles, sb, nullptr);
  void* recv = nullptr;
  if (root && send) {
    DevBuf* sendb = nullptr;
    for (DevBuf* b : {&c->shtiles, &c->ws.wave, &c->frames, &c->gathered, &c->avg})
      if (b->p == send) sendb = b;
    recv = pick(c->gathered, rb, sendb);
  }
  if (send && (!root || recv) && hipMemsetAsync(send, 0, sb, c->stream) == hipSuccess) {
    (void)rccl_settle(R, c->comm, R->Gather(send, recv, per * 4, ncclFloat32, 0, c->comm, c->stream));
  } else if (R->CommAbort) {
    (void)R->CommAbort(c->comm);
    c->comm = nullptr;  // unusable from here on: later sharded frames fail up front
  }
  last_error() = why;
}

// Sharded frame: every rank renders its tiles into shtiles, rank 0 gathers [world][per] and untiles.
// RCCL: one ncclGather per frame on this rank's stream.  Local group: each member renders on its own stream
// and copies its tile buffer into member 0's gathered buffer (peer copy over xGMI across devices); member 0
// waits for those copies, and the members' next copies wait for member 0's untile.
int render_sharded(prt_ctx* c, const prt_render_params* p, float4* avg_dev, uint32_t* rgb_dev, prt_stats* stats,
                   bool sync) {
  const int32_t W = p->width, H = p->height, ts = c->sh_tile, world = c->sh_world;
  if (c->pfx.enabled && c->pfx.aberration != 0)
    return fail(PRT_ERR_UNSUPPORTED, "chromatic aberration needs the accumulators of neighbouring tiles");
  const TileMap M0 = make_tilemap(W, H, ts, 0, world);
  const size_t per = M0.items;  // tile-buffer elements per rank (rank 0 owns the most)
  std::vector<prt_ctx*> all{c};
  all.insert(all.end(), c->members.begin(), c->members.end());
  const bool root = c->sh_rank == 0;
  const bool coll = c->sh_kind == 1;  // RCCL: the peers of this rank meet it in this frame's ncclGather
  if (coll && !c->comm) return fail(PRT_ERR_HIP, "the RCCL communicator was aborted by an earlier failed frame");
  const Rccl* R = coll ? rccl(nullptr) : nullptr;
  // frames in flight (RCCL shards): the frame's chain, gather and untile on the slot's stream; the accumulation
  // waits for the previous call's untile, so the gathers stay in call order on every rank
  Flight* f = coll ? flight_for(c, stats != nullptr || sync) : nullptr;
  if (!f) {
    const int jrc = join_flights(c);
    if (jrc) return jrc;
  }
  const hipStream_t st = f ? f->stream : c->stream;
  // 1. everything that can fail, on every member, before any render work is enqueued: a failure leaves every
  //    member's accumulation state as it was (the next frame is the one the failed call would have been)
  std::vector<RenderPlan> plans(all.size());
  auto prepare_all = [&]() -> int {
    for (size_t k = 0; k < all.size(); k++) {
      prt_ctx* m = all[k];
      const int32_t rank = c->sh_kind == 2 ? (int32_t)k : c->sh_rank;
      HIP_TRY(hipSetDevice(m->device));
      HIP_TRY(m->shtiles.ensure(per * sizeof(float4)));
      const int rc = prepare_render(m, p, make_tilemap(W, H, ts, rank, world), rank, plans[k], f);
      if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (root) HIP_TRY(c->gathered.ensure((size_t)world * per * sizeof(float4)));
    if (coll && !R) {
      const char* why = "RCCL not loaded";
      (void)rccl(&why);
      return fail(PRT_ERR_UNSUPPORTED, why);
    }
    return PRT_OK;
  };
  // 2. the renders
  auto enqueue_all = [&]() -> int {
    if (f) {
      const int frc = fork_flight(c, *f);
      if (frc) return frc;
    }
    for (size_t k = 0; k < all.size(); k++) {
      prt_ctx* m = all[k];
      const int32_t rank = c->sh_kind == 2 ? (int32_t)k : c->sh_rank;
      HIP_TRY(hipSetDevice(m->device));
      const TileMap M = make_tilemap(W, H, ts, rank, world);
      const hipStream_t ms = f ? st : m->stream;
      if (per > M.items)  // the tail of a shorter rank's buffer (zeros over zeros while a previous gather reads it)
        HIP_TRY(hipMemsetAsync(m->shtiles.as<float4>() + M.items, 0, sizeof(float4) * (per - M.items), ms));
      const int rc = enqueue_render(m, p, M, plans[k], nullptr, nullptr, m->shtiles.as<float4>(), stats != nullptr,
                                    f, f ? flight_after(c) : nullptr);
      if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    return PRT_OK;
  };
  int rc = prepare_all();
  bool forked = false;
  if (!rc) {
    rc = enqueue_all();
    forked = f != nullptr;
  }
  if (rc) {
    // RCCL: the other ranks are already (or soon) inside this frame's ncclGather; post this rank's part (zeros)
    // so they complete, then report the local error (frames in flight: after the earlier calls' gathers)
    const std::string why = last_error();
    if (forked) (void)land_flight(c, *f);
    (void)join_flights(c);
    last_error() = why;
    if (coll) post_zero_gather(c, per);
    return rc;
  }
  float4* g = root ? c->gathered.as<float4>() : nullptr;
  if (coll) {
    const ncclResult_t r = rccl_settle(R, c->comm, R->Gather(c->shtiles.p, g, per * 4, ncclFloat32, 0, c->comm, st));
    if (r != ncclSuccess) {
      if (f) (void)land_flight(c, *f);
      return fail(PRT_ERR_HIP, std::string("ncclGather: ") + R->GetErrorString(r));
    }
  } else {
    HIP_TRY(hipMemcpyAsync(g, c->shtiles.p, per * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    for (size_t k = 1; k < all.size(); k++) {
      prt_ctx* m = all[k];
      HIP_TRY(hipSetDevice(m->device));
      HIP_TRY(hipStreamWaitEvent(m->stream, c->sh_ev, 0));  // member 0's previous untile read g
      float4* dst = g + k * per;
      if (m->device == c->device)
        HIP_TRY(hipMemcpyAsync(dst, m->shtiles.p, per * sizeof(float4), hipMemcpyDeviceToDevice, m->stream));
      else
        HIP_TRY(hipMemcpyPeerAsync(dst, c->device, m->shtiles.p, m->device, per * sizeof(float4), m->stream));
      HIP_TRY(hipEventRecord(m->sh_ev, m->stream));
    }
    HIP_TRY(hipSetDevice(c->device));
    for (size_t k = 1; k < all.size(); k++) HIP_TRY(hipStreamWaitEvent(c->stream, all[k]->sh_ev, 0));
  }
  if (root && (avg_dev || rgb_dev)) {
    LaunchCfg L{st, occ_for(c)};
    const PostDev P = post_params(c, W, H);
    HIP_TRY(launch_untile(L, W, H, ts, world, (uint32_t)per, g, avg_dev, rgb_dev, c->pfx.enabled ? &P : nullptr));
  }
  if (f) return land_flight(c, *f);
  if (c->sh_ev) HIP_TRY(hipEventRecord(c->sh_ev, c->stream));
  if (stats) {
    prt_stats sum{};
    for (size_t k = 0; k < all.size(); k++) {
      prt_stats st{};
      HIP_TRY(hipSetDevice(all[k]->device));
      int rc = read_stats(all[k], &st);
      if (rc) return rc;
      if (k == 0) sum = st;
      else {
        sum.segments += st.segments;
        sum.shadow_rays += st.shadow_rays;
        sum.paths += st.paths;
        sum.ms = std::max(sum.ms, st.ms);
        sum.ms_trace = std::max(sum.ms_trace, st.ms_trace);
        sum.ms_closest += st.ms_closest;
        sum.stack_overflows = (sum.stack_overflows == ~0ull || st.stack_overflows == ~0ull)
                                  ? ~0ull : sum.stack_overflows + st.stack_overflows;  // ~0: unreadable
      }
    }
    sum.ranks = (int32_t)all.size();
    HIP_TRY(hipSetDevice(c->device));
    if (c->sh_kind == 1) {
      // the gather is part of the frame; a communicator that failed asynchronously (a peer's error, a lost link) or
      // a gather whose peers never arrive is reported within the time limit, not waited on
      const int wrc = rccl_wait(c, c->stream, "sharded frame");
      if (wrc) return wrc;
    }
    *stats = sum;
  }
  return PRT_OK;
}

}  // namespace

int prt::host::shard_setup(prt_ctx* c, int32_t tile) {
  if (tile <= 0 || (tile % 8) != 0) return fail(PRT_ERR_INVALID_ARGUMENT, "tile_size must be a positive multiple of 8");
  c->sh_tile = tile;
  if (!c->sh_ev) HIP_TRY(hipEventCreateWithFlags(&c->sh_ev, hipEventDisableTiming));
  return PRT_OK;
}

extern "C" {

// ---- checkpoint / resume of the accumulation state (include/prt.h): header + accumulator (float4) + samples
// (int32) + distances (float), n = accW * accH entries each
namespace {
struct AccHeader {
  char magic[8];
  uint32_t version, header_bytes;
  int32_t w, h, sh_rank, sh_world, sh_tile, sh_kind;
  uint64_t n;
};
constexpr char kAccMagic[8] = {'P', 'R', 'T', 'A', 'C', 'C', 'U', 'M'};
constexpr uint32_t kAccVersion = 1;
uint64_t acc_blob_bytes(uint64_t n) { return sizeof(AccHeader) + n * (16 + 4 + 4); }
}  // namespace

int prt_ray_totals(prt_ctx* c, uint64_t* segments, uint64_t* shadow_rays, int32_t reset) {
  if (!c || !segments || !shadow_rays) return fail(PRT_ERR_INVALID_ARGUMENT, "bad ray totals arguments");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  std::vector<prt_ctx*> all{c};
  all.insert(all.end(), c->members.begin(), c->members.end());
  uint64_t seg = 0, sh = 0;
  for (prt_ctx* m : all) {
    HIP_TRY(hipSetDevice(m->device));
    Counters h{};
    uint32_t dg[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&h, ray_totals_dev(m), sizeof(h), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(dg, m->diag.p, 12, hipMemcpyDeviceToHost, m->stream));
    if (reset) HIP_TRY(hipMemsetAsync(ray_totals_dev(m), 0, sizeof(Counters), m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (dg[1] != 0) return fail(PRT_ERR_HIP, "k_shade2: kernel-argument layout check failed (Shade2Args)");
    if (dg[2] != 0) return fail(PRT_ERR_HIP, "the stream's wait for an instance-BVH build timed out");
    seg += h.segments;
    sh += h.shadow;
  }
  HIP_TRY(hipSetDevice(c->device));
  *segments = seg;
  *shadow_rays = sh;
  return PRT_OK;
}

int prt_primary_rays(prt_ctx* c, uint64_t* traced, uint64_t* reused, int32_t reset) {
  if (!c || !traced || !reused) return fail(PRT_ERR_INVALID_ARGUMENT, "bad primary ray counter arguments");
  // host bookkeeping of the calls enqueued so far (enqueue_render_body): no device counter, no wait
  uint64_t t = c->prim_traced, r = c->prim_reused;
  if (reset) c->prim_traced = c->prim_reused = 0;
  for (prt_ctx* m : c->members) {
    t += m->prim_traced;
    r += m->prim_reused;
    if (reset) m->prim_traced = m->prim_reused = 0;
  }
  *traced = t;
  *reused = r;
  return PRT_OK;
}

int prt_shadow_reuse(prt_ctx* c, uint64_t* reused, int32_t reset) {
  if (!c || !reused) return fail(PRT_ERR_INVALID_ARGUMENT, "bad shadow reuse counter arguments");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  std::vector<prt_ctx*> all{c};
  all.insert(all.end(), c->members.begin(), c->members.end());
  uint64_t n = 0;
  for (prt_ctx* m : all) {  // the device's count (prt_shade2.h lvis_total), 8 bytes behind the ray totals
    HIP_TRY(hipSetDevice(m->device));
    unsigned long long h = 0;
    void* dev = ray_totals_dev(m) + 1;
    HIP_TRY(hipMemcpyAsync(&h, dev, sizeof(h), hipMemcpyDeviceToHost, m->stream));
    if (reset) HIP_TRY(hipMemsetAsync(dev, 0, sizeof(h), m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    n += h;
  }
  HIP_TRY(hipSetDevice(c->device));
  *reused = n;
  return PRT_OK;
}

int prt_surface_reuse(prt_ctx* c, uint64_t* reused, int32_t reset) {
  if (!c || !reused) return fail(PRT_ERR_INVALID_ARGUMENT, "bad surface reuse counter arguments");
  // host bookkeeping of the calls enqueued so far, as prt_primary_rays: no device counter, no wait
  uint64_t r = c->surf_reused;
  if (reset) c->surf_reused = 0;
  for (prt_ctx* m : c->members) {
    r += m->surf_reused;
    if (reset) m->surf_reused = 0;
  }
  *reused = r;
  return PRT_OK;
}

int prt_shadow_dead(prt_ctx* c, uint64_t* dead, int32_t reset) {
  if (!c || !dead) return fail(PRT_ERR_INVALID_ARGUMENT, "bad dead shadow ray counter arguments");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  std::vector<prt_ctx*> all{c};
  all.insert(all.end(), c->members.begin(), c->members.end());
  uint64_t n = 0;
  for (prt_ctx* m : all) {  // the device's count (prt_wave2.hip dead_total), 16 bytes behind the ray totals
    HIP_TRY(hipSetDevice(m->device));
    unsigned long long h = 0;
    void* dev = reinterpret_cast<unsigned long long*>(ray_totals_dev(m) + 1) + 1;
    HIP_TRY(hipMemcpyAsync(&h, dev, sizeof(h), hipMemcpyDeviceToHost, m->stream));
    if (reset) HIP_TRY(hipMemsetAsync(dev, 0, sizeof(h), m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    n += h;
  }
  HIP_TRY(hipSetDevice(c->device));
  *dead = n;
  return PRT_OK;
}

int prt_accumulation_bytes(prt_ctx* c, uint64_t* bytes) {
  if (!c || !bytes) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx/bytes is NULL");
  if (!c->members.empty()) return fail(PRT_ERR_UNSUPPORTED, "accumulation checkpoints of a local group");
  *bytes = c->acc.p ? acc_blob_bytes((uint64_t)c->accW * c->accH) : 0;
  return PRT_OK;
}

int prt_save_accumulation(prt_ctx* c, void* blob, uint64_t bytes) {
  if (!c || !blob) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx/blob is NULL");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  if (!c->members.empty()) return fail(PRT_ERR_UNSUPPORTED, "accumulation checkpoints of a local group");
  if (!c->acc.p) return fail(PRT_ERR_NOT_READY, "nothing accumulated yet");
  const uint64_t n = (uint64_t)c->accW * c->accH;
  if (bytes < acc_blob_bytes(n)) return fail(PRT_ERR_INVALID_ARGUMENT, "blob smaller than prt_accumulation_bytes");
  AccHeader hd{};
  std::memcpy(hd.magic, kAccMagic, 8);
  hd.version = kAccVersion;
  hd.header_bytes = sizeof(AccHeader);
  hd.w = c->accW;
  hd.h = c->accH;
  hd.sh_rank = c->sh_rank;
  hd.sh_world = c->sh_world;
  hd.sh_tile = c->sh_tile;
  hd.sh_kind = c->sh_kind;
  hd.n = n;
  char* b = static_cast<char*>(blob);
  std::memcpy(b, &hd, sizeof(hd));
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(b + sizeof(hd), c->acc.p, 16 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(b + sizeof(hd) + 16 * n, c->nsamp.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(b + sizeof(hd) + 20 * n, c->dist.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PRT_OK;
}

int prt_load_accumulation(prt_ctx* c, const void* blob, uint64_t bytes) {
  if (!c || !blob) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx/blob is NULL");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  if (!c->members.empty()) return fail(PRT_ERR_UNSUPPORTED, "accumulation checkpoints of a local group");
  AccHeader hd{};
  if (bytes < sizeof(hd)) return fail(PRT_ERR_INVALID_ARGUMENT, "truncated accumulation blob");
  std::memcpy(&hd, blob, sizeof(hd));
  if (std::memcmp(hd.magic, kAccMagic, 8) != 0 || hd.version != kAccVersion || hd.header_bytes != sizeof(hd))
    return fail(PRT_ERR_INVALID_ARGUMENT, "not an accumulation blob of this ABI");
  if (hd.w <= 0 || hd.h <= 0 || hd.n != (uint64_t)hd.w * (uint64_t)hd.h || bytes != acc_blob_bytes(hd.n))
    return fail(PRT_ERR_INVALID_ARGUMENT, "accumulation blob size does not match its header");
  if (hd.sh_rank != c->sh_rank || hd.sh_world != c->sh_world || hd.sh_tile != c->sh_tile || hd.sh_kind != c->sh_kind)
    return fail(PRT_ERR_INVALID_ARGUMENT, "accumulation blob of another shard geometry");
  HIP_TRY(hipSetDevice(c->device));
  const int rc = ensure_state(c, hd.w, hd.h);
  if (rc) return rc;
  const char* b = static_cast<const char*>(blob);
  const uint64_t n = hd.n;
  HIP_TRY(hipMemcpyAsync(c->acc.p, b + sizeof(hd), 16 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->nsamp.p, b + sizeof(hd) + 16 * n, 4 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->dist.p, b + sizeof(hd) + 20 * n, 4 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PRT_OK;
}

int prt_render(prt_ctx* c, const prt_render_params* p, float* avg_rgba, uint32_t* rgb8, uint32_t out_flags,
               prt_stats* stats) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  int rc = check_params(p);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t np = (size_t)p->width * p->height;
  float4* avg_dev = nullptr;
  uint32_t* rgb_dev = nullptr;
  const bool dev_out = (out_flags & PRT_OUT_DEVICE) != 0;
  const bool root = c->sh_kind == 0 || c->sh_rank == 0;  // the rank whose outputs receive the frame
  if (avg_rgba && root) {
    if (dev_out) avg_dev = reinterpret_cast<float4*>(avg_rgba);
    else { HIP_TRY(c->avg.ensure(np * 16)); avg_dev = c->avg.as<float4>(); }
  }
  if (rgb8 && root) {
    if (dev_out) rgb_dev = rgb8;
    else { HIP_TRY(c->rgb8.ensure(np * 4)); rgb_dev = c->rgb8.as<uint32_t>(); }
  }
  // frames in flight only for device outputs without stats (prt_set_frames_in_flight)
  const bool sync = !dev_out || stats;
  if (c->sh_kind != 0) {
    rc = render_sharded(c, p, avg_dev, rgb_dev, stats, sync);
  } else {
    const TileMap M = make_tilemap(p->width, p->height, 8, 0, 1);
    rc = run_render(c, p, M, avg_dev, rgb_dev, nullptr, stats != nullptr, 0, sync);
    if (!rc && stats) rc = read_stats(c, stats);
  }
  if (rc) return rc;
  if (!dev_out && root) {
    if (avg_rgba) HIP_TRY(hipMemcpyAsync(avg_rgba, avg_dev, np * 16, hipMemcpyDeviceToHost, c->stream));
    if (rgb8) HIP_TRY(hipMemcpyAsync(rgb8, rgb_dev, np * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return PRT_OK;
}

int prt_tile_buffer_pixels(int32_t W, int32_t H, int32_t ts, int32_t world, int64_t* px) {
  if (!px || W <= 0 || H <= 0 || ts <= 0 || (ts % 8) != 0 || world <= 0)
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad tile geometry (tile_size must be a positive multiple of 8)");
  const TileMap M0 = make_tilemap(W, H, ts, 0, world);  // rank 0 owns the most tiles
  *px = (int64_t)M0.items;
  return PRT_OK;
}

int prt_tile_pixel_map(int32_t W, int32_t H, int32_t ts, int32_t rank, int32_t world, int32_t* out) {
  int64_t per = 0;
  int rc = prt_tile_buffer_pixels(W, H, ts, world, &per);
  if (rc) return rc;
  if (!out || rank < 0 || rank >= world) return fail(PRT_ERR_INVALID_ARGUMENT, "bad rank / output");
  const TileMap M = make_tilemap(W, H, ts, rank, world);
  for (int64_t r = 0; r < per; r++) {
    int32_t x = 0, y = 0;
    out[r] = ((uint64_t)r < M.items && item_pixel(M, (uint32_t)r, x, y)) ? y * W + x : -1;
  }
  return PRT_OK;
}

int prt_render_tiles(prt_ctx* c, const prt_render_params* p, int32_t ts, int32_t rank, int32_t world,
                     float* tiles_dev, prt_stats* stats) {
  if (!c || !tiles_dev) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx/tiles is NULL");
    int rc = check_params(p);
  if (rc) return rc;
  if (ts <= 0 || (ts % 8) != 0 || world <= 0 || rank < 0 || rank >= world)
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad tile geometry");
  HIP_TRY(hipSetDevice(c->device));
  const TileMap M = make_tilemap(p->width, p->height, ts, rank, world);
  const TileMap M0 = make_tilemap(p->width, p->height, ts, 0, world);
  if (M0.items > M.items)  // pad the tail of the (equal-size) per-rank buffer
    HIP_TRY(hipMemsetAsync(reinterpret_cast<float4*>(tiles_dev) + M.items, 0, sizeof(float4) * (M0.items - M.items),
                           c->stream));
  // (device tile buffer: a frame in flight unless stats are asked for)
  rc = run_render(c, p, M, nullptr, nullptr, reinterpret_cast<float4*>(tiles_dev), stats != nullptr, rank,
                  stats != nullptr);
  if (!rc && stats) rc = read_stats(c, stats);
  return rc;
}

int prt_untile(prt_ctx* c, const float* gathered, int32_t W, int32_t H, int32_t ts, int32_t world, float* avg_dev,
               uint32_t* rgb8_dev) {
  if (!c || !gathered) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx/gathered is NULL");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  int64_t per = 0;
  int rc = prt_tile_buffer_pixels(W, H, ts, world, &per);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (c->pfx.enabled && c->pfx.aberration != 0 && rgb8_dev)
    return fail(PRT_ERR_UNSUPPORTED, "chromatic aberration needs the accumulators of neighbouring tiles");
  LaunchCfg L{c->stream, occ_for(c)};
  const PostDev P = post_params(c, W, H);
  HIP_TRY(launch_untile(L, W, H, ts, world, (uint32_t)per, reinterpret_cast<const float4*>(gathered),
                        reinterpret_cast<float4*>(avg_dev), rgb8_dev, c->pfx.enabled ? &P : nullptr));
  return PRT_OK;
}

}  // extern "C"
