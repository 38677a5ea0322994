// prt_api.cpp -- C-ABI implementation (include/prt.h): the context, device residency of the scene (textures, lights,
// camera, sky), the pinned staging pool, the queries, the AOVs, the shards.  One host thread per context; all device
// work on one HIP stream.  The context itself is prt_ctx.h; the mesh entry points (BLAS build, in-place update,
// skinning, snapshots, read-back) are prt_api_mesh.cpp, the instance entry points and the instance state (records,
// instance BVH, its updates and rebuilds) are prt_api_instance.cpp, the render path (prt_render and what it calls) is
// prt_api_render.cpp, the image-space passes (denoisers, reprojections) are prt_api_image.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "prt_ctx.h"
#include "prt_deform.h"
#include "prt_denoise.h"
#include "prt_instance_host.h"
#include "prt_motion.h"

using namespace prt;
using namespace prt::host;

static thread_local std::string g_err;  // prt_last_error's text: the one copy, behind fail for the other files

int prt::host::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
std::string& prt::host::last_error() { return g_err; }

namespace {

// tree levels one lane's stack must cover: the deepest BLAS, plus the instance BVH's levels when it is walked
// (its groups sit below the BLAS's: at most one per TLAS level, the last one the remaining instances of a leaf)
int stack_depth(const prt_ctx* c) { return c->max_depth + (c->use_tlas ? c->tlas_depth : 0); }

}  // namespace

bool prt::host::depth_ok(const prt_ctx* c) { return stack_depth(c) <= kMaxBvhDepth; }

// frames in flight: the context stream waits for every call still in flight.  Every entry point but an in-flight
// prt_render starts with it, so its work (and the host waits of drain()) comes after those frames
int prt::host::join_flights(prt_ctx* c) {
  if (c->last_fl < 0) return PRT_OK;
  HIP_TRY(hipSetDevice(c->device));
  for (Flight& f : c->fl)
    if (f.pending) {
      HIP_TRY(hipStreamWaitEvent(c->stream, f.done, 0));
      f.pending = false;
    }
  c->last_fl = -1;  // the next call's accumulation is ordered through the context stream again
  return PRT_OK;
}

namespace {

// RCCL calls and waits that involve the peers are bounded (failure detection): a rank whose peers never
// arrive -- at communicator set-up or in a frame's ncclGather -- fails after PRT_RCCL_TIMEOUT_S seconds (default
// 120) with the communicator aborted, instead of hanging in the call or in a later stream wait
double rccl_timeout_s() {
  const char* e = std::getenv("PRT_RCCL_TIMEOUT_S");
  const double v = e ? std::atof(e) : 120.0;
  return v > 0.0 ? v : 120.0;
}

}  // namespace

// a non-blocking communicator's call returned ncclInProgress: poll its async state until it settles (bounded)
ncclResult_t prt::host::rccl_settle(const Rccl* R, ncclComm_t comm, ncclResult_t r) {
  const auto t0 = std::chrono::steady_clock::now();
  const double lim = rccl_timeout_s();
  while (r == ncclInProgress) {
    ncclResult_t st = ncclSuccess;
    if (R->CommGetAsyncError(comm, &st) != ncclSuccess) return ncclSystemError;
    r = st;
    if (r != ncclInProgress) break;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > lim) return ncclInProgress;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
  return r;
}
// wait for `s` on an RCCL-sharded context: stream completion, the communicator's async error, or the time limit
// (then the communicator is aborted, which also ends its kernels, and the context cannot shard any more)
int prt::host::rccl_wait(prt_ctx* c, hipStream_t s, const char* what) {
  const Rccl* R = rccl(nullptr);
  const auto t0 = std::chrono::steady_clock::now();
  const double lim = rccl_timeout_s();
  while (true) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) return fail(PRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    ncclResult_t ae = ncclSuccess;
    const bool bad = R && c->comm && R->CommGetAsyncError(c->comm, &ae) == ncclSuccess && ae != ncclSuccess &&
                     ae != ncclInProgress;
    const bool late = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > lim;
    if (bad || late) {
      if (R && c->comm && R->CommAbort) (void)R->CommAbort(c->comm);
      c->comm = nullptr;  // unusable from here on: later sharded frames fail up front
      (void)hipStreamSynchronize(s);  // the aborted collective's kernels end
      return fail(PRT_ERR_HIP, std::string(what) + (bad ? std::string(": RCCL communicator error: ") + R->GetErrorString(ae)
                                                         : ": the RCCL collective did not complete within the time limit "
                                                           "(PRT_RCCL_TIMEOUT_S); communicator aborted"));
    }
    std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
  (void)hipGetLastError();  // hipStreamQuery's hipErrorNotReady
  return PRT_OK;
}

// wait for the context stream (bounded on an RCCL-sharded context)
int prt::host::wait_stream(prt_ctx* c, const char* what) {
  if (c->sh_kind == 1 && c->comm) return rccl_wait(c, c->stream, what);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PRT_OK;
}

// finish the frames queued on the context stream (and the frames in flight) before a setter overwrites (or frees)
// resident buffers
int prt::host::drain(prt_ctx* c) {
  PRT_JOIN(c);
  HIP_TRY(hipSetDevice(c->device));
  return wait_stream(c, "waiting for the context's frames");
}

// waves/SIMD of the persistent traversal kernels for the context's stack depth (prt_instance_host.h occ_at)
int prt::host::occ_for(const prt_ctx* c) { return occ_at(stack_depth(c)); }

namespace {
// a slot's pinned buffer replaced by one of `bytes` (its copies have run: the slot is free)
int stage_grow(StageSlot& st, size_t bytes) {
  if (st.p) HIP_TRY(hipHostFree(st.p));
  st.p = nullptr;
  st.bytes = 0;
  HIP_TRY(hipHostMalloc(&st.p, bytes, hipHostMallocDefault));
  st.bytes = bytes;
  return PRT_OK;
}
}  // namespace

// The staging buffers of an instance set's updates, each of which takes at most `bytes`: the pool filled to
// kStageSlots slots, the slots' flag words, and every idle slot below `bytes` grown to it -- when the set is first
// built, so that no later update allocates pinned memory (StageSlot says what that costs).  Nothing to do while the
// pool is full and was last sized for as much.
int prt::host::stage_reserve(prt_ctx* c, size_t bytes) {
  if (c->stage.size() >= kStageSlots && c->stage_bytes >= bytes) return PRT_OK;
  c->stage_bytes = bytes;
  for (size_t k = c->stage.size(); k < kStageSlots; k++) c->stage.emplace_back();
  if (!c->stage_flag) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->stage_flag), kStageSlots * 64, hipHostMallocCoherent));
    std::memset(c->stage_flag, 0, kStageSlots * 64);
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->stage_flag_dev), c->stage_flag, 0));
  }
  for (StageSlot& t : c->stage) {
    if (t.used && hipEventQuery(t.ev) == hipSuccess) t.used = false;
    (void)hipGetLastError();  // (hipErrorNotReady of a buffer still in use)
    if (!t.used && !t.lost && t.bytes < bytes) PRT_TRY(stage_grow(t, bytes));
  }
  return PRT_OK;
}

// a pinned staging buffer of at least `bytes` (prt_ctx::stage): a free one (its copies have run), a new one while
// the pool holds fewer than kStageSlots, else the oldest once its copies have run (the only host wait)
int prt::host::stage_acquire(prt_ctx* c, size_t bytes, StageSlot*& out) {
  StageSlot* pick = nullptr;
  for (StageSlot& t : c->stage) {
    if (t.lost) continue;
    if (t.used) {
      const hipError_t q = hipEventQuery(t.ev);
      if (q == hipErrorNotReady) {
        (void)hipGetLastError();
        continue;
      }
      HIP_TRY(q);
      t.used = false;
    }
    if (!pick || (pick->bytes < bytes && t.bytes >= bytes)) pick = &t;
  }
  if (!pick && c->stage.size() < kStageSlots) {
    c->stage.emplace_back();
    pick = &c->stage.back();
  }
  if (!pick) {  // every buffer in use: wait for the one acquired first
    for (StageSlot& t : c->stage)
      if (!t.lost && (!pick || t.seq < pick->seq)) pick = &t;
    if (!pick) return fail(PRT_ERR_HIP, "no usable staging buffer (earlier updates failed)");
    HIP_TRY(hipEventSynchronize(pick->ev));
    pick->used = false;
  }
  pick->seq = ++c->stage_seq;
  StageSlot& st = *pick;
  if (st.bytes < bytes) PRT_TRY(stage_grow(st, bytes));
  if (!st.ev) HIP_TRY(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
  out = &st;
  return PRT_OK;
}
// the copies out of the buffer are enqueued: it is free again once the stream has run them
int prt::host::stage_release(prt_ctx*, StageSlot& st, hipStream_t s) {
  HIP_TRY(hipEventRecord(st.ev, s));
  st.used = true;
  return PRT_OK;
}

// `bytes` of host memory into device memory at dst in the context stream's order: copied into a pinned staging
// buffer now (the caller's memory is free on return), uploaded from there
int prt::host::stage_upload(prt_ctx* c, void* dst, const void* src, size_t bytes) {
  StageSlot* st = nullptr;
  PRT_TRY(stage_acquire(c, bytes, st));
  st->lost = true;  // until the copy out of it is enqueued (a failure below leaves it out of the pool)
  std::memcpy(st->p, src, bytes);
  HIP_TRY(hipMemcpyAsync(dst, st->p, bytes, hipMemcpyHostToDevice, c->stream));
  PRT_TRY(stage_release(c, *st, c->stream));
  st->lost = false;
  return PRT_OK;
}

// HBM spill columns for BVHs deeper than the LDS stacks hold (prt_traverse8.h LaneStack): levels beyond the
// query kernels' 16 (the persistent spill form holds 18 in LDS, so this covers it too), one uint2 per level for
// every thread of the launch: `threads` for a query, the persistent spill grid for renders
int prt::host::ensure_spill(prt_ctx* c, SceneDev& S, size_t threads) {
  const int levels = stack_depth(c) - 1 - kQueryStack;
  S.spill = nullptr;
  S.spill_levels = 0;
  if (levels <= 0) return PRT_OK;
  const size_t need = sizeof(uint2) * (size_t)levels * std::max<size_t>(threads, (size_t)kSpillTraceBlocks * 64u);
  if (c->spill.bytes < need) {
    PRT_TRY(drain(c));
    HIP_TRY(c->spill.ensure(need));
  }
  S.spill = c->spill.as<uint2>();
  S.spill_levels = levels;
  return PRT_OK;
}

int prt::host::scene_ready(prt_ctx* c, SceneDev& S) {
  if (c->mesh_host.empty()) return fail(PRT_ERR_NOT_READY, "no meshes: call prt_set_meshes");
  if (c->inst_mesh.empty()) return fail(PRT_ERR_NOT_READY, "no instances: call prt_set_instances");
  PRT_TRY(ensure_instances(c));
  std::memset(&S, 0, sizeof(S));
  S.diag = c->diag.as<uint32_t>();
  S.nodes8 = c->nodes8.as<Node8>();
  S.tris = c->tris.as<TriMT>();
  S.stri = c->stri.as<ShadeTri>();
  S.srgb = c->srgb.as<float>();
  S.texels = c->texels.as<uint32_t>();
  S.tex = c->tex.as<TexDev>();
  S.inst = c->isets[c->icur].inst.as<InstDev>();
  S.mesh = c->mesh.as<MeshDev>();
  S.sky = (c->skyw > 0) ? c->sky.as<float>() : nullptr;
  S.ninst = (int32_t)c->inst_mesh.size();
  S.tlas = c->use_tlas ? 1 : 0;
  S.tlas8 = c->use_tlas ? c->isets[c->icur].tlas8.as<Node8>() : nullptr;
  S.tlas_slot = c->use_tlas ? c->isets[c->icur].tlas_slot.as<uint32_t>() : nullptr;
  {  // packed hit word: prim bits for the largest mesh, instance bits above
    uint32_t maxt = 1;
    for (const MeshDev& m : c->mesh_host) maxt = std::max(maxt, m.tri_count);
    uint32_t pb = 1, ib = 0;
    while (pb < 32 && (1ull << pb) < maxt) pb++;
    while ((1ull << ib) < (uint64_t)S.ninst) ib++;
    if (pb + ib > 32) return fail(PRT_ERR_UNSUPPORTED, "mesh size x instance count exceed the 32-bit hit word");
    S.pbits = pb;
  }
  S.skyw = c->skyw;
  S.skyh = c->skyh;
  const prt_lights& L = c->lights;
  std::memcpy(S.ppos, L.point_pos, sizeof(S.ppos));
  std::memcpy(S.pcol, L.point_color, sizeof(S.pcol));
  std::memcpy(S.dpos, L.dir_pos, 12);
  std::memcpy(S.dcol, L.dir_color, 12);
  std::memcpy(S.spos, L.spot_pos, 12);
  std::memcpy(S.scol, L.spot_color, 12);
  std::memcpy(S.srot, L.spot_rot, 12);
  std::memcpy(S.cam, c->cam.pos, 12);
  std::memcpy(S.cam + 3, c->cam.top_left, 12);
  std::memcpy(S.cam + 6, c->cam.top_right, 12);
  std::memcpy(S.cam + 9, c->cam.bottom_left, 12);
  std::memcpy(S.basis, c->cam.right, 12);
  std::memcpy(S.basis + 3, c->cam.up, 12);
  std::memcpy(S.basis + 6, c->cam.ahead, 12);
  S.panini = c->pfx.enabled ? 1 : 0;
  S.pan_d = c->pfx.distortion;
  S.pan_b = panini_scale(c->pfx.fov, c->pfx.distortion);
  std::memcpy(S.al, c->al, sizeof(S.al));
  S.area = c->area;
  S.area_two_sided = c->area_two_sided;
  S.has_diel = 0;
  for (size_t i = 0; i < c->inst_mesh.size() && i < c->inst_kind.size(); i++)
    if (c->inst_kind[i] == kMatDielectric) S.has_diel = 1;
  return PRT_OK;
}

PostDev prt::host::post_params(const prt_ctx* c, int32_t W, int32_t H) {
  PostDev P{};
  for (int k = 0; k < 4; k++) P.grade[k] = c->pfx.color_grading[k];
  P.vig_int = c->pfx.vignette_intensity;
  P.vig_rad = c->pfx.vignette_radius;
  P.aberration = c->pfx.aberration;
  P.W = W;
  P.H = H;
  return P;
}

extern "C" {

int prt_abi_version(void) { return PRT_ABI_VERSION; }
const char* prt_last_error(void) { return g_err.c_str(); }

int prt_device_count(int32_t* count) {
  if (!count) return fail(PRT_ERR_INVALID_ARGUMENT, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  *count = (e == hipSuccess) ? n : 0;
  return PRT_OK;
}

int prt_create(const prt_device_desc* desc, prt_ctx** out) {
  if (!out) return fail(PRT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(PRT_ERR_NO_DEVICE, "no HIP device visible");
  const int dev = desc ? desc->device : 0;
  if (dev < 0 || dev >= n) return fail(PRT_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  HIP_TRY(hipSetDevice(dev));
  prt_ctx* c = new prt_ctx();
  c->device = dev;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(PRT_ERR_HIP, "hipStreamCreate failed");
  }
  c->stream = c->own_stream;
  {
    // srgbToLinear of every albedo byte (Scene.cpp:171 on texel/255, BRDF.cpp srgbToLinear); the same
    // float ops and double-precision pow rounded once as the oracle, evaluated on the host
    float lut[256];
    for (int b = 0; b < 256; b++) {
      const float x = (float)b * (1.0f / 255.0f);
      lut[b] = (x <= 0.04045f) ? (x / 12.92f) : (float)std::pow((double)((x + 0.055f) / 1.055f), (double)2.4f);
    }
    if (upload(c->srgb, lut, sizeof(lut)) != hipSuccess) {
      delete c;
      return fail(PRT_ERR_HIP, "srgb table upload failed");
    }
    if (c->diag.ensure(64) != hipSuccess || hipMemset(c->diag.p, 0, 64) != hipSuccess) {
      delete c;
      return fail(PRT_ERR_HIP, "diagnostics buffer allocation failed");
    }
  }
  for (auto& e : c->ev) {
    if (hipEventCreate(&e) != hipSuccess) {
      delete c;
      return fail(PRT_ERR_HIP, "hipEventCreate failed");
    }
  }
  for (auto& e : c->wt.ev) {  // per-launch timers only: no system-scope fence / cache writeback per record
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess && hipEventCreate(&e) != hipSuccess) {
      delete c;
      return fail(PRT_ERR_HIP, "hipEventCreate failed");
    }
  }
  *out = c;
  return PRT_OK;
}

int prt_destroy(prt_ctx* c) {
  if (!c) return PRT_OK;
  for (prt_ctx* m : c->members) (void)prt_destroy(m);
  c->members.clear();
  (void)hipSetDevice(c->device);
  (void)join_flights(c);
  if (c->sh_kind == 1 && c->comm) (void)rccl_wait(c, c->stream, "prt_destroy");  // (a stuck gather: aborted)
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (Flight& f : c->fl) {
    if (f.stream) (void)hipStreamSynchronize(f.stream);
    if (f.done) (void)hipEventDestroy(f.done);
    if (f.stream) (void)hipStreamDestroy(f.stream);
  }
  if (c->fl_fork) (void)hipEventDestroy(c->fl_fork);
  if (c->comm && c->own_comm) {
    const Rccl* R = rccl(nullptr);
    if (R) (void)R->CommDestroy(c->comm);
  }
  c->comm = nullptr;
  if (c->sh_ev) (void)hipEventDestroy(c->sh_ev);
  c->tlas_worker.reset();  // every job is done: each one's stream wait ran before the synchronisations above
  for (InstSet& I : c->isets)
    for (auto& u : I.uses) (void)hipEventDestroy(u.second);
  if (c->rf.ev) (void)hipEventDestroy(c->rf.ev);
  if (c->rf.pin) (void)hipHostFree(c->rf.pin);
  if (c->rf.res_host) (void)hipHostFree(c->rf.res_host);
  if (c->stage_flag) (void)hipHostFree(c->stage_flag);
  for (StageSlot& st : c->stage) {  // the pinned upload ring (its copies ran: the streams are synchronised)
    if (st.ev) (void)hipEventDestroy(st.ev);
    if (st.p) (void)hipHostFree(st.p);
  }
  for (auto e : c->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto e : c->wt.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto e : c->dn_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // DevBuf members free their device memory
  return PRT_OK;
}

int prt_set_stream(prt_ctx* c, void* s) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_TRY(join_flights(c));  // the frames in flight complete in the old stream's order
  c->stream = s ? reinterpret_cast<hipStream_t>(s) : c->own_stream;
  c->ws.pvalid = false;  // the kept primary hits were written in the old stream's order: trace them again in the new
  return PRT_OK;
}

int prt_set_frames_in_flight(prt_ctx* c, int32_t n) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (n < 1 || n > kMaxFlights) return fail(PRT_ERR_INVALID_ARGUMENT, "frames in flight must be 1 to 8");
  if (n > 1 && c->sh_kind == 2) return fail(PRT_ERR_UNSUPPORTED, "frames in flight on a local shard group");
  PRT_JOIN(c);
  HIP_TRY(hipSetDevice(c->device));
  if (n > 1) {
    // only the slots used get a stream: HIP deals a process's streams over its hardware queues (GPU_MAX_HW_QUEUES,
    // 4 by default) as they are created, so streams created and never used would still share queues with the
    // chains that are
    for (int32_t k = 0; k < n; k++) {
      Flight& f = c->fl[k];
      if (!f.stream) HIP_TRY(hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
      if (!f.done) HIP_TRY(hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
    }
    if (!c->fl_fork) HIP_TRY(hipEventCreateWithFlags(&c->fl_fork, hipEventDisableTiming));
  }
  c->inflight = n;
  c->next_fl = 0;
  return PRT_OK;
}

int prt_finish(prt_ctx* c) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_JOIN(c);
  return PRT_OK;
}

int prt_set_textures(prt_ctx* c, const prt_texture* t, int32_t n) {
  if (!c || (n > 0 && !t) || n < 0) return fail(PRT_ERR_INVALID_ARGUMENT, "bad textures");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  c->shade_epoch++;  // what a kept primary surface was shaded from changes (prt_ctx::shade_epoch)
  std::vector<uint32_t> all;
  std::vector<TexDev> host(n);
  for (int32_t i = 0; i < n; i++) {
    if (t[i].width <= 0 || t[i].height <= 0 || !t[i].pixels) return fail(PRT_ERR_INVALID_ARGUMENT, "bad texture");
    host[i].offset = (uint32_t)all.size();
    host[i].w = t[i].width;
    host[i].h = t[i].height;
    host[i].pad = 0;
    all.insert(all.end(), t[i].pixels, t[i].pixels + (size_t)t[i].width * t[i].height);
  }
  PRT_TRY(drain(c));
  HIP_TRY(upload(c->texels, all.data(), all.size() * 4));
  HIP_TRY(upload(c->tex, host.data(), host.size() * sizeof(TexDev)));
  c->tex_host = host;
  PRT_FOR_MEMBERS(prt_set_textures(m, t, n));
  return PRT_OK;
}

int prt_set_area_lights(prt_ctx* c, const prt_area_light* a, int32_t n) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  if (n < 0 || n > 1 || (n == 1 && !a)) return fail(PRT_ERR_UNSUPPORTED, "at most one area light");
  if (n == 0) {
    c->area = 0;
    PRT_FOR_MEMBERS(prt_set_area_lights(m, a, n));
    return PRT_OK;
  }
  const float* u = a->edge_u;
  const float* v = a->edge_v;
  const float cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
  const float area = sqrtf(cx * cx + cy * cy + cz * cz);
  if (!(area > 0.0f)) return fail(PRT_ERR_INVALID_ARGUMENT, "degenerate area light");
  const float inv = 1.0f / sqrtf(cx * cx + cy * cy + cz * cz);  // normalize(): v * (1 / sqrtf(dot(v, v)))
  const float al[16] = {a->corner[0], a->corner[1], a->corner[2], u[0], u[1], u[2], v[0], v[1], v[2],
                        cx * inv, cy * inv, cz * inv, a->radiance[0], a->radiance[1], a->radiance[2], area};
  std::memcpy(c->al, al, sizeof(al));
  c->area = 1;
  c->area_two_sided = a->two_sided ? 1 : 0;
  PRT_FOR_MEMBERS(prt_set_area_lights(m, a, n));
  return PRT_OK;
}

int prt_set_lights(prt_ctx* c, const prt_lights* l) {
  if (!c || !l) return fail(PRT_ERR_INVALID_ARGUMENT, "bad lights");
  c->lights = *l;
  c->have_lights = true;
  PRT_FOR_MEMBERS(prt_set_lights(m, l));
  return PRT_OK;
}

int prt_set_sky(prt_ctx* c, const float* rgb, int32_t w, int32_t h) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  c->shade_epoch++;  // what a kept primary surface was shaded from changes (prt_ctx::shade_epoch)
  PRT_TRY(drain(c));
  if (!rgb || w <= 0 || h <= 0) {
    c->skyw = c->skyh = 0;
    PRT_FOR_MEMBERS(prt_set_sky(m, rgb, w, h));
    return PRT_OK;
  }
  HIP_TRY(upload(c->sky, rgb, (size_t)w * h * 3 * 4));
  c->skyw = w;
  c->skyh = h;
  PRT_FOR_MEMBERS(prt_set_sky(m, rgb, w, h));
  return PRT_OK;
}

int prt_set_camera(prt_ctx* c, const prt_camera* cam) {
  if (!c || !cam) return fail(PRT_ERR_INVALID_ARGUMENT, "bad camera");
  c->cam = *cam;
  c->have_camera = true;
  PRT_FOR_MEMBERS(prt_set_camera(m, cam));
  return PRT_OK;
}

// Camera::Camera (Core/Camera.cpp:29-36): tmpl8 normalize = v * (1/sqrtf(dot))
int prt_camera_look_at(const float pos[3], const float target[3], float aspect, prt_camera* o) {
  if (!pos || !target || !o) return fail(PRT_ERR_INVALID_ARGUMENT, "bad look_at arguments");
  auto nrm = [](V3 v) { return prt::normalize(v); };
  const V3 P = v3(pos[0], pos[1], pos[2]), Tg = v3(target[0], target[1], target[2]);
  const V3 ahead = nrm(Tg - P);
  const V3 right = nrm(cross(ahead, v3(0, 1, 0)));
  const V3 up = nrm(cross(right, ahead));
  const V3 a2 = ahead * 2.0f, ar = aspect * right;
  const V3 TL = P + a2 - ar + up, TR = P + a2 + ar + up, BL = P + a2 - ar - up;
  for (int k = 0; k < 3; k++) o->pos[k] = pos[k];
  o->top_left[0] = TL.x; o->top_left[1] = TL.y; o->top_left[2] = TL.z;
  o->top_right[0] = TR.x; o->top_right[1] = TR.y; o->top_right[2] = TR.z;
  o->bottom_left[0] = BL.x; o->bottom_left[1] = BL.y; o->bottom_left[2] = BL.z;
  o->right[0] = right.x; o->right[1] = right.y; o->right[2] = right.z;
  o->up[0] = up.x; o->up[1] = up.y; o->up[2] = up.z;
  o->ahead[0] = ahead.x; o->ahead[1] = ahead.y; o->ahead[2] = ahead.z;
  return PRT_OK;
}

int prt_postfx_preset(int32_t preset, prt_postfx* o) {
  if (!o || preset < 0 || preset > 1) return fail(PRT_ERR_INVALID_ARGUMENT, "bad post-process preset");
  std::memset(o, 0, sizeof(*o));
  o->enabled = 1;
  if (preset == 0) {  // Camera member defaults (Core/Camera.h:12,23,27): float4{1.f} is all ones
    o->fov = 40.f; o->distortion = 40.f; o->vignette_intensity = 20.f; o->vignette_radius = 0.3f; o->aberration = 0;
    for (int k = 0; k < 4; k++) o->color_grading[k] = 1.f;
  } else {            // P1 (Core/Camera.cpp:18-23, Camera.h:11,20,28); vignetteRadius = vignetteRadius keeps 0.3
    o->fov = 90.f; o->distortion = 2.f; o->vignette_intensity = 5.5f; o->vignette_radius = 0.3f; o->aberration = -1;
    o->color_grading[0] = 1.f; o->color_grading[1] = 1.f; o->color_grading[2] = 1.2f; o->color_grading[3] = 0.f;
  }
  return PRT_OK;
}

int prt_set_postfx(prt_ctx* c, const prt_postfx* pfx) {
  if (!c || !pfx) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx/postfx is NULL");
  c->pfx = *pfx;
  PRT_FOR_MEMBERS(prt_set_postfx(m, pfx));
  return PRT_OK;
}

int prt_reset_accumulation(prt_ctx* c, int32_t full) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  PRT_FOR_MEMBERS(prt_reset_accumulation(m, full));
  if (!c->acc.p) return PRT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->accW * c->accH;
  HIP_TRY(hipMemsetAsync(c->acc.p, 0, n * 16, c->stream));
  if (full) {
    HIP_TRY(hipMemsetAsync(c->nsamp.p, 0, n * 4, c->stream));
    std::vector<float> d(n, -1.0f);
    HIP_TRY(hipMemcpyAsync(c->dist.p, d.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PRT_OK;
}

int prt_trace_primary(prt_ctx* c, int32_t W, int32_t H, prt_hit* hits, uint32_t out_flags, prt_stats* stats) {
  if (!c || !hits || W <= 0 || H <= 0) return fail(PRT_ERR_INVALID_ARGUMENT, "bad arguments");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  SceneDev S;
  PRT_TRY(scene_ready(c, S));
  if (!c->have_camera) return fail(PRT_ERR_NOT_READY, "no camera");
  if (!depth_ok(c)) return fail(PRT_ERR_UNSUPPORTED, "BVH deeper than 64 levels");
  const TileMap M = make_tilemap(W, H, 8, 0, 1);
  const size_t n = (size_t)W * H;
  PRT_TRY(ensure_spill(c, S, (size_t)M.items + 256));
  HitOut* out = reinterpret_cast<HitOut*>(hits);
  Staging io(c, out_flags);
  PRT_TRY(io.out(c->hits, out, n * sizeof(HitOut)));
  HIP_TRY(c->counters.ensure(sizeof(Counters)));
  HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(Counters), c->stream));
  LaunchCfg L{c->stream, occ_for(c)};
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  HIP_TRY(launch_primary_hits(L, S, M, out, c->counters.as<Counters>()));
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  PRT_TRY(io.finish());
  if (stats) {
    if (io.dev) HIP_TRY(hipStreamSynchronize(c->stream));
    Counters h{};
    HIP_TRY(hipMemcpy(&h, c->counters.p, sizeof(h), hipMemcpyDeviceToHost));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[2]));
    std::memset(stats, 0, sizeof(*stats));
    stats->ms_closest = ms;
    stats->segments = h.segments;
    stats->shadow_rays = 0;
    stats->paths = n;
    stats->ms = ms;
    stats->ms_trace = ms;
    stats->stack_overflows = diag_overflows(c);
  }
  return PRT_OK;
}

static int ray_query(prt_ctx* c, int32_t n, const float* O, const float* D, const float* tmax, void* out, bool any) {
  if (!c || n < 0 || (n > 0 && (!O || !D || !out)) || (any && n > 0 && !tmax))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad ray query arguments");
  PRT_JOIN(c);
  if (n == 0) return PRT_OK;
  HIP_TRY(hipSetDevice(c->device));
  SceneDev S;
  PRT_TRY(scene_ready(c, S));
  if (!depth_ok(c)) return fail(PRT_ERR_UNSUPPORTED, "BVH deeper than 64 levels");
  PRT_TRY(ensure_spill(c, S, (size_t)n + 256));
  DevBuf dO, dD, dT, dOut;
  auto cleanup = [&]() { dO.release(); dD.release(); dT.release(); dOut.release(); };
  const size_t outb = (size_t)n * (any ? 4 : sizeof(HitOut));
  if (upload(dO, O, (size_t)n * 12) != hipSuccess || upload(dD, D, (size_t)n * 12) != hipSuccess ||
      (tmax && upload(dT, tmax, (size_t)n * 4) != hipSuccess) || dOut.ensure(outb) != hipSuccess) {
    cleanup();
    return fail(PRT_ERR_OUT_OF_MEMORY, "ray buffers");
  }
  LaunchCfg L{c->stream, occ_for(c)};
  hipError_t e = any ? launch_occluded(L, S, n, dO.as<float>(), dD.as<float>(), dT.as<float>(), dOut.as<int32_t>())
                     : launch_intersect(L, S, n, dO.as<float>(), dD.as<float>(), tmax ? dT.as<float>() : nullptr,
                                        dOut.as<HitOut>());
  if (e == hipSuccess) e = hipMemcpyAsync(out, dOut.p, outb, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  cleanup();
  if (e != hipSuccess) return fail(PRT_ERR_HIP, std::string("ray query: ") + hipGetErrorString(e));
  return PRT_OK;
}

int prt_intersect(prt_ctx* c, int32_t n, const float* O, const float* D, const float* tmax, prt_hit* hits) {
  return ray_query(c, n, O, D, tmax, hits, false);
}
int prt_occluded(prt_ctx* c, int32_t n, const float* O, const float* D, const float* tmax, int32_t* occ) {
  return ray_query(c, n, O, D, tmax, occ, true);
}

// ---- first-hit AOVs and the a-trous denoiser (prt_denoise.hip)
namespace {
// prt_render_aov / prt_render_aov_ids / prt_render_aov_deform: one primary-hit pass, then k_aov, k_aov_ids and / or
// k_aov_deform over its hits
int render_aov(prt_ctx* c, int32_t W, int32_t H, uint32_t flags, float* albedo, float* normal_depth,
               uint32_t* instance, float* offset, uint32_t out_flags) {
  if (!c || W <= 0 || H <= 0 || W > 16384 || H > 16384) return fail(PRT_ERR_INVALID_ARGUMENT, "bad AOV arguments");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  SceneDev S;
  PRT_TRY(scene_ready(c, S));
  if (!c->have_camera) return fail(PRT_ERR_NOT_READY, "no camera");
  if (!depth_ok(c)) return fail(PRT_ERR_UNSUPPORTED, "BVH deeper than 64 levels");
  if (!albedo && !normal_depth && !instance && !offset) return PRT_OK;
  const TileMap M = make_tilemap(W, H, 8, 0, 1);
  const size_t n = (size_t)W * H;
  PRT_TRY(ensure_spill(c, S, (size_t)M.items + 256));
  const bool timed = (out_flags & PRT_OUT_TIMED) != 0;
  HIP_TRY(c->aov_hits.ensure(n * sizeof(HitOut)));
  HIP_TRY(c->counters.ensure(sizeof(Counters)));  // the launch's own ray count: not the running totals
  float4* a = reinterpret_cast<float4*>(albedo);
  float4* g = reinterpret_cast<float4*>(normal_depth);
  uint32_t* ids = instance;
  float4* off = reinterpret_cast<float4*>(offset);
  Staging io(c, out_flags);
  PRT_TRY(io.out(c->aov_alb, a, n * sizeof(float4)));
  PRT_TRY(io.out(c->aov_nd, g, n * sizeof(float4)));
  PRT_TRY(io.out(c->aov_ids, ids, n * 4));
  PRT_TRY(io.out(c->aov_off, off, n * sizeof(float4)));
  LaunchCfg L{c->stream, occ_for(c)};
  if (timed) PRT_TRY(dn_event(c, 0));
  HIP_TRY(launch_primary_hits(L, S, M, c->aov_hits.as<HitOut>(), c->counters.as<Counters>()));
  if (a || g)
    HIP_TRY(launch_aov(c->stream, S, W, H, (flags & PRT_FLAG_NORMALMAP) != 0, c->aov_hits.as<HitOut>(), a, g));
  if (ids) HIP_TRY(launch_aov_ids(c->stream, W, H, c->aov_hits.as<HitOut>(), ids));
  if (off)  // (no snapshot since the last prt_set_meshes: no table, every pixel gets zeros)
    HIP_TRY(launch_aov_deform(c->stream, S, W, H, c->aov_hits.as<HitOut>(),
                              c->snap.empty() ? nullptr : c->snap_tab.as<const float*>(), off));
  if (timed) {
    PRT_TRY(dn_event(c, 1));
    c->dn_timed_aov = 1;
  }
  return io.finish();
}
}  // namespace

int prt_render_aov(prt_ctx* c, int32_t W, int32_t H, uint32_t flags, float* albedo, float* normal_depth,
                   uint32_t out_flags) {
  return render_aov(c, W, H, flags, albedo, normal_depth, nullptr, nullptr, out_flags);
}
int prt_render_aov_ids(prt_ctx* c, int32_t W, int32_t H, uint32_t flags, float* albedo, float* normal_depth,
                       uint32_t* instance, uint32_t out_flags) {
  return render_aov(c, W, H, flags, albedo, normal_depth, instance, nullptr, out_flags);
}
int prt_render_aov_deform(prt_ctx* c, int32_t W, int32_t H, uint32_t flags, float* albedo, float* normal_depth,
                          uint32_t* instance, float* offset, uint32_t out_flags) {
  return render_aov(c, W, H, flags, albedo, normal_depth, instance, offset, out_flags);
}

int prt_brdf_probe(prt_ctx* c, int32_t op, int32_t n, const float* in, float* out) {
  if (!c || n < 0 || (n > 0 && (!in || !out)) || op < PRT_PROBE_EVAL || op > PRT_PROBE_TEXEL)
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad BRDF probe arguments");
  if (n == 0) return PRT_OK;
  if (op == PRT_PROBE_TEXEL)
    for (int32_t i = 0; i < n; i++)
      for (int k = 2; k < 4; k++) {
        const float d = in[24 * (size_t)i + k];  // the kernel divides by it
        if (!(d >= 1.0f && d <= 16384.0f) || d != (float)(int32_t)d)
          return fail(PRT_ERR_INVALID_ARGUMENT, "texel probe: w and h must be integers in 1..16384");
      }
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  DevBuf din, dout;
  HIP_TRY(upload(din, in, 24ull * 4 * (size_t)n));
  HIP_TRY(dout.ensure(8ull * 4 * (size_t)n));
  hipError_t e = launch_brdf_probe(c->stream, op, n, din.as<float>(), dout.as<float>());
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, 8ull * 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(PRT_ERR_HIP, std::string("BRDF probe: ") + hipGetErrorString(e));
  return PRT_OK;
}

int prt_shard_unique_id(uint8_t id[PRT_SHARD_ID_BYTES]) {
  if (!id) return fail(PRT_ERR_INVALID_ARGUMENT, "id is NULL");
  static_assert(sizeof(ncclUniqueId) == PRT_SHARD_ID_BYTES, "ncclUniqueId size");
  const char* why = nullptr;
  const Rccl* R = rccl(&why);
  if (!R) return fail(PRT_ERR_UNSUPPORTED, why);
  ncclUniqueId u;
  const ncclResult_t r = R->GetUniqueId(&u);
  if (r != ncclSuccess) return fail(PRT_ERR_HIP, std::string("ncclGetUniqueId: ") + R->GetErrorString(r));
  std::memcpy(id, &u, sizeof(u));
  return PRT_OK;
}

int prt_shard_init_rccl(prt_ctx* c, const uint8_t id[PRT_SHARD_ID_BYTES], int32_t rank, int32_t world, int32_t tile) {
  if (!c || !id || world <= 0 || rank < 0 || rank >= world) return fail(PRT_ERR_INVALID_ARGUMENT, "bad shard rank / world");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  if (c->sh_kind != 0) return fail(PRT_ERR_INVALID_ARGUMENT, "context is already sharded");
  PRT_TRY(shard_setup(c, tile));
  const char* why = nullptr;
  const Rccl* R = rccl(&why);
  if (!R) return fail(PRT_ERR_UNSUPPORTED, why);
  HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  ncclComm_t comm = nullptr;
  ncclResult_t r;
  if (R->CommInitRankConfig) {  // non-blocking set-up, polled: ranks that never join make it fail, not hang
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    r = R->CommInitRankConfig(&comm, world, u, rank, &cfg);
    if (comm && (r == ncclSuccess || r == ncclInProgress)) r = rccl_settle(R, comm, r);
    if (r == ncclInProgress) {
      if (R->CommAbort) (void)R->CommAbort(comm);
      return fail(PRT_ERR_HIP, "ncclCommInitRank: the other ranks did not join within the time limit (PRT_RCCL_TIMEOUT_S)");
    }
    if (r != ncclSuccess && comm && R->CommAbort) (void)R->CommAbort(comm);
  } else {
    r = R->CommInitRank(&comm, world, u, rank);
  }
  if (r != ncclSuccess) return fail(PRT_ERR_HIP, std::string("ncclCommInitRank: ") + R->GetErrorString(r));
  c->comm = comm;
  c->own_comm = true;
  c->sh_kind = 1;
  c->sh_rank = rank;
  c->sh_world = world;
  return PRT_OK;
}

int prt_shard_attach_rccl(prt_ctx* c, void* comm, int32_t tile) {
  if (!c || !comm) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx / comm is NULL");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  if (c->sh_kind != 0) return fail(PRT_ERR_INVALID_ARGUMENT, "context is already sharded");
  PRT_TRY(shard_setup(c, tile));
  const char* why = nullptr;
  const Rccl* R = rccl(&why);
  if (!R) return fail(PRT_ERR_UNSUPPORTED, why);
  ncclComm_t cm = reinterpret_cast<ncclComm_t>(comm);
  int n = 0, r = 0;
  if (R->CommCount(cm, &n) != ncclSuccess || R->CommUserRank(cm, &r) != ncclSuccess)
    return fail(PRT_ERR_INVALID_ARGUMENT, "not a usable ncclComm_t");
  c->comm = cm;
  c->own_comm = false;
  c->sh_kind = 1;
  c->sh_rank = r;
  c->sh_world = n;
  return PRT_OK;
}

int prt_create_group(const prt_device_desc* devs, int32_t n, int32_t tile, prt_ctx** out) {
  if (!out) return fail(PRT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (!devs || n <= 0 || n > 64) return fail(PRT_ERR_INVALID_ARGUMENT, "1..64 devices");
  prt_ctx* g = nullptr;
  PRT_TRY(prt_create(&devs[0], &g));
  int rc = shard_setup(g, tile);
  for (int32_t k = 1; k < n && !rc; k++) {
    prt_ctx* m = nullptr;
    rc = prt_create(&devs[k], &m);
    if (!rc) {
      g->members.push_back(m);
      rc = shard_setup(m, tile);
    }
  }
  if (!rc) {  // peer access between distinct devices (the tile copies go device to device)
    for (prt_ctx* m : g->members) {
      if (m->device == g->device) continue;
      (void)hipSetDevice(m->device);
      const hipError_t e = hipDeviceEnablePeerAccess(g->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
    }
    (void)hipSetDevice(g->device);
  }
  if (rc) {
    const std::string msg = g_err;
    (void)prt_destroy(g);
    return fail(rc, msg);
  }
  g->sh_kind = 2;
  g->sh_rank = 0;
  g->sh_world = n;
  *out = g;
  return PRT_OK;
}

int prt_get_shard_info(prt_ctx* c, prt_shard_info* info) {
  if (!c || !info) return fail(PRT_ERR_INVALID_ARGUMENT, "bad arguments");
  info->rank = c->sh_rank;
  info->world = c->sh_world;
  info->tile_size = c->sh_tile;
  info->transport = c->sh_kind;
  return PRT_OK;
}

int prt_get_scene_info(prt_ctx* c, prt_scene_info* info) {
  if (!c || !info) return fail(PRT_ERR_INVALID_ARGUMENT, "bad arguments");
  std::memset(info, 0, sizeof(*info));
  for (const MeshHost& m : c->mesh_info) {
    info->blas_nodes += m.nodes;
    info->blas_leaves += m.leaves;
    info->triangles += m.tris;
  }
  info->max_depth = c->max_depth;
  info->tlas_depth = c->use_tlas ? c->tlas_depth : 0;
  info->tlas_rebuilds = c->tlas_rebuilds;
  info->tlas_async = c->tlas_async;
  info->tlas_median = 0;
  info->tlas_build_ms = info->tlas_build_cpu_ms = 0.0f;
  if (c->tlas_worker) {
    const TlasWorker::Stats ws = c->tlas_worker->stats();
    info->tlas_median = ws.median;
    info->tlas_build_ms = (float)ws.ms;
    info->tlas_build_cpu_ms = (float)ws.cpu_ms;
  }
  info->build_ms = c->build_ms;
  info->builder = c->built_with;
  size_t ib = 0;
  for (const InstSet& I : c->isets) ib += I.inst.bytes + I.inst_src.bytes + I.tlas8.bytes + I.tlas_slot.bytes;
  info->device_bytes = (int64_t)(c->nodes8.bytes + c->tris.bytes + c->stri.bytes + c->texels.bytes + c->sky.bytes + ib);
  return PRT_OK;
}

}  // extern "C"
