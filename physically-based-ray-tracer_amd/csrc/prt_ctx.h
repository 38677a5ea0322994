// prt_ctx.h -- the context (struct prt_ctx) and what the host translation units of the C ABI (prt_api.cpp,
// prt_api_mesh.cpp, prt_api_instance.cpp, prt_api_render.cpp, prt_api_image.cpp, prt_api_query.cpp) share: error
// reporting, device buffers, the context's parts, and the helpers they call across files.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/prt.h"
#include "prt_blas_refit_gpu.h"
#include "prt_launch.h"
#include "prt_rccl.h"
#include "prt_refit.h"
#include "prt_skin_gpu.h"
#include "prt_tlas_worker.h"

namespace prt::host {

// sets the calling thread's prt_last_error text (prt_api.cpp) and returns code; the text as it stands
int fail(int code, const std::string& msg);
std::string& last_error();

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return ::prt::host::fail(PRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
// return a failed call's code (prt_last_error is already set)
#define PRT_TRY(call)          \
  do {                         \
    const int rct_ = (call);   \
    if (rct_) return rct_;     \
  } while (0)

// device allocation owned by its holder (move-only; freed on destruction)
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // (re)allocate to at least n bytes; contents are not preserved
  hipError_t ensure(size_t n) {
    if (n <= bytes && p) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, n ? n : 16);
    if (e == hipSuccess) bytes = n ? n : 16;
    return e;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// blocking host -> device copy into a resident buffer.  Callers that may overwrite (or reallocate) a buffer
// that queued frames still read first drain the context stream (drain()).
inline hipError_t upload(DevBuf& b, const void* src, size_t n) {
  hipError_t e = b.ensure(n);
  if (e != hipSuccess) return e;
  if (n) return hipMemcpy(b.p, src, n, hipMemcpyHostToDevice);
  return hipSuccess;
}

// wavefront state of one item group: the context's own (prt_ctx::ws), or of a concurrent group (prt_ctx::grp)
// What the hit of a tile-map entry's path-1 primary ray (WaveBufs::phit) is a function of: the camera as the
// kernels get it (SceneDev cam .. panini: the Panini post-process bends the primary rays), the resolution, the tile
// map, and the epochs of the geometry and of the instance state (prt_ctx::scene_epoch / inst_epoch).  Zeroed before
// it is filled (no padding), compared by its bytes.
struct PrimKey {
  float cam[12], basis[9], pan_b, pan_d;
  int32_t panini, W, H, ts, rank, world;
  uint64_t scene_epoch, inst_epoch;
};
struct WaveState {
  DevBuf wave;
  WaveBufs wb = {};
  uint32_t n = 0, levels = 0;
  bool ext = false, merge = false;
  bool hasR = false;  // the (result) stack R is allocated: every pass but one with a deferred resolve needs it
  // deferred resolve (prt_wave2.hip k_resolve_pass): the record planes, one per wavefront iteration (point_planes);
  // allocated by the first call that defers on this state
  DevBuf planes;
  // primary-hit reuse: this state's own copy of the records and the key they were traced under (its stamp)
  DevBuf phit;
  PrimKey pkey = {};
  bool pvalid = false;
  // light-visibility record (WaveBufs::lvis): valid for the phit it was learned on (pgen counts this state's
  // dense passes, lgen is the count the record belongs to) and for the lights' positions (lpos: point,
  // directional, spot; colours, the spot's direction and the flags shape no shadow ray)
  DevBuf lvis;
  uint64_t pgen = 0, lgen = 0;
  float lpos[18] = {};
  bool lvalid = false;
  // primary-surface record (SurfBufs: three 16-byte planes in surf, the emission plane in surf_e when some mesh has
  // an emission texture): valid for the phit it was filled on (sgen, as lgen), for the context's shading epoch
  // (sepoch) and for the call's normal-map and skybox flags (sflags); semis: it was filled with an emission plane
  DevBuf surf, surf_e;
  uint64_t sgen = 0, sepoch = 0;
  uint32_t sflags = 0;
  bool semis = false, svalid = false;
};
// a frame in flight (prt_set_frames_in_flight): the wavefront chain of one call on its own stream.  Slot 0 uses the
// context's own wavefront state and frame buffer, the others their own; done = the call's last work (the
// accumulation, and for a sharded frame its gather and untile), which the next call's accumulation waits for
constexpr int kMaxFlights = 8;
struct Flight {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  WaveState ws;
  DevBuf frames;
  bool pending = false;  // done is not yet in the context stream's order
};

// one pinned staging buffer of ensure_instances' uploads (prt_ctx::stage): reused once its copies have run.  The
// kStageSlots buffers are allocated when an instance set is first built (stage_reserve: pinned allocation in the update path cost
// 20-190 ms per buffer on the GPU box, profiles/r06_tlas_drift.txt); an update that finds all of them in use waits
// for the oldest one's copies (the host at most kStageSlots updates ahead of the GPU)
constexpr size_t kStageSlots = 8;
// the stream's wait for a worker build: a build takes ~6 ms at 10,000 instances and the jobs of up to kStageSlots
// queued updates run one after another, so the limit only catches a producer that never comes
constexpr double kHostWaitLimitS = 120.0;
struct StageSlot {
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
  bool lost = false;  // an update failed while enqueuing from it: never handed out again (its copies may be pending)
  uint64_t seq = 0;   // when it was last acquired
};
// One copy of the instance state the frames read (prt_ctx::isets): instance records, their refit input, the instance
// BVH.  An update writes the next copy in the ring while the frames in flight still read theirs; a copy is
// rewritten only after the context stream has waited for the frames that read it (one event per stream they ran on)
struct InstSet {
  DevBuf inst, inst_src, tlas8, tlas_slot;
  std::vector<std::pair<hipStream_t, hipEvent_t>> uses;  // the last frame that read this copy, per stream
  size_t nuse = 0;
};

// One mesh's skin binding (prt_set_mesh_skin): the bind pose as uploaded (`in`: positions, normals, joints, weights,
// indices back to back, each part 256-byte aligned), the matrices of a call with host matrices (`mats`, 48 bytes per
// joint) and the scratch of prt_skin_mesh (`work`: the skinned positions and normals, 16 bytes per vertex each, then
// the fat triangles, 48 bytes per triangle).  dev: what the kernels get (matrices set per call).  Unbound: joints = 0.
struct SkinBinding {
  DevBuf in, mats, work;
  SkinDev dev = {};
  int32_t joints = 0;
  bool skinned = false;  // a prt_skin_mesh has run on this binding: `work` holds its fat triangles (prt_rebuild_mesh)
};

struct MeshHost {
  float bmin[3], bmax[3];
  int depth;
  int64_t nodes, leaves;
  int32_t tris;
  // prt_update_mesh: the mesh's TriMT records [rec_base, rec_base + recs) (more than tris after spatial splits; its
  // nodes are [MeshDev::root, + nodes)), its vertex count, and the tree levels of the node pass (empty until the
  // mesh's first update): level d's nodes are order[level_ends[d - 1] .. level_ends[d]) of the mesh's part of
  // prt_ctx::rf.order
  uint32_t rec_base = 0, recs = 0;
  int32_t verts = 0;
  std::vector<uint32_t> level_ends;
  // prt_rebuild_mesh: the sizes of the mesh's regions in the concatenated arrays, which a rebuilt tree must fit --
  // node_cap nodes from MeshDev::root (what prt_set_meshes gave it, or the region a larger tree was moved to) and
  // rec_cap records from rec_base (>= tris: the surplus of a spatial-split build goes unused after a rebuild)
  int64_t node_cap = 0;
  uint32_t rec_cap = 0;
};

// The scratch of the refit (prt_update_mesh / prt_skin_mesh, prt_blas_refit.h; prt_ctx::rf), allocated at a context's
// first update for the scene as it stands and kept: six floats per node (the uninflated boxes), the nodes of every
// refitted mesh ordered by tree level, the 28-byte result (root box, bad-index flag) and its pinned host copy; for
// host arrays, the six arrays back to back in one pinned buffer (written again once ev says the previous update's
// copy has run) and their device copy
struct RefitScratch {
  DevBuf box, order, res, in;
  RefitResult* res_host = nullptr;
  // One dedicated buffer, not a slot of the prt_ctx::stage ring: at C4 it is 143 MiB, and stage_acquire hands out the
  // first free slot and grows it on demand, which would pin up to kStageSlots such buffers and put hipHostMalloc
  // (20-190 ms, profiles/r06_tlas_drift.txt) back into the update path
  void* pin = nullptr;
  size_t pin_bytes = 0;
  hipEvent_t ev = nullptr;
  bool pin_used = false;
};

}  // namespace prt::host

struct prt_ctx {
  using DevBuf = prt::host::DevBuf;
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // textures
  std::vector<prt::TexDev> tex_host;
  DevBuf texels, tex;
  // meshes
  std::vector<prt::MeshDev> mesh_host;
  std::vector<prt::host::MeshHost> mesh_info;
  DevBuf nodes8, tris, stri, mesh;
  // Node8 entries of nodes8 in use: the meshes' regions back to back (prt_rebuild_mesh appends a region for a tree
  // that outgrew its mesh's; the region it leaves stays, unused).  The refit scratch is indexed by node position
  uint64_t nodes_len = 0;
  int max_depth = 0;
  int builder = -1;  // BLAS builder (prt_set_bvh_builder): PRT_BUILDER_* (-1: PRT_BUILDER_HOST_SAH)
  double build_ms = 0;  // wall time of the last prt_set_meshes BLAS builds
  int built_with = PRT_BUILDER_HOST_SAH;
  // instances
  std::vector<float> inst_xf;
  std::vector<uint32_t> inst_mesh;
  std::vector<uint32_t> inst_kind;  // prt_set_instance_materials (PRT_MAT_*), textured by default
  std::vector<prt::InstSrc> inst_stage;  // host side of the refit input (prt_refit.h)
  // the device instance state, one copy per frame in flight + 1 (InstSet); isets[icur] is what the next frame reads
  std::vector<prt::host::InstSet> isets = std::vector<prt::host::InstSet>(1);
  size_t icur = 0;
  // instance BVH (more than kLinearInstances instances, or PRT_TLAS=1), rebuilt for every prt_set_instances as the
  // reference rebuilds its TLAS every frame (Core/Renderer.cpp:33-41, Core/tiny_bvh.h:1732-1770): the host SAH
  // build + SAH-optimal collapse (bvh_build.h build_tlas8), on the calling thread when the instance set changes,
  // on the worker thread (tlas_worker) for every later update, the stream waiting for that build in a one-lane
  // kernel before the tree's upload (prt_api_instance.cpp ensure_instances; TlasWorker says why no host function)
  bool use_tlas = false;
  int tlas_depth = 0;    // levels the traversal stacks are sized for (>= the current tree's depth)
  int32_t tlas_n = -1;   // instance count of the current tree (-1: none)
  std::unique_ptr<prt::host::TlasWorker> tlas_worker;
  int32_t tlas_rebuilds = 0, tlas_async = 0;  // since the instance count last changed (diagnostics)
  // pinned staging buffers of ensure_instances' uploads (instance sources, a new tree's nodes / slots / refit order;
  // hipMemcpyAsync from pageable memory may block the host): a buffer is written again only after its copies have
  // run, so the host never waits on queued frames unless it is kStageSlots updates ahead of the GPU
  std::vector<prt::host::StageSlot> stage;
  uint64_t stage_seq = 0;  // acquisitions so far (StageSlot::seq: the oldest buffer is waited for when all are in use)
  size_t stage_bytes = 0;  // the size the pool was last allocated for
  uint32_t* stage_flag = nullptr;      // one coherent pinned word per staging buffer (64-B stride): TlasJob::flag
  uint32_t* stage_flag_dev = nullptr;  // its device address
  prt::host::RefitScratch rf;  // prt_update_mesh / prt_skin_mesh
  // prt_rebuild_mesh: where the device builder leaves a mesh's new tree before it is committed (room for T Node8 and
  // T TriMT, T the largest mesh's triangle count; sized by the first rebuild after a prt_set_meshes and kept)
  DevBuf rb_nodes, rb_tris;
  // prt_blas_cost: the node pass's per-block sums and the root area, then the result (allocated at first use, kept)
  DevBuf cost_part;
  DevBuf spill;  // traversal stack levels beyond the LDS ones (BVHs deeper than 17 levels)
  DevBuf diag;   // SceneDev::diag device counters ([0] traversal stack overflows, cumulative per context)
  // area light (prt_set_area_lights): p0, eu, ev, n, Le, area
  float al[16] = {};
  int32_t area = 0, area_two_sided = 0;
  bool inst_dirty = true;  // the device instance records (k_refit) are out of date
  bool tlas_dirty = true;  // transforms or meshes changed since the instance BVH was last built / refitted
  // prt_update_instances (prt_tlas_refit.h): new transforms for the instance set, the instance BVH refitted on the
  // device.  iset_n: the instance count isets[icur] was last written for (-1: never).  xf_device: the transforms
  // came from device memory and live in isets[icur].inst_src alone -- inst_xf is stale and nothing reads it; every
  // refresh of the records (ensure_instances) goes through the device path until the next prt_set_instances or
  // host-memory update.  The live tree's topology, taken from the worker's last tree at the first update after a
  // build and kept until the next build: tlas_nodes nodes, ordered by level in tlas_order (level d's nodes are
  // tlas_order[tlas_level_ends[d - 1] .. tlas_level_ends[d])); tlas_box: six floats per node of scratch.  inst_tab:
  // what a device-side refill needs besides the transforms -- mesh ids, kinds, then the per-mesh boxes -- uploaded
  // when it is not what the host holds (inst_tab_ok; the records were dirty, or a host-side refill came between).
  // All sized with the instance sets (ensure_instances)
  int32_t iset_n = -1;
  bool xf_device = false;
  bool tlas_topo = false;
  uint32_t tlas_nodes = 0;
  std::vector<uint32_t> tlas_level_ends;
  DevBuf tlas_order, tlas_box, inst_tab;
  bool inst_tab_ok = false;
  // prt_rebuild_instances (prt_tlas_build.h): where the device builder reads the instances' fat triangles (48 bytes
  // per instance) and leaves the new tree (80 bytes of nodes, 48 of records per instance) before it is committed to the
  // next copy of the ring; sized by the first rebuild of an instance count and kept.  Once the builder is through
  // with its input, tb_fat holds the canonical level order of the commit (12 bytes per node)
  DevBuf tb_fat, tb_nodes, tb_tris;
  // sky, lights, camera
  DevBuf sky;
  int32_t skyw = 0, skyh = 0;
  DevBuf srgb;  // 256-entry sRGB -> linear table of the albedo decode
  prt_lights lights{};
  bool have_lights = false;
  prt_camera cam{};
  bool have_camera = false;
  prt_postfx pfx{};  // post-processing off until prt_set_postfx
  DevBuf accprev;    // accumulator before the last frame of a call (screen-pass aberration)
  // accumulation state (Core/Renderer.h:61-63) and scratch
  DevBuf acc, nsamp, dist;
  int32_t accW = 0, accH = 0;
  DevBuf frames, avg, rgb8, counters, hits, tl;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  // wavefront state of the merged pipeline (frame-in-flight slot 0 and calls in the context stream's order)
  prt::host::WaveState ws;
  prt::WaveTimers wt = {};
  // the last enqueued render, for its stats (read_stats)
  uint32_t last_iters = 0;
  bool last_defer = false;  // the last call's passes ran the deferred resolve (prt_stats::pipeline)
  bool last_timers = false;
  uint64_t last_paths = 0;
  uint64_t carry_segments = 0, carry_shadow = 0;  // ray counts of a call's earlier frame passes
  // primary-hit reuse (PrimKey): scene_epoch counts the calls that change geometry or BLASes (prt_set_meshes,
  // prt_set_bvh_builder), inst_epoch those that change the instance records, the instance BVH or the hit word's
  // encoding (prt_set_instances); prim_traced / prim_reused: path-1 primary rays handed to a dense pass / taken
  // from phit by the calls so far (host bookkeeping, prt_primary_rays)
  uint64_t scene_epoch = 0, inst_epoch = 0;
  uint64_t prim_traced = 0, prim_reused = 0;
  // primary-surface record (WaveState::surf): shade_epoch counts the calls that change what iteration 0 shades a
  // fixed primary hit from -- every call that bumps one of the two epochs above, and prt_set_textures, prt_set_sky
  // and prt_set_instance_materials, which leave the hits alone; surf_reused: items shaded from the record by the calls
  // so far (host bookkeeping, prt_surface_reuse)
  uint64_t shade_epoch = 0;
  uint64_t surf_reused = 0;
  // sharding (prt_shard_init_rccl / prt_shard_attach_rccl / prt_create_group)
  int32_t sh_kind = 0;  // 0 none, 1 RCCL, 2 local group (this context is member 0)
  int32_t sh_rank = 0, sh_world = 1, sh_tile = 32;
  ncclComm_t comm = nullptr;
  bool own_comm = false;
  std::vector<prt_ctx*> members;  // local group: members 1..world-1, owned by member 0
  DevBuf shtiles, gathered;       // this rank's tile buffer; rank 0: [world][tile buffer] gathered
  hipEvent_t sh_ev = nullptr;     // member: tiles handed to member 0; member 0: untile done
  bool layout_checked = false;    // check_layout_once done
  // frames in flight (prt_set_frames_in_flight): 1 = every call complete in the context stream's order
  int32_t inflight = 1;
  prt::host::Flight fl[prt::host::kMaxFlights];
  int32_t next_fl = 0, last_fl = -1;  // the slot of the next call / of the last call still ordering accumulation
  hipEvent_t fl_fork = nullptr;
  // first-hit AOVs and the denoiser (prt_render_aov / prt_denoise): primary hits, staging of host inputs / outputs,
  // the packed unit normal + depth, and the two buffers the filter iterations alternate between
  DevBuf aov_hits, aov_alb, aov_nd;
  DevBuf dn_in[3], dn_geo, dn_pp[2], dn_out, dn_rgb8;
  hipEvent_t dn_ev[2 + PRT_DENOISE_TIMINGS] = {};  // PRT_OUT_TIMED: [0..1] the AOV pass, [2..] prep + iterations
  int32_t dn_timed_aov = 0, dn_timed_passes = 0;   // what the last timed calls recorded
  // temporal reprojection (prt_reproject): staging of host images (colour, normal_depth, history, its normal_depth)
  DevBuf rp_in[4], rp_out, rp_rgb8;
  // instance ids and motion (prt_render_aov_ids / prt_reproject_motion): the id output's staging, the staging of host
  // id images (this view's, the previous view's) and the motion matrices on the device
  DevBuf aov_ids, rp_ids[2], rp_motion;
  // moments and variance (prt_reproject_moments / prt_denoise_variance): the staging of host moments images (the
  // previous one, the output; the filter's input) and of the filter's variance output
  DevBuf rp_mom[2], dn_mom, dn_var;
  // deforming meshes (prt_snapshot_mesh / prt_render_aov_deform / prt_reproject_deform): per mesh the snapshot of its
  // primitives' corners (nine floats each; empty until the mesh's first snapshot), the device table of their
  // addresses (one per mesh, null = no snapshot; allocated by a context's first snapshot) and its host copy; the
  // staging of the offset output and of a host offset image.  prt_set_meshes discards the snapshots.  The previous
  // transforms' rows follow the motion matrices in rp_motion.
  std::vector<DevBuf> snap;
  std::vector<const float*> snap_host;
  DevBuf snap_tab;
  DevBuf aov_off, rp_off;
  // ray queries (prt_query_rays / prt_query_surface, prt_api_query.cpp): the staging of host rays (origins, directions,
  // tmax) and of the hit / occlusion outputs, the fetch counters of k_query (kParts, cleared in stream order before each
  // launch); the staging of host hit records and their tmax, and of the four surface outputs.  Allocated at first use
  DevBuf q_in[3], q_hits, q_occ, q_ctr;
  DevBuf qs_in[2], qs_out[4];
  // skinning (prt_set_mesh_skin / prt_skin_mesh, prt_skin.h): one binding per mesh (empty until the first binding
  // after a prt_set_meshes, which discards them all)
  std::vector<prt::host::SkinBinding> skin;
};

namespace prt::host {

// prt_api.cpp: the context stream waits for the frames in flight (every entry point but an in-flight prt_render
// starts with it); a pinned staging buffer (prt_ctx::stage) and its return once the copies out of it are enqueued;
// the pool allocated ahead for uploads of up to `bytes` (stage_reserve); host memory into device memory through one
// staging buffer, in the context stream's order (stage_upload)
int join_flights(prt_ctx* c);
#define PRT_JOIN(ctx) PRT_TRY(::prt::host::join_flights(ctx))
int stage_acquire(prt_ctx* c, size_t bytes, StageSlot*& out);
int stage_release(prt_ctx*, StageSlot& st, hipStream_t s);
int stage_reserve(prt_ctx* c, size_t bytes);
int stage_upload(prt_ctx* c, void* dst, const void* src, size_t bytes);
// prt_api_instance.cpp: the device instance state brought up to the host's instances, when it is out of date
// (scene_ready calls it before every frame); the mark of a frame's read of the instance state
int ensure_instances(prt_ctx* c);
int record_inst_use(prt_ctx* c, hipStream_t st);
// prt_api.cpp, for the render path: finish the queued frames before resident buffers are overwritten or freed; the
// bounded RCCL waits; the traversal occupancy and whether the stacks cover the BVH; the HBM spill columns of S; the
// scene as the kernels get it; the screen pass's parameters
int drain(prt_ctx* c);
ncclResult_t rccl_settle(const Rccl* R, ncclComm_t comm, ncclResult_t r);
int rccl_wait(prt_ctx* c, hipStream_t s, const char* what);
int occ_for(const prt_ctx* c);
bool depth_ok(const prt_ctx* c);
int ensure_spill(prt_ctx* c, SceneDev& S, size_t threads);
int scene_ready(prt_ctx* c, SceneDev& S);
PostDev post_params(const prt_ctx* c, int32_t W, int32_t H);
// prt_api.cpp, for the mesh and instance entry points (prt_api_mesh.cpp, prt_api_instance.cpp): wait for the context stream (bounded on an RCCL-sharded
// context, as drain())
int wait_stream(prt_ctx* c, const char* what);
// a setter of a local group applies to every member (member 0 = the group context itself)
#define PRT_FOR_MEMBERS(call) \
  for (prt_ctx* m : c->members) PRT_TRY(call)
// the mesh index of an entry point that needs the meshes set
inline int mesh_arg(const prt_ctx* c, int32_t mi) {
  if (c->mesh_host.empty()) return fail(PRT_ERR_NOT_READY, "no meshes: call prt_set_meshes");
  if (mi < 0 || (size_t)mi >= c->mesh_host.size()) return fail(PRT_ERR_INVALID_ARGUMENT, "mesh index out of range");
  return PRT_OK;
}
// prt_api_render.cpp: the context's traversal stack overflow count (waits for the context stream); a shard's tile size
// and event
uint64_t diag_overflows(prt_ctx* c, bool* layout_ok = nullptr, bool* wait_ok = nullptr);
int shard_setup(prt_ctx* c, int32_t tile);
// prt_api_image.cpp: record timing event k (prt_ctx::dn_ev) on the context stream
int dn_event(prt_ctx* c, int k);

// Host images of an image-space entry point, staged through context buffers.  With PRT_OUT_DEVICE the caller's
// pointers are device pointers and every operation leaves them alone.  Otherwise in() copies a host input into its
// context buffer on the context stream, out() hands out the context buffer in an output's place, and both make the
// pointer name that buffer; finish() copies the outputs back, in the order they were registered, and waits for the
// stream.  A null pointer stays null.
struct Staging {
  prt_ctx* c;
  bool dev;
  struct Back { void* host; const void* devp; size_t bytes; } back[4] = {};
  int nback = 0;
  Staging(prt_ctx* ctx, uint32_t out_flags) : c(ctx), dev((out_flags & PRT_OUT_DEVICE) != 0) {}
  template <class T>
  int in(DevBuf& b, const T*& p, size_t bytes) {
    if (dev || !p) return PRT_OK;
    HIP_TRY(b.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(b.p, p, bytes, hipMemcpyHostToDevice, c->stream));
    p = b.as<const T>();
    return PRT_OK;
  }
  template <class T>
  int out(DevBuf& b, T*& p, size_t bytes) {
    if (dev || !p) return PRT_OK;
    if (nback == 4) return fail(PRT_ERR_INVALID_ARGUMENT, "too many staged outputs");
    HIP_TRY(b.ensure(bytes));
    back[nback++] = {p, b.p, bytes};
    p = b.as<T>();
    return PRT_OK;
  }
  int finish() {
    if (dev) return PRT_OK;
    for (int k = 0; k < nback; k++)
      HIP_TRY(hipMemcpyAsync(back[k].host, back[k].devp, back[k].bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRT_OK;
  }
};

}  // namespace prt::host
