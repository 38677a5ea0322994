// prt_api_instance.cpp -- the instance entry points of the C ABI (include/prt.h): prt_set_instances,
// prt_set_instance_materials, prt_update_instances, prt_rebuild_instances, prt_tlas_cost, prt_read_tlas, and the
// instance state they advance: the ring of copies the frames read (InstSet), the instance BVH's builds on the calling
// thread, the worker thread and the device, the live tree's topology.  Each step of an update stands once, as a helper
// below; what needs no device is prt_instance_host.h.  The context and the pinned staging pool are prt_ctx.h /
// prt_api.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bvh_build.h"
#include "bvh_gpu.h"
#include "prt_blas_cost_gpu.h"
#include "prt_ctx.h"
#include "prt_instance_host.h"
#include "prt_mesh_host.h"
#include "prt_tlas_refit_gpu.h"

using namespace prt;
using namespace prt::host;

static_assert(sizeof(InstSrc) == kInstSrcBytes && sizeof(InstDev) == kInstDevBytes, "prt_instance_host.h record sizes");

namespace {

// The device buffers of an instance state of n instances: every copy of the ring (frames in flight + 1) and the
// scratch of prt_update_instances, sized for n (at least the linear-list size; a tree over n instances has at most
// max(n, 1) nodes), so that later updates never reallocate.  A reallocation frees what queued frames read: it drains
// first, a host wait.  Only a buffer that is too small is replaced (its contents are lost: a copy that holds the
// current state is large enough).
int size_instance_state(prt_ctx* c, int32_t n, bool use_tlas) {
  if (c->isets.size() < (size_t)c->inflight + 1) c->isets.resize((size_t)c->inflight + 1);
  const InstBufBytes B = inst_buffer_bytes(n, kLinearInstances, c->mesh_host.size(), use_tlas);
  // every buffer with its size, and the flag that says its contents are current (a replaced buffer has none)
  auto each = [&](auto&& f) {
    for (InstSet& I : c->isets) {
      f(I.inst, B.inst, nullptr);
      f(I.inst_src, B.inst_src, nullptr);
      f(I.tlas8, B.tlas8, nullptr);
      f(I.tlas_slot, B.tlas_slot, nullptr);
    }
    f(c->inst_tab, B.inst_tab, &c->inst_tab_ok);
    f(c->tlas_order, B.tlas_order, &c->tlas_topo);
    f(c->tlas_box, B.tlas_box, nullptr);
  };
  bool fit = true;
  each([&](DevBuf& b, size_t need, bool*) { fit = fit && b.bytes >= need; });
  if (fit) return PRT_OK;
  PRT_TRY(drain(c));
  hipError_t grown = hipSuccess;
  each([&](DevBuf& b, size_t need, bool* current) {
    if (grown != hipSuccess || b.bytes >= need) return;
    grown = b.ensure(need);
    if (current) *current = false;
  });
  HIP_TRY(grown);
  return PRT_OK;
}

int worker_ok(prt_ctx* c) {
  if (!c->tlas_worker) return PRT_OK;
  const TlasWorker::Stats ws = c->tlas_worker->stats();
  if (ws.failed) return fail(PRT_ERR_HIP, "instance BVH build failed on the worker thread: " + ws.err);
  return PRT_OK;
}

// The worker's queue runs empty (a host condition variable, no GPU involved: at most the queued builds) and none of
// its builds failed: its last tree is then what the last upload on the stream carries
int worker_settled(prt_ctx* c) {
  if (!c->tlas_worker) return fail(PRT_ERR_NOT_READY, "no instance BVH");
  c->tlas_worker->wait_idle();
  return worker_ok(c);
}

// The live tree's topology as a device refit reads it: n_nodes nodes, ordered by level in tlas_order (level d's nodes
// are order[ends[d - 1] .. ends[d])), uploaded in the context stream's order
int set_tlas_topology(prt_ctx* c, const std::vector<uint32_t>& order, std::vector<uint32_t>& ends, uint32_t n_nodes) {
  PRT_TRY(stage_upload(c, c->tlas_order.p, order.data(), 4 * (size_t)n_nodes));
  c->tlas_nodes = n_nodes;
  c->tlas_level_ends = std::move(ends);
  c->tlas_topo = true;
  return PRT_OK;
}

// The topology of the instance BVH the device holds (or will hold once the stream has run the queued uploads), once
// per build: the worker's last tree (worker_settled); tree_levels checks every link and orders the nodes by level.
// An update's staging buffer holds cap_nodes records of which only these are the tree's: no kernel ever runs over
// more than tlas_nodes.
int tlas_topology(prt_ctx* c, int32_t n) {
  if (c->tlas_topo) return PRT_OK;
  PRT_TRY(worker_settled(c));
  std::vector<Node8> nodes;
  std::vector<uint32_t> slot;
  c->tlas_worker->last_tree(nodes, slot);
  const size_t nn = nodes.size();
  if (!nn || nn > tlas_node_cap(n) || slot.size() != 8 * nn) return fail(PRT_ERR_HIP, "instance BVH: no usable tree");
  std::vector<uint32_t> ends, order;
  const char* err = nullptr;
  if (!tree_levels(nodes.data(), nn, 0u, 0u, (uint32_t)(8 * nn), ends, order, &err))
    return fail(PRT_ERR_HIP, std::string("instance BVH: ") + err);
  return set_tlas_topology(c, order, ends, (uint32_t)nn);
}

// The first step of every update: the copy of the instance state it writes, isets[nx], the next one in the ring
// (frames in flight + 1 copies), once the context stream has waited for the frames that read it.  Every copy and the
// scratch of prt_update_instances are sized here, for the instance count, so that later updates never reallocate.  The
// current copy and icur are left alone until commit_copy: a failure in between leaves a half-written copy that no
// frame reads.
int begin_next_copy(prt_ctx* c, bool use_tlas, size_t& nx) {
  const int32_t n = (int32_t)c->inst_mesh.size();
  for (int32_t i = 0; i < n; i++)
    if (c->inst_mesh[i] >= c->mesh_host.size()) return fail(PRT_ERR_INVALID_ARGUMENT, "instance references a missing mesh");
  PRT_TRY(size_instance_state(c, n, use_tlas));
  nx = (c->icur + 1) % c->isets.size();
  InstSet& X = c->isets[nx];
  for (size_t k = 0; k < X.nuse; k++) HIP_TRY(hipStreamWaitEvent(c->stream, X.uses[k].second, 0));
  X.nuse = 0;
  return PRT_OK;
}

// The last step: the frames read copy nx, written for n instances, from here on.  What differs between the callers
// (inst_tab_ok, the topology, use_tlas / tlas_depth / tlas_n, the counters, the worker's seed) stays with them.
void commit_copy(prt_ctx* c, size_t nx, int32_t n) {
  c->icur = nx;
  c->iset_n = n;
  c->inst_dirty = false;
  c->tlas_dirty = false;
}

// the refit input of every instance (prt_refit.h) from host transforms xf (16 floats each: the host's inst_xf, or a
// call's own before it commits them), the mesh boxes and the kinds
void fill_ctx_inst_src(const prt_ctx* c, const float* xf, InstSrc* src) {
  prt::host::fill_inst_src((int32_t)c->inst_mesh.size(), c->inst_mesh.data(), c->inst_kind.data(), c->inst_kind.size(),
                           c->mesh_info.data(), xf, src);
}

// The records of copy X (inst, by k_refit) from the sources the stream has put at X.inst_src by then
int refit_records(prt_ctx* c, InstSet& X, int32_t n) {
  HIP_TRY(launch_refit(c->stream, X.inst_src.as<InstSrc>(), n, X.inst.as<InstDev>()));
  return PRT_OK;
}

// What prt_update_instances and prt_rebuild_instances share: the records of the copy begun (isets[nx]: inst_src, then
// inst) from new transforms, or from the same ones under new kinds or mesh boxes.  xf_host: 16 floats per instance in
// host memory; xf_dev: packed 4x4 matrices in device memory; both null: the transforms kept in the current copy's
// inst_src (device-resident transforms; the caller passes the host's inst_xf otherwise).  The caller puts a tree into
// the same copy and commits.
int next_instance_records(prt_ctx* c, size_t nx, const float* xf_host, const float* xf_dev) {
  const int32_t n = (int32_t)c->inst_mesh.size();
  InstSet& cur = c->isets[c->icur];
  InstSet& X = c->isets[nx];
  if (xf_host) {  // the records' input filled on the host, as ensure_instances fills it
    c->inst_stage.resize(n);
    fill_ctx_inst_src(c, xf_host, c->inst_stage.data());
    PRT_TRY(stage_upload(c, X.inst_src.p, c->inst_stage.data(), sizeof(InstSrc) * (size_t)n));
    c->inst_tab_ok = false;  // (the table was not brought up to what this refill read)
  } else {
    const InstTabLayout L = inst_tab_layout(inst_cap(n, kLinearInstances), c->mesh_host.size());
    if (!c->inst_tab_ok || c->inst_dirty) {  // mesh ids, kinds and the meshes' current root boxes
      std::vector<char> tab(L.total);
      fill_inst_tab(n, c->inst_mesh.data(), c->inst_kind.data(), c->inst_kind.size(), c->mesh_info.data(),
                    c->mesh_info.size(), L, tab.data());
      PRT_TRY(stage_upload(c, c->inst_tab.p, tab.data(), L.total));
      c->inst_tab_ok = true;
    }
    const char* t = c->inst_tab.as<char>();
    const InstTabDev tab = {reinterpret_cast<const uint32_t*>(t), reinterpret_cast<const uint32_t*>(t + L.kind),
                            reinterpret_cast<const float4*>(t + L.box), (uint32_t)c->mesh_host.size()};
    if (xf_dev) HIP_TRY(launch_inst_src(c->stream, reinterpret_cast<const float4*>(xf_dev), 4u, tab, n, X.inst_src.as<InstSrc>()));
    else if (&X != &cur) HIP_TRY(launch_inst_src(c->stream, cur.inst_src.as<const float4>(), 6u, tab, n, X.inst_src.as<InstSrc>()));
    else return fail(PRT_ERR_HIP, "instance update: one copy of the instance state");  // (the ring holds at least two)
  }
  return refit_records(c, X, n);
}

// prt_update_instances and, while the transforms are device-resident, every refresh of the instance records: the
// next copy of the instance state from new transforms (or from the same ones under new kinds or mesh boxes), with the
// instance BVH refitted over it (prt_tlas_refit.h).  xf_dev: packed 4x4 matrices in device memory; null: the host's
// inst_xf, or, while prt_ctx::xf_device, the transforms kept in the current copy's inst_src.  Everything is enqueued on
// the context stream: no host build, no worker job, no wait for the GPU.
int refit_instances(prt_ctx* c, const float* xf_dev) {
  const int32_t n = (int32_t)c->inst_mesh.size();
  const bool use_tlas = c->use_tlas;
  const bool on_dev = xf_dev || c->xf_device;
  PRT_TRY(worker_ok(c));
  size_t nx = 0;
  PRT_TRY(begin_next_copy(c, use_tlas, nx));
  if (use_tlas) PRT_TRY(tlas_topology(c, n));
  PRT_TRY(next_instance_records(c, nx, on_dev ? nullptr : c->inst_xf.data(), xf_dev));
  InstSet& cur = c->isets[c->icur];
  InstSet& X = c->isets[nx];
  if (use_tlas)  // deepest level first, the root last: every child's box is written before its parent reads it
    for (size_t lv = c->tlas_level_ends.size(); lv-- > 0;) {
      const uint32_t b = lv ? c->tlas_level_ends[lv - 1] : 0u;
      HIP_TRY(launch_tlas_refit_level(c->stream, cur.tlas8.as<Node8>(), cur.tlas_slot.as<uint32_t>(), X.tlas8.as<Node8>(),
                                      X.tlas_slot.as<uint32_t>(), X.inst.as<InstDev>(), (uint32_t)n,
                                      c->tlas_box.as<float>(), c->tlas_order.as<uint32_t>() + b,
                                      c->tlas_level_ends[lv] - b, c->tlas_nodes));
    }
  commit_copy(c, nx, n);
  return PRT_OK;
}

}  // namespace

// Instance records on the device (prt_refit.h: MESA inverse, normal matrix, inflated world box): one async copy of
// the transforms + k_refit on the render stream, so frames already queued keep reading the previous instances.
// The instance BVH over those boxes (the same refit_instance on the host) is rebuilt for every update, as the
// reference rebuilds its TLAS every frame (Core/Renderer.cpp:33-41, Core/tiny_bvh.h:1732-1770 BVH::Build over the
// BLASInstances), by the host SAH build + SAH-optimal collapse: on the calling thread when the instance set changes
// (its depth sizes the traversal stacks), and for every later update on the context's worker thread, the render
// stream waiting for that update's build in a one-lane kernel before its upload (TlasWorker says why no host
// function).  The caller only copies the update's transforms; every frame walks the tree built over its own instances.
int prt::host::ensure_instances(prt_ctx* c) {
  if (!c->inst_dirty) return PRT_OK;
  // device-resident transforms (prt_update_instances with PRT_IN_DEVICE): the host copy is stale; the records come
  // from the transforms kept on the device, under the new kinds and mesh boxes, and the tree is refitted
  if (c->xf_device) return refit_instances(c, nullptr);
  const int32_t n = (int32_t)c->inst_mesh.size();
  const char* te = std::getenv("PRT_TLAS");  // 1: the instance BVH at any instance count (tests)
  // (a materials-only update, prt_set_instance_materials, moves no box: the records' kinds are rewritten over
  // unchanged inverses and boxes, and the instance BVH is left as it is)
  const InstRefresh plan = plan_instance_refresh(n, kLinearInstances, te && std::atoi(te) == 1, c->use_tlas, c->tlas_n,
                                                 c->tlas_dirty, c->tlas_worker != nullptr);
  const bool use_tlas = plan.use_tlas, tree_work = plan.tree_work, async = plan.async;
  PRT_TRY(worker_ok(c));
  size_t nx = 0;
  PRT_TRY(begin_next_copy(c, use_tlas, nx));
  InstSet& cur = c->isets[c->icur];
  InstSet& X = c->isets[nx];
  // (filled in ordinary memory and copied into the pinned staging buffer in one memcpy: field-by-field stores into
  // pinned memory cost ~10 ms per 10,000 instances on the GPU box, profiles/r06_tlas_drift.txt)
  std::vector<InstSrc>& src = c->inst_stage;
  src.resize(n);
  fill_ctx_inst_src(c, c->inst_xf.data(), src.data());
  // a new instance set: its first tree on the calling thread; the stacks are sized for the largest depth that keeps
  // the traversal's occupancy (and at least the median-split tree's), the cap of the worker's builds
  BuiltTlas8 tree;
  int depth_cap = c->tlas_depth;
  if (tree_work && !async) {
    std::vector<float> boxes(6 * (size_t)n);
    for (int32_t i = 0; i < n; i++) {
      InstDev I;
      refit_instance(src[i], I);
      std::memcpy(&boxes[6 * (size_t)i], I.bmin, 12);
      std::memcpy(&boxes[6 * (size_t)i + 3], I.bmax, 12);
    }
    tree = build_tlas8(boxes.data(), n);
    depth_cap = tlas_depth_cap(c->max_depth, tree.depth, n);
  }
  const size_t cap_nodes = tlas_node_cap(n);
  // Uploads through ONE pinned staging slot: the instance sources, then the tree's nodes and slots.  The worker reads
  // job->src from that slot, and the slot's event is what keeps it from being handed out again until the tree's upload
  // has run: with the sources in a slot of their own (stage_upload) that slot could be rewritten before the worker has
  // read them.  So the records step shared with next_instance_records starts at "the sources are on their way to
  // X.inst_src" (refit_records).
  const InstStageBytes sb = inst_stage_bytes(n, plan, tree.nodes.size());
  PRT_TRY(stage_reserve(c, sb.per));  // (the staging buffers this instance set's updates use: none allocated later)
  StageSlot* st = nullptr;
  PRT_TRY(stage_acquire(c, sb.src + sb.nodes + sb.slot, st));
  char* hp = static_cast<char*>(st->p);
  st->lost = true;  // until the copies out of it are enqueued (a failure below leaves it out of the pool)
  std::memcpy(hp, src.data(), sb.src);  // (the worker reads the sources from here)
  HIP_TRY(hipMemcpyAsync(X.inst_src.p, hp, sb.src, hipMemcpyHostToDevice, c->stream));
  PRT_TRY(refit_records(c, X, n));
  if (tree_work) {
    char* q = hp + sb.src;
    if (async) {  // the worker writes the tree into q; the stream's upload waits for it
      const size_t k = (size_t)(st - c->stage.data());  // this buffer's flag word (free with the buffer)
      auto job = std::make_shared<TlasJob>();
      job->src = reinterpret_cast<const InstSrc*>(hp);
      job->n = n;
      job->dst = q;
      job->cap = cap_nodes;
      job->max_depth = c->tlas_depth;
      job->flag = c->stage_flag + 16 * k;
      __atomic_store_n(job->flag, 0u, __ATOMIC_RELAXED);
      HIP_TRY(launch_wait_host(c->stream, c->stage_flag_dev + 16 * k, c->diag.as<uint32_t>() + 2, kHostWaitLimitS));
      c->tlas_worker->submit(job);
    } else {
      std::memcpy(q, tree.nodes.data(), sb.nodes);
      std::memcpy(q + sb.nodes, tree.slot.data(), sb.slot);
    }
    HIP_TRY(hipMemcpyAsync(X.tlas8.p, q, sb.nodes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(X.tlas_slot.p, q + sb.nodes, sb.slot, hipMemcpyHostToDevice, c->stream));
  } else if (use_tlas && &X != &cur) {  // a materials-only update: the current tree, into this copy
    HIP_TRY(hipMemcpyAsync(X.tlas8.p, cur.tlas8.p, cap_nodes * sizeof(Node8), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(X.tlas_slot.p, cur.tlas_slot.p, cap_nodes * kSlotBytes, hipMemcpyDeviceToDevice, c->stream));
  }
  PRT_TRY(stage_release(c, *st, c->stream));
  st->lost = false;
  c->use_tlas = use_tlas;
  if (!use_tlas) {
    c->tlas_depth = 0;
    c->tlas_n = -1;
  } else if (tree_work && !async) {  // a new instance set
    if (!c->tlas_worker) c->tlas_worker.reset(new TlasWorker());
    c->tlas_worker->seed(tree);
    c->tlas_depth = depth_cap;
    c->tlas_rebuilds = c->tlas_async = 0;
    c->tlas_n = n;
  } else if (async) {
    c->tlas_rebuilds++;
    c->tlas_async++;
  }
  commit_copy(c, nx, n);
  c->inst_tab_ok = false;               // (a device-side refill uploads what this one read)
  if (tree_work) c->tlas_topo = false;  // a new tree: the next prt_update_instances takes its topology
  return PRT_OK;
}

// a frame enqueued on stream st reads the current copy of the instance state: the next update that rewrites it
// waits for this point of st (InstSet)
int prt::host::record_inst_use(prt_ctx* c, hipStream_t st) {
  InstSet& I = c->isets[c->icur];
  for (size_t k = 0; k < I.nuse; k++)
    if (I.uses[k].first == st) {
      HIP_TRY(hipEventRecord(I.uses[k].second, st));
      return PRT_OK;
    }
  if (I.nuse == I.uses.size()) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    I.uses.push_back({st, e});
  }
  I.uses[I.nuse].first = st;
  HIP_TRY(hipEventRecord(I.uses[I.nuse].second, st));
  I.nuse++;
  return PRT_OK;
}

namespace {

// The arguments of an update of a kept instance set (prt_update_instances, prt_rebuild_instances; `who` names the
// call in the texts), after the call's own null checks.  xf null: the transforms the context holds (a rebuild).
// dev_in: xf is device memory.
int check_kept_set_update(prt_ctx* c, const std::string& who, const float* xf, int32_t n, uint32_t in_flags, bool& dev_in) {
  if (in_flags & ~PRT_IN_DEVICE) return fail(PRT_ERR_INVALID_ARGUMENT, "unknown input flags");
  if (!xf && in_flags) return fail(PRT_ERR_INVALID_ARGUMENT, who + " without transforms takes no input flags");
  if (c->mesh_host.empty()) return fail(PRT_ERR_NOT_READY, "no meshes: call prt_set_meshes");
  if (c->inst_mesh.empty()) return fail(PRT_ERR_NOT_READY, "no instances: call prt_set_instances");
  if (n != (int32_t)c->inst_mesh.size())
    return fail(PRT_ERR_INVALID_ARGUMENT, who + ": the instance count must stay (a new set needs prt_set_instances)");
  dev_in = xf && (in_flags & PRT_IN_DEVICE) != 0;
  if (dev_in && c->sh_kind == 2) return fail(PRT_ERR_UNSUPPORTED, "device transforms on a local shard group");
  if (dev_in && (reinterpret_cast<uintptr_t>(xf) & 15u))
    return fail(PRT_ERR_INVALID_ARGUMENT, "device transforms must be 16-byte aligned");
  return worker_ok(c);
}

// The set was never brought to the device (prt_set_instances came before the meshes): its first build, from the
// host's transforms, decides between the list and the tree; device transforms then move it.  *first: it was built here
int first_build_if_needed(prt_ctx* c, int32_t n, bool* first = nullptr) {
  const bool f = c->iset_n != n;
  if (first) *first = f;
  if (!f) return PRT_OK;
  c->inst_dirty = true;
  c->tlas_dirty = true;
  return ensure_instances(c);
}

// A call's own transforms become the context's: host transforms are kept in inst_xf, which is current again; device
// transforms live in the current copy's inst_src alone (prt_ctx::xf_device)
void keep_call_transforms(prt_ctx* c, const float* xf, int32_t n, bool dev_in) {
  if (!dev_in) c->inst_xf.assign(xf, xf + 16 * (size_t)n);
  c->xf_device = dev_in;
}

// the instance state as the next frame reads it, and the live tree's node count (0: the rays walk the linear list)
int tlas_current(prt_ctx* c, uint32_t& n_nodes) {
  if (c->mesh_host.empty()) return fail(PRT_ERR_NOT_READY, "no meshes: call prt_set_meshes");
  if (c->inst_mesh.empty()) return fail(PRT_ERR_NOT_READY, "no instances: call prt_set_instances");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  PRT_TRY(ensure_instances(c));
  n_nodes = 0;
  if (!c->use_tlas) return PRT_OK;
  if (c->tlas_topo) {
    n_nodes = c->tlas_nodes;
  } else {  // the worker's last tree is the one the stream uploads last (tlas_topology)
    PRT_TRY(worker_settled(c));
    n_nodes = (uint32_t)c->tlas_worker->last_tree_nodes();
  }
  return PRT_OK;
}

}  // namespace

extern "C" {

int prt_set_instances(prt_ctx* c, const float* xf, const uint32_t* mi, int32_t n) {
  if (!c || !xf || !mi || n <= 0) return fail(PRT_ERR_INVALID_ARGUMENT, "bad instances");
  // (no join of the frames in flight: the update writes the next copy of the instance state, InstSet)
  if (n > kMaxInstances) return fail(PRT_ERR_UNSUPPORTED, "more than 2^24 instances");
  if ((size_t)n != c->inst_mesh.size()) c->inst_kind.clear();  // materials survive transform updates only
  c->inst_mesh.assign(mi, mi + n);
  keep_call_transforms(c, xf, n, false);  // (prt_update_instances with device transforms made the host copy stale)
  c->inst_dirty = true;
  c->tlas_dirty = true;
  c->shade_epoch++;
  c->inst_epoch++;  // transforms, boxes, the instance BVH and the hit word's instance bits: kept primary hits are stale
  HIP_TRY(hipSetDevice(c->device));
  if (!c->mesh_host.empty()) {
    PRT_TRY(ensure_instances(c));
  }
  PRT_FOR_MEMBERS(prt_set_instances(m, xf, mi, n));
  return PRT_OK;
}

int prt_set_instance_materials(prt_ctx* c, const int32_t* kinds, int32_t n) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  // (no join of the frames in flight: the update writes the next copy of the instance state, InstSet)
  if (n == 0 || !kinds) {
    c->inst_kind.clear();
  } else {
    if (n != (int32_t)c->inst_mesh.size()) return fail(PRT_ERR_INVALID_ARGUMENT, "one material kind per instance");
    for (int32_t i = 0; i < n; i++)
      if (kinds[i] < PRT_MAT_TEXTURED || kinds[i] > PRT_MAT_MIRROR) return fail(PRT_ERR_INVALID_ARGUMENT, "bad material kind");
    c->inst_kind.assign(kinds, kinds + n);
  }
  // No inst_epoch bump: a kept primary hit is (t, u, v, prim | inst << pbits), and a materials-only update moves no
  // transform, box or tree (ensure_instances) and leaves pbits alone; the kind is read at shading, from the
  // instance record.  Dielectric kinds switch to the extension kernels, which neither read nor write phit.
  c->shade_epoch++;  // ... but a kept primary surface holds the material the kind shaped
  c->inst_dirty = true;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->mesh_host.empty() && !c->inst_mesh.empty()) {
    PRT_TRY(ensure_instances(c));
  }
  PRT_FOR_MEMBERS(prt_set_instance_materials(m, kinds, n));
  return PRT_OK;
}

int prt_update_instances(prt_ctx* c, const float* xf, int32_t n, uint32_t in_flags) {
  if (!c || !xf) return fail(PRT_ERR_INVALID_ARGUMENT, "bad instance update arguments");
  bool dev_in = false;
  PRT_TRY(check_kept_set_update(c, "instance update", xf, n, in_flags, dev_in));
  // (no join of the frames in flight: the update writes the next copy of the instance state, InstSet)
  HIP_TRY(hipSetDevice(c->device));
  if (!dev_in) keep_call_transforms(c, xf, n, false);  // (the first build and the refit read inst_xf)
  bool first = false;
  PRT_TRY(first_build_if_needed(c, n, &first));
  if (dev_in || !first) PRT_TRY(refit_instances(c, dev_in ? xf : nullptr));
  if (dev_in) keep_call_transforms(c, xf, n, true);  // (not before: a first build is from the host's transforms)
  c->shade_epoch++;
  c->inst_epoch++;  // transforms, boxes and the instance BVH changed: kept primary hits and light visibility are stale
  PRT_FOR_MEMBERS(prt_update_instances(m, xf, n, in_flags));
  return PRT_OK;
}

int prt_rebuild_instances(prt_ctx* c, const float* xf, int32_t n, uint32_t in_flags, int32_t builder) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (builder == PRT_BUILDER_HOST_SAH || builder == PRT_BUILDER_HOST_SBVH)
    return fail(PRT_ERR_UNSUPPORTED, "instance rebuild: the host builders rebuild through prt_set_instances only");
  if (builder != PRT_BUILDER_GPU_LBVH && builder != PRT_BUILDER_GPU_PLOC)
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad instance BVH builder");
  bool dev_in = false;
  PRT_TRY(check_kept_set_update(c, "instance rebuild", xf, n, in_flags, dev_in));
  // (no join of the frames in flight: the rebuild writes the next copy of the instance state, InstSet)
  HIP_TRY(hipSetDevice(c->device));
  PRT_TRY(first_build_if_needed(c, n));
  if (!c->use_tlas) {  // the linear list has no tree: the call is prt_update_instances (every member included)
    if (!xf) return PRT_OK;
    return prt_update_instances(c, xf, n, in_flags);
  }
  const size_t N = (size_t)n;
  if (c->tb_fat.bytes < 48 * N || c->tb_nodes.bytes < sizeof(Node8) * N || c->tb_tris.bytes < sizeof(TriMT) * N) {
    PRT_TRY(wait_stream(c, "prt_rebuild_instances"));  // (an earlier rebuild's kernels read the scratch this frees)
    HIP_TRY(c->tb_fat.ensure(48 * N));
    HIP_TRY(c->tb_nodes.ensure(sizeof(Node8) * N));
    HIP_TRY(c->tb_tris.ensure(sizeof(TriMT) * N));
  }
  // The next copy's records, then the builder's input from their boxes.  Nothing the frames read changes before the
  // commit below: a failure from here on leaves a half-written copy that is not the current one.
  size_t nx = 0;
  PRT_TRY(begin_next_copy(c, c->use_tlas, nx));
  PRT_TRY(next_instance_records(c, nx, dev_in ? nullptr : xf ? xf : c->xf_device ? nullptr : c->inst_xf.data(),
                                dev_in ? xf : nullptr));
  InstSet& X = c->isets[nx];
  HIP_TRY(launch_tlas_prims(c->stream, X.inst.as<InstDev>(), n, c->tb_fat.as<float4>()));
  // The build, into the context's scratch.  The builder synchronises the context stream once per PLOC iteration and
  // once per tree level; the wait before it is the bounded one of an RCCL context.
  PRT_TRY(wait_stream(c, "prt_rebuild_instances"));
  GpuBlasInfo gi = {};
  std::vector<uint32_t> ends;
  const hipError_t be = gpu_build_blas8(c->stream, c->tb_fat.as<float>(), n, /*max_leaf*/ 1, c->tb_nodes.as<Node8>(),
                                        c->tb_tris.as<TriMT>(), &gi, builder == PRT_BUILDER_GPU_PLOC, &ends);
  if (be != hipSuccess) {
    (void)hipGetLastError();
    return fail(PRT_ERR_HIP, std::string("instance rebuild: the device build failed: ") + hipGetErrorString(be));
  }
  bool ok = gi.nodes >= 1 && gi.nodes <= (uint32_t)n && gi.tris == (uint32_t)n && gi.depth >= 1 &&
            ends.size() == (size_t)gi.depth && ends.back() == gi.nodes;
  for (size_t d = 1; ok && d < ends.size(); d++) ok = ends[d] > ends[d - 1];
  if (!ok) return fail(PRT_ERR_HIP, "instance rebuild: the device build returned no usable tree");
  if (const char* tr = std::getenv("PRT_REBUILD_TRACE"); tr && std::atoi(tr) == 1)  // (scripts/instance_rebuild_time.py)
    std::fprintf(stderr, "prt_rebuild_instances: %d instances, %s: %u nodes, %d levels, the builder waited for the stream %u times\n",
                 n, builder == PRT_BUILDER_GPU_PLOC ? "GPU_PLOC" : "GPU_LBVH", gi.nodes, gi.depth, gi.syncs);
  if (c->max_depth + gi.depth > kMaxBvhDepth)
    return fail(PRT_ERR_UNSUPPORTED, "instance rebuild: the new instance BVH is deeper than the traversal stacks cover");
  // The commit, in the context stream's order: the tree as an instance BVH into the next copy, the level order of a
  // later refit (the builder emits level d as [ends[d - 1], ends[d]): the identity), then the host's view of it
  // (the builder is through with its input: the fat triangles' 48 bytes per instance are the 12 per node of the order)
  HIP_TRY(launch_tlas_finish(c->stream, c->tb_nodes.as<Node8>(), c->tb_tris.as<TriMT>(), gi.tris, gi.nodes, (uint32_t)n,
                             ends.data(), ends.size(), c->tb_fat.as<uint32_t>(), X.tlas8.as<Node8>(),
                             X.tlas_slot.as<uint32_t>()));
  std::vector<uint32_t> order(gi.nodes);
  for (uint32_t j = 0; j < gi.nodes; j++) order[j] = j;
  // (with the topology set here, prt_read_tlas / prt_tlas_cost and the next refit never ask the worker for its stale tree)
  PRT_TRY(set_tlas_topology(c, order, ends, gi.nodes));
  // a deeper tree than the stacks were sized for: they are sized from stack_depth(c) at every launch
  if (gi.depth > c->tlas_depth) c->tlas_depth = gi.depth;
  commit_copy(c, nx, n);
  if (xf) keep_call_transforms(c, xf, n, dev_in);
  c->shade_epoch++;
  c->inst_epoch++;  // transforms, boxes and the instance BVH changed: kept primary hits and light visibility are stale
  PRT_FOR_MEMBERS(prt_rebuild_instances(m, xf, n, in_flags, builder));
  return PRT_OK;
}

int prt_tlas_cost(prt_ctx* c, double* cost) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!cost) return fail(PRT_ERR_INVALID_ARGUMENT, "cost is NULL");
  uint32_t nn = 0;
  PRT_TRY(tlas_current(c, nn));
  if (!nn) {
    *cost = 0.0;
    return PRT_OK;
  }
  const size_t slots = (size_t)blas_cost_blocks(nn) + 2;  // the blocks' sums, the root area, the result
  if (c->cost_part.bytes < 8 * slots) {
    PRT_TRY(wait_stream(c, "prt_tlas_cost"));  // (an earlier call's kernels were waited for; a larger tree)
    HIP_TRY(c->cost_part.ensure(8 * slots));
  }
  double* part = c->cost_part.as<double>();
  double* out = part + (slots - 1);
  HIP_TRY(launch_blas_cost(c->stream, c->isets[c->icur].tlas8.as<Node8>(), nn, part, out));
  double v = 0.0;
  HIP_TRY(hipMemcpyAsync(&v, out, 8, hipMemcpyDeviceToHost, c->stream));
  PRT_TRY(wait_stream(c, "prt_tlas_cost"));
  *cost = v;
  return PRT_OK;
}

int prt_read_tlas(prt_ctx* c, void* nodes, uint64_t node_bytes, uint32_t* slots, uint64_t slot_bytes,
                  uint64_t* nodes_needed, uint64_t* slots_needed) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  uint32_t nn = 0;
  PRT_TRY(tlas_current(c, nn));
  const uint64_t nb = (uint64_t)nn * sizeof(Node8), sb = (uint64_t)nn * kSlotBytes;
  if (nodes_needed) *nodes_needed = nb;
  if (slots_needed) *slots_needed = sb;
  if (!nodes || !slots) return PRT_OK;
  if (node_bytes < nb || slot_bytes < sb) return fail(PRT_ERR_INVALID_ARGUMENT, "prt_read_tlas: buffer too small");
  if (nn) {
    const InstSet& I = c->isets[c->icur];
    HIP_TRY(hipMemcpyAsync(nodes, I.tlas8.p, nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(slots, I.tlas_slot.p, sb, hipMemcpyDeviceToHost, c->stream));
  }
  return wait_stream(c, "prt_read_tlas");
}

}  // extern "C"
