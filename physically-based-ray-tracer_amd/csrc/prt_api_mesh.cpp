// prt_api_mesh.cpp -- the mesh entry points of the C ABI (include/prt.h): prt_set_meshes and the BLAS builds, the
// in-place update and skinning with their one refit (refit_mesh), the rebuild of one mesh's BLAS and its SAH measure,
// snapshots, skin bindings, the BLAS read-back.  What they decide without a device is prt_mesh_host.h; the context,
// instances and queries are prt_api.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "bvh_gpu.h"
#include "prt_blas_cost_gpu.h"
#include "prt_ctx.h"
#include "prt_deform.h"
#include "prt_mesh_host.h"

using namespace prt;
using namespace prt::host;

namespace {

// triangles per leaf slot the builders may form (binary SAH leaves and the collapse's leaf slots; 2 / 4 measured
// no better on C4)
int max_leaf_tris() { return 3; }

// byte offsets of a mesh's six arrays (prt_mesh order) in the staging buffers of host-array updates
struct RefitStage { size_t off[6], bytes[6], total; };
RefitStage refit_stage(size_t T, size_t V) {
  RefitStage r = {{}, {48 * T, 48 * T, 24 * T, 12 * T, 12 * V, 12 * T}, 0};
  r.total = packed_layout(r.bytes, r.off);
  return r;
}

// The scratch of the scene as it stands, allocated by the first update after a prt_set_meshes (which drained the
// context, so nothing queued reads what a larger allocation replaces) and kept: later updates allocate nothing.
int refit_scratch(prt_ctx* c, bool host_arrays) {
  RefitScratch& rf = c->rf;
  // box and order are indexed by node position: sized for the node array's length, which is more than the sum of
  // the live nodes once a rebuilt tree was moved to the array's end (prt_rebuild_mesh)
  const size_t nodes = (size_t)c->nodes_len;
  size_t stage = 0;
  for (const MeshHost& m : c->mesh_info) stage = std::max(stage, refit_stage((size_t)m.tris, (size_t)m.verts).total);
  HIP_TRY(rf.box.ensure(24 * nodes));
  HIP_TRY(rf.order.ensure(4 * nodes));
  HIP_TRY(rf.res.ensure(sizeof(RefitResult)));
  if (!rf.res_host)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&rf.res_host), sizeof(RefitResult), hipHostMallocDefault));
  if (!rf.ev) HIP_TRY(hipEventCreateWithFlags(&rf.ev, hipEventDisableTiming));
  if (host_arrays) {
    HIP_TRY(rf.in.ensure(stage));
    if (rf.pin_bytes < stage) {
      if (rf.pin_used) HIP_TRY(hipEventSynchronize(rf.ev));
      rf.pin_used = false;
      if (rf.pin) HIP_TRY(hipHostFree(rf.pin));
      rf.pin = nullptr;
      rf.pin_bytes = 0;
      HIP_TRY(hipHostMalloc(&rf.pin, stage, hipHostMallocDefault));
      rf.pin_bytes = stage;
    }
  }
  return PRT_OK;
}

// The tree levels of mesh mi, once: its nodes are read back, tree_levels (prt_mesh_host.h) checks every link and
// orders the nodes by level, and the order goes to the mesh's part of rf.order.
int refit_levels(prt_ctx* c, int32_t mi) {
  MeshHost& mh = c->mesh_info[mi];
  if (!mh.level_ends.empty()) return PRT_OK;
  const uint32_t root = c->mesh_host[mi].root;
  const size_t n = (size_t)mh.nodes;
  std::vector<Node8> nd(n);
  HIP_TRY(hipMemcpyAsync(nd.data(), c->nodes8.as<Node8>() + root, n * sizeof(Node8), hipMemcpyDeviceToHost, c->stream));
  PRT_TRY(wait_stream(c, "reading the mesh's BLAS"));
  std::vector<uint32_t> ends, order;
  const char* err = nullptr;
  if (!tree_levels(nd.data(), n, root, mh.rec_base, mh.recs, ends, order, &err)) return fail(PRT_ERR_HIP, err);
  HIP_TRY(hipMemcpyAsync(c->rf.order.as<uint32_t>() + root, order.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  PRT_TRY(wait_stream(c, "uploading the mesh's tree levels"));
  mh.level_ends = std::move(ends);
  return PRT_OK;
}

// The refit of mesh mi from the fat triangles d.triangles (device memory), enqueued on the context stream: the record
// pass (with its ShadeTri kernel over d's other arrays when `shade`; otherwise the caller wrote those words), then
// one launch per tree level, deepest first and the root last.  Then the mesh's new box, which the instance records
// and the instance BVH (built on the host) start from: computed here from host_tris, the same triangles in host
// memory, while the device works; with host_tris null read back with the bad-index flag, *bad (28 bytes: the only
// host wait).  The geometry changed: the instance state is dirty, kept primary hits and light visibility are stale.
int refit_mesh(prt_ctx* c, int32_t mi, const RefitMeshDev& d, bool shade, const float* host_tris, bool* bad) {
  const MeshDev& md = c->mesh_host[mi];
  MeshHost& mh = c->mesh_info[mi];
  RefitScratch& rf = c->rf;
  RefitResult* res = rf.res.as<RefitResult>();
  RefitMeshDev r = d;
  if (shade) HIP_TRY(hipMemsetAsync(&res->bad_index, 0, 4, c->stream));
  else r.tri_count = 0;  // (launch_refit_records: no ShadeTri kernel)
  HIP_TRY(launch_refit_records(c->stream, c->tris.as<TriMT>() + mh.rec_base, mh.recs,
                               shade ? c->stri.as<ShadeTri>() + md.prim_base : nullptr, r, res));
  for (size_t lv = mh.level_ends.size(); lv-- > 0;) {
    const uint32_t b = lv ? mh.level_ends[lv - 1] : 0u;
    HIP_TRY(launch_refit_level(c->stream, c->nodes8.as<Node8>(), c->tris.as<TriMT>(), d.triangles, rf.box.as<float>(),
                               rf.order.as<uint32_t>() + md.root + b, mh.level_ends[lv] - b, md.root, res));
  }
  if (!host_tris) {
    HIP_TRY(hipMemcpyAsync(rf.res_host, res, sizeof(RefitResult), hipMemcpyDeviceToHost, c->stream));
    PRT_TRY(wait_stream(c, shade ? "reading the updated mesh's box" : "reading the skinned mesh's box"));
    std::memcpy(mh.bmin, rf.res_host->bmin, sizeof(mh.bmin));
    std::memcpy(mh.bmax, rf.res_host->bmax, sizeof(mh.bmax));
    if (bad) *bad = rf.res_host->bad_index != 0;
  } else {
    refit_box_reset(mh.bmin, mh.bmax);
    for (size_t p = 0; p < (size_t)mh.tris; p++) {
      const float* a = host_tris + 12 * p;
      float lo[3], hi[3];
      refit_box_reset(lo, hi);
      refit_box_grow(lo, hi, a);
      refit_box_grow(lo, hi, a + 4);
      refit_box_grow(lo, hi, a + 8);
      refit_box_merge(mh.bmin, mh.bmax, lo, hi);
    }
  }
  c->inst_dirty = true;
  c->tlas_dirty = true;
  c->shade_epoch++;
  c->scene_epoch++;
  return PRT_OK;
}

// What prt_update_mesh and prt_rebuild_mesh check of *M before anything changes (`who` names the call in the
// message): the arrays, the counts and texture ids against the mesh's, host indices against vertex_count.
int update_args(prt_ctx* c, int32_t mi, const prt_mesh* M, uint32_t in_flags, const std::string& who = "mesh update") {
  const bool dev_in = (in_flags & PRT_IN_DEVICE) != 0;
  if (dev_in && c->sh_kind == 2) return fail(PRT_ERR_UNSUPPORTED, "device arrays on a local shard group");
  std::string why = check_mesh_arrays(*M, kMeshArrays, who, c->tex_host.data(), 0);
  if (!why.empty()) return fail(PRT_ERR_INVALID_ARGUMENT, why);
  if (M->tri_count != c->mesh_info[mi].tris || M->vertex_count != c->mesh_info[mi].verts)
    return fail(PRT_ERR_INVALID_ARGUMENT, who + ": the triangle and vertex counts must stay (topology changes need prt_set_meshes)");
  const int32_t tx[4] = {M->albedo_tex, M->normal_tex, M->metalness_tex, M->emission_tex};
  for (int k = 0; k < 4; k++)
    if (tx[k] != c->mesh_host[mi].tex[k]) return fail(PRT_ERR_INVALID_ARGUMENT, who + ": the texture ids must stay");
  if (!dev_in) why = check_mesh_arrays(*M, kMeshIndices, who, c->tex_host.data(), 0);
  if (!why.empty()) return fail(PRT_ERR_INVALID_ARGUMENT, why);
  return PRT_OK;
}

// The six arrays of *M as the kernels read them, into d: device arrays as they are; host arrays through the
// context's pinned buffer, one copy on the context stream (refit_scratch(c, true) sized both buffers).
int stage_mesh(prt_ctx* c, const prt_mesh* M, bool dev_in, RefitMeshDev& d) {
  const void* src[6] = {M->triangles, M->fixed_normals, M->fixed_uvs, M->indices, M->vertices, M->face_normals};
  if (!dev_in) {
    RefitScratch& rf = c->rf;
    const RefitStage st = refit_stage((size_t)M->tri_count, (size_t)M->vertex_count);
    if (rf.pin_used) HIP_TRY(hipEventSynchronize(rf.ev));  // the previous update's copy out of it has run
    rf.pin_used = false;
    char* pin = static_cast<char*>(rf.pin);
    for (int k = 0; k < 6; k++) std::memcpy(pin + st.off[k], src[k], st.bytes[k]);
    HIP_TRY(hipMemcpyAsync(rf.in.p, pin, st.total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(rf.ev, c->stream));
    rf.pin_used = true;
    for (int k = 0; k < 6; k++) src[k] = rf.in.as<char>() + st.off[k];
  }
  d = {static_cast<const float*>(src[0]), static_cast<const float*>(src[1]), static_cast<const float*>(src[2]),
       static_cast<const int32_t*>(src[3]), static_cast<const float*>(src[4]), static_cast<const float*>(src[5]),
       M->tri_count, M->vertex_count};
  return PRT_OK;
}

// A larger tree than mesh mi's node region holds: the node array grows by `need` nodes and the mesh's region becomes
// the new end (the region it leaves stays where it is, unused: no other mesh's nodes move).  The only step of a
// rebuild that drains and reallocates; the refit scratch, indexed by node position, is dropped with every mesh's tree
// levels and comes back at the next update.
int grow_nodes(prt_ctx* c, int32_t mi, uint32_t need) {
  if (c->nodes_len + need >= (1ull << 32)) return fail(PRT_ERR_UNSUPPORTED, "too many BLAS nodes");
  PRT_TRY(drain(c));
  DevBuf grown;
  HIP_TRY(grown.ensure(sizeof(Node8) * (size_t)(c->nodes_len + need)));
  HIP_TRY(hipMemcpy(grown.p, c->nodes8.p, sizeof(Node8) * (size_t)c->nodes_len, hipMemcpyDeviceToDevice));
  c->nodes8 = std::move(grown);
  c->mesh_host[mi].root = (uint32_t)c->nodes_len;
  c->mesh_info[mi].node_cap = need;
  c->nodes_len += need;
  HIP_TRY(upload(c->mesh, c->mesh_host.data(), c->mesh_host.size() * sizeof(MeshDev)));
  c->rf.box.release();
  c->rf.order.release();
  for (MeshHost& m : c->mesh_info) m.level_ends.clear();
  return PRT_OK;
}

// prt_read_blas / prt_read_blas_tris: the size query (*needed; no buffer: nothing more), then the `need` bytes at src
// into the caller's buffer, complete on return
int read_back(prt_ctx* c, const char* who, const void* src, uint64_t need, void* out, uint64_t bytes, uint64_t* needed) {
  if (needed) *needed = need;
  if (!out) return PRT_OK;
  if (bytes < need) return fail(PRT_ERR_INVALID_ARGUMENT, std::string(who) + ": buffer too small");
  PRT_JOIN(c);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, src, need, hipMemcpyDeviceToHost, c->stream));
  return wait_stream(c, who);
}

}  // namespace

extern "C" {

int prt_set_meshes(prt_ctx* c, const prt_mesh* m_in, int32_t n) {
  if (!c || !m_in || n <= 0) return fail(PRT_ERR_INVALID_ARGUMENT, "bad meshes");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  const int builder = c->builder < 0 ? PRT_BUILDER_HOST_SAH : c->builder;
  const bool gpu = builder == PRT_BUILDER_GPU_LBVH || builder == PRT_BUILDER_GPU_PLOC;
  PRT_TRY(drain(c));
  const auto t_build0 = std::chrono::steady_clock::now();
  struct GpuMesh { DevBuf nodes, tris; GpuBlasInfo gi; uint32_t node_base, tri_base, prim_base; };
  std::vector<GpuMesh> gm(gpu ? n : 0);
  uint32_t gpu_nodes = 0, gpu_tris = 0;
  std::vector<Node8> nodes8;
  std::vector<TriMT> tris;
  std::vector<ShadeTri> stri;
  std::vector<MeshDev> mh(n);
  std::vector<MeshHost> info(n);
  int maxd = 0;
  for (int32_t i = 0; i < n; i++) {
    const prt_mesh& M = m_in[i];
    const std::string why =
        check_mesh_arrays(M, kMeshAll, "mesh " + std::to_string(i), c->tex_host.data(), (int32_t)c->tex_host.size());
    if (!why.empty()) return fail(PRT_ERR_INVALID_ARGUMENT, why);
    const uint32_t tri_base = gpu ? gpu_tris : (uint32_t)tris.size();
    float bmin[3], bmax[3];
    int depth = 0;
    int64_t nnodes = 0, nleaves = 0;
    if (gpu) {  // LBVH or PLOC + SAH-optimal 8-wide collapse on the device (bvh_gpu.hip)
      GpuMesh& g = gm[i];
      DevBuf fat;
      HIP_TRY(upload(fat, M.triangles, 48ull * (size_t)M.tri_count));
      HIP_TRY(g.nodes.ensure(sizeof(Node8) * (size_t)M.tri_count));
      HIP_TRY(g.tris.ensure(sizeof(TriMT) * (size_t)M.tri_count));
      HIP_TRY(gpu_build_blas8(c->stream, fat.as<float>(), M.tri_count, max_leaf_tris(), g.nodes.as<Node8>(), g.tris.as<TriMT>(), &g.gi,
                              builder == PRT_BUILDER_GPU_PLOC));
      fat.release();
      if ((uint64_t)gpu_nodes + g.gi.nodes >= (1ull << 32) || (uint64_t)gpu_tris + g.gi.tris >= (1ull << 32))
        return fail(PRT_ERR_UNSUPPORTED, "too many triangles");
      g.node_base = gpu_nodes;
      g.tri_base = gpu_tris;
      gpu_nodes += g.gi.nodes;
      gpu_tris += g.gi.tris;
      mh[i].root = g.node_base;
      for (int k = 0; k < 3; k++) { bmin[k] = g.gi.bmin[k]; bmax[k] = g.gi.bmax[k]; }
      depth = g.gi.depth; nnodes = g.gi.nodes; nleaves = g.gi.leaves;
    } else {
      // rebase child / triangle offsets into the concatenated arrays
      auto append = [&](BuiltBlas8&& built, std::vector<Node8>& all) -> bool {
        const uint32_t node_base = (uint32_t)all.size();
        if ((uint64_t)tri_base + built.tris.size() >= (1ull << 32) ||
            (uint64_t)node_base + built.nodes.size() >= (1ull << 32))
          return false;
        for (auto& nd : built.nodes) {
          nd.child_base += node_base;
          nd.tri_base += tri_base;
        }
        all.insert(all.end(), built.nodes.begin(), built.nodes.end());
        tris.insert(tris.end(), built.tris.begin(), built.tris.end());
        mh[i].root = node_base;
        std::memcpy(bmin, built.bmin, sizeof(bmin));
        std::memcpy(bmax, built.bmax, sizeof(bmax));
        depth = built.depth; nnodes = (int64_t)built.nodes.size(); nleaves = built.leaves;
        return true;
      };
      const bool ok = append(build_blas8(M.triangles, M.tri_count, max_leaf_tris(), builder == PRT_BUILDER_HOST_SBVH),
                             nodes8);
      if (!ok) return fail(PRT_ERR_UNSUPPORTED, "too many triangles");
    }
    mh[i].prim_base = (uint32_t)stri.size();
    mh[i].vert_base = 0;
    mh[i].tri_count = (uint32_t)M.tri_count;
    const int32_t tx[4] = {M.albedo_tex, M.normal_tex, M.metalness_tex, M.emission_tex};
    for (int k = 0; k < 4; k++) mh[i].tex[k] = tx[k];
    stri.resize(stri.size() + (size_t)M.tri_count);
    for (size_t p = 0; p < (size_t)M.tri_count; p++) fill_shade_tri(stri[mh[i].prim_base + p], p, M);
    // ShadeTri.pad[0]: the primitive's TriMT record (the cooperative traversal tail re-tests a helper's
    // winning triangle from its primitive id, prt_persist.h)
    if (gpu) gm[i].prim_base = mh[i].prim_base;
    else
      for (size_t g = tri_base; g < tris.size(); g++) stri[mh[i].prim_base + tris[g].prim].pad[0] = (uint32_t)g;

    for (int k = 0; k < 3; k++) { info[i].bmin[k] = bmin[k]; info[i].bmax[k] = bmax[k]; }
    info[i].depth = depth;
    info[i].nodes = nnodes;
    info[i].leaves = nleaves;
    info[i].tris = M.tri_count;
    info[i].rec_base = tri_base;
    info[i].recs = gpu ? gm[i].gi.tris : (uint32_t)(tris.size() - tri_base);
    info[i].verts = M.vertex_count;
    info[i].node_cap = nnodes;
    info[i].rec_cap = info[i].recs;
    maxd = std::max(maxd, depth);
  }
  c->nodes8.release();
  if (gpu) {  // concatenate the per-mesh device results, rebase offsets, primitive -> triangle records
    HIP_TRY(c->nodes8.ensure(sizeof(Node8) * (size_t)gpu_nodes));
    HIP_TRY(c->tris.ensure(sizeof(TriMT) * (size_t)gpu_tris));
    HIP_TRY(upload(c->stri, stri.data(), stri.size() * sizeof(ShadeTri)));
    for (int32_t i = 0; i < n; i++) {
      GpuMesh& g = gm[i];
      HIP_TRY(hipMemcpyAsync(c->nodes8.as<Node8>() + g.node_base, g.nodes.p, sizeof(Node8) * (size_t)g.gi.nodes,
                             hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(c->tris.as<TriMT>() + g.tri_base, g.tris.p, sizeof(TriMT) * (size_t)g.gi.tris,
                             hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(gpu_blas_finish(c->stream, c->nodes8.as<Node8>() + g.node_base, g.gi.nodes, g.node_base,
                              c->tris.as<TriMT>() + g.tri_base, g.gi.tris, g.tri_base, c->stri.as<ShadeTri>(),
                              g.prim_base));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    gm.clear();  // the per-mesh device builds were copied into the concatenated arrays
  } else {
    HIP_TRY(upload(c->nodes8, nodes8.data(), nodes8.size() * sizeof(Node8)));
    HIP_TRY(upload(c->tris, tris.data(), tris.size() * sizeof(TriMT)));
    HIP_TRY(upload(c->stri, stri.data(), stri.size() * sizeof(ShadeTri)));
  }
  c->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
  c->built_with = builder;
  HIP_TRY(upload(c->mesh, mh.data(), mh.size() * sizeof(MeshDev)));
  c->mesh_host = mh;
  c->mesh_info = info;
  c->nodes_len = gpu ? (uint64_t)gpu_nodes : (uint64_t)nodes8.size();
  c->max_depth = maxd;
  c->snap.clear();  // the snapshots of the previous meshes (prt_snapshot_mesh): nothing queued reads them (drain)
  c->snap_host.clear();
  c->snap_tab.release();
  c->skin.clear();  // the skin bindings of the previous meshes (prt_set_mesh_skin), likewise
  c->inst_dirty = true;
  c->tlas_dirty = true;
  c->shade_epoch++;
  c->scene_epoch++;  // new geometry and BLASes (and prim bits of the hit word): kept primary hits are stale
  PRT_FOR_MEMBERS(prt_set_meshes(m, m_in, n));
  return PRT_OK;
}

int prt_update_mesh(prt_ctx* c, int32_t mi, const prt_mesh* M, uint32_t in_flags) {
  if (!c || !M) return fail(PRT_ERR_INVALID_ARGUMENT, "bad arguments");
  if (in_flags & ~PRT_IN_DEVICE) return fail(PRT_ERR_INVALID_ARGUMENT, "unknown input flags");
  PRT_TRY(mesh_arg(c, mi));
  PRT_TRY(update_args(c, mi, M, in_flags));
  const bool dev_in = (in_flags & PRT_IN_DEVICE) != 0;
  PRT_JOIN(c);  // frames in flight complete first: they read the geometry this call rewrites in place
  HIP_TRY(hipSetDevice(c->device));
  PRT_TRY(refit_scratch(c, !dev_in));
  PRT_TRY(refit_levels(c, mi));
  RefitMeshDev d;
  PRT_TRY(stage_mesh(c, M, dev_in, d));
  bool bad = false;
  PRT_TRY(refit_mesh(c, mi, d, true, dev_in ? nullptr : M->triangles, &bad));
  if (bad) return fail(PRT_ERR_INVALID_ARGUMENT, "mesh update: an index in device memory is out of range (vertex 0 was read in its place)");
  PRT_FOR_MEMBERS(prt_update_mesh(m, mi, M, in_flags));
  return PRT_OK;
}

int prt_snapshot_mesh(prt_ctx* c, int32_t mi) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_TRY(mesh_arg(c, mi));
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  const size_t nmesh = c->mesh_host.size();
  const MeshDev& md = c->mesh_host[mi];
  if (c->snap.size() != nmesh) {  // the context's first snapshot of these meshes: the table, no snapshot anywhere
    c->snap.clear();
    c->snap.resize(nmesh);
    c->snap_host.assign(nmesh, nullptr);
    HIP_TRY(c->snap_tab.ensure(nmesh * sizeof(const float*)));
    HIP_TRY(hipMemsetAsync(c->snap_tab.p, 0, nmesh * sizeof(const float*), c->stream));
  }
  if (!c->snap[mi].p) {  // the mesh's first snapshot: its storage, and its entry in the table (the one host wait)
    HIP_TRY(c->snap[mi].ensure(36 * (size_t)md.tri_count));
    c->snap_host[mi] = c->snap[mi].as<const float>();
    PRT_TRY(wait_stream(c, "prt_snapshot_mesh"));
    HIP_TRY(hipMemcpy(c->snap_tab.as<const float*>() + mi, &c->snap_host[mi], sizeof(const float*),
                      hipMemcpyHostToDevice));
  }
  HIP_TRY(launch_snapshot_mesh(c->stream, c->stri.as<ShadeTri>() + md.prim_base, md.tri_count,
                               c->snap[mi].as<float>()));
  PRT_FOR_MEMBERS(prt_snapshot_mesh(m, mi));
  return PRT_OK;
}

int prt_set_mesh_skin(prt_ctx* c, int32_t mi, const prt_skin* S) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_TRY(mesh_arg(c, mi));
  if (S) {  // every check on the host, before anything changes
    const MeshHost& mh = c->mesh_info[mi];
    if (S->vertex_count != mh.verts || S->tri_count != mh.tris)
      return fail(PRT_ERR_INVALID_ARGUMENT, "mesh skin: the vertex and triangle counts must equal the mesh's");
    if (S->joint_count < 1 || S->joint_count > 65536)
      return fail(PRT_ERR_INVALID_ARGUMENT, "mesh skin: joint_count must be 1..65536");
    if (!S->positions || !S->normals || !S->indices || !S->joints || !S->weights)
      return fail(PRT_ERR_INVALID_ARGUMENT, "mesh skin: missing arrays");
    for (size_t k = 0; k < 3 * (size_t)S->tri_count; k++)
      if (S->indices[k] < 0 || S->indices[k] >= S->vertex_count) return fail(PRT_ERR_INVALID_ARGUMENT, "mesh skin: index out of range");
    for (size_t k = 0; k < 4 * (size_t)S->vertex_count; k++)
      if ((int32_t)S->joints[k] >= S->joint_count) return fail(PRT_ERR_INVALID_ARGUMENT, "mesh skin: joint out of range");
  }
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  // an earlier prt_skin_mesh's kernels may still read the binding this call replaces or removes
  PRT_TRY(wait_stream(c, "prt_set_mesh_skin"));
  if (c->skin.size() != c->mesh_host.size()) {
    c->skin.clear();
    c->skin.resize(c->mesh_host.size());
  }
  SkinBinding& b = c->skin[mi];
  b.joints = 0;
  b.skinned = false;
  if (!S) {
    b = SkinBinding();
    PRT_FOR_MEMBERS(prt_set_mesh_skin(m, mi, S));
    return PRT_OK;
  }
  const size_t V = (size_t)S->vertex_count, T = (size_t)S->tri_count, J = (size_t)S->joint_count;
  const void* src[5] = {S->positions, S->normals, S->joints, S->weights, S->indices};
  const size_t bytes[5] = {12 * V, 12 * V, 8 * V, 16 * V, 12 * T};
  size_t off[5];
  HIP_TRY(b.in.ensure(packed_layout(bytes, off)));
  HIP_TRY(b.mats.ensure(48 * J));
  HIP_TRY(b.work.ensure(32 * V + 48 * T));
  for (int k = 0; k < 5; k++)
    if (bytes[k]) HIP_TRY(hipMemcpy(b.in.as<char>() + off[k], src[k], bytes[k], hipMemcpyHostToDevice));
  SkinDev& d = b.dev;
  d.positions = reinterpret_cast<const float*>(b.in.as<char>() + off[0]);
  d.normals = reinterpret_cast<const float*>(b.in.as<char>() + off[1]);
  d.joints = reinterpret_cast<const uint2*>(b.in.as<char>() + off[2]);
  d.weights = reinterpret_cast<const float4*>(b.in.as<char>() + off[3]);
  d.indices = reinterpret_cast<const int32_t*>(b.in.as<char>() + off[4]);
  d.matrices = b.mats.as<const float4>();
  d.vpos = b.work.as<float4>();
  d.vnrm = d.vpos + V;
  d.triangles = d.vnrm + V;
  d.vertex_count = S->vertex_count;
  d.tri_count = S->tri_count;
  d.joint_count = S->joint_count;
  b.joints = S->joint_count;
  PRT_FOR_MEMBERS(prt_set_mesh_skin(m, mi, S));
  return PRT_OK;
}

int prt_skin_mesh(prt_ctx* c, int32_t mi, const float* M, int32_t J, uint32_t in_flags) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (in_flags & ~PRT_IN_DEVICE) return fail(PRT_ERR_INVALID_ARGUMENT, "unknown input flags");
  PRT_TRY(mesh_arg(c, mi));
  const bool dev_in = (in_flags & PRT_IN_DEVICE) != 0;
  if (dev_in && c->sh_kind == 2) return fail(PRT_ERR_UNSUPPORTED, "device matrices on a local shard group");
  if (c->skin.size() != c->mesh_host.size() || !c->skin[mi].joints)
    return fail(PRT_ERR_NOT_READY, "no skin bound to the mesh: call prt_set_mesh_skin");
  SkinBinding& b = c->skin[mi];
  if (!M) return fail(PRT_ERR_INVALID_ARGUMENT, "joint_matrices is NULL");
  if (J != b.joints) return fail(PRT_ERR_INVALID_ARGUMENT, "joint_count differs from the binding's");
  if (dev_in && (reinterpret_cast<uintptr_t>(M) & 15u))
    return fail(PRT_ERR_INVALID_ARGUMENT, "device joint matrices must be 16-byte aligned");
  PRT_JOIN(c);  // frames in flight complete first: they read the geometry this call rewrites in place
  HIP_TRY(hipSetDevice(c->device));
  PRT_TRY(refit_scratch(c, false));
  PRT_TRY(refit_levels(c, mi));
  SkinDev d = b.dev;
  if (dev_in) {
    d.matrices = reinterpret_cast<const float4*>(M);
  } else {  // copied into a pinned staging buffer now, uploaded in stream order
    StageSlot* st = nullptr;
    PRT_TRY(stage_acquire(c, 48 * (size_t)J, st));
    std::memcpy(st->p, M, 48 * (size_t)J);
    HIP_TRY(hipMemcpyAsync(b.mats.p, st->p, 48 * (size_t)J, hipMemcpyHostToDevice, c->stream));
    PRT_TRY(stage_release(c, *st, c->stream));
  }
  HIP_TRY(launch_skin_mesh(c->stream, d, c->stri.as<ShadeTri>() + c->mesh_host[mi].prim_base));
  // the refit over the scratch's fat triangles, without the ShadeTri kernel: k_skin_prims wrote those words
  RefitMeshDev r = {};
  r.triangles = reinterpret_cast<const float*>(d.triangles);
  PRT_TRY(refit_mesh(c, mi, r, false, nullptr, nullptr));
  b.skinned = true;
  PRT_FOR_MEMBERS(prt_skin_mesh(m, mi, M, J, in_flags));
  return PRT_OK;
}

int prt_rebuild_mesh(prt_ctx* c, int32_t mi, const prt_mesh* M, uint32_t in_flags, int32_t builder) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (in_flags & ~PRT_IN_DEVICE) return fail(PRT_ERR_INVALID_ARGUMENT, "unknown input flags");
  PRT_TRY(mesh_arg(c, mi));
  if (builder == PRT_BUILDER_HOST_SAH || builder == PRT_BUILDER_HOST_SBVH)
    return fail(PRT_ERR_UNSUPPORTED, "mesh rebuild: the host builders rebuild through prt_set_meshes only");
  if (builder != PRT_BUILDER_GPU_LBVH && builder != PRT_BUILDER_GPU_PLOC)
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad BLAS builder");
  const bool dev_in = M && (in_flags & PRT_IN_DEVICE) != 0;
  if (M) PRT_TRY(update_args(c, mi, M, in_flags, "mesh rebuild"));
  else if (c->skin.size() != c->mesh_host.size() || !c->skin[mi].joints || !c->skin[mi].skinned)
    return fail(PRT_ERR_NOT_READY, "mesh rebuild without arrays: no skin bound to the mesh, or no prt_skin_mesh on it yet");
  PRT_JOIN(c);  // frames in flight complete first: they read the tree this call replaces
  HIP_TRY(hipSetDevice(c->device));
  MeshHost& mh = c->mesh_info[mi];
  size_t most = 0;
  for (const MeshHost& m : c->mesh_info) most = std::max(most, (size_t)m.tris);
  HIP_TRY(c->rb_nodes.ensure(sizeof(Node8) * most));
  HIP_TRY(c->rb_tris.ensure(sizeof(TriMT) * most));
  RefitMeshDev d = {};
  if (M) {
    PRT_TRY(refit_scratch(c, !dev_in));
    PRT_TRY(stage_mesh(c, M, dev_in, d));
  } else {
    d.triangles = reinterpret_cast<const float*>(c->skin[mi].dev.triangles);
  }
  // The build, into the context's scratch: the scene is untouched until it has succeeded.  The builder synchronises
  // the context stream once per tree level; the wait before it is the bounded one of an RCCL context.
  PRT_TRY(wait_stream(c, "prt_rebuild_mesh"));
  GpuBlasInfo gi = {};
  const hipError_t be = gpu_build_blas8(c->stream, d.triangles, mh.tris, max_leaf_tris(), c->rb_nodes.as<Node8>(),
                                        c->rb_tris.as<TriMT>(), &gi, builder == PRT_BUILDER_GPU_PLOC);
  if (be != hipSuccess) return fail(PRT_ERR_HIP, std::string("mesh rebuild: the device build failed: ") + hipGetErrorString(be));
  constexpr int kMaxBlasDepth = 64;  // what the traversal stacks cover (depth_ok, prt_api.cpp)
  if (gi.depth > kMaxBlasDepth) return fail(PRT_ERR_UNSUPPORTED, "mesh rebuild: the new BLAS is deeper than 64 levels");
  if (gi.tris > mh.rec_cap) return fail(PRT_ERR_HIP, "mesh rebuild: more records than the mesh's region holds");
  if ((int64_t)gi.nodes > mh.node_cap) PRT_TRY(grow_nodes(c, mi, gi.nodes));
  // The commit, in the context stream's order: the nodes and records into the mesh's regions, the ShadeTri words of
  // *M by the update's kernel (a skinned mesh's are there already), then the rebase and every primitive's record.
  const MeshDev& md = c->mesh_host[mi];
  Node8* nodes = c->nodes8.as<Node8>() + md.root;
  TriMT* recs = c->tris.as<TriMT>() + mh.rec_base;
  HIP_TRY(hipMemcpyAsync(nodes, c->rb_nodes.p, sizeof(Node8) * (size_t)gi.nodes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(recs, c->rb_tris.p, sizeof(TriMT) * (size_t)gi.tris, hipMemcpyDeviceToDevice, c->stream));
  RefitResult* res = c->rf.res.as<RefitResult>();
  if (M) {
    HIP_TRY(hipMemsetAsync(&res->bad_index, 0, 4, c->stream));
    HIP_TRY(launch_refit_records(c->stream, nullptr, 0, c->stri.as<ShadeTri>() + md.prim_base, d, res));
  }
  HIP_TRY(gpu_blas_finish(c->stream, nodes, gi.nodes, md.root, recs, gi.tris, mh.rec_base, c->stri.as<ShadeTri>(),
                          md.prim_base));
  bool bad = false;
  if (dev_in) {  // the bad-index flag of device arrays: the one host wait after the builder's
    HIP_TRY(hipMemcpyAsync(c->rf.res_host, res, sizeof(RefitResult), hipMemcpyDeviceToHost, c->stream));
    PRT_TRY(wait_stream(c, "reading the rebuilt mesh's index flag"));
    bad = c->rf.res_host->bad_index != 0;
  }
  // everything derived from the tree
  std::memcpy(mh.bmin, gi.bmin, sizeof(mh.bmin));
  std::memcpy(mh.bmax, gi.bmax, sizeof(mh.bmax));
  mh.depth = gi.depth;
  mh.nodes = gi.nodes;
  mh.leaves = gi.leaves;
  mh.recs = gi.tris;
  mh.level_ends.clear();  // the next update or skin reads the new nodes back once (refit_levels)
  int maxd = 0;
  for (const MeshHost& m : c->mesh_info) maxd = std::max(maxd, m.depth);
  if (maxd != c->max_depth) {
    // the stacks and spill columns are sized from max_depth at every launch; the instance BVH's depth cap was
    // computed from it when the instance set was seeded (ensure_instances): the next update seeds again
    c->max_depth = maxd;
    c->tlas_n = -1;
  }
  c->inst_dirty = true;
  c->tlas_dirty = true;
  c->shade_epoch++;
  c->scene_epoch++;
  if (bad) return fail(PRT_ERR_INVALID_ARGUMENT, "mesh rebuild: an index in device memory is out of range (vertex 0 was read in its place)");
  PRT_FOR_MEMBERS(prt_rebuild_mesh(m, mi, M, in_flags, builder));
  return PRT_OK;
}

int prt_blas_cost(prt_ctx* c, int32_t mi, double* cost) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!cost) return fail(PRT_ERR_INVALID_ARGUMENT, "cost is NULL");
  PRT_TRY(mesh_arg(c, mi));
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  const MeshHost& mh = c->mesh_info[mi];
  // the partials of the largest tree the node array can hold, the root area and the result: one allocation
  const size_t slots = (size_t)blas_cost_blocks(c->nodes_len) + 2;
  if (c->cost_part.bytes < 8 * slots) {
    PRT_TRY(wait_stream(c, "prt_blas_cost"));  // (an earlier call's kernels were waited for; a larger node array)
    HIP_TRY(c->cost_part.ensure(8 * slots));
  }
  double* part = c->cost_part.as<double>();
  double* out = part + (slots - 1);
  HIP_TRY(launch_blas_cost(c->stream, c->nodes8.as<Node8>() + c->mesh_host[mi].root, (uint32_t)mh.nodes, part, out));
  double v = 0.0;
  HIP_TRY(hipMemcpyAsync(&v, out, 8, hipMemcpyDeviceToHost, c->stream));
  PRT_TRY(wait_stream(c, "prt_blas_cost"));
  *cost = v;
  return PRT_OK;
}

int prt_read_blas(prt_ctx* c, int32_t mi, void* nodes, uint64_t bytes, uint64_t* needed) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_TRY(mesh_arg(c, mi));
  const MeshHost& mh = c->mesh_info[mi];
  const uint32_t root = c->mesh_host[mi].root;
  PRT_TRY(read_back(c, "prt_read_blas", c->nodes8.as<Node8>() + root, (uint64_t)mh.nodes * sizeof(Node8), nodes, bytes, needed));
  if (!nodes) return PRT_OK;
  Node8* nd = static_cast<Node8*>(nodes);  // offsets relative to the mesh, as the builders return them
  for (int64_t j = 0; j < mh.nodes; j++) {
    Node8 x;
    std::memcpy(&x, nd + j, sizeof(x));
    x.child_base -= root;
    x.tri_base -= mh.rec_base;
    std::memcpy(nd + j, &x, sizeof(x));
  }
  return PRT_OK;
}

int prt_read_blas_tris(prt_ctx* c, int32_t mi, void* tris, uint64_t bytes, uint64_t* needed) {
  if (!c) return fail(PRT_ERR_INVALID_ARGUMENT, "ctx is NULL");
  PRT_TRY(mesh_arg(c, mi));
  const MeshHost& mh = c->mesh_info[mi];
  // (prim is mesh-local in the device array too: nothing to make relative)
  return read_back(c, "prt_read_blas_tris", c->tris.as<TriMT>() + mh.rec_base, (uint64_t)mh.recs * sizeof(TriMT), tris, bytes, needed);
}

int prt_set_bvh_builder(prt_ctx* c, int32_t builder) {
  if (!c || builder < PRT_BUILDER_HOST_SAH || builder > PRT_BUILDER_GPU_PLOC)
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad BLAS builder");
  c->builder = builder;
  c->shade_epoch++;
  c->scene_epoch++;  // (the BLASes change at the next prt_set_meshes, which bumps it again)
  PRT_FOR_MEMBERS(prt_set_bvh_builder(m, builder));
  return PRT_OK;
}

}  // extern "C"
