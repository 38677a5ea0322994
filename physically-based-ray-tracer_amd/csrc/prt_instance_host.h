// prt_instance_host.h -- what the instance entry points (prt_api_instance.cpp) decide without a device: which kind of
// refresh a call is, the stack depth a new instance BVH is given, the byte sizes of the staging slot and of the
// device buffers, the refit input of every instance and the table a device-side refill reads.  Plain C++ with no HIP
// include: the host code and tests/cpp/instance_host_check.cpp compile the same text.  prt_scene.h needs HIP, so
// InstSrc and the mesh boxes are template arguments, the records' sizes stand here as numbers (prt_api_instance.cpp
// asserts them against the structs) and kLinearInstances is passed in (`linear`).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "bvh_build.h"

namespace prt::host {

// The traversal stacks hold one group per tree level below the root: 8-18 in LDS (by occupancy; 16 in the query
// kernels), deeper levels in HBM spill columns (ensure_spill), up to tinybvh's 64-entry stack (tiny_bvh.h:6315)
constexpr int kMaxBvhDepth = 64;

// waves/SIMD of the persistent traversal kernels: the LDS stack (9 / 11 / 14 / 18 groups at 7 / 6 / 5 / 4
// waves) must hold max_depth - 1 groups; deeper BVHs (depth_ok caps them at kMaxBvhDepth = 64 levels) run the
// 4-wave form with HBM spill columns (ensure_spill)
inline int occ_at(int d) {  // the occupancy a stack of d levels allows (7 waves: re-measured best, profiles/r05_occupancy.txt)
  if (d <= 10) return 7;
  if (d <= 12) return 6;
  if (d <= 15) return 5;
  return 4;
}

// The levels the stacks are sized for when a new instance set's first tree has tree_depth levels over BLASes of
// max_depth: the largest depth that keeps the traversal's occupancy (at most four levels of room, never past
// kMaxBvhDepth), and at least the median-split tree's.  It is the cap of the worker's later builds.
inline int tlas_depth_cap(int max_depth, int tree_depth, int32_t n) {
  const int occ = occ_at(max_depth + tree_depth);
  int cap = std::max(tree_depth, tlas8_median_depth(n));
  while (cap < tree_depth + 4 && occ_at(max_depth + cap + 1) == occ && max_depth + cap + 1 <= kMaxBvhDepth) cap++;
  return cap;
}

// What a refresh of the instance records from host transforms is.  use_tlas: the rays walk an instance BVH (more than
// `linear` instances, or forced: PRT_TLAS=1).  tree_work: a tree is built -- not for a materials-only update, which
// moves no box (tlas_dirty clear, the same count over a live tree).  async: on the worker thread, when the live tree
// is over the same count; else the instance set is new and its first tree is built on the calling thread.
struct InstRefresh { bool use_tlas, tree_work, async; };
inline InstRefresh plan_instance_refresh(int32_t n, int32_t linear, bool force_tlas, bool had_tlas, int32_t tlas_n,
                                         bool tlas_dirty, bool has_worker) {
  InstRefresh p;
  p.use_tlas = n > linear || force_tlas;
  p.tree_work = p.use_tlas && (tlas_dirty || !had_tlas || tlas_n != n);
  p.async = p.tree_work && had_tlas && tlas_n == n && has_worker;
  return p;
}

// record sizes: InstSrc, InstDev, a Node8's eight instance-slot words
constexpr size_t kInstSrcBytes = 96, kInstDevBytes = 160, kSlotBytes = 32;
inline size_t inst_cap(int32_t n, int32_t linear) { return (size_t)std::max(n, linear); }  // at least the list's size
inline size_t tlas_node_cap(int32_t n) { return (size_t)std::max(n, 1); }  // a tree over n instances has no more nodes

// The pinned staging slot of a refresh: the instance sources, then the tree's nodes and slot words.  The worker writes
// a tree of unknown size, so an async update moves the cap; a first build moves its tree's tree_nodes; `per` is what
// every slot of the pool is sized for, the largest an update of this instance set takes.
struct InstStageBytes { size_t src, nodes, slot, per; };
inline InstStageBytes inst_stage_bytes(int32_t n, const InstRefresh& p, size_t tree_nodes) {
  const size_t moved = !p.tree_work ? 0 : p.async ? tlas_node_cap(n) : tree_nodes;
  const size_t src = kInstSrcBytes * (size_t)n;
  return {src, moved * sizeof(Node8), moved * kSlotBytes, src + (p.use_tlas ? tlas_node_cap(n) * (sizeof(Node8) + kSlotBytes) : 0)};
}

// prt_ctx::inst_tab: n mesh ids, n kinds, then two float4 per mesh, each part 16-byte aligned
struct InstTabLayout { size_t kind, box, total; };
inline InstTabLayout inst_tab_layout(size_t n, size_t nmesh) {
  const size_t w = (4 * n + 15) & ~size_t(15);
  return {w, 2 * w, 2 * w + 32 * nmesh};
}

// The device buffers of an instance state of n instances: of every copy of the ring (records, their refit input, the
// tree's nodes and slot words) and of the context (the refill table; the level order and box scratch of a device
// refit).  The tree's are zero without one.
struct InstBufBytes { size_t inst, inst_src, tlas8, tlas_slot, inst_tab, tlas_order, tlas_box; };
inline InstBufBytes inst_buffer_bytes(int32_t n, int32_t linear, size_t nmesh, bool use_tlas) {
  const size_t cap = inst_cap(n, linear), nodes = use_tlas ? tlas_node_cap(n) : 0;
  return {kInstDevBytes * cap, kInstSrcBytes * cap, nodes * sizeof(Node8), nodes * kSlotBytes,
          inst_tab_layout(cap, nmesh).total, 4 * nodes, 24 * nodes};
}

// The refit input of n instances (prt_refit.h InstSrc) from host transforms xf (16 floats each), the mesh ids, the
// kinds (nkind of them: n, or none = textured) and the meshes' root boxes (any type with bmin[3] / bmax[3]).  Every
// mesh id is in range (the caller checked).
template <class InstSrcT, class MeshBox>
void fill_inst_src(int32_t n, const uint32_t* mesh, const uint32_t* kind, size_t nkind, const MeshBox* mesh_box,
                   const float* xf, InstSrcT* src) {
  static_assert(sizeof(InstSrcT) == kInstSrcBytes, "InstSrc is 96 bytes");
  for (int32_t i = 0; i < n; i++) {
    InstSrcT& s = src[i];
    const uint32_t m = mesh[i];
    std::memcpy(s.T, xf + 16 * (size_t)i, sizeof(s.T));
    std::memcpy(s.bmin, mesh_box[m].bmin, sizeof(s.bmin));
    std::memcpy(s.bmax, mesh_box[m].bmax, sizeof(s.bmax));
    s.mesh = m;
    s.kind = (size_t)i < nkind ? kind[i] : 0u;
  }
}

// The table of a device-side refill (k_inst_src) in L's layout, L.total bytes at tab: what fill_inst_src reads besides
// the transforms, so that the refill writes the InstSrc the host would have.  Unused bytes are zero.
template <class MeshBox>
void fill_inst_tab(int32_t n, const uint32_t* mesh, const uint32_t* kind, size_t nkind, const MeshBox* mesh_box,
                   size_t nmesh, const InstTabLayout& L, char* tab) {
  std::memset(tab, 0, L.total);
  std::memcpy(tab, mesh, 4 * (size_t)n);
  if (nkind) std::memcpy(tab + L.kind, kind, 4 * std::min((size_t)n, nkind));
  for (size_t m = 0; m < nmesh; m++) {
    std::memcpy(tab + L.box + 32 * m, mesh_box[m].bmin, 12);
    std::memcpy(tab + L.box + 32 * m + 16, mesh_box[m].bmax, 12);
  }
}

}  // namespace prt::host
