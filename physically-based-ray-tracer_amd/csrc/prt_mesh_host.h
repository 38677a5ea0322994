// prt_mesh_host.h -- what the mesh entry points (prt_api_mesh.cpp) decide without a device: the checks on a caller's
// arrays, a primitive's ShadeTri, the 256-byte-aligned layout of arrays packed into one buffer, the tree levels of a
// refit.  Plain C++ with no HIP include: the host code and tests/cpp/mesh_host_check.cpp compile the same text.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prt.h"
#include "prt_blas_refit.h"

namespace prt::host {

// What prt_set_meshes requires of one mesh, in the order it is checked (empty: the mesh passes).  prt_update_mesh
// asks for kMeshArrays and, for host arrays, kMeshIndices: the rules it shares.  who: "mesh 3" / "mesh update".
// tex: the context's textures (their w and h are read), for kMeshTextures.
enum : unsigned { kMeshCounts = 1, kMeshArrays = 2, kMeshTextures = 4, kMeshIndices = 8, kMeshAll = 15 };
template <class Tex>
std::string check_mesh_arrays(const prt_mesh& M, unsigned what, const std::string& who, const Tex* tex, int32_t ntex) {
  if (((what & kMeshCounts) && (M.tri_count <= 0 || M.vertex_count <= 0)) ||
      ((what & kMeshArrays) &&
       (!M.triangles || !M.fixed_normals || !M.fixed_uvs || !M.indices || !M.vertices || !M.face_normals)))
    return who + ": missing arrays";
  if (what & kMeshTextures) {
    if (M.albedo_tex < 0 || M.albedo_tex >= ntex) return who + ": albedo texture required (Scene.cpp:160)";
    const int32_t tx[4] = {M.albedo_tex, M.normal_tex, M.metalness_tex, M.emission_tex};
    const Tex& A = tex[M.albedo_tex];
    for (int k = 1; k < 4; k++) {
      if (tx[k] >= ntex) return "texture id out of range";
      // every map is read at the flat texel iu + iv * albedo width, iu and iv taken with the albedo dimensions
      // (Scene.cpp:79-85,160-165): the map needs that many texels, whatever its own width (a narrower, taller map
      // renders in the reference and must here)
      if (tx[k] >= 0 && tex[tx[k]].w * (int64_t)tex[tx[k]].h < (int64_t)A.w * A.h)
        return "texture smaller than the albedo map (indexed with albedo dims)";
    }
  }
  if (what & kMeshIndices)
    for (int64_t k = 0; k < 3 * (int64_t)M.tri_count; k++)
      if (M.indices[k] < 0 || M.indices[k] >= M.vertex_count) return "index out of range";
  return std::string();
}

// Primitive p's ShadeTri (prt_scene.h; a template so that this file needs no HIP header) from a mesh's host arrays:
// words 0..26 in refit_shade_word's order, where the layout stands once, the five pad words zero (prt_set_meshes
// sets pad[0]).  The indices are in range (check_mesh_arrays).
template <class ShadeTriT>
void fill_shade_tri(ShadeTriT& st, size_t p, const prt_mesh& M) {
  static_assert(sizeof(ShadeTriT) == 128, "ShadeTri is 32 words");
  float w[27];
  uint32_t bad = 0;
  for (int k = 0; k < 27; k++)
    w[k] = refit_shade_word(k, p, M.fixed_normals, M.fixed_uvs, M.indices, M.vertices, M.face_normals, M.vertex_count, &bad);
  std::memset(&st, 0, sizeof(st));
  std::memcpy(&st, w, sizeof(w));
}

// Arrays back to back in one buffer, each part 256-byte aligned: part k's offset into off[k]; returns the total.
template <size_t N>
size_t packed_layout(const size_t (&bytes)[N], size_t (&off)[N]) {
  size_t at = 0;
  for (size_t k = 0; k < N; k++) {
    off[k] = at;
    at += (bytes[k] + 255) & ~size_t(255);
  }
  return at;
}

// The tree levels of one mesh's BLAS as it lies in the scene's arrays: nodes[0 .. n) are Node8[root .. root + n),
// its records TriMT[rec_base .. rec_base + recs).  Every link is checked (an interior child after its parent and
// inside the mesh's nodes, a leaf slot's records inside the mesh's records).  order: the node indices (root + j)
// sorted by level, parents' order kept; level d's nodes are order[level_ends[d - 1] .. level_ends[d]).  A refit
// runs the levels last to first, so that every child's box is written before its parent reads it.  false: a link
// is wrong, *err says which, the outputs are untouched.
inline bool tree_levels(const Node8* nodes, size_t n, uint32_t root, uint32_t rec_base, uint32_t recs,
                        std::vector<uint32_t>& level_ends, std::vector<uint32_t>& order, const char** err) {
  auto refuse = [err](const char* why) { return *err = why, false; };
  std::vector<uint32_t> level(n, 0);
  uint32_t depth = 1;
  for (size_t j = 0; j < n; j++) {
    uint32_t child = nodes[j].child_base;
    for (int s = 0; s < 8; s++) {
      if ((nodes[j].imask >> s) & 1u) {
        const uint64_t l = (uint64_t)child++ - root;
        if (child <= root || l <= j || l >= n) return refuse("BLAS refit: an interior child is not below its parent");
        level[l] = level[j] + 1;
        depth = level[l] + 1 > depth ? level[l] + 1 : depth;
      } else if (nodes[j].meta[s]) {
        const uint64_t first = (uint64_t)nodes[j].tri_base + (nodes[j].meta[s] >> 3), cnt = nodes[j].meta[s] & 7u;
        if (first < rec_base || first + cnt > (uint64_t)rec_base + recs)
          return refuse("BLAS refit: a leaf slot's records lie outside the mesh");
      }
    }
  }
  std::vector<uint32_t> ends(depth, 0), ord(n), next(depth);
  for (size_t j = 0; j < n; j++) ends[level[j]]++;
  uint32_t at = 0;
  for (uint32_t d = 0; d < depth; d++) {
    next[d] = at;
    at += ends[d];
    ends[d] = at;
  }
  for (size_t j = 0; j < n; j++) ord[next[level[j]]++] = root + (uint32_t)j;
  level_ends = std::move(ends);
  order = std::move(ord);
  return true;
}

}  // namespace prt::host
