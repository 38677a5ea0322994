// tlas_build_check -- the per-instance and per-node code of prt_rebuild_instances (csrc/prt_tlas_build.h, what
// k_tlas_prims and k_tlas_finish run) on the CPU, around the host collapse build_blas8 (bvh_build.cpp), which emits
// the device builder's output format.
//   fat   <boxes.bin>       tlas_fat_record of every box: min / max over the three vertices (the builders' fminf /
//                           fmaxf and the host's `<` form) equal the box bit for bit; the third vertex lies in [lo, hi]
//   build <boxes.bin>       tlas_finish_node8 applied to build_blas8(fat, n, 1): the tree has build_tlas8's form (every
//                           instance in exactly one leaf slot with count 1, tri_base = 8j, 0xFFFFFFFF in every other
//                           slot word, interior children consecutive from child_base, in range and after their parent),
//                           and refit_tlas8 (prt_tlas_refit.h) over the same boxes reproduces its bytes
//   tree  <nodes.bin> <slots.bin> <src.bin>              (only with TLAS_CHECK_INSTANCES, which needs the HIP headers for
//                           prt_refit.h) a tree read back from a context: the same form, each level's nodes contiguous as
//                           well, and the refit over refit_instance() of the InstSrc records reproduces its bytes
//   refit <nodes.bin> <slots.bin> <src.bin> <nodes.out>  (likewise) that tree refitted over refit_instance() of other
//                           records, written as raw Node8 bytes
// boxes.bin: float32 {lo[3], hi[3]} per instance.  Prints one JSON line; exit status 0 = ok.  Build with
// -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh_build.h"
#include "prt_tlas_build.h"
#include "prt_tlas_refit.h"
#ifdef TLAS_CHECK_INSTANCES
#include "prt_refit.h"
#endif

using namespace prt;

struct BoxInst { float bmin[3], bmax[3]; };

template <class R>
static bool read_records(const char* path, std::vector<R>& v) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  bool ok = bytes >= 0 && bytes % (long)sizeof(R) == 0;
  if (ok) {
    v.resize((size_t)bytes / sizeof(R));
    ok = v.empty() || std::fread(v.data(), sizeof(R), v.size(), f) == v.size();
  }
  std::fclose(f);
  return ok;
}

static int fail(const char* what, long at = -1) {
  std::printf("{\"ok\": false, \"what\": \"%s\", \"at\": %ld}\n", what, at);
  return 1;
}

static bool same_bits(float a, float b) { return !std::memcmp(&a, &b, 4); }

static int fat(const std::vector<BoxInst>& b) {
  for (size_t i = 0; i < b.size(); i++) {
    float t[12];
    tlas_fat_record(b[i].bmin, b[i].bmax, t);
    for (int k = 0; k < 3; k++) {
      const float v[3] = {t[k], t[4 + k], t[8 + k]};
      // the device builder's bounds (k_boxes / k_ploc_leaves) and the host's (Box::grow)
      const float lo = std::fmin(std::fmin(v[0], v[1]), v[2]), hi = std::fmax(std::fmax(v[0], v[1]), v[2]);
      float glo = 1e30f, ghi = -1e30f;
      for (int j = 0; j < 3; j++) { glo = v[j] < glo ? v[j] : glo; ghi = v[j] > ghi ? v[j] : ghi; }
      if (!same_bits(lo, b[i].bmin[k]) || !same_bits(hi, b[i].bmax[k])) return fail("fminf / fmaxf over the vertices is not the box", (long)i);
      if (!same_bits(glo, b[i].bmin[k]) || !same_bits(ghi, b[i].bmax[k])) return fail("the grown bounds are not the box", (long)i);
      if (!(v[2] >= b[i].bmin[k] && v[2] <= b[i].bmax[k])) return fail("the third vertex leaves the box", (long)i);
    }
    if (t[3] != 0.0f || t[7] != 0.0f || t[11] != 0.0f) return fail("a w word is not 0", (long)i);
  }
  std::printf("{\"ok\": true, \"boxes\": %zu}\n", b.size());
  return 0;
}

// build_tlas8's form ("Tree shape", include/prt.h prt_rebuild_instances).  levels: each level's nodes are contiguous
// too (the device builder's order); ends gets the level ends
static const char* shape(const std::vector<Node8>& nodes, const std::vector<uint32_t>& slot, size_t n, bool levels,
                         std::vector<uint32_t>& ends) {
  if (nodes.empty() || slot.size() != 8 * nodes.size()) return "slot table size";
  std::vector<int> seen(n, 0), level(nodes.size(), -1), parents(nodes.size(), 0);
  level[0] = 0;
  for (size_t j = 0; j < nodes.size(); j++) {
    const Node8& nd = nodes[j];
    if (level[j] < 0) return "a node has no parent before it";
    if (nd.tri_base != 8 * j) return "tri_base is not 8 * node";
    uint32_t child = nd.child_base;
    for (int s = 0; s < 8; s++) {
      if ((nd.imask >> s) & 1u) {
        if (nd.meta[s]) return "an interior slot has a count";
        if (child <= j || child >= nodes.size()) return "an interior child is not after its parent";
        if (parents[child]++) return "a node has two parents";
        level[child] = level[j] + 1;
        child++;
        if (slot[8 * j + s] != 0xFFFFFFFFu) return "an interior slot names an instance";
      } else if (nd.meta[s]) {
        if ((nd.meta[s] & 7u) != 1u) return "a leaf slot's count is not 1";
        const uint32_t id = slot[8 * j + s];
        if (id >= n) return "a leaf slot's instance is out of range";
        seen[id]++;
      } else if (slot[8 * j + s] != 0xFFFFFFFFu) {
        return "an empty slot names an instance";
      }
    }
  }
  for (size_t i = 0; i < n; i++)
    if (seen[i] != 1) return "an instance is not in exactly one leaf slot";
  for (size_t j = 1; j < nodes.size(); j++)
    if (parents[j] != 1) return "a node is not the child of exactly one slot";
  ends.clear();
  if (levels) {
    for (size_t j = 1; j < nodes.size(); j++) {
      if (level[j] < level[j - 1] || level[j] > level[j - 1] + 1) return "a level's nodes are not contiguous";
      if (level[j] != level[j - 1]) ends.push_back((uint32_t)j);
    }
    ends.push_back((uint32_t)nodes.size());
  }
  return nullptr;
}

template <class Inst>
static const char* refit_identity(const std::vector<Node8>& nodes, const std::vector<uint32_t>& slot,
                                  const std::vector<Inst>& inst, long* at) {
  std::vector<Node8> t = nodes;
  std::vector<float> boxes(6 * t.size());
  refit_tlas8(t.data(), t.size(), slot.data(), inst.data(), (uint32_t)inst.size(), boxes.data());
  for (size_t j = 0; j < t.size(); j++)
    if (std::memcmp(&t[j], &nodes[j], sizeof(Node8))) {
      *at = (long)j;
      return "the refit over the same boxes changed a node";
    }
  return nullptr;
}

static int build(const std::vector<BoxInst>& b) {
  const size_t n = b.size();
  std::vector<float> tri(12 * n);
  for (size_t i = 0; i < n; i++) tlas_fat_record(b[i].bmin, b[i].bmax, &tri[12 * i]);
  BuiltBlas8 w = build_blas8(tri.data(), (int32_t)n, 1);
  if (w.tris.size() != n) return fail("the collapse did not emit one record per instance");
  for (int k = 0; k < 3; k++) {
    float lo = 1e30f, hi = -1e30f;
    for (size_t i = 0; i < n; i++) { lo = b[i].bmin[k] < lo ? b[i].bmin[k] : lo; hi = b[i].bmax[k] > hi ? b[i].bmax[k] : hi; }
    if (!same_bits(lo, w.bmin[k]) || !same_bits(hi, w.bmax[k])) return fail("the root bounds are not the union of the boxes");
  }
  std::vector<uint32_t> slot(8 * w.nodes.size(), 0u);
  for (size_t j = 0; j < w.nodes.size(); j++) {
    Node8 nd = w.nodes[j];
    for (int s = 0; s < 8; s++)
      if (!((nd.imask >> s) & 1u) && nd.meta[s] && nd.meta[s] != (uint8_t)(((nd.meta[s] >> 3) << 3) | 1u))
        return fail("a leaf slot's meta is not (offset << 3) | 1", (long)j);
    tlas_finish_node8(nd, (uint32_t)j, w.tris.data(), (uint32_t)w.tris.size(), (uint32_t)n, &slot[8 * j]);
    w.nodes[j] = nd;
  }
  std::vector<uint32_t> ends;
  if (const char* why = shape(w.nodes, slot, n, false, ends)) return fail(why);
  long at = -1;
  if (const char* why = refit_identity(w.nodes, slot, b, &at)) return fail(why, at);
  std::printf("{\"ok\": true, \"nodes\": %zu, \"depth\": %d, \"instances\": %zu}\n", w.nodes.size(), w.depth, n);
  return 0;
}

#ifdef TLAS_CHECK_INSTANCES
static int tree(const char* nodes_path, const char* slots_path, const char* src_path, const char* out_path) {
  std::vector<Node8> nodes;
  std::vector<uint32_t> slot;
  std::vector<InstSrc> src;
  if (!read_records(nodes_path, nodes) || !read_records(slots_path, slot) || !read_records(src_path, src) ||
      nodes.empty() || src.empty())
    return fail("cannot read the tree or the instances");
  std::vector<uint32_t> ends;
  if (const char* why = shape(nodes, slot, src.size(), true, ends)) return fail(why);
  std::vector<InstDev> inst(src.size());
  for (size_t i = 0; i < src.size(); i++) refit_instance(src[i], inst[i]);
  if (!out_path) {
    long at = -1;
    if (const char* why = refit_identity(nodes, slot, inst, &at)) return fail(why, at);
  } else {
    std::vector<float> boxes(6 * nodes.size());
    refit_tlas8(nodes.data(), nodes.size(), slot.data(), inst.data(), (uint32_t)inst.size(), boxes.data());
    FILE* f = std::fopen(out_path, "wb");
    if (!f) return fail("cannot write the nodes");
    const bool ok = std::fwrite(nodes.data(), sizeof(Node8), nodes.size(), f) == nodes.size();
    if (std::fclose(f) != 0 || !ok) return fail("cannot write the nodes");
  }
  std::printf("{\"ok\": true, \"nodes\": %zu, \"instances\": %zu, \"depth\": %zu, \"level_ends\": [", nodes.size(), src.size(),
              ends.size());
  for (size_t d = 0; d < ends.size(); d++) std::printf("%s%u", d ? ", " : "", ends[d]);
  std::printf("]}\n");
  return 0;
}
#endif

int main(int argc, char** argv) {
#ifdef TLAS_CHECK_INSTANCES
  if (argc == 5 && !std::strcmp(argv[1], "tree")) return tree(argv[2], argv[3], argv[4], nullptr);
  if (argc == 6 && !std::strcmp(argv[1], "refit")) return tree(argv[2], argv[3], argv[4], argv[5]);
#endif
  std::vector<BoxInst> b;
  if (argc != 3 || !read_records(argv[2], b) || b.empty()) return fail("usage: tlas_build_check <fat|build> <boxes.bin>");
  if (!std::strcmp(argv[1], "fat")) return fat(b);
  if (!std::strcmp(argv[1], "build")) return build(b);
  return fail("unknown mode");
}
