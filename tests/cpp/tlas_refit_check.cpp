// tlas_refit_check -- refit_tlas8() of csrc/prt_tlas_refit.h (the per-node code k_tlas_refit_level runs) on the CPU,
// against build_tlas8 (bvh_build.cpp).
//   identity  <b0.bin> <max_depth>           a refit over the builder's own boxes reproduces its nodes byte for byte
//   thereback <b0.bin> <max_depth> <b1.bin>  refit to B1 (something moves), then back to B0: the original bytes
//   contain   <b0.bin> <max_depth> <b1.bin>  after the refit to B1: every instance box inside the decoded box of its
//                                            slot, every slot box of a child (as the refit defines it) inside the
//                                            parent's decoded box for that child, the root's box the exact union, the
//                                            topology untouched
//   nan       <b0.bin> <max_depth> <index> <coord 0..5>
//                                            one coordinate of one box NaN: every node's box is the union that skips
//                                            it, the encoding stays finite, every other instance stays contained
//   cost      <nodes.bin>                    the SAH measure (prt_blas_cost.h, the per-node code of prt_tlas_cost's
//                                            kernels) of a tree given as raw Node8 bytes, its terms added in node order
//                                            (blas_cost8, what cost_check prints) and in the kernels' order
//   refit     <nodes.bin> <slots.bin> <src.bin> <nodes.out>      (only with TLAS_CHECK_INSTANCES, which needs the HIP
//                                            headers for prt_refit.h) the tree read back from a context refitted over
//                                            refit_instance() of the InstSrc records, written as raw Node8 bytes
// b*.bin: float32 {lo[3], hi[3]} per instance.  max_depth 0: the SAH tree; > 0: build_tlas8's cap (the median-split
// tree when the SAH tree is deeper).  Prints one JSON line; exit status 0 = ok.  Build with -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh_build.h"
#include "prt_blas_cost.h"
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

static bool same_bytes(const std::vector<Node8>& a, const std::vector<Node8>& b) {
  return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(Node8));
}

static BuiltTlas8 build(const std::vector<BoxInst>& b, int max_depth) {
  return build_tlas8(reinterpret_cast<const float*>(b.data()), (int32_t)b.size(), max_depth);
}
static std::vector<float> refit(BuiltTlas8& t, const std::vector<BoxInst>& b) {
  std::vector<float> boxes(6 * t.nodes.size());
  refit_tlas8(t.nodes.data(), t.nodes.size(), t.slot.data(), b.data(), (uint32_t)b.size(), boxes.data());
  return boxes;
}

// what the issue's scratch run found of build_tlas8's trees, which the refit relies on
static const char* shape(const BuiltTlas8& t, size_t n) {
  if (t.slot.size() != 8 * t.nodes.size()) return "slot table size";
  std::vector<int> seen(n, 0);
  for (size_t j = 0; j < t.nodes.size(); j++) {
    const Node8& nd = t.nodes[j];
    if (nd.tri_base != 8 * j) return "tri_base is not 8 * node";
    uint32_t child = nd.child_base;
    for (int s = 0; s < 8; s++) {
      if ((nd.imask >> s) & 1u) {
        if (child <= j || child >= t.nodes.size()) return "an interior child is not after its parent";
        child++;
        if (t.slot[8 * j + s] != 0xFFFFFFFFu) return "an interior slot names an instance";
      } else if (nd.meta[s]) {
        if ((nd.meta[s] & 7u) != 1u) return "a leaf slot's count is not 1";
        const uint32_t id = t.slot[8 * j + s];
        if (id >= n) return "a leaf slot's instance is out of range";
        seen[id]++;
      } else if (t.slot[8 * j + s] != 0xFFFFFFFFu) {
        return "an empty slot names an instance";
      }
    }
  }
  for (size_t i = 0; i < n; i++)
    if (seen[i] != 1) return "an instance is not in exactly one leaf slot";
  return nullptr;
}

static void decode(const Node8& nd, int s, double lo[3], double hi[3]) {
  const double o[3] = {nd.px, nd.py, nd.pz};
  const double sc[3] = {std::ldexp(1.0, (int)nd.ex - 127), std::ldexp(1.0, (int)nd.ey - 127), std::ldexp(1.0, (int)nd.ez - 127)};
  const double ql[3] = {(double)nd.qlox[s], (double)nd.qloy[s], (double)nd.qloz[s]};
  const double qh[3] = {(double)nd.qhix[s], (double)nd.qhiy[s], (double)nd.qhiz[s]};
  for (int k = 0; k < 3; k++) { lo[k] = o[k] + ql[k] * sc[k]; hi[k] = o[k] + qh[k] * sc[k]; }
}

// Every instance box (but `skip`) inside its slot's decoded box; every occupied slot's box of a child node, as the
// refit defines it (a leaf slot: its instance's box; an interior slot: the grandchild's scratch box), inside the
// parent's decoded box for that child.  Their decoded forms need not nest: a child's grid rounds outward by up to one
// of its own steps.  contained: the boxes checked
static const char* containment(const BuiltTlas8& t, const std::vector<BoxInst>& b, const std::vector<float>& boxes,
                               long skip, long* contained, long* at) {
  *contained = 0;
  for (size_t j = 0; j < t.nodes.size(); j++) {
    const Node8& nd = t.nodes[j];
    uint32_t child = nd.child_base;
    for (int s = 0; s < 8; s++) {
      double lo[3], hi[3];
      decode(nd, s, lo, hi);
      *at = (long)(8 * j + s);
      if ((nd.imask >> s) & 1u) {
        const size_t cj = child++;
        const Node8& c = t.nodes[cj];
        uint32_t grand = c.child_base;
        for (int cs = 0; cs < 8; cs++) {
          const float *clo, *chi;
          if ((c.imask >> cs) & 1u) {
            clo = &boxes[6 * (size_t)grand];
            chi = clo + 3;
            grand++;
          } else if (c.meta[cs]) {
            const uint32_t id = t.slot[8 * cj + cs];
            if ((long)id == skip) continue;
            clo = b[id].bmin;
            chi = b[id].bmax;
          } else {
            continue;
          }
          for (int k = 0; k < 3; k++)
            if (!((double)clo[k] >= lo[k] && (double)chi[k] <= hi[k])) return "a child's slot box leaves the parent's box for the child";
          (*contained)++;
        }
      } else if (nd.meta[s]) {
        const uint32_t id = t.slot[8 * j + s];
        if ((long)id == skip) continue;
        for (int k = 0; k < 3; k++)
          if (!((double)b[id].bmin[k] >= lo[k] && (double)b[id].bmax[k] <= hi[k])) return "an instance box leaves its slot's box";
        (*contained)++;
      }
    }
  }
  return nullptr;
}

static bool topology_kept(const BuiltTlas8& a, const BuiltTlas8& b) {
  if (a.nodes.size() != b.nodes.size() || a.slot != b.slot) return false;
  for (size_t j = 0; j < a.nodes.size(); j++) {
    const Node8 &x = a.nodes[j], &y = b.nodes[j];
    if (x.imask != y.imask || x.child_base != y.child_base || x.tri_base != y.tri_base || std::memcmp(x.meta, y.meta, 8))
      return false;
  }
  return true;
}

static int identity(const std::vector<BoxInst>& b0, int max_depth) {
  const BuiltTlas8 built = build(b0, max_depth);
  if (const char* why = shape(built, b0.size())) return fail(why);
  BuiltTlas8 t = built;
  refit(t, b0);
  if (!same_bytes(t.nodes, built.nodes)) return fail("the refit over the builder's boxes changed the nodes");
  std::printf("{\"ok\": true, \"nodes\": %zu, \"depth\": %d, \"median\": %s}\n", built.nodes.size(), built.depth,
              built.median ? "true" : "false");
  return 0;
}

static int thereback(const std::vector<BoxInst>& b0, int max_depth, const std::vector<BoxInst>& b1) {
  const BuiltTlas8 built = build(b0, max_depth);
  BuiltTlas8 t = built;
  refit(t, b1);
  const bool moved = !same_bytes(t.nodes, built.nodes);
  if (!topology_kept(t, built)) return fail("the refit changed the topology");
  refit(t, b0);
  if (!same_bytes(t.nodes, built.nodes)) return fail("refitting back did not restore the built bytes");
  std::printf("{\"ok\": true, \"nodes\": %zu, \"moved\": %s}\n", built.nodes.size(), moved ? "true" : "false");
  return 0;
}

static int contain(const std::vector<BoxInst>& b0, int max_depth, const std::vector<BoxInst>& b1) {
  const BuiltTlas8 built = build(b0, max_depth);
  BuiltTlas8 t = built;
  const std::vector<float> boxes = refit(t, b1);
  if (!topology_kept(t, built)) return fail("the refit changed the topology");
  long contained = 0, at = -1;
  if (const char* why = containment(t, b1, boxes, -1, &contained, &at)) return fail(why, at);
  std::printf("{\"ok\": true, \"nodes\": %zu, \"contained\": %ld, \"bmin\": [%.9g, %.9g, %.9g], \"bmax\": [%.9g, %.9g, %.9g]}\n",
              t.nodes.size(), contained, boxes[0], boxes[1], boxes[2], boxes[3], boxes[4], boxes[5]);
  return 0;
}

// the union of the boxes below node j that skips NaN coordinates, by a recursion of its own
static void union_below(const BuiltTlas8& t, const std::vector<BoxInst>& b, size_t j, float lo[3], float hi[3]) {
  for (int k = 0; k < 3; k++) { lo[k] = 1e30f; hi[k] = -1e30f; }
  const Node8& nd = t.nodes[j];
  uint32_t child = nd.child_base;
  for (int s = 0; s < 8; s++) {
    float clo[3], chi[3];
    if ((nd.imask >> s) & 1u) {
      union_below(t, b, child++, clo, chi);
    } else if (nd.meta[s]) {
      const BoxInst& x = b[t.slot[8 * j + s]];
      for (int k = 0; k < 3; k++) { clo[k] = x.bmin[k]; chi[k] = x.bmax[k]; }
    } else {
      continue;
    }
    for (int k = 0; k < 3; k++) {
      if (!std::isnan(clo[k]) && clo[k] < lo[k]) lo[k] = clo[k];
      if (!std::isnan(chi[k]) && chi[k] > hi[k]) hi[k] = chi[k];
    }
  }
}

static int nan_case(const std::vector<BoxInst>& b0, int max_depth, long index, int coord) {
  if (index < 0 || (size_t)index >= b0.size() || coord < 0 || coord > 5) return fail("bad index");
  const BuiltTlas8 built = build(b0, max_depth);
  std::vector<BoxInst> b1 = b0;
  (coord < 3 ? b1[index].bmin[coord] : b1[index].bmax[coord - 3]) = std::nanf("");
  BuiltTlas8 t = built;
  const std::vector<float> boxes = refit(t, b1);
  if (!topology_kept(t, built)) return fail("the refit changed the topology");
  for (size_t j = 0; j < t.nodes.size(); j++) {
    float lo[3], hi[3];
    union_below(t, b1, j, lo, hi);
    for (int k = 0; k < 3; k++)
      if (boxes[6 * j + k] != lo[k] || boxes[6 * j + 3 + k] != hi[k]) return fail("a node's box is not the union without the NaN", (long)j);
    const Node8& nd = t.nodes[j];
    if (!std::isfinite(nd.px) || !std::isfinite(nd.py) || !std::isfinite(nd.pz)) return fail("a node's origin is not finite", (long)j);
    if (nd.ex < 1 || nd.ex > 254 || nd.ey < 1 || nd.ey > 254 || nd.ez < 1 || nd.ez > 254) return fail("a grid exponent out of range", (long)j);
  }
  long contained = 0, at = -1;
  if (const char* why = containment(t, b1, boxes, index, &contained, &at)) return fail(why, at);
  std::printf("{\"ok\": true, \"nodes\": %zu, \"contained\": %ld}\n", t.nodes.size(), contained);
  return 0;
}

// The sum of a block of prt_blas_cost.hip (block_sum): 256 lanes as four waves of 64; within a wave six shuffle-down
// steps (lane i adds lane i + off, its own value where that lane does not exist), then the waves' lane 0 in order.
static double block_sum(const double* lanes) {
  double t = 0.0;
  for (int w = 0; w < 4; w++) {
    double v[64], u[64];
    std::memcpy(v, lanes + 64 * w, sizeof(v));
    for (int off = 32; off > 0; off >>= 1) {
      for (int i = 0; i < 64; i++) u[i] = v[i] + (i + off < 64 ? v[i + off] : v[i]);
      std::memcpy(v, u, sizeof(v));
    }
    t += v[0];
  }
  return t;
}

// k_cost_nodes (one lane per node, one sum per block of 256) and k_cost_total (lane t adds its contiguous run of the
// blocks' sums in index order, then the block's sum) on the host: the same additions in the same order
static double cost_in_kernel_order(const std::vector<Node8>& nodes) {
  const size_t nb = (nodes.size() + 255) / 256;
  std::vector<double> part(nb);
  for (size_t b = 0; b < nb; b++) {
    double lanes[256];
    for (size_t t = 0; t < 256; t++) lanes[t] = 256 * b + t < nodes.size() ? cost_node8(nodes[256 * b + t]) : 0.0;
    part[b] = block_sum(lanes);
  }
  const size_t run = (nb + 255) / 256;
  double lanes[256];
  for (size_t t = 0; t < 256; t++) {
    double v = 0.0;
    for (size_t i = t * run; i < t * run + run && i < nb; i++) v += part[i];
    lanes[t] = v;
  }
  return cost_finish(block_sum(lanes), cost_root_area(nodes[0]));
}

static int cost(const char* nodes_path) {
  std::vector<Node8> nodes;
  if (!read_records(nodes_path, nodes) || nodes.empty()) return fail("cannot read the nodes");
  std::printf("{\"ok\": true, \"nodes\": %zu, \"cost\": %.17g, \"kernel_order\": %.17g}\n", nodes.size(),
              blas_cost8(nodes.data(), nodes.size()), cost_in_kernel_order(nodes));
  return 0;
}

#ifdef TLAS_CHECK_INSTANCES
static int refit_read(const char* nodes_path, const char* slots_path, const char* src_path, const char* out_path) {
  BuiltTlas8 t;
  std::vector<InstSrc> src;
  if (!read_records(nodes_path, t.nodes) || !read_records(slots_path, t.slot) || !read_records(src_path, src) ||
      t.nodes.empty() || t.slot.size() != 8 * t.nodes.size() || src.empty())
    return fail("cannot read the tree or the instances");
  if (const char* why = shape(t, src.size())) return fail(why);
  std::vector<InstDev> inst(src.size());
  for (size_t i = 0; i < src.size(); i++) refit_instance(src[i], inst[i]);
  std::vector<float> boxes(6 * t.nodes.size());
  refit_tlas8(t.nodes.data(), t.nodes.size(), t.slot.data(), inst.data(), (uint32_t)inst.size(), boxes.data());
  FILE* f = std::fopen(out_path, "wb");
  if (!f) return fail("cannot write the nodes");
  const bool ok = std::fwrite(t.nodes.data(), sizeof(Node8), t.nodes.size(), f) == t.nodes.size();
  if (std::fclose(f) != 0 || !ok) return fail("cannot write the nodes");
  std::printf("{\"ok\": true, \"nodes\": %zu, \"instances\": %zu}\n", t.nodes.size(), src.size());
  return 0;
}
#endif

int main(int argc, char** argv) {
#ifdef TLAS_CHECK_INSTANCES
  if (argc == 6 && !std::strcmp(argv[1], "refit")) return refit_read(argv[2], argv[3], argv[4], argv[5]);
#endif
  if (argc == 3 && !std::strcmp(argv[1], "cost")) return cost(argv[2]);
  std::vector<BoxInst> b0, b1;
  if (argc < 4 || !read_records(argv[2], b0) || b0.empty()) return fail("usage: tlas_refit_check <mode> <b0.bin> <max_depth> ...");
  const int max_depth = std::atoi(argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "identity")) return identity(b0, max_depth);
  if (argc == 5 && (!std::strcmp(argv[1], "thereback") || !std::strcmp(argv[1], "contain"))) {
    if (!read_records(argv[4], b1) || b1.size() != b0.size()) return fail("cannot read the moved boxes");
    return argv[1][0] == 't' ? thereback(b0, max_depth, b1) : contain(b0, max_depth, b1);
  }
  if (argc == 6 && !std::strcmp(argv[1], "nan")) return nan_case(b0, max_depth, std::atol(argv[4]), std::atoi(argv[5]));
  return fail("unknown mode");
}
