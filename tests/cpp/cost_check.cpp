// cost_check -- blas_cost8() of csrc/prt_blas_cost.h (the per-node code the kernels of prt_blas_cost run) on the CPU.
//   host <tris.bin> <spatial 0|1>   the host builder's tree over the triangles: its cost, to be compared with what
//                                   bvh_check's `blas` mode reports for the same build; the cost after one occupied
//                                   slot's box was changed (`changed`, another value), and after every unoccupied
//                                   slot's box bytes were overwritten (`unoccupied`, the same bits: occupancy decides)
//   tree <nodes.bin>                the cost of a tree given as raw Node8 bytes (bvh_check dump, or prt_read_blas)
//   refit <v0.bin> <v1.bin> <nodes.out> <recs.out>
//                                   the host SAH tree over V0 refitted to V1 by refit_blas8 (prt_blas_refit.h, the
//                                   update's host path): its cost and depth, the tree written as raw Node8 / TriMT
//                                   bytes for bvh_check's `tree` mode
// tris.bin: float32 fat triangles (3 x float4 per triangle).  Prints one JSON line; exit status 0 = ok.  Build with
// -ffp-contract=off, as the library is built.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh_build.h"
#include "prt_blas_cost.h"
#include "prt_blas_refit.h"

using namespace prt;

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

static int fail(const char* what) {
  std::printf("{\"ok\": false, \"what\": \"%s\"}\n", what);
  return 1;
}

static int host(const char* tris_path, bool spatial) {
  std::vector<float> t;
  if (!read_records(tris_path, t) || t.empty() || t.size() % 12) return fail("cannot read the triangles");
  BuiltBlas8 b = build_blas8(t.data(), (int32_t)(t.size() / 12), 3, spatial);
  const double cost = blas_cost8(b.nodes.data(), b.nodes.size());
  // one occupied slot of the last node (a root slot when the tree is one node): its upper x bound moves one step
  std::vector<Node8> moved = b.nodes;
  Node8& m = moved.back();
  int slot = -1;
  for (int s = 0; s < 8 && slot < 0; s++)
    if (cost_slot_occupied(m, s)) slot = s;
  if (slot < 0) return fail("a node without an occupied slot");
  m.qhix[slot] = (uint8_t)(m.qhix[slot] < 255 ? m.qhix[slot] + 1 : m.qhix[slot] - 1);
  const double changed = blas_cost8(moved.data(), moved.size());
  // every unoccupied slot: arbitrary box bytes
  std::vector<Node8> junk = b.nodes;
  long unoccupied = 0;
  for (Node8& n : junk)
    for (int s = 0; s < 8; s++)
      if (!cost_slot_occupied(n, s)) {
        n.qlox[s] = 3; n.qloy[s] = 0; n.qloz[s] = 17;
        n.qhix[s] = 250; n.qhiy[s] = 255; n.qhiz[s] = 99;
        unoccupied++;
      }
  const double same = blas_cost8(junk.data(), junk.size());
  std::printf("{\"ok\": true, \"nodes\": %zu, \"refs\": %zu, \"cost\": %.17g, \"changed\": %.17g, \"unoccupied\": %.17g, "
              "\"unoccupied_slots\": %ld}\n",
              b.nodes.size(), b.tris.size(), cost, changed, same, unoccupied);
  return 0;
}

static int tree(const char* nodes_path) {
  std::vector<Node8> nodes;
  if (!read_records(nodes_path, nodes) || nodes.empty()) return fail("cannot read the nodes");
  std::printf("{\"ok\": true, \"nodes\": %zu, \"cost\": %.17g}\n", nodes.size(), blas_cost8(nodes.data(), nodes.size()));
  return 0;
}

template <class R>
static bool write_records(const char* path, const std::vector<R>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(R), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok;
}

static int refit(const char* v0_path, const char* v1_path, const char* nodes_out, const char* recs_out) {
  std::vector<float> v0, v1;
  if (!read_records(v0_path, v0) || !read_records(v1_path, v1) || v0.empty() || v0.size() % 12 || v1.size() != v0.size())
    return fail("cannot read the triangles");
  BuiltBlas8 b = build_blas8(v0.data(), (int32_t)(v0.size() / 12), 3, false);
  const double before = blas_cost8(b.nodes.data(), b.nodes.size());
  std::vector<float> boxes(6 * b.nodes.size());
  refit_blas8(b.nodes.data(), b.nodes.size(), b.tris.data(), b.tris.size(), v1.data(), boxes.data());
  if (!write_records(nodes_out, b.nodes) || !write_records(recs_out, b.tris)) return fail("cannot write the tree");
  std::printf("{\"ok\": true, \"nodes\": %zu, \"depth\": %d, \"built\": %.17g, \"cost\": %.17g}\n", b.nodes.size(), b.depth,
              before, blas_cost8(b.nodes.data(), b.nodes.size()));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "host")) return host(argv[2], std::atoi(argv[3]) != 0);
  if (argc == 3 && !std::strcmp(argv[1], "tree")) return tree(argv[2]);
  if (argc == 6 && !std::strcmp(argv[1], "refit")) return refit(argv[2], argv[3], argv[4], argv[5]);
  return fail("usage: cost_check host <tris.bin> <spatial> | tree <nodes.bin> | refit <v0.bin> <v1.bin> <nodes.out> <recs.out>");
}
