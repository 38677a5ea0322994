// instance_host_check.cpp -- what the instance entry points decide without a device (physically-based-ray-tracer_amd/
// csrc/prt_instance_host.h) on the CPU, driven by tests/test_instance_host.py, which holds the expected values:
//   plan <linear>          plan_instance_refresh over every combination of n, force, had_tlas, tlas_n (-1, n, n + 1),
//                          tlas_dirty, has_worker: one row [inputs..., use_tlas, tree_work, async] each
//   depthcap               tlas_depth_cap over max_depth x tree_depth x n: rows [max_depth, tree_depth, n, cap,
//                          tlas8_median_depth(n)]; occ_at(0 .. 80); kMaxBvhDepth
//   sizes <linear>         inst_stage_bytes and inst_buffer_bytes for n in {1, 64, 65, 10000}, with and without a tree,
//                          for an async update, a first build of <nodes> nodes and no tree work; inst_tab_layout
//   table <n> <nmesh> <kinds> <seed>
//                          random transforms, mesh ids, kinds (kinds = 0: the empty kind list) and mesh boxes:
//                          fill_inst_src's array equals, byte for byte, what k_inst_src (prt_tlas_refit.hip), transcribed
//                          below, writes from fill_inst_tab's bytes, from packed matrices (stride 4) and from an InstSrc
//                          array (stride 6); the table's unused bytes are zero
// Prints one JSON line; exit status 0 = the check holds (plan, depthcap, sizes: the rows were printed).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "prt_instance_host.h"

using namespace prt;
using namespace prt::host;

static int fail(const char* what, long a, long b) {
  std::printf("{\"ok\": false, \"what\": \"%s\", \"a\": %ld, \"b\": %ld}\n", what, a, b);
  return 1;
}

static int print_plan(int32_t linear) {
  std::printf("{\"ok\": true, \"rows\": [");
  bool first = true;
  for (int32_t n : {1, 64, 65, 300})
    for (int force = 0; force < 2; force++)
      for (int had = 0; had < 2; had++)
        for (int32_t tn : {-1, n, n + 1})
          for (int dirty = 0; dirty < 2; dirty++)
            for (int worker = 0; worker < 2; worker++) {
              const InstRefresh p = plan_instance_refresh(n, linear, force != 0, had != 0, tn, dirty != 0, worker != 0);
              std::printf("%s[%d, %d, %d, %d, %d, %d, %d, %d, %d]", first ? "" : ", ", n, force, had, tn, dirty, worker,
                          (int)p.use_tlas, (int)p.tree_work, (int)p.async);
              first = false;
            }
  std::printf("]}\n");
  return 0;
}

static int print_depthcap() {
  std::printf("{\"ok\": true, \"max_bvh_depth\": %d, \"occ\": [", kMaxBvhDepth);
  for (int d = 0; d <= 80; d++) std::printf("%s%d", d ? ", " : "", occ_at(d));
  std::printf("], \"rows\": [");
  bool first = true;
  for (int md : {1, 6, 9, 10, 11, 14, 15, 40, 59})
    for (int td : {1, 2, 4, 5})
      for (int32_t n : {1, 9, 65, 5000}) {
        std::printf("%s[%d, %d, %d, %d, %d]", first ? "" : ", ", md, td, n, tlas_depth_cap(md, td, n), tlas8_median_depth(n));
        first = false;
      }
  std::printf("]}\n");
  return 0;
}

static int print_sizes(int32_t linear) {
  std::printf("{\"ok\": true, \"node8\": %zu, \"rows\": [", sizeof(Node8));
  bool first = true;
  for (int32_t n : {1, 64, 65, 10000}) {
    const size_t first_nodes = (size_t)(n + 2) / 3;  // some tree of a first build: fewer nodes than the cap
    const InstRefresh list = {false, false, false}, async = {true, true, true}, build = {true, true, false},
                      none = {true, false, false};
    const InstStageBytes sl = inst_stage_bytes(n, list, 0), sa = inst_stage_bytes(n, async, 0),
                         sf = inst_stage_bytes(n, build, first_nodes), sn = inst_stage_bytes(n, none, 0);
    const InstBufBytes bl = inst_buffer_bytes(n, linear, 3, false), bt = inst_buffer_bytes(n, linear, 3, true);
    std::printf("%s{\"n\": %d, \"first_nodes\": %zu, \"cap\": %zu, \"node_cap\": %zu, ", first ? "" : ", ", n, first_nodes,
                inst_cap(n, linear), tlas_node_cap(n));
    auto stage = [](const char* k, const InstStageBytes& s) {
      std::printf("\"%s\": [%zu, %zu, %zu, %zu], ", k, s.src, s.nodes, s.slot, s.per);
    };
    stage("list", sl);
    stage("async", sa);
    stage("build", sf);
    stage("none", sn);
    auto bufs = [](const char* k, const InstBufBytes& b, const char* end) {
      std::printf("\"%s\": [%zu, %zu, %zu, %zu, %zu, %zu, %zu]%s", k, b.inst, b.inst_src, b.tlas8, b.tlas_slot, b.inst_tab,
                  b.tlas_order, b.tlas_box, end);
    };
    bufs("buf_list", bl, ", ");
    bufs("buf_tree", bt, "}");
    first = false;
  }
  const InstTabLayout L = inst_tab_layout(inst_cap(65, linear), 3);
  std::printf("], \"tab65\": [%zu, %zu, %zu]}\n", L.kind, L.box, L.total);
  return 0;
}

// prt_refit.h's InstSrc restated (that header needs HIP), and mesh boxes inside a larger record, as the context keeps them
struct InstSrc {
  float T[16];
  float bmin[3];
  uint32_t mesh;
  float bmax[3];
  uint32_t kind;
};
struct MeshBox {
  float bmin[3], bmax[3];
  int other[5];
};

// k_inst_src (prt_tlas_refit.hip), one instance: the transform as four 16-byte words at xf + stride4 * i (in 16-byte
// units), the mesh id and kind from the table, the mesh's box as two 16-byte words whose last components become the id
// and the kind; six 16-byte words stored
static void k_inst_src(const char* xf, uint32_t stride4, const char* mesh, const char* kind, const char* mesh_box,
                       uint32_t nmesh, uint32_t i, char* out) {
  char t[64], lo[16], hi[16];
  std::memcpy(t, xf + 16 * (size_t)stride4 * i, 64);
  uint32_t m, k;
  std::memcpy(&m, mesh + 4 * (size_t)i, 4);
  std::memcpy(&k, kind + 4 * (size_t)i, 4);
  if (m >= nmesh) m = 0;
  std::memcpy(lo, mesh_box + 32 * (size_t)m, 16);
  std::memcpy(hi, mesh_box + 32 * (size_t)m + 16, 16);
  std::memcpy(lo + 12, &m, 4);
  std::memcpy(hi + 12, &k, 4);
  std::memcpy(out + 96 * (size_t)i, t, 64);
  std::memcpy(out + 96 * (size_t)i + 64, lo, 16);
  std::memcpy(out + 96 * (size_t)i + 80, hi, 16);
}

static int check_table(int32_t n, uint32_t nmesh, bool kinds, uint32_t seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> uf(-10.0f, 10.0f);
  std::vector<float> xf(16 * (size_t)n);
  for (float& v : xf) v = uf(rng);
  std::vector<uint32_t> mesh(n), kind(kinds ? n : 0);
  for (uint32_t& m : mesh) m = rng() % nmesh;
  for (uint32_t& k : kind) k = rng() % 3u;
  std::vector<MeshBox> box(nmesh);
  for (MeshBox& b : box) {
    for (int k = 0; k < 3; k++) { b.bmin[k] = uf(rng); b.bmax[k] = b.bmin[k] + 1.0f + uf(rng) * uf(rng); }
    for (int& o : b.other) o = (int)rng();
  }
  // the host-side fill, over records that start as 0xA5 bytes (InstSrc has no padding: every byte is written)
  std::vector<InstSrc> host(n);
  std::memset(host.data(), 0xA5, sizeof(InstSrc) * (size_t)n);
  fill_inst_src(n, mesh.data(), kind.data(), kind.size(), box.data(), xf.data(), host.data());
  // the table, in a buffer that starts as 0xA5 bytes with a guard behind it
  const InstTabLayout L = inst_tab_layout((size_t)(n > 64 ? n : 64), nmesh);
  if (L.kind % 16 || L.box % 16 || L.kind < 4 * (size_t)n || L.box < L.kind + 4 * (size_t)n || L.total != L.box + 32 * (size_t)nmesh)
    return fail("inst_tab_layout: parts overlap or are not 16-byte aligned", (long)L.kind, (long)L.box);
  std::vector<char> tab(L.total + 64, (char)0xA5);
  fill_inst_tab(n, mesh.data(), kind.data(), kind.size(), box.data(), nmesh, L, tab.data());
  for (size_t b = L.total; b < tab.size(); b++)
    if (tab[b] != (char)0xA5) return fail("fill_inst_tab wrote past the table", (long)b, (long)L.total);
  // the unused bytes: behind the n mesh ids, behind the n kinds (all of them with no kind list), each box's fourth word
  auto zero = [&](size_t from, size_t to) {
    for (size_t b = from; b < to; b++)
      if (tab[b]) return false;
    return true;
  };
  if (!zero(4 * (size_t)n, L.kind) || !zero(L.kind + (kinds ? 4 * (size_t)n : 0), L.box)) return fail("pad bytes are not zero", 0, 0);
  for (uint32_t m = 0; m < nmesh; m++)
    if (!zero(L.box + 32 * m + 12, L.box + 32 * m + 16) || !zero(L.box + 32 * m + 28, L.box + 32 * m + 32))
      return fail("a mesh box's fourth word is not zero", m, 0);
  // the device-side refill from that table: from the packed matrices, and from the InstSrc array itself
  for (uint32_t stride4 : {4u, 6u}) {
    std::vector<char> dev(96 * (size_t)n, (char)0x5A);
    const char* t = stride4 == 4 ? reinterpret_cast<const char*>(xf.data()) : reinterpret_cast<const char*>(host.data());
    for (int32_t i = 0; i < n; i++) k_inst_src(t, stride4, tab.data(), tab.data() + L.kind, tab.data() + L.box, nmesh, (uint32_t)i, dev.data());
    if (std::memcmp(dev.data(), host.data(), dev.size())) {
      size_t b = 0;
      while (dev[b] == reinterpret_cast<const char*>(host.data())[b]) b++;
      return fail("the refill from the table differs from fill_inst_src: instance, byte", (long)(b / 96), (long)(b % 96));
    }
  }
  std::printf("{\"ok\": true, \"instances\": %d, \"table_bytes\": %zu}\n", n, L.total);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "depthcap")) return print_depthcap();
  if (argc < 3) return 2;
  if (!std::strcmp(argv[1], "plan")) return print_plan(std::atoi(argv[2]));
  if (!std::strcmp(argv[1], "sizes")) return print_sizes(std::atoi(argv[2]));
  if (!std::strcmp(argv[1], "table") && argc == 6)
    return check_table(std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), std::atoi(argv[4]) != 0, (uint32_t)std::atoi(argv[5]));
  return 2;
}
