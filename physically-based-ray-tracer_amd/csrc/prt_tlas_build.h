// prt_tlas_build.h -- instance BVH rebuild on the device (prt_rebuild_instances): what comes before and after the
// device builder (bvh_gpu.hip gpu_build_blas8 with max_leaf = 1), per instance and per node.
//
// The builder reads "fat triangles" (three float4 per primitive) and emits a BLAS: Node8 records whose leaf slots
// point at TriMT records.  An instance BVH is that tree over one degenerate triangle per instance box, with the
// records replaced by an instance-slot table, as the host's build_tlas8 (bvh_build.cpp) makes it:
//
//   before   tlas_fat_record     instance box {lo, hi} -> the triangle {lo, hi, 0.5 lo + 0.5 hi}.  The builder bounds a
//                                primitive by min / max over its three vertices and sorts and clusters it by their
//                                mean.  The third vertex lies in [lo, hi] (each half is exact, the sum is rounded once,
//                                and rounding is monotone), so the bounds are the box bit for bit, and the mean of the
//                                three is the box centre -- with the host's {lo, hi, lo} it would be (2 lo + hi) / 3
//   after    tlas_finish_node8   build_tlas8's tail: leaf slot s of node j names the instance whose record the slot's
//                                meta points at (slot[8j + s] = tris[tri_base + (meta[s] >> 3)].prim; with max_leaf = 1
//                                every leaf slot has the count 1), every other slot gets kTlasNoInstance, and tri_base
//                                becomes 8j.  Boxes, imask, meta and child_base are the builder's
// Every function here is __host__ __device__: the kernels (prt_tlas_build.hip) and the CPU checker
// (tests/cpp/tlas_build_check.cpp) run the same code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "prt_blas_refit.h"

namespace prt {

constexpr uint32_t kTlasNoInstance = 0xFFFFFFFFu;  // (prt_node8.h kNoInstance; BuiltTlas8::slot)

// the fat triangle of one instance box: 12 floats (three float4, w = 0)
PRT_RHD void tlas_fat_record(const float* lo, const float* hi, float* out) {
  for (int k = 0; k < 3; k++) {
    out[k] = lo[k];
    out[4 + k] = hi[k];
    out[8 + k] = 0.5f * lo[k] + 0.5f * hi[k];
  }
  out[3] = out[7] = out[11] = 0.0f;
}

// Node nd (a copy of the builder's node j; the caller stores it back) and its eight instance-slot words.  tris: the
// builder's records, n_tris of them; a slot that points outside them, or whose record names no instance (>= ninst),
// gets kTlasNoInstance and reads nothing out of range (the builder emits neither).
PRT_RHD void tlas_finish_node8(Node8& nd, uint32_t j, const TriMT* tris, uint32_t n_tris, uint32_t ninst, uint32_t* slot) {
  PRT_RUNROLL
  for (int s = 0; s < 8; s++) {
    uint32_t id = kTlasNoInstance;
    if (!((nd.imask >> s) & 1u) && nd.meta[s]) {
      const uint32_t g = nd.tri_base + (uint32_t)(nd.meta[s] >> 3);
      if (g < n_tris) id = tris[g].prim;
      if (id >= ninst) id = kTlasNoInstance;
    }
    slot[s] = id;
  }
  nd.tri_base = 8u * j;
}

}  // namespace prt
