// prt_tlas_refit.h -- instance BVH refit: the instances move, the tree keeps its topology (prt_update_instances).
//
// The nodes, their slots, imask, meta, child_base, tri_base and the instance-slot table stay; the boxes are recomputed
// bottom-up from the instance records.  Every function here is __host__ __device__: the device kernel
// (prt_tlas_refit.hip) and the plain host refit_tlas8() below run the same code, compiled without FMA contraction on
// both sides, so the two produce the same bytes.  The encoding is refit_encode8 (prt_blas_refit.h), the second half of
// build_wide8 unchanged: a refit over the boxes build_tlas8 was given reproduces its Node8 array byte for byte.
//
//   leaf slot s of node j   box = the InstDev box (bmin / bmax, as refit_instance inflated it) of instance
//                           slot[8j + s]; build_tlas8 gives every leaf slot the count 1
//   interior slot           box = the child node's box
//   node                    box = union of its occupied slots' boxes, uninflated, six floats in scratch
// A leaf slot whose table entry names no instance (>= ninst) and an interior slot whose child lies outside the tree
// (>= n_nodes) are left as they are and read nothing: a damaged table costs a box, never an out-of-range read.
// Boxes grow with the builders' own operation, which ignores a NaN coordinate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "prt_blas_refit.h"

namespace prt {

// Node nd (a copy; the caller stores it back), its eight instance-slot words `slot`: the per-node code of the refit.
// inst: the instance records (any type with bmin[3] / bmax[3]: InstDev); boxes: six floats per node, lo then hi.
template <class Inst>
PRT_RHD void refit_tlas_node8(Node8& nd, const uint32_t* slot, const Inst* inst, uint32_t ninst, const float* boxes,
                              uint32_t n_nodes, float* box_out) {
  float clo[8][3], chi[8][3];
  uint32_t occupied = 0;
  PRT_RUNROLL
  for (int s = 0; s < 8; s++) {
    if ((nd.imask >> s) & 1u) {
      const uint32_t child = nd.child_base + (uint32_t)__builtin_popcount((uint32_t)nd.imask & ((1u << s) - 1u));
      if (child >= n_nodes) continue;
      const float* b = boxes + 6 * (size_t)child;
      for (int k = 0; k < 3; k++) { clo[s][k] = b[k]; chi[s][k] = b[3 + k]; }
      occupied |= 1u << s;
    } else if (nd.meta[s] & 7u) {
      const uint32_t id = slot[s];
      if (id >= ninst) continue;
      for (int k = 0; k < 3; k++) { clo[s][k] = inst[id].bmin[k]; chi[s][k] = inst[id].bmax[k]; }
      occupied |= 1u << s;
    }
  }
  refit_encode8(nd, occupied, clo, chi, box_out);
}

// The sequential host refit of an instance BVH as build_tlas8 returns it: the nodes last to first -- every interior
// child has a larger index than its parent.  boxes: 6 floats per node (the root's, boxes[0..5], is the scene's box).
template <class Inst>
inline void refit_tlas8(Node8* nodes, size_t n_nodes, const uint32_t* slot, const Inst* inst, uint32_t ninst, float* boxes) {
  for (size_t j = n_nodes; j-- > 0;) {
    Node8 nd = nodes[j];
    refit_tlas_node8(nd, slot + 8 * j, inst, ninst, boxes, (uint32_t)n_nodes, boxes + 6 * j);
    nodes[j] = nd;
  }
}

}  // namespace prt
