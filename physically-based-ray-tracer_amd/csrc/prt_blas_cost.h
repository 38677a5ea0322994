// prt_blas_cost.h -- the SAH cost of a BLAS as it stands (prt_blas_cost): the definition.
//
// The measure is the one tests/cpp/bvh_check.cpp reports for a checked tree (kWideNodeCost = kWideTriCost = 1 of
// bvh_build.cpp): over all nodes, every interior slot's decoded box area plus every leaf slot's decoded box area times
// its count (meta & 7), divided by the area of the box around the root node's occupied slots; 0 when that area is 0.
// A slot's box is what the traversal's planes decode to, origin + q * 2^(e - 127), in double; area is
// dx*dy + dy*dz + dz*dx.  An unoccupied slot (imask bit clear, count 0; prt_node8.h) contributes nothing, whatever
// its box bytes say.  Every function here is __host__ __device__: the kernels (prt_blas_cost.hip) and the plain host
// blas_cost8() below run the same per-node arithmetic, compiled without FMA contraction on both sides.  Only the
// order of the sum over nodes differs (the host adds in node order, the device per block and then over the blocks),
// which is worth at most terms x 2^-52 relative: every term is non-negative.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bvh_build.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PRT_CHD __host__ __device__ inline
#define PRT_CUNROLL _Pragma("unroll")
#else
#define PRT_CHD inline
#define PRT_CUNROLL
#endif

namespace prt {

PRT_CHD double cost_pow2(int e) {  // 2^e for -1022 <= e <= 1023 (a node's grid scale: e = ex - 127, -127 .. 128)
  const uint64_t b = (uint64_t)(e + 1023) << 52;
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}

PRT_CHD bool cost_slot_occupied(const Node8& n, int s) { return ((n.imask >> s) & 1u) || (n.meta[s] & 7u); }

// slot s of node n as the traversal decodes it
PRT_CHD void cost_slot_box(const Node8& n, int s, double lo[3], double hi[3]) {
  const double o[3] = {(double)n.px, (double)n.py, (double)n.pz};
  const double sc[3] = {cost_pow2((int)n.ex - 127), cost_pow2((int)n.ey - 127), cost_pow2((int)n.ez - 127)};
  const double ql[3] = {(double)n.qlox[s], (double)n.qloy[s], (double)n.qloz[s]};
  const double qh[3] = {(double)n.qhix[s], (double)n.qhiy[s], (double)n.qhiz[s]};
  for (int k = 0; k < 3; k++) {
    lo[k] = o[k] + ql[k] * sc[k];
    hi[k] = o[k] + qh[k] * sc[k];
  }
}

PRT_CHD double cost_area(const double lo[3], const double hi[3]) {
  const double d[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
  return d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
}

// one node's part of the sum: interior slots' areas + leaf slots' areas x count, slots in order
PRT_CHD double cost_node8(const Node8& n) {
  double sum = 0.0;
  PRT_CUNROLL
  for (int s = 0; s < 8; s++) {
    if (!cost_slot_occupied(n, s)) continue;
    double lo[3], hi[3];
    cost_slot_box(n, s, lo, hi);
    const double a = cost_area(lo, hi);
    sum += ((n.imask >> s) & 1u) ? a : a * (double)(n.meta[s] & 7u);
  }
  return sum;
}

// the area of the box around the root node's occupied slots (0 for a root without one)
PRT_CHD double cost_root_area(const Node8& n) {
  double rlo[3] = {1e300, 1e300, 1e300}, rhi[3] = {-1e300, -1e300, -1e300};
  bool any = false;
  PRT_CUNROLL
  for (int s = 0; s < 8; s++) {
    if (!cost_slot_occupied(n, s)) continue;
    double lo[3], hi[3];
    cost_slot_box(n, s, lo, hi);
    for (int k = 0; k < 3; k++) {
      rlo[k] = lo[k] < rlo[k] ? lo[k] : rlo[k];
      rhi[k] = hi[k] > rhi[k] ? hi[k] : rhi[k];
    }
    any = true;
  }
  return any ? cost_area(rlo, rhi) : 0.0;
}

PRT_CHD double cost_finish(double area_sum, double root_area) { return root_area > 0.0 ? area_sum / root_area : 0.0; }

// The sequential host measure of one tree (node 0 = the root; offsets play no part): the nodes' parts in node order.
inline double blas_cost8(const Node8* nodes, size_t n_nodes) {
  if (!n_nodes) return 0.0;
  double sum = 0.0;
  for (size_t j = 0; j < n_nodes; j++) sum += cost_node8(nodes[j]);
  return cost_finish(sum, cost_root_area(nodes[0]));
}

}  // namespace prt
