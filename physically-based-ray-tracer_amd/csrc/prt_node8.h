// prt_node8.h -- one visit of a Node8 node (bvh_build.h), for the device traversals and for the host.
//
// Every function here is __host__ __device__ and works on the node's five 16-byte words as the kernels load them
// (any type with members x, y, z, w: uint4 on the device, Node8Word on the host), so prt_traverse8.h, prt_persist.h,
// tests/cpp/trav_check.cpp and scripts/trav_stats.cpp run the same arithmetic: the explicit fma, the same operation
// order, no contraction (-ffp-contract=off on both sides).
//
// The rule: NO TRAVERSAL ACTS ON AN UNOCCUPIED SLOT.  A slot is occupied when its imask bit is set (an interior
// child) or its meta count (meta & 7) is not 0 (a leaf child; build_tlas8 gives an instance slot the count 1).  The
// builders give an unoccupied slot the inverted box qlo = 255, qhi = 0, which fails the slab test only while 255 * b
// is not absorbed by a in fma(q, b, a): once the node's extent is below about half an ulp of the ray's distance to
// it, all eight slots decode to the same interval and the slab test passes them all.  The inverted box
// is therefore a hint that saves a few steps at ordinary scales; occupancy decides.
//   node8_slabs()     the raw slab mask: may name unoccupied slots (never an interior one: imask bits are occupied)
//   node8_occupied()  the occupancy mask
//   node8_hits()      their intersection
// Where the rule is enforced (the cost in k_trace2 decided it):
//   instance BVH      at the visit: tlas_traverse8 (prt_traverse8.h) and the persistent kernels' instance-BVH visit
//                     (prt_persist.h node_step) mask the leaf slots with node8_occupied(); an unoccupied slot's entry in
//                     the instance-slot table is kNoInstance and must never index the instance array
//   BLAS              at the consumers, through node8_leaf(): a slot with the count 0 holds no record.  blas_traverse8
//                     loops `count` times; the persistent kernels' tri_step drops the step's result and takes nothing
//                     off the count (it used to test one record and let the count wrap to 0xFFFFFFFF)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PRT_NHD __host__ __device__ __forceinline__
#define PRT_NUNROLL _Pragma("unroll")
#else
#define PRT_NHD inline
#define PRT_NUNROLL
#endif

namespace prt {

// both pads of the slab interval on the near side: tn * kPadRatio <= tf accepts whatever tn * 0.99999 <= tf * 1.00001
// accepts, and tn * kPadRatio <= tlimit whatever tn * 0.99999 <= tlimit does (prt_traverse.h kNearPad, kFarPad)
constexpr float kPadRatio = 0.99998f;

// a node's 16-byte word on the host (the device uses uint4)
struct Node8Word {
  uint32_t x, y, z, w;
};

PRT_NHD float n8_bits_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
PRT_NHD float n8_byte(uint32_t w, int k) { return (float)((w >> (8 * k)) & 0xFFu); }

// raw slab mask (physical slots) of the 8 children; near/far plane choice by the sign of rD.  May name unoccupied
// leaf slots (see above).
template <class W4, class V>
PRT_NHD uint32_t node8_slabs(const W4& a, const W4& c, const W4& d, const W4& e, const V& O, const V& rD, float tlimit) {
  const float sx = n8_bits_float((a.w & 0xFFu) << 23), sy = n8_bits_float(((a.w >> 8) & 0xFFu) << 23),
              sz = n8_bits_float(((a.w >> 16) & 0xFFu) << 23);
  const float ax = (n8_bits_float(a.x) - O.x) * rD.x, ay = (n8_bits_float(a.y) - O.y) * rD.y,
              az = (n8_bits_float(a.z) - O.z) * rD.z;
  const float bx = sx * rD.x, by = sy * rD.y, bz = sz * rD.z;
  // near / far quantised planes per axis: words (lo0-3, lo4-7) / (hi0-3, hi4-7)
  const bool px = rD.x >= 0.0f, py = rD.y >= 0.0f, pz = rD.z >= 0.0f;
  const uint32_t nx0 = px ? c.x : d.z, nx1 = px ? c.y : d.w, fx0 = px ? d.z : c.x, fx1 = px ? d.w : c.y;
  const uint32_t ny0 = py ? c.z : e.x, ny1 = py ? c.w : e.y, fy0 = py ? e.x : c.z, fy1 = py ? e.y : c.w;
  const uint32_t nz0 = pz ? d.x : e.z, nz1 = pz ? d.y : e.w, fz0 = pz ? e.z : d.x, fz1 = pz ? e.w : d.y;
  uint32_t hits = 0;
  PRT_NUNROLL
  for (int k = 0; k < 8; k++) {
    const int b = k & 3;
    const uint32_t wnx = k < 4 ? nx0 : nx1, wny = k < 4 ? ny0 : ny1, wnz = k < 4 ? nz0 : nz1;
    const uint32_t wfx = k < 4 ? fx0 : fx1, wfy = k < 4 ? fy0 : fy1, wfz = k < 4 ? fz0 : fz1;
    const float tnx = __builtin_fmaf(n8_byte(wnx, b), bx, ax), tfx = __builtin_fmaf(n8_byte(wfx, b), bx, ax);
    const float tny = __builtin_fmaf(n8_byte(wny, b), by, ay), tfy = __builtin_fmaf(n8_byte(wfy, b), by, ay);
    const float tnz = __builtin_fmaf(n8_byte(wnz, b), bz, az), tfz = __builtin_fmaf(n8_byte(wfz, b), bz, az);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, 0.0f)) * kPadRatio;  // both pads
    const float tf = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
    if (tn <= tf && tn <= tlimit) hits |= 1u << k;
  }
  return hits;
}

// bit k set when byte k of w has a count (byte & 7) other than 0
PRT_NHD uint32_t n8_counted(uint32_t w) {
  // per byte: (count + 0x7F) carries into bit 7 exactly when count >= 1 (count <= 7: no carry leaves the byte);
  // the multiply gathers bits 0, 8, 16, 24 into bits 21..24 (the partial products land on distinct bits)
  const uint32_t nz = (((w & 0x07070707u) + 0x7F7F7F7Fu) >> 7) & 0x01010101u;
  return ((nz * 0x00204081u) >> 21) & 0xFu;
}

// occupied slots: interior children (imask) and leaf children with a count; a = word 0, b = word 1 of the node
template <class W4>
PRT_NHD uint32_t node8_occupied(const W4& a, const W4& b) {
  return (a.w >> 24) | n8_counted(b.z) | (n8_counted(b.w) << 4);
}

// the visit: occupied slots whose box the ray's interval [0, tlimit] meets
template <class W4, class V>
PRT_NHD uint32_t node8_hits(const W4& a, const W4& b, const W4& c, const W4& d, const W4& e, const V& O, const V& rD,
                            float tlimit) {
  return node8_slabs(a, c, d, e, O, rD, tlimit) & node8_occupied(a, b);
}

// physical-slot mask -> traversal-order mask (bit k ^ oct)
PRT_NHD uint32_t order_mask(uint32_t m, uint32_t oct) {
  if (oct & 1u) m = ((m & 0x55u) << 1) | ((m >> 1) & 0x55u);
  if (oct & 2u) m = ((m & 0x33u) << 2) | ((m >> 2) & 0x33u);
  if (oct & 4u) m = ((m & 0x0Fu) << 4) | ((m >> 4) & 0x0Fu);
  return m;
}

// leaf slot k of a node with meta words (meta0 = slots 0-3, meta1 = slots 4-7): its first triangle record and its
// count; false (count 0) for an unoccupied slot, which holds no record: the caller tests none.
PRT_NHD bool node8_leaf(uint32_t tri_base, uint32_t meta0, uint32_t meta1, uint32_t k, uint32_t& first, uint32_t& count) {
  const uint32_t meta = ((k < 4 ? meta0 : meta1) >> (8 * (k & 3))) & 0xFFu;
  first = tri_base + (meta >> 3);
  count = meta & 7u;
  return count != 0u;
}

// the instance-slot table (BuiltTlas8::slot) holds kNoInstance for every slot that is not an occupied leaf slot
constexpr uint32_t kNoInstance = 0xFFFFFFFFu;
PRT_NHD bool node8_instance_valid(uint32_t id, uint32_t ninst) { return id < ninst; }

}  // namespace prt
