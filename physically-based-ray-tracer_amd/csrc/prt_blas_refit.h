// prt_blas_refit.h -- BLAS refit: a mesh's triangles change, its tree keeps its topology (prt_update_mesh).
//
// The nodes, their slots and the order of the triangle records stay; the records and the boxes are recomputed
// bottom-up from the new triangles.  Every function here is __host__ __device__: the device kernels
// (prt_blas_refit.hip) and the plain host refit_blas8() below run the same code, compiled without FMA contraction
// (-ffp-contract=off) on both sides, so the two produce the same bytes.  The encoding is the second half of
// build_wide8 (bvh_build.cpp) / collapse_task (bvh_gpu.hip) unchanged: a refit with the build's own triangles
// reproduces the builder's Node8 and TriMT arrays byte for byte.
//
//   record g       v0 = a, e1 = b - a, e2 = c - a of triangles[tris[g].prim]; prim and the pads are kept
//   leaf slot      box = union of the full bounds of the triangles of its records (the corners, not v0 + e)
//   interior slot  box = the child node's box
//   node           box = union of its occupied slots' boxes, uninflated, six floats in scratch
//   encoding       inflate_box per occupied slot, origin = (float) union-in-double lo, exponents from the extent,
//                  qlo = floor, qhi = ceil on the node grid; imask, child_base, tri_base, meta untouched
// Boxes grow with the builders' own operation (lo = p < lo ? p : lo), which ignores a NaN coordinate.
#pragma once
#include <stdint.h>

#include "bvh_build.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PRT_RHD __host__ __device__ inline
#define PRT_RUNROLL _Pragma("unroll")
#else
#define PRT_RHD inline
#define PRT_RUNROLL
#endif

namespace prt {

// Box::reset / Box::grow of bvh_build.cpp
PRT_RHD void refit_box_reset(float* lo, float* hi) {
  for (int k = 0; k < 3; k++) { lo[k] = 1e30f; hi[k] = -1e30f; }
}
PRT_RHD void refit_box_grow(float* lo, float* hi, const float* p) {
  for (int k = 0; k < 3; k++) {
    lo[k] = p[k] < lo[k] ? p[k] : lo[k];
    hi[k] = p[k] > hi[k] ? p[k] : hi[k];
  }
}
PRT_RHD void refit_box_merge(float* lo, float* hi, const float* blo, const float* bhi) {
  for (int k = 0; k < 3; k++) {
    lo[k] = blo[k] < lo[k] ? blo[k] : lo[k];
    hi[k] = bhi[k] > hi[k] ? bhi[k] : hi[k];
  }
}

// inflate_box (bvh_build.cpp)
PRT_RHD void refit_inflate(float* lo, float* hi) {
  for (int k = 0; k < 3; k++) {
    const float al = __builtin_fabsf(lo[k]), ah = __builtin_fabsf(hi[k]);
    const float ext = al < ah ? ah : al;
    const float pad = ext * 1e-6f + 1e-7f;
    lo[k] -= pad;
    hi[k] += pad;
  }
}

// grid_exponent(ext, 255) (bvh_build.cpp), exactly: the smallest biased exponent e with 255 * 2^(e - 127) >= ext,
// clamped to 1..254; 1 when ext is not positive.  From the double's exponent field: ext = m * 2^x with m in
// [0.5, 1), and 255 * 2^(x - 8) >= ext exactly when m <= 255/256.
PRT_RHD uint8_t refit_grid_exponent(double ext) {
  if (!(ext > 0)) return 1;
  uint64_t b;
  __builtin_memcpy(&b, &ext, 8);
  const int bx = (int)((b >> 52) & 0x7FFu);
  if (bx == 0) return 1;        // subnormal: below 255 * 2^-126
  if (bx == 0x7FF) return 254;  // infinite
  const int x = bx - 1022;
  const uint64_t frac = b & ((1ull << 52) - 1);
  const int e = x - ((frac <= (127ull << 45)) ? 8 : 7) + 127;
  return (uint8_t)(e < 1 ? 1 : e > 254 ? 254 : e);
}

PRT_RHD double refit_pow2(int e) {  // 2^e for -1022 <= e <= 1023
  const uint64_t b = (uint64_t)(e + 1023) << 52;
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}

// one TriMT record from its primitive's corners (prim and the pads are kept)
PRT_RHD void refit_record(TriMT& t, const float* triangles) {
  const float* a = triangles + 12 * (size_t)t.prim;
  for (int k = 0; k < 3; k++) {
    t.v0[k] = a[k];
    t.e1[k] = a[4 + k] - a[k];
    t.e2[k] = a[8 + k] - a[k];
  }
}

// word w (0..26) of a primitive's ShadeTri as prt_set_meshes fills it: n[9] | uv[6] | p[9] | fn[3].  An index
// outside [0, vertex_count) reads vertex 0 and sets *bad (never an out-of-range read).
PRT_RHD float refit_shade_word(int w, size_t p, const float* fixed_normals, const float* fixed_uvs, const int32_t* indices,
                               const float* vertices, const float* face_normals, int32_t vertex_count, uint32_t* bad) {
  if (w < 9) return fixed_normals[4 * (3 * p + (size_t)(w / 3)) + (size_t)(w % 3)];
  if (w < 15) return fixed_uvs[6 * p + (size_t)(w - 9)];
  if (w < 24) {
    int32_t i = indices[3 * p + (size_t)((w - 15) / 3)];
    if (i < 0 || i >= vertex_count) {
      i = 0;
      *bad = 1u;
    }
    return vertices[3 * (size_t)i + (size_t)((w - 15) % 3)];
  }
  return face_normals[3 * p + (size_t)(w - 24)];
}

// Slot s of node nd: its box as the refit defines it, into lo / hi -- an interior slot's is the child node's box
// (`boxes`: six floats per node, lo then hi, indexed like child_base; interior children are contiguous from
// child_base in slot order), a leaf slot's the union of the full bounds of its records' triangles (`tris` indexed
// like tri_base).  false: an empty slot.
PRT_RHD bool refit_slot_box(const Node8& nd, int s, const TriMT* tris, const float* triangles, const float* boxes,
                            float* lo, float* hi) {
  if ((nd.imask >> s) & 1u) {
    const uint32_t child = nd.child_base + (uint32_t)__builtin_popcount((uint32_t)nd.imask & ((1u << s) - 1u));
    const float* b = boxes + 6 * (size_t)child;
    for (int k = 0; k < 3; k++) { lo[k] = b[k]; hi[k] = b[3 + k]; }
    return true;
  }
  if (!nd.meta[s]) return false;
  refit_box_reset(lo, hi);
  const uint32_t first = nd.tri_base + (uint32_t)(nd.meta[s] >> 3), cnt = nd.meta[s] & 7u;
  for (uint32_t g = first; g < first + cnt; g++) {
    const float* a = triangles + 12 * (size_t)tris[g].prim;
    float tlo[3], thi[3];
    refit_box_reset(tlo, thi);
    refit_box_grow(tlo, thi, a);
    refit_box_grow(tlo, thi, a + 4);
    refit_box_grow(tlo, thi, a + 8);
    refit_box_merge(lo, hi, tlo, thi);
  }
  return true;
}

// Node nd (a copy; the caller stores it back) from its occupied slots' boxes clo / chi (inflated here): its own
// uninflated box into box_out, its grid and quantised child bounds re-encoded.  An empty slot keeps its inverted
// encoding.
PRT_RHD void refit_encode8(Node8& nd, uint32_t occupied, float (*clo)[3], float (*chi)[3], float* box_out) {
  float blo[3], bhi[3];
  refit_box_reset(blo, bhi);
  double nlo[3] = {1e300, 1e300, 1e300}, nhi[3] = {-1e300, -1e300, -1e300};
  PRT_RUNROLL
  for (int s = 0; s < 8; s++) {
    if (!((occupied >> s) & 1u)) continue;
    refit_box_merge(blo, bhi, clo[s], chi[s]);
    refit_inflate(clo[s], chi[s]);
    for (int k = 0; k < 3; k++) {
      nlo[k] = (double)clo[s][k] < nlo[k] ? (double)clo[s][k] : nlo[k];
      nhi[k] = (double)chi[s][k] > nhi[k] ? (double)chi[s][k] : nhi[k];
    }
  }
  for (int k = 0; k < 3; k++) { box_out[k] = blo[k]; box_out[3 + k] = bhi[k]; }
  nd.px = (float)nlo[0]; nd.py = (float)nlo[1]; nd.pz = (float)nlo[2];
  const double p[3] = {(double)nd.px, (double)nd.py, (double)nd.pz};
  uint8_t e[3];
  for (int k = 0; k < 3; k++) e[k] = refit_grid_exponent(nhi[k] - p[k]);
  nd.ex = e[0]; nd.ey = e[1]; nd.ez = e[2];
  // (x - p) * 2^(127 - e) is the quotient (x - p) / 2^(e - 127) bit for bit: the scale is a power of two
  const double isc[3] = {refit_pow2(127 - (int)e[0]), refit_pow2(127 - (int)e[1]), refit_pow2(127 - (int)e[2])};
  PRT_RUNROLL
  for (int s = 0; s < 8; s++) {
    if (!((occupied >> s) & 1u)) continue;
    uint8_t q[6];
    for (int k = 0; k < 3; k++) {
      double l = __builtin_floor(((double)clo[s][k] - p[k]) * isc[k]);
      double h = __builtin_ceil(((double)chi[s][k] - p[k]) * isc[k]);
      l = l > 0.0 ? l : 0.0; l = l < 255.0 ? l : 255.0;  // min(255, max(0, x)), as std::min / std::max order them
      h = h > 0.0 ? h : 0.0; h = h < 255.0 ? h : 255.0;
      q[k] = (uint8_t)l;
      q[3 + k] = (uint8_t)h;
    }
    nd.qlox[s] = q[0]; nd.qloy[s] = q[1]; nd.qloz[s] = q[2];
    nd.qhix[s] = q[3]; nd.qhiy[s] = q[4]; nd.qhiz[s] = q[5];
  }
}

// one node, start to end: what the device kernel runs per lane and the host refit per node
PRT_RHD void refit_node8(Node8& nd, const TriMT* tris, const float* triangles, const float* boxes, float* box_out) {
  float clo[8][3], chi[8][3];
  uint32_t occupied = 0;
  PRT_RUNROLL
  for (int s = 0; s < 8; s++)
    if (refit_slot_box(nd, s, tris, triangles, boxes, clo[s], chi[s])) occupied |= 1u << s;
  refit_encode8(nd, occupied, clo, chi, box_out);
}

// The sequential host refit of one mesh's tree (offsets relative to the mesh, as the builders return them): records,
// then the nodes last to first -- every interior child has a larger index than its parent.  boxes: 6 floats per
// node (the root's, boxes[0..5], is the mesh's new bmin / bmax).
inline void refit_blas8(Node8* nodes, size_t n_nodes, TriMT* tris, size_t n_tris, const float* triangles, float* boxes) {
  for (size_t g = 0; g < n_tris; g++) refit_record(tris[g], triangles);
  for (size_t j = n_nodes; j-- > 0;) {
    Node8 nd = nodes[j];
    refit_node8(nd, tris, triangles, boxes, boxes + 6 * j);
    nodes[j] = nd;
  }
}

}  // namespace prt
