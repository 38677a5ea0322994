// prt_skin.h -- linear-blend skinning of a bound mesh (prt_set_mesh_skin / prt_skin_mesh): the definition.
//
// A mesh's bind pose (positions P, normals N, four joint indices j and four weights w per vertex, the corner
// indices) is bound once; every call brings J row-major 3 x 4 joint matrices M (a joint's world matrix times its
// inverse bind matrix, acting in the mesh's object space) and derives everything prt_update_mesh takes.  Every
// function here is __host__ __device__: the kernels (prt_skin.hip) and the plain host skin_mesh_host() below run the
// same code, compiled without FMA contraction (-ffp-contract=off) on both sides; every operation is one correctly
// rounded f32 operation in the order written, so the two produce the same bytes.
//
//   vertex v     B[r][c] = ((w0*M[j0][r][c] + w1*M[j1][r][c]) + w2*M[j2][r][c]) + w3*M[j3][r][c]   (12 entries)
//                P'_r = ((B[r][0]*P.x + B[r][1]*P.y) + B[r][2]*P.z) + B[r][3]
//                n_r  = (B[r][0]*N.x + B[r][1]*N.y) + B[r][2]*N.z
//                N'   = n * (1.0f / sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z))      prt_math.h's (tmpl8's) normalize
//                N'   = (0, 1, 0) if any component of it is not finite
//   primitive p  corners i_k = indices[3p + k]:  triangles[3p + k] = (P'[i_k], 0), fixed_normals[3p + k] =
//                (N'[i_k], 0), vertices = P', face_normals[p] = normalize(cross(P'[i_1] - P'[i_0], P'[i_2] - P'[i_0]))
//                with prt_math.h's cross and normalize, (0, 0, 0) if any component of it is not finite
//                (tests/deform.py, scenes._mesh_from_grid); fixed_uvs, the texture ids and the pad words stay
//
// The weights are used as given, never renormalised; a weight of 0 still names a joint that must be in range.  The
// normal goes through B's 3 x 3 part itself, not its inverse transpose: exact for rotations and uniform scales,
// approximate otherwise -- the choice prt_reproject_motion documents for its normals (include/prt.h).
// cross / normalize are restated here in prt_math.h's expression order (that header needs the HIP runtime; this one
// also compiles as plain C++ for tests/cpp/skin_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PRT_SHD __host__ __device__ inline
#else
#define PRT_SHD inline
#endif

namespace prt {

PRT_SHD bool skin_finite(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return (b & 0x7F800000u) != 0x7F800000u;
}

// prt_math.h normalize: v * (1 / sqrtf(dot(v, v))), dot = x*x + y*y + z*z left to right
PRT_SHD void skin_normalize(const float* v, float* out) {
  const float inv = 1.0f / __builtin_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  out[0] = v[0] * inv;
  out[1] = v[1] * inv;
  out[2] = v[2] * inv;
}

// The blended matrix of one vertex: m0..m3 are the vertex's four joint matrices (12 floats each), w its weights.
PRT_SHD void skin_blend(const float* m0, const float* m1, const float* m2, const float* m3, const float* w, float* B) {
  for (int e = 0; e < 12; e++) B[e] = ((w[0] * m0[e] + w[1] * m1[e]) + w[2] * m2[e]) + w[3] * m3[e];
}

// One vertex through its blended matrix: the skinned position and the unit normal ((0, 1, 0) when not finite).
PRT_SHD void skin_vertex(const float* B, const float* P, const float* N, float* Pout, float* Nout) {
  float n[3];
  for (int r = 0; r < 3; r++) {
    const float* b = B + 4 * r;
    Pout[r] = ((b[0] * P[0] + b[1] * P[1]) + b[2] * P[2]) + b[3];
    n[r] = (b[0] * N[0] + b[1] * N[1]) + b[2] * N[2];
  }
  skin_normalize(n, Nout);
  if (!(skin_finite(Nout[0]) && skin_finite(Nout[1]) && skin_finite(Nout[2]))) {
    Nout[0] = 0.0f;
    Nout[1] = 1.0f;
    Nout[2] = 0.0f;
  }
}

// One primitive's face normal from its three skinned corners ((0, 0, 0) when not finite).
PRT_SHD void skin_face_normal(const float* a, const float* b, const float* c, float* fn) {
  const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float x[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  skin_normalize(x, fn);
  if (!(skin_finite(fn[0]) && skin_finite(fn[1]) && skin_finite(fn[2]))) fn[0] = fn[1] = fn[2] = 0.0f;
}

// The sequential host skinning of one mesh.  In: the binding (positions / normals 3 x V, joints / weights 4 x V,
// indices 3 x T) and J x 12 matrices; every joint < J and every index < V (the caller checked).  Out: triangles and
// fixed_normals (12 x T floats each, w = 0), vertices (3 x V), face_normals (3 x T); nrm_tmp: 3 x V floats of scratch.
inline void skin_mesh_host(int32_t V, int32_t T, const float* positions, const float* normals, const int32_t* indices,
                           const uint16_t* joints, const float* weights, const float* M, float* triangles,
                           float* fixed_normals, float* vertices, float* face_normals, float* nrm_tmp) {
  for (size_t v = 0; v < (size_t)V; v++) {
    const uint16_t* j = joints + 4 * v;
    float B[12];
    skin_blend(M + 12 * (size_t)j[0], M + 12 * (size_t)j[1], M + 12 * (size_t)j[2], M + 12 * (size_t)j[3],
               weights + 4 * v, B);
    skin_vertex(B, positions + 3 * v, normals + 3 * v, vertices + 3 * v, nrm_tmp + 3 * v);
  }
  for (size_t p = 0; p < (size_t)T; p++) {
    const float* c[3];
    for (int k = 0; k < 3; k++) {
      const size_t i = (size_t)indices[3 * p + k];
      c[k] = vertices + 3 * i;
      for (int a = 0; a < 3; a++) {
        triangles[4 * (3 * p + k) + a] = c[k][a];
        fixed_normals[4 * (3 * p + k) + a] = nrm_tmp[3 * i + a];
      }
      triangles[4 * (3 * p + k) + 3] = 0.0f;
      fixed_normals[4 * (3 * p + k) + 3] = 0.0f;
    }
    skin_face_normal(c[0], c[1], c[2], face_normals + 3 * p);
  }
}

}  // namespace prt
