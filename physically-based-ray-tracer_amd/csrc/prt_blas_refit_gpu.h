// prt_blas_refit_gpu.h -- launches of the device BLAS refit (prt_blas_refit.hip; the definition: prt_blas_refit.h).
#pragma once
#include <hip/hip_runtime.h>

#include "prt_scene.h"

namespace prt {

// the six arrays of a prt_mesh in device memory
struct RefitMeshDev {
  const float* triangles;      // 3 x float4 per triangle
  const float* fixed_normals;  // 3 x float4 per triangle
  const float* fixed_uvs;      // 3 x float2 per triangle
  const int32_t* indices;      // 3 per triangle
  const float* vertices;       // 3 per vertex
  const float* face_normals;   // 3 per triangle
  int32_t tri_count, vertex_count;
};

// what an update leaves for the host: the mesh's new root box and the bad-index flag (28 bytes)
struct RefitResult {
  float bmin[3], bmax[3];
  uint32_t bad_index;  // some index was outside [0, vertex_count): vertex 0 was read in its place
};

// The record pass: the n_recs TriMT records from `tris` on (the mesh's leaf-order records) and the mesh's tri_count
// ShadeTri records from `stri` on.  res->bad_index must be zero beforehand (hipMemsetAsync in stream order).
hipError_t launch_refit_records(hipStream_t s, TriMT* tris, uint32_t n_recs, ShadeTri* stri, const RefitMeshDev& m,
                                RefitResult* res);
// One level of the node pass: the nodes order[0 .. n) (indices into nodes8), whose interior children were refitted
// by an earlier launch.  nodes8 / tris / boxes are the scene's concatenated arrays (child_base and tri_base index
// them as they are); the node `root` also leaves its box in res.
hipError_t launch_refit_level(hipStream_t s, Node8* nodes8, const TriMT* tris, const float* triangles, float* boxes,
                              const uint32_t* order, uint32_t n, uint32_t root, RefitResult* res);

}  // namespace prt
