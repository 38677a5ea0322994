// prt_skin_gpu.h -- launch of the device skinning (prt_skin.hip; the definition: prt_skin.h).
#pragma once
#include <hip/hip_runtime.h>

#include "prt_scene.h"

namespace prt {

// joints whose matrices a block stages in LDS (12 KiB); a binding with more reads them through L2
constexpr int kSkinLdsJoints = 256;

// a bound mesh on the device: the binding's arrays, this call's matrices and the per-mesh scratch
struct SkinDev {
  const float* positions;   // 3 x V, bind pose
  const float* normals;     // 3 x V
  const uint2* joints;      // 4 x uint16 per vertex, one 8-byte load
  const float4* weights;    // 4 per vertex, one 16-byte load
  const int32_t* indices;   // 3 x T
  const float4* matrices;   // 3 x J (row-major 3 x 4 each), 16-byte aligned
  float4* vpos;             // scratch, V: (P', 0)
  float4* vnrm;             // scratch, V: (N', 0)
  float4* triangles;        // scratch, 3 x T: the fat triangles the refit's record and node passes read
  int32_t vertex_count, tri_count, joint_count;
};

// Skins the vertices, then writes every primitive's fat triangle into m.triangles and the words n[9], p[9], fn[3] of
// its ShadeTri (stri: the mesh's first; uv[6] and the pad words are kept).  Every joint < joint_count and every index
// < vertex_count (prt_set_mesh_skin checked them on the host).
hipError_t launch_skin_mesh(hipStream_t s, const SkinDev& m, ShadeTri* stri);

}  // namespace prt
