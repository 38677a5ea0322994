// prt_deform.h -- host-side launchers of the passes that let the temporal reprojection follow a deforming mesh
// (prt_deform.hip; include/prt.h prt_snapshot_mesh / prt_render_aov_deform / prt_reproject_deform, DESIGN.md
// "Deforming meshes").
#pragma once
#include <hip/hip_runtime.h>

#include "prt_launch.h"
#include "prt_scene.h"
#include "prt_variance.h"

namespace prt {

// prt_reproject_moments' pass (Q, filled as for launch_reproject_moments) with the point carried back displaced by
// the pixel's object-space offset under the instance's previous transform
struct DeformPass {
  MomentsPass Q;
  const float4* offset;  // this view's launch_aov_deform output: (delta, 1), or (0, 0, 0, 0) where nothing is known
  const float4* prev_l;  // Q.M.count x three float4 rows: xyz = the previous transform's upper-left 3 x 3 (w unread)
};

// snap[9 p + k] = stri[p].p[k] for the tris primitives of one mesh (stri: the mesh's first ShadeTri)
hipError_t launch_snapshot_mesh(hipStream_t s, const ShadeTri* stri, uint32_t tris, float* snap);
// HitOut of launch_primary_hits -> the interpolated displacement from the hit primitive's current corners to the
// snapshotted ones.  snaps: one pointer per mesh, nullptr = the mesh has no snapshot; snaps itself may be nullptr.
hipError_t launch_aov_deform(hipStream_t s, const SceneDev& S, int32_t W, int32_t H, const HitOut* hits,
                             const float* const* snaps, float4* offset);
// P.Q.M.R.hist, P.offset and P.prev_l must be set; P.Q.M.R.out must not alias P.Q.M.R.color
hipError_t launch_reproject_deform(hipStream_t s, const DeformPass& P);

}  // namespace prt
