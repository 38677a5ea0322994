// prt_motion.h -- host-side launchers of the instance-id AOV and the motion-aware temporal reprojection pass
// (prt_motion.hip; include/prt.h prt_render_aov_ids / prt_reproject_motion, DESIGN.md "Moving instances").
#pragma once
#include <hip/hip_runtime.h>

#include "prt_launch.h"
#include "prt_temporal.h"

namespace prt {

// prt_reproject's pass (R, filled as for launch_reproject) with every pixel's first hit carried back by its
// instance's motion matrix before it is projected into the previous view
struct MotionPass {
  ReprojectPass R;
  const uint32_t* inst;       // this view's instance ids (a miss: 0xFFFFFFFF); read only when R.hist != nullptr
  const uint32_t* hist_inst;  // the previous view's ids; nullptr: taps are not compared by instance
  const float4* motion;       // count row-major 3 x 4 matrices prev * inverse(cur): three float4 rows each
  int32_t count;              // a hit pixel whose id is >= count starts over, no matrix is read for it
};

// HitOut of launch_primary_hits -> the first hit's instance index, 0xFFFFFFFF for a miss
hipError_t launch_aov_ids(hipStream_t s, int32_t W, int32_t H, const HitOut* hits, uint32_t* instance);
hipError_t launch_reproject_motion(hipStream_t s, const MotionPass& P);

}  // namespace prt
