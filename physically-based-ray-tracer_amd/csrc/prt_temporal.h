// prt_temporal.h -- host-side launcher of the temporal reprojection pass
// (prt_temporal.hip; include/prt.h prt_reproject, DESIGN.md "Temporal reprojection").
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/prt.h"

namespace prt {

// one reprojection of a W x H float4 history onto this view (make_reproject_pass fills the camera terms)
struct ReprojectPass {
  int32_t W, H;
  float depth_tol, normal_min, max_history;
  float pos[3], tl[3], du[3], dv[3];          // this view: pos, TL, TR - TL, BL - TL
  float ppos[3], cuv[3], cv0[3], c0u[3], det;  // previous view: pos' and the constants of the definition
  const float4* color;    // this frame, w ignored
  const float4* nd;       // this view's normal_depth
  const float4* hist;     // previous out (rgb, w = history length); nullptr starts a history
  const float4* hist_nd;  // previous view's normal_depth
  float4* out;            // nullable; may be color, must not be hist / hist_nd (taps are gathered)
  uint32_t* rgb8;         // RGBF32_to_RGB8 of out (nullable)
};

// the camera terms of P in f32, in the order DESIGN.md writes them (prev may be null when there is no history)
void make_reproject_pass(ReprojectPass& P, const prt_camera& cam, const prt_camera* prev);
hipError_t launch_reproject(hipStream_t s, const ReprojectPass& P);

}  // namespace prt
