// prt_variance.h -- host-side launchers of the reprojection pass that carries luminance moments and of the
// variance-guided a-trous filter (prt_variance.hip; include/prt.h prt_reproject_moments / prt_denoise_variance,
// DESIGN.md "Variance guidance").
#pragma once
#include <hip/hip_runtime.h>

#include "prt_denoise.h"
#include "prt_motion.h"

namespace prt {

// prt_reproject_motion's pass (M, filled as for launch_reproject_motion; M.inst is always read here) with the
// luminance moments gathered and blended next to the colour, a variance estimate and an optional clamp of the history
struct MomentsPass {
  MotionPass M;
  const float4* hist_mom;  // previous out_moments; read only when M.R.hist != nullptr
  float4* mom;             // out: (m1, m2, variance, 0)
  float clamp_k;           // 0: the 3 x 3 window of M.R.color is not read
  float min_temporal;      // history length from which the temporal variance is used
};

// one variance-guided a-trous iteration over a W x H image whose w holds the variance
struct VarDenoisePass {
  DenoisePass D;           // D.color / D.out: (rgb, V); D.sc2 = sc_i^2
  float variance_floor;
  const float4* restore;   // last pass: the image whose w D.out receives; earlier passes: nullptr, out.w = V_{i+1}
  float* variance;         // last pass: V_{i+1} per pixel (nullable)
};

// M.R.out must not alias M.R.color (the clamp and the spatial estimate read its neighbours)
hipError_t launch_reproject_moments(hipStream_t s, const MomentsPass& P);
// geo as launch_denoise_prep, and iv = (color.rgb, moments.z)
hipError_t launch_denoise_var_prep(hipStream_t s, int32_t W, int32_t H, const float4* normal_depth,
                                   const float4* color, const float4* moments, float4* geo, float4* iv);
// P.D.out must not alias P.D.color
hipError_t launch_denoise_var_pass(hipStream_t s, const VarDenoisePass& P);

}  // namespace prt
