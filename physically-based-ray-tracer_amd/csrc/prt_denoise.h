// prt_denoise.h -- host-side launchers of the first-hit AOV pass and the edge-avoiding a-trous filter
// (prt_denoise.hip; include/prt.h prt_render_aov / prt_denoise, DESIGN.md "Denoiser").
#pragma once
#include <hip/hip_runtime.h>

#include "prt_launch.h"

namespace prt {

// one a-trous iteration (step 2^i) over a W x H float4 image
struct DenoisePass {
  int32_t W, H;
  int32_t step;           // 2^i
  int32_t normal_power;   // the normal weight is squared this many times
  float sc2;              // (sigma_color * 2^-i)^2
  float sigma_depth;
  float sa2;              // sigma_albedo^2 (read only when albedo != nullptr)
  const float4* color;    // I_i: rgb, w carried through
  const float4* geo;      // unit normal, w = primary hit t (>= 1e30: miss); launch_denoise_prep
  const float4* albedo;   // nullptr: albedo is no guide (sigma_albedo == 0)
  float4* out;            // I_{i+1} (nullable in the last pass)
  uint32_t* rgb8;         // last pass: RGBF32_to_RGB8 of out (nullable)
};

// HitOut of launch_primary_hits -> albedo (base colour, w = 1; miss 0) and normal_depth (shading normal as Trace
// uses it, w = t; miss 0,0,0,1e30); either output may be null
hipError_t launch_aov(hipStream_t s, const SceneDev& S, int32_t W, int32_t H, bool normalmapped, const HitOut* hits,
                      float4* albedo, float4* normal_depth);
// geo = (N / |N|, Z) of normal_depth (a miss keeps 0,0,0,Z)
hipError_t launch_denoise_prep(hipStream_t s, int32_t W, int32_t H, const float4* normal_depth, float4* geo);
// P.out must not alias P.color
hipError_t launch_denoise_pass(hipStream_t s, const DenoisePass& P);

}  // namespace prt
