// prt_tlas_refit_gpu.h -- launches of the device instance update (prt_tlas_refit.hip; the definition: prt_tlas_refit.h).
#pragma once
#include <hip/hip_runtime.h>

#include "prt_refit.h"
#include "prt_scene.h"

namespace prt {

// The per-instance table of a device-side record refill (prt_ctx::inst_tab): what an InstSrc holds besides its
// transform.  mesh / kind: one word per instance; mesh_box: two float4 per mesh, the BLAS root's lo.xyz and hi.xyz.
struct InstTabDev {
  const uint32_t* mesh;
  const uint32_t* kind;
  const float4* mesh_box;
  uint32_t nmesh;
};

// The refit input of n instances into out: instance i's transform is the four float4 at xf + stride4 * i (4: packed
// row-major 4x4 matrices; 6: the T of an InstSrc array), the rest comes from tab.  xf is 16-byte aligned; out may
// not overlap xf.
hipError_t launch_inst_src(hipStream_t s, const float4* xf, uint32_t stride4, const InstTabDev& tab, int32_t n,
                           InstSrc* out);

// One level of the instance BVH refit: the nodes order[0 .. n) of the tree src[0 .. n_nodes) with the slot table
// src_slot, whose interior children were refitted by an earlier launch, re-encoded over the instance records inst
// into dst / dst_slot (the same indices; dst may be src).  boxes: six floats per node of scratch.
hipError_t launch_tlas_refit_level(hipStream_t s, const Node8* src, const uint32_t* src_slot, Node8* dst,
                                   uint32_t* dst_slot, const InstDev* inst, uint32_t ninst, float* boxes,
                                   const uint32_t* order, uint32_t n, uint32_t n_nodes);

}  // namespace prt
