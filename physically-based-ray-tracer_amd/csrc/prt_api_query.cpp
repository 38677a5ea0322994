// prt_api_query.cpp -- ray queries on caller arrays (include/prt.h prt_query_rays / prt_query_surface): the persistent
// traversal engine and the kernels' hit_attributes on arrays in host or device memory, in the context stream's order.
// Host arrays go through the context's staging buffers (Staging, prt_ctx.h); with device arrays a call enqueues its
// kernels and returns.  prt_intersect / prt_occluded (prt_api.cpp ray_query) stay the lock-step reference.
#include "prt_ctx.h"

using namespace prt;
using namespace prt::host;

namespace {
constexpr int32_t kMaxQuery = 1 << 28;  // rays (records) of one call: both kinds of entry fit the 32-bit live range
}

int prt_query_rays(prt_ctx* c, int32_t n, const float* origins, const float* dirs, const float* tmax, prt_hit* hits,
                   int32_t* occluded, uint32_t io_flags) {
  if (!c || n < 0 || n > kMaxQuery || (io_flags & ~(uint32_t)PRT_OUT_DEVICE) || (!hits && !occluded) ||
      (n > 0 && (!origins || !dirs)))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad ray query arguments");
  if (n == 0) return PRT_OK;
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  SceneDev S;
  PRT_TRY(scene_ready(c, S));
  if (!depth_ok(c)) return fail(PRT_ERR_UNSUPPORTED, "BVH deeper than 64 levels");
  PRT_TRY(ensure_spill(c, S, 0));
  // the fetch counters: the context's, cleared in stream order (allocated by the context's first query)
  const size_t ctr_bytes = sizeof(uint32_t) * kParts * kCtrStride;
  HIP_TRY(c->q_ctr.ensure(ctr_bytes));
  HitOut* out = reinterpret_cast<HitOut*>(hits);
  Staging io(c, io_flags);
  PRT_TRY(io.in(c->q_in[0], origins, (size_t)n * 12));
  PRT_TRY(io.in(c->q_in[1], dirs, (size_t)n * 12));
  PRT_TRY(io.in(c->q_in[2], tmax, (size_t)n * 4));
  PRT_TRY(io.out(c->q_hits, out, (size_t)n * sizeof(HitOut)));
  PRT_TRY(io.out(c->q_occ, occluded, (size_t)n * 4));
  HIP_TRY(hipMemsetAsync(c->q_ctr.p, 0, ctr_bytes, c->stream));
  QueryArgs Q{};
  Q.O = origins;
  Q.D = dirs;
  Q.tmax = tmax;
  Q.hits = out;
  Q.occ = occluded;
  Q.fctr = c->q_ctr.as<uint32_t>();
  Q.nclosest = out ? (uint32_t)n : 0u;
  Q.total = Q.nclosest + (occluded ? (uint32_t)n : 0u);
  Q.coop_tail = read_tunables().coop_tail ? 1 : 0;
  const LaunchCfg L{c->stream, occ_for(c)};
  const hipError_t e = launch_query(L, S, Q);
  const int urc = record_inst_use(c, c->stream);  // a later instance update waits for this read, as for a frame
  if (e != hipSuccess) return fail(PRT_ERR_HIP, std::string("ray query: ") + hipGetErrorString(e));
  PRT_TRY(urc);
  return io.finish();
}

int prt_query_surface(prt_ctx* c, int32_t n, const prt_hit* hits, const float* tmax, uint32_t flags,
                      float* albedo_rgba, float* normal_depth, float* geometry_normal, float* material,
                      uint32_t io_flags) {
  if (!c || n < 0 || n > kMaxQuery || (io_flags & ~(uint32_t)PRT_OUT_DEVICE) || (n > 0 && !hits))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad surface query arguments");
  if (n == 0) return PRT_OK;
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  SceneDev S;
  PRT_TRY(scene_ready(c, S));
  if (!albedo_rgba && !normal_depth && !geometry_normal && !material) return PRT_OK;
  const HitOut* in = reinterpret_cast<const HitOut*>(hits);
  float4* a = reinterpret_cast<float4*>(albedo_rgba);
  float4* g = reinterpret_cast<float4*>(normal_depth);
  float4* gn = reinterpret_cast<float4*>(geometry_normal);
  float4* m = reinterpret_cast<float4*>(material);
  Staging io(c, io_flags);
  PRT_TRY(io.in(c->qs_in[0], in, (size_t)n * sizeof(HitOut)));
  PRT_TRY(io.in(c->qs_in[1], tmax, (size_t)n * 4));
  PRT_TRY(io.out(c->qs_out[0], a, (size_t)n * sizeof(float4)));
  PRT_TRY(io.out(c->qs_out[1], g, (size_t)n * sizeof(float4)));
  PRT_TRY(io.out(c->qs_out[2], gn, (size_t)n * sizeof(float4)));
  PRT_TRY(io.out(c->qs_out[3], m, (size_t)n * 2 * sizeof(float4)));
  const hipError_t e = launch_query_surface(c->stream, S, n, (flags & PRT_FLAG_NORMALMAP) != 0, in, tmax, a, g, gn, m);
  const int urc = record_inst_use(c, c->stream);
  if (e != hipSuccess) return fail(PRT_ERR_HIP, std::string("surface query: ") + hipGetErrorString(e));
  PRT_TRY(urc);
  return io.finish();
}
