// prt_api_image.cpp -- the image-space passes of the C ABI (include/prt.h): the a-trous denoisers and the temporal
// reprojections.  They read and write images only (no scene); host images go through the context's staging buffers
// (Staging, prt_ctx.h).
#include <cmath>
#include <cstring>

#include "prt_ctx.h"
#include "prt_deform.h"
#include "prt_denoise.h"
#include "prt_motion.h"
#include "prt_temporal.h"
#include "prt_variance.h"

using namespace prt;
using namespace prt::host;

int prt::host::dn_event(prt_ctx* c, int k) {
  if (!c->dn_ev[k]) HIP_TRY(hipEventCreate(&c->dn_ev[k]));
  HIP_TRY(hipEventRecord(c->dn_ev[k], c->stream));
  return PRT_OK;
}

namespace {

bool sigma_ok(float v, bool zero_ok) { return std::isfinite(v) && (zero_ok ? v >= 0.0f : v > 0.0f); }

bool size_ok(int32_t W, int32_t H) { return W > 0 && H > 0 && W <= 16384 && H <= 16384; }

// what the iterations of a filter call share: everything of a DenoisePass but step, sc2, color, out and rgb8
DenoisePass denoise_pass(int32_t W, int32_t H, int32_t normal_power, float sigma_depth, float sigma_albedo,
                         const float4* geo, const float4* albedo) {
  DenoisePass P{};
  P.W = W;
  P.H = H;
  P.normal_power = normal_power;
  P.sigma_depth = sigma_depth;
  P.sa2 = sigma_albedo * sigma_albedo;
  P.geo = geo;
  P.albedo = albedo;
  return P;
}

// ---- the three reprojections: prt_reproject is the core, prt_reproject_motion adds the motion group (id images and
// the instances' motion matrices), prt_reproject_moments adds the moments group on top of that; the pass structs nest
// the same way (MomentsPass > MotionPass > ReprojectPass); prt_reproject_deform is the moments level with an offset
// image and the previous transforms (DeformPass > MomentsPass)
enum ReprojectLevel { kCore = 0, kMotion = 1, kMoments = 2 };

bool reproject_params_ok(float depth_tol, float normal_min, float max_history) {
  return sigma_ok(depth_tol, true) && normal_min >= -1.0f && normal_min <= 1.0f && std::isfinite(max_history) &&
         max_history >= 1.0f;
}

// the core's pass over the caller's images (host or device pointers: reproject() stages them)
ReprojectPass reproject_pass(int32_t W, int32_t H, float depth_tol, float normal_min, float max_history,
                             const prt_camera* cam, const prt_camera* prev_cam, const float* color,
                             const float* normal_depth, const float* history, const float* history_nd, float* out_rgba,
                             uint32_t* out_rgb8) {
  ReprojectPass P{};
  P.W = W;
  P.H = H;
  P.depth_tol = depth_tol;
  P.normal_min = normal_min;
  P.max_history = max_history;
  make_reproject_pass(P, *cam, prev_cam);
  P.color = reinterpret_cast<const float4*>(color);
  P.nd = reinterpret_cast<const float4*>(normal_depth);
  P.hist = reinterpret_cast<const float4*>(history);
  P.hist_nd = reinterpret_cast<const float4*>(history_nd);
  P.out = reinterpret_cast<float4*>(out_rgba);
  P.rgb8 = out_rgb8;
  return P;
}

// the motion matrices, and with prev_xf (count row-major 4 x 4 transforms) their first three rows after them: copied
// into a pinned staging buffer now, uploaded in stream order (no host wait)
int upload_motion(prt_ctx* c, const float* motion, const float* prev_xf, int32_t count) {
  const size_t mb = 12 * sizeof(float) * (size_t)count, all = prev_xf ? 2 * mb : mb;
  HIP_TRY(c->rp_motion.ensure(all));
  StageSlot* st = nullptr;
  PRT_TRY(stage_acquire(c, all, st));
  std::memcpy(st->p, motion, mb);
  for (int32_t k = 0; prev_xf && k < count; k++)
    std::memcpy(static_cast<char*>(st->p) + mb + 48 * (size_t)k, prev_xf + 16 * (size_t)k, 48);
  HIP_TRY(hipMemcpyAsync(c->rp_motion.p, st->p, all, hipMemcpyHostToDevice, c->stream));
  return stage_release(c, *st, c->stream);
}

// After an entry point's argument checks: stage the images of the groups this level has, launch its kernel, copy
// back.  Q holds the caller's pointers (the groups above `level` unset); motion is null without a history.  offset
// and prev_xf (prt_reproject_deform: kMoments with a history, both or neither) select k_reproject_deform.
int reproject(prt_ctx* c, ReprojectLevel level, MomentsPass Q, const float* motion, uint32_t out_flags,
              const float* offset = nullptr, const float* prev_xf = nullptr) {
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  MotionPass& M = Q.M;
  ReprojectPass& R = M.R;
  const size_t n = (size_t)R.W * R.H, bytes = n * sizeof(float4);
  Staging io(c, out_flags);
  PRT_TRY(io.in(c->rp_in[0], R.color, bytes));
  PRT_TRY(io.in(c->rp_in[1], R.nd, bytes));
  PRT_TRY(io.in(c->rp_in[2], R.hist, bytes));
  PRT_TRY(io.in(c->rp_in[3], R.hist_nd, bytes));
  if (level >= kMotion) {
    PRT_TRY(io.in(c->rp_ids[0], M.inst, n * 4));
    PRT_TRY(io.in(c->rp_ids[1], M.hist_inst, n * 4));
  }
  if (level == kMoments) PRT_TRY(io.in(c->rp_mom[0], Q.hist_mom, bytes));
  PRT_TRY(io.in(c->rp_off, offset, bytes));
  PRT_TRY(io.out(c->rp_out, R.out, bytes));
  if (level == kMoments) PRT_TRY(io.out(c->rp_mom[1], Q.mom, bytes));
  PRT_TRY(io.out(c->rp_rgb8, R.rgb8, n * 4));
  if (motion) {
    PRT_TRY(upload_motion(c, motion, prev_xf, M.count));
    M.motion = c->rp_motion.as<float4>();
  }
  if (offset) {
    DeformPass D{Q, reinterpret_cast<const float4*>(offset), M.motion + 3 * (size_t)M.count};
    HIP_TRY(launch_reproject_deform(c->stream, D));
    return io.finish();
  }
  if (level == kCore) HIP_TRY(launch_reproject(c->stream, R));
  else if (level == kMotion) HIP_TRY(launch_reproject_motion(c->stream, M));
  else HIP_TRY(launch_reproject_moments(c->stream, Q));
  return io.finish();
}

}  // namespace

extern "C" {

// ---- the a-trous denoiser (prt_denoise.hip)
int prt_denoise_defaults(prt_denoise_params* out) {
  if (!out) return fail(PRT_ERR_INVALID_ARGUMENT, "out is NULL");
  out->iterations = 5;
  out->normal_power = 3;
  out->sigma_color = 4.0f;
  out->sigma_depth = 0.1f;
  out->sigma_albedo = 0.25f;
  return PRT_OK;
}

int prt_denoise(prt_ctx* c, const prt_denoise_params* p, int32_t W, int32_t H, const float* color, const float* albedo,
                const float* normal_depth, float* out_rgba, uint32_t* out_rgb8, uint32_t out_flags) {
  if (!c || !p || !color || !normal_depth || (!out_rgba && !out_rgb8) || !size_ok(W, H))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad denoise arguments");
  if (p->iterations < 1 || p->iterations > 8 || p->normal_power < 0 || p->normal_power > 7 ||
      !sigma_ok(p->sigma_color, false) || !sigma_ok(p->sigma_depth, false) || !sigma_ok(p->sigma_albedo, true))
    return fail(PRT_ERR_INVALID_ARGUMENT, "denoise parameters out of range");
  const bool use_albedo = p->sigma_albedo > 0.0f;
  if (use_albedo && !albedo) return fail(PRT_ERR_INVALID_ARGUMENT, "albedo is NULL with sigma_albedo > 0");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)W * H, bytes = n * sizeof(float4);
  const bool timed = (out_flags & PRT_OUT_TIMED) != 0;
  const float4* src[3] = {reinterpret_cast<const float4*>(color), reinterpret_cast<const float4*>(normal_depth),
                          use_albedo ? reinterpret_cast<const float4*>(albedo) : nullptr};
  float4* dst = reinterpret_cast<float4*>(out_rgba);
  uint32_t* dst8 = out_rgb8;
  Staging io(c, out_flags);
  for (int k = 0; k < 3; k++) PRT_TRY(io.in(c->dn_in[k], src[k], bytes));
  PRT_TRY(io.out(c->dn_out, dst, bytes));
  PRT_TRY(io.out(c->dn_rgb8, dst8, n * 4));
  HIP_TRY(c->dn_geo.ensure(bytes));
  if (p->iterations > 1 || dst == src[0]) {
    HIP_TRY(c->dn_pp[0].ensure(bytes));
    if (p->iterations > 2) HIP_TRY(c->dn_pp[1].ensure(bytes));
  }
  if (timed) PRT_TRY(dn_event(c, 2));
  HIP_TRY(launch_denoise_prep(c->stream, W, H, src[1], c->dn_geo.as<float4>()));
  if (timed) PRT_TRY(dn_event(c, 3));
  const float4* in = src[0];
  if (p->iterations == 1 && dst == in) {  // a single pass in place: filter a copy
    HIP_TRY(hipMemcpyAsync(c->dn_pp[0].p, in, bytes, hipMemcpyDeviceToDevice, c->stream));
    in = c->dn_pp[0].as<float4>();
  }
  DenoisePass P = denoise_pass(W, H, p->normal_power, p->sigma_depth, p->sigma_albedo, c->dn_geo.as<float4>(), src[2]);
  for (int32_t i = 0; i < p->iterations; i++) {
    const bool last = i == p->iterations - 1;
    const float sc = p->sigma_color * std::ldexp(1.0f, -i);
    P.step = 1 << i;
    P.sc2 = sc * sc;
    P.color = in;
    P.out = last ? dst : c->dn_pp[i & 1].as<float4>();
    P.rgb8 = last ? dst8 : nullptr;
    HIP_TRY(launch_denoise_pass(c->stream, P));
    if (timed) PRT_TRY(dn_event(c, 4 + i));
    in = P.out;
  }
  if (timed) c->dn_timed_passes = p->iterations;
  return io.finish();
}

int prt_denoise_timings(prt_ctx* c, float* ms, int32_t count) {
  if (!c || !ms || count < 1 || count > PRT_DENOISE_TIMINGS) return fail(PRT_ERR_INVALID_ARGUMENT, "bad timing arguments");
  PRT_JOIN(c);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float t[PRT_DENOISE_TIMINGS] = {};
  if (c->dn_timed_aov) HIP_TRY(hipEventElapsedTime(&t[0], c->dn_ev[0], c->dn_ev[1]));
  for (int32_t k = 0; c->dn_timed_passes > 0 && k < 1 + c->dn_timed_passes; k++)
    HIP_TRY(hipEventElapsedTime(&t[1 + k], c->dn_ev[2 + k], c->dn_ev[3 + k]));
  for (int32_t k = 0; k < count; k++) ms[k] = t[k];
  return PRT_OK;
}

// ---- temporal reprojection (prt_temporal.hip)
int prt_reproject_defaults(prt_reproject_params* out) {
  if (!out) return fail(PRT_ERR_INVALID_ARGUMENT, "out is NULL");
  out->depth_tol = 0.05f;
  out->normal_min = 0.9f;
  out->max_history = 16.0f;
  return PRT_OK;
}

int prt_reproject(prt_ctx* c, const prt_reproject_params* p, int32_t W, int32_t H, const prt_camera* cam,
                  const float* color, const float* normal_depth, const prt_camera* prev_cam, const float* history,
                  const float* history_nd, float* out_rgba, uint32_t* out_rgb8, uint32_t out_flags) {
  if (!c || !p || !cam || !color || !normal_depth || (!out_rgba && !out_rgb8) || !size_ok(W, H))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad reproject arguments");
  if (!reproject_params_ok(p->depth_tol, p->normal_min, p->max_history))
    return fail(PRT_ERR_INVALID_ARGUMENT, "reproject parameters out of range");
  const int given = (prev_cam ? 1 : 0) + (history ? 1 : 0) + (history_nd ? 1 : 0);
  if (given != 0 && given != 3)
    return fail(PRT_ERR_INVALID_ARGUMENT, "prev_camera, history_rgba and history_normal_depth go together");
  if (out_rgba && given && (out_rgba == history || out_rgba == history_nd))
    return fail(PRT_ERR_INVALID_ARGUMENT, "out_rgba must not be a history buffer");
  MomentsPass Q{};
  Q.M.R = reproject_pass(W, H, p->depth_tol, p->normal_min, p->max_history, cam, prev_cam, color, normal_depth, history,
                         history_nd, out_rgba, out_rgb8);
  return reproject(c, kCore, Q, nullptr, out_flags);
}

// ---- moving instances in the temporal reprojection (prt_motion.hip)
int prt_instance_motion(const float* transforms, const float* prev_transforms, int32_t count, float* motion) {
  if (count < 0 || (count > 0 && (!transforms || !prev_transforms || !motion)))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad instance motion arguments");
  static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int32_t k = 0; k < count; k++) {
    const float* T = transforms + 16 * (size_t)k;
    const float* Q = prev_transforms + 16 * (size_t)k;
    float* A = motion + 12 * (size_t)k;
    std::memcpy(A, kIdentity, sizeof(kIdentity));
    if (std::memcmp(T, Q, 16 * sizeof(float)) == 0) continue;  // at rest: the exact identity
    double m[3][3], t[3];
    bool finite = true;
    for (int r = 0; r < 3; r++) {
      for (int j = 0; j < 3; j++) m[r][j] = T[4 * r + j];
      t[r] = T[4 * r + 3];
      for (int j = 0; j < 4; j++) finite = finite && std::isfinite(T[4 * r + j]);
    }
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2],
                 c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    if (!finite || det == 0.0 || !std::isfinite(1.0 / det)) continue;  // no visible pixel: identity
    const double id = 1.0 / det;
    const double inv[3][3] = {
        {c00 * id, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id},
        {c01 * id, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id},
        {c02 * id, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id}};
    for (int r = 0; r < 3; r++) {  // A = [Mp * inv, tp - Mp * inv * t]
      double row[3], tr = Q[4 * r + 3];
      for (int j = 0; j < 3; j++) {
        row[j] = ((double)Q[4 * r] * inv[0][j] + (double)Q[4 * r + 1] * inv[1][j]) + (double)Q[4 * r + 2] * inv[2][j];
        tr -= row[j] * t[j];
      }
      for (int j = 0; j < 3; j++) A[4 * r + j] = (float)row[j];
      A[4 * r + 3] = (float)tr;
    }
  }
  return PRT_OK;
}

int prt_reproject_motion(prt_ctx* c, const prt_reproject_params* p, int32_t W, int32_t H, const prt_camera* cam,
                         const float* color, const float* normal_depth, const uint32_t* instance,
                         const prt_camera* prev_cam, const float* history, const float* history_nd,
                         const uint32_t* history_inst, const float* motion, int32_t count, float* out_rgba,
                         uint32_t* out_rgb8, uint32_t out_flags) {
  if (!c || !p || !cam || !color || !normal_depth || (!out_rgba && !out_rgb8) || !size_ok(W, H))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad reproject arguments");
  if (!reproject_params_ok(p->depth_tol, p->normal_min, p->max_history))
    return fail(PRT_ERR_INVALID_ARGUMENT, "reproject parameters out of range");
  const int given = (prev_cam ? 1 : 0) + (history ? 1 : 0) + (history_nd ? 1 : 0) + (motion ? 1 : 0) + (count ? 1 : 0);
  if (count < 0 || (given != 0 && given != 5) || (given == 0 && history_inst))
    return fail(PRT_ERR_INVALID_ARGUMENT,
                "prev_camera, history_rgba, history_normal_depth, motion and count > 0 go together");
  if (given && !instance) return fail(PRT_ERR_INVALID_ARGUMENT, "instance is NULL with a history");
  if (out_rgba && given && (out_rgba == history || out_rgba == history_nd))
    return fail(PRT_ERR_INVALID_ARGUMENT, "out_rgba must not be a history buffer");
  if (out_rgb8 && history_inst && out_rgb8 == history_inst)
    return fail(PRT_ERR_INVALID_ARGUMENT, "out_rgb8 must not be history_instance");
  MomentsPass Q{};
  Q.M.R = reproject_pass(W, H, p->depth_tol, p->normal_min, p->max_history, cam, prev_cam, color, normal_depth, history,
                         history_nd, out_rgba, out_rgb8);
  Q.M.inst = given ? instance : nullptr;  // the ids are read (and staged) only with a history
  Q.M.hist_inst = history_inst;
  Q.M.count = count;
  return reproject(c, kMotion, Q, motion, out_flags);
}

// ---- luminance moments and the variance-guided filter (prt_variance.hip)
int prt_temporal_defaults(prt_temporal_params* out) {
  if (!out) return fail(PRT_ERR_INVALID_ARGUMENT, "out is NULL");
  out->depth_tol = 0.05f;
  out->normal_min = 0.9f;
  out->max_history = 16.0f;
  out->clamp_k = 0.0f;
  out->min_temporal = 4.0f;
  return PRT_OK;
}

// prt_reproject_moments, and with offset and prev_xf prt_reproject_deform
static int reproject_moments(prt_ctx* c, const prt_temporal_params* p, int32_t W, int32_t H, const prt_camera* cam,
                             const float* color, const float* normal_depth, const uint32_t* instance,
                             const prt_camera* prev_cam, const float* history, const float* history_nd,
                             const uint32_t* history_inst, const float* motion, int32_t count,
                             const float* history_mom, const float* offset, const float* prev_xf, float* out_rgba,
                             float* out_mom, uint32_t* out_rgb8, uint32_t out_flags) {
  if (!c || !p || !cam || !color || !normal_depth || !instance || !out_mom || (!out_rgba && !out_rgb8) ||
      !size_ok(W, H))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad reproject arguments");
  if (!reproject_params_ok(p->depth_tol, p->normal_min, p->max_history) || !sigma_ok(p->clamp_k, true) ||
      !std::isfinite(p->min_temporal) || p->min_temporal < 1.0f)
    return fail(PRT_ERR_INVALID_ARGUMENT, "temporal parameters out of range");
  const int given = (prev_cam ? 1 : 0) + (history ? 1 : 0) + (history_nd ? 1 : 0) + (motion ? 1 : 0) +
                    (count ? 1 : 0) + (history_mom ? 1 : 0);
  if (count < 0 || (given != 0 && given != 6) || (given == 0 && history_inst))
    return fail(PRT_ERR_INVALID_ARGUMENT,
                "prev_camera, history_rgba, history_normal_depth, motion, count > 0 and history_moments go together");
  if ((offset != nullptr) != (prev_xf != nullptr) || (offset && !given))
    return fail(PRT_ERR_INVALID_ARGUMENT, "offset and prev_transforms go together, and with a history");
  if (offset && (static_cast<const void*>(offset) == out_rgba || static_cast<const void*>(offset) == out_mom))
    return fail(PRT_ERR_INVALID_ARGUMENT, "offset must not be an output");
  if (out_rgba == color)  // the clamp and the spatial estimate read the neighbours of color_rgba
    return fail(PRT_ERR_INVALID_ARGUMENT, "out_rgba must not be color_rgba");
  if (out_rgba && (out_rgba == normal_depth || out_rgba == out_mom ||
                   (given && (out_rgba == history || out_rgba == history_nd || out_rgba == history_mom))))
    return fail(PRT_ERR_INVALID_ARGUMENT, "out_rgba must not be an input or out_moments");
  if (out_mom == color || out_mom == normal_depth ||
      (given && (out_mom == history_mom || out_mom == history || out_mom == history_nd)))
    return fail(PRT_ERR_INVALID_ARGUMENT, "out_moments must not be an input");
  if (out_rgb8 && (out_rgb8 == instance || (history_inst && out_rgb8 == history_inst)))
    return fail(PRT_ERR_INVALID_ARGUMENT, "out_rgb8 must not be an instance buffer");
  MomentsPass Q{};
  Q.M.R = reproject_pass(W, H, p->depth_tol, p->normal_min, p->max_history, cam, prev_cam, color, normal_depth, history,
                         history_nd, out_rgba, out_rgb8);
  Q.M.inst = instance;
  Q.M.hist_inst = history_inst;
  Q.M.count = count;
  Q.hist_mom = reinterpret_cast<const float4*>(history_mom);
  Q.mom = reinterpret_cast<float4*>(out_mom);
  Q.clamp_k = p->clamp_k;
  Q.min_temporal = p->min_temporal;
  return reproject(c, kMoments, Q, motion, out_flags, offset, prev_xf);
}

int prt_reproject_moments(prt_ctx* c, const prt_temporal_params* p, int32_t W, int32_t H, const prt_camera* cam,
                          const float* color, const float* normal_depth, const uint32_t* instance,
                          const prt_camera* prev_cam, const float* history, const float* history_nd,
                          const uint32_t* history_inst, const float* motion, int32_t count, const float* history_mom,
                          float* out_rgba, float* out_mom, uint32_t* out_rgb8, uint32_t out_flags) {
  return reproject_moments(c, p, W, H, cam, color, normal_depth, instance, prev_cam, history, history_nd, history_inst,
                           motion, count, history_mom, nullptr, nullptr, out_rgba, out_mom, out_rgb8, out_flags);
}

// ---- deforming meshes in the reprojection (prt_deform.hip; prt_snapshot_mesh: prt_api_mesh.cpp, prt_render_aov_deform:
// prt_api.cpp)
int prt_reproject_deform(prt_ctx* c, const prt_temporal_params* p, int32_t W, int32_t H, const prt_camera* cam,
                         const float* color, const float* normal_depth, const uint32_t* instance,
                         const prt_camera* prev_cam, const float* history, const float* history_nd,
                         const uint32_t* history_inst, const float* motion, int32_t count, const float* history_mom,
                         const float* offset, const float* prev_transforms, float* out_rgba, float* out_mom,
                         uint32_t* out_rgb8, uint32_t out_flags) {
  return reproject_moments(c, p, W, H, cam, color, normal_depth, instance, prev_cam, history, history_nd, history_inst,
                           motion, count, history_mom, offset, prev_transforms, out_rgba, out_mom, out_rgb8, out_flags);
}

int prt_denoise_variance_defaults(prt_denoise_variance_params* out) {
  if (!out) return fail(PRT_ERR_INVALID_ARGUMENT, "out is NULL");
  out->iterations = 5;
  out->normal_power = 3;
  out->sigma_color = 2.0f;
  out->sigma_depth = 0.1f;
  out->sigma_albedo = 0.25f;
  out->color_decay = 1.0f;
  out->variance_floor = 1e-6f;
  return PRT_OK;
}

int prt_denoise_variance(prt_ctx* c, const prt_denoise_variance_params* p, int32_t W, int32_t H, const float* color,
                         const float* moments, const float* albedo, const float* normal_depth, float* out_rgba,
                         float* out_variance, uint32_t* out_rgb8, uint32_t out_flags) {
  if (!c || !p || !color || !moments || !normal_depth || (!out_rgba && !out_rgb8) || !size_ok(W, H))
    return fail(PRT_ERR_INVALID_ARGUMENT, "bad denoise arguments");
  if (p->iterations < 1 || p->iterations > 8 || p->normal_power < 0 || p->normal_power > 7 ||
      !sigma_ok(p->sigma_color, false) || !sigma_ok(p->sigma_depth, false) || !sigma_ok(p->sigma_albedo, true) ||
      !sigma_ok(p->color_decay, false) || !sigma_ok(p->variance_floor, false))
    return fail(PRT_ERR_INVALID_ARGUMENT, "denoise parameters out of range");
  const bool use_albedo = p->sigma_albedo > 0.0f;
  if (use_albedo && !albedo) return fail(PRT_ERR_INVALID_ARGUMENT, "albedo is NULL with sigma_albedo > 0");
  PRT_JOIN(c);  // frames in flight complete first (prt_set_frames_in_flight)
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)W * H, bytes = n * sizeof(float4);
  const bool timed = (out_flags & PRT_OUT_TIMED) != 0;
  const float4* src[3] = {reinterpret_cast<const float4*>(color), reinterpret_cast<const float4*>(normal_depth),
                          use_albedo ? reinterpret_cast<const float4*>(albedo) : nullptr};
  const float4* mom = reinterpret_cast<const float4*>(moments);
  float4* dst = reinterpret_cast<float4*>(out_rgba);
  float* dstv = out_variance;
  uint32_t* dst8 = out_rgb8;
  Staging io(c, out_flags);
  for (int k = 0; k < 3; k++) PRT_TRY(io.in(c->dn_in[k], src[k], bytes));
  PRT_TRY(io.in(c->dn_mom, mom, bytes));
  PRT_TRY(io.out(c->dn_out, dst, bytes));
  PRT_TRY(io.out(c->dn_var, dstv, n * 4));
  PRT_TRY(io.out(c->dn_rgb8, dst8, n * 4));
  HIP_TRY(c->dn_geo.ensure(bytes));
  HIP_TRY(c->dn_pp[0].ensure(bytes));  // (rgb, V): iteration i reads dn_pp[i & 1]
  if (p->iterations > 1) HIP_TRY(c->dn_pp[1].ensure(bytes));
  if (timed) PRT_TRY(dn_event(c, 2));
  HIP_TRY(launch_denoise_var_prep(c->stream, W, H, src[1], src[0], mom, c->dn_geo.as<float4>(),
                                  c->dn_pp[0].as<float4>()));
  if (timed) PRT_TRY(dn_event(c, 3));
  float sc = p->sigma_color;
  VarDenoisePass Q{};
  Q.D = denoise_pass(W, H, p->normal_power, p->sigma_depth, p->sigma_albedo, c->dn_geo.as<float4>(), src[2]);
  Q.variance_floor = p->variance_floor;
  for (int32_t i = 0; i < p->iterations; i++) {
    const bool last = i == p->iterations - 1;
    DenoisePass& P = Q.D;
    P.step = 1 << i;
    P.sc2 = sc * sc;
    P.color = c->dn_pp[i & 1].as<float4>();
    P.out = last ? dst : c->dn_pp[(i + 1) & 1].as<float4>();
    P.rgb8 = last ? dst8 : nullptr;
    Q.restore = last ? src[0] : nullptr;
    Q.variance = last ? dstv : nullptr;
    HIP_TRY(launch_denoise_var_pass(c->stream, Q));
    if (timed) PRT_TRY(dn_event(c, 4 + i));
    sc = sc * p->color_decay;
  }
  if (timed) c->dn_timed_passes = p->iterations;
  return io.finish();
}

}  // extern "C"
