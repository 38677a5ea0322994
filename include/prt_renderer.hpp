// prt_renderer.hpp -- C++ host mirror of the reference's Renderer / Scene / Camera API surface
// (Core/Renderer.h:12-112, Core/Scene.h:12-80, Core/Camera.h:11-37, Core/Model.h:36-44) on top of the C ABI
// in prt.h.  Header-only C++17; link libprt.so.  The names and meanings of the public members follow the
// reference so a Renderer::Tick port reads like the original; the hot path (Tick's pixel loop +
// Renderer::Trace, Core/Renderer.cpp:43-141,150-406) runs on the GPU through prt_render().
//
// Differences from the reference, all outside the hot path: the Scene is filled by the caller (the
// reference's assimp / JSON loading, Core/Scene.cpp:10-28,279-340, stays where it is), physics and UI
// are not part of this header, and errors surface as prt::Error exceptions instead of crashes.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "prt.h"

namespace prt {

class Error : public std::runtime_error {
 public:
  Error(int code, const std::string& what) : std::runtime_error(what), code(code) {}
  int code;
};

inline void check(int rc) {
  if (rc != PRT_OK) throw Error(rc, std::string("prt error ") + std::to_string(rc) + ": " + prt_last_error());
}

// Model (Core/Model.h:36-44): the fat per-corner arrays the hot path reads, owned here.
struct Model {
  std::vector<float> triangles;           // float4 x 3T (Model::triangles)
  std::vector<float> fixedNormals;        // float4 x 3T
  std::vector<float> fixedTextureCoords;  // float2 x 3T
  std::vector<int32_t> indices;           // 3T
  std::vector<float> vertices;            // float3 x V
  std::vector<float> faceNormals;         // float3 x T
  int32_t albedoTexture = -1, normalTexture = -1, metalnessTexture = -1, emissionTexture = -1;  // Scene::textures ids
  int32_t TriCount() const { return (int32_t)(indices.size() / 3); }
};

// A model's skin (prt_set_mesh_skin): the bind pose and, per vertex, four joints and four weights; the corner indices
// are the model's own
struct Skin {
  std::vector<float> positions;   // float3 x V, bind pose
  std::vector<float> normals;     // float3 x V
  std::vector<uint16_t> joints;   // 4 x V
  std::vector<float> weights;     // 4 x V
  int32_t jointCount = 0;
};

// Surface (template/surface.h:49-94): packed 0x00RRGGBB pixels
struct Texture {
  int32_t width = 0, height = 0;
  std::vector<uint32_t> pixels;
};

// GameObject + BLASInstance (Core/GameObject.h, Core/tiny_bvh.h:1243-1256): row-major 4x4 and model index
struct GameObject {
  std::array<float, 16> transform{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  uint32_t modelIndex = 0;
  int32_t material = PRT_MAT_TEXTURED;  // the model index Scene.cpp:193-205 should have tested: DIELECTRIC / MIRROR
};

class Scene {
 public:
  std::vector<Model> models;
  std::vector<Texture> textures;
  std::vector<GameObject> gameobjects;
  prt_lights lights{};              // Renderer point-light SoA + directionalLights[0] + spotlights[0]
  std::vector<float> skyPixels;     // Camera::skyPixels, float RGB equirect (empty = no sky)
  int32_t skyWidth = 0, skyHeight = 0;
  std::vector<prt_area_light> areaLights;  // Scene::areaLights (Core/AreaLight.h): at most one, sampled with MIS
  std::map<int32_t, Skin> skins;           // model index -> its skin (SetSkin); Upload binds them again

  // everything the hot path reads, copied to HBM (Scene::Init + BuildTLAS, Core/Scene.cpp:10-28,220-223)
  void Upload(prt_ctx* ctx) const {
    std::vector<prt_texture> tex;
    for (const Texture& t : textures) tex.push_back({t.width, t.height, t.pixels.data()});
    check(prt_set_textures(ctx, tex.data(), (int32_t)tex.size()));
    std::vector<prt_mesh> ms;
    for (const Model& m : models) {
      prt_mesh d{};
      d.tri_count = m.TriCount();
      d.vertex_count = (int32_t)(m.vertices.size() / 3);
      d.triangles = m.triangles.data();
      d.fixed_normals = m.fixedNormals.data();
      d.fixed_uvs = m.fixedTextureCoords.data();
      d.indices = m.indices.data();
      d.vertices = m.vertices.data();
      d.face_normals = m.faceNormals.data();
      d.albedo_tex = m.albedoTexture;
      d.normal_tex = m.normalTexture;
      d.metalness_tex = m.metalnessTexture;
      d.emission_tex = m.emissionTexture;
      ms.push_back(d);
    }
    check(prt_set_meshes(ctx, ms.data(), (int32_t)ms.size()));
    UploadInstances(ctx);
    check(prt_set_lights(ctx, &lights));
    check(prt_set_area_lights(ctx, areaLights.empty() ? nullptr : areaLights.data(), (int32_t)areaLights.size()));
    check(prt_set_sky(ctx, skyPixels.empty() ? nullptr : skyPixels.data(), skyWidth, skyHeight));
    for (const auto& kv : skins) BindSkin(ctx, kv.first, kv.second);  // (prt_set_meshes discarded the bindings)
  }
  // models[index] is skinned from now on: the scene keeps `skin` and the device takes it (prt_set_mesh_skin; ctx may
  // be null before the first Upload, which binds every kept skin).  Renderer::SkinModel then poses the model.
  void SetSkin(prt_ctx* ctx, int32_t index, Skin skin) {
    if (ctx) BindSkin(ctx, index, skin);
    skins[index] = std::move(skin);
  }
  void RemoveSkin(prt_ctx* ctx, int32_t index) {
    if (ctx) check(prt_set_mesh_skin(ctx, index, nullptr));
    skins.erase(index);
  }
  void BindSkin(prt_ctx* ctx, int32_t index, const Skin& k) const {
    const Model& m = models.at((size_t)index);
    prt_skin d{};
    d.vertex_count = (int32_t)(k.positions.size() / 3);
    d.tri_count = m.TriCount();
    d.joint_count = k.jointCount;
    d.positions = k.positions.data();
    d.normals = k.normals.data();
    d.indices = m.indices.data();
    d.joints = k.joints.data();
    d.weights = k.weights.data();
    if (k.normals.size() != k.positions.size() || k.joints.size() != 4 * (size_t)d.vertex_count ||
        k.weights.size() != k.joints.size())
      throw Error(PRT_ERR_INVALID_ARGUMENT, "Skin: positions, normals, joints and weights differ in vertex count");
    check(prt_set_mesh_skin(ctx, index, &d));
  }
  // models[index] was deformed in place (same topology): its arrays go to the device and its BLAS is refitted there
  // (prt_update_mesh); the instance boxes and the instance BVH follow at the next frame
  void UpdateModel(prt_ctx* ctx, int32_t index) const {
    const prt_mesh d = MeshDesc(index);
    check(prt_update_mesh(ctx, index, &d, 0));
  }
  // the same with a fresh device build of the model's BLAS in place of the refit (prt_rebuild_mesh; builder:
  // PRT_BUILDER_GPU_LBVH or PRT_BUILDER_GPU_PLOC): what brings back the tree quality a long deformation cost
  void RebuildModel(prt_ctx* ctx, int32_t index, int32_t builder = PRT_BUILDER_GPU_PLOC) const {
    const prt_mesh d = MeshDesc(index);
    check(prt_rebuild_mesh(ctx, index, &d, 0, builder));
  }
  prt_mesh MeshDesc(int32_t index) const {
    const Model& m = models.at((size_t)index);
    prt_mesh d{};
    d.tri_count = m.TriCount();
    d.vertex_count = (int32_t)(m.vertices.size() / 3);
    d.triangles = m.triangles.data();
    d.fixed_normals = m.fixedNormals.data();
    d.fixed_uvs = m.fixedTextureCoords.data();
    d.indices = m.indices.data();
    d.vertices = m.vertices.data();
    d.face_normals = m.faceNormals.data();
    d.albedo_tex = m.albedoTexture;
    d.normal_tex = m.normalTexture;
    d.metalness_tex = m.metalnessTexture;
    d.emission_tex = m.emissionTexture;
    return d;
  }
  // GameObject::Synchronise moved an instance: new transforms, TLAS rebuilt (Core/Renderer.cpp:33-41)
  void UploadInstances(prt_ctx* ctx) const {
    std::vector<float> xf;
    std::vector<uint32_t> mi;
    std::vector<int32_t> mat;
    bool any = false;
    for (const GameObject& g : gameobjects) {
      xf.insert(xf.end(), g.transform.begin(), g.transform.end());
      mi.push_back(g.modelIndex);
      mat.push_back(g.material);
      any = any || g.material != PRT_MAT_TEXTURED;
    }
    check(prt_set_instances(ctx, xf.data(), mi.data(), (int32_t)mi.size()));
    check(prt_set_instance_materials(ctx, any ? mat.data() : nullptr, any ? (int32_t)mat.size() : 0));
  }
  // the game objects moved (the same objects, models and materials): their transforms alone go to the device, where
  // the instance BVH is refitted (prt_update_instances) -- no host build, no wait for the GPU
  void UpdateInstances(prt_ctx* ctx) const {
    std::vector<float> xf;
    for (const GameObject& g : gameobjects) xf.insert(xf.end(), g.transform.begin(), g.transform.end());
    check(prt_update_instances(ctx, xf.data(), (int32_t)gameobjects.size(), 0u));
  }
  // the same with a fresh device build of the instance BVH in place of the refit (prt_rebuild_instances; builder:
  // PRT_BUILDER_GPU_LBVH or PRT_BUILDER_GPU_PLOC)
  void RebuildInstances(prt_ctx* ctx, int32_t builder = PRT_BUILDER_GPU_PLOC) const {
    std::vector<float> xf;
    for (const GameObject& g : gameobjects) xf.insert(xf.end(), g.transform.begin(), g.transform.end());
    check(prt_rebuild_instances(ctx, xf.data(), (int32_t)gameobjects.size(), 0u, builder));
  }
};

// Camera (Core/Camera.h:11-31): position, target, the screen plane GetPrimaryRay interpolates, its basis
// and the post-process members (defaults of Camera.h; read when Renderer::isPostProcessed is set)
class Camera {
 public:
  float camPos[3] = {0, 0, -1}, camTarget[3] = {0, 0, 0};
  float aspect = 1.0f;
  float topLeft[3] = {}, topRight[3] = {}, bottomLeft[3] = {};
  float right[3] = {}, up[3] = {}, ahead[3] = {};
  float colorGrading[4] = {1.f, 1.f, 1.f, 1.f};
  float fov = 40.f, distortion = 40.f, vignetteIntensity = 20.f, vignetteRadius = 0.3f;
  int32_t abberationIntensity = 0;

  Camera() = default;
  Camera(const float pos[3], const float target[3], float aspect_) : aspect(aspect_) {
    for (int k = 0; k < 3; k++) { camPos[k] = pos[k]; camTarget[k] = target[k]; }
    Update();
  }
  // the basis of Camera::Camera / HandleInput (Core/Camera.cpp:29-36)
  void Update() {
    prt_camera c{};
    check(prt_camera_look_at(camPos, camTarget, aspect, &c));
    for (int k = 0; k < 3; k++) {
      topLeft[k] = c.top_left[k]; topRight[k] = c.top_right[k]; bottomLeft[k] = c.bottom_left[k];
      right[k] = c.right[k]; up[k] = c.up[k]; ahead[k] = c.ahead[k];
    }
  }
  prt_camera Plane() const {
    prt_camera c{};
    for (int k = 0; k < 3; k++) {
      c.pos[k] = camPos[k]; c.top_left[k] = topLeft[k]; c.top_right[k] = topRight[k]; c.bottom_left[k] = bottomLeft[k];
      c.right[k] = right[k]; c.up[k] = up[k]; c.ahead[k] = ahead[k];
    }
    return c;
  }
  prt_postfx PostFx(bool enabled) const {
    prt_postfx p{};
    p.enabled = enabled ? 1 : 0;
    p.aberration = abberationIntensity;
    p.fov = fov; p.distortion = distortion;
    p.vignette_intensity = vignetteIntensity; p.vignette_radius = vignetteRadius;
    for (int k = 0; k < 4; k++) p.color_grading[k] = colorGrading[k];
    return p;
  }
};

// Renderer (Core/Renderer.h:12-112): the public switches of the reference and Tick()
class Renderer {
 public:
  enum class RENDER_STATES { BRDF, BASECOLOR, GEOMETRYNORMAL, SHADINGNORMAL, METAL, ROUGHNESS, EMMISIVE };

  bool accumulates = true;
  int bounces = 2;
  RENDER_STATES renderingMode = RENDER_STATES::BRDF;
  bool LIGHTED = true, GAMMACORRECTED = true, NORMALMAPPED = true, SKYBOX = true, AA = true, isStochastic = true;
  bool isPostProcessed = false;

  Scene scene;
  Camera camera;
  std::vector<float> accumulator;  // float4 x W*H: accumulator / samplesPerPixel (the displayed average)
  std::vector<uint32_t> screen;    // 0x00RRGGBB x W*H (RGBF32_to_RGB8 of the average)

  Renderer(int32_t width, int32_t height, int32_t device = 0) : width_(width), height_(height) {
    prt_device_desc d{device, 0};
    check(prt_create(&d, &ctx_));
    accumulator.assign(4 * (size_t)width * height, 0.0f);
    screen.assign((size_t)width * height, 0u);
  }
  // One process, several GPUs (prt_create_group): pixel tiles of tile x tile rendered concurrently on the
  // devices (a device may repeat), gathered on devices[0]; accumulator / screen hold the whole frame.
  Renderer(int32_t width, int32_t height, const std::vector<int32_t>& devices, int32_t tile = 32)
      : width_(width), height_(height) {
    std::vector<prt_device_desc> d;
    for (int32_t dev : devices) d.push_back(prt_device_desc{dev, 0});
    check(prt_create_group(d.data(), (int32_t)d.size(), tile, &ctx_));
    accumulator.assign(4 * (size_t)width * height, 0.0f);
    screen.assign((size_t)width * height, 0u);
  }
  // One process per GPU: rank 0 calls UniqueId(), the host program carries the bytes to the other ranks
  // (MPI, a socket, a file), and every rank calls JoinRccl before Init().  Tick() then renders this rank's
  // tiles and gathers the frame on rank 0 (accumulator / screen are filled on rank 0 only).
  static std::vector<uint8_t> UniqueId() {
    std::vector<uint8_t> id(PRT_SHARD_ID_BYTES);
    check(prt_shard_unique_id(id.data()));
    return id;
  }
  void JoinRccl(const std::vector<uint8_t>& id, int32_t rank, int32_t world, int32_t tile = 32) {
    if (id.size() != PRT_SHARD_ID_BYTES) throw Error(PRT_ERR_INVALID_ARGUMENT, "RCCL id must be 128 bytes");
    check(prt_shard_init_rccl(ctx_, id.data(), rank, world, tile));
  }
  ~Renderer() { prt_destroy(ctx_); }
  Renderer(const Renderer&) = delete;
  Renderer& operator=(const Renderer&) = delete;

  // Renderer::Init (Core/Renderer.cpp:7-16): scene + camera to the device, fresh accumulation state
  void Init() {
    scene.Upload(ctx_);
    const prt_camera c = camera.Plane();
    check(prt_set_camera(ctx_, &c));
    check(prt_reset_accumulation(ctx_, 1));
    frame_ = 0;
  }

  // Renderer::Tick (Core/Renderer.cpp:22-148): `frames` reference frames (2 camera paths per pixel each
  // with AA) folded into the progressive accumulator; accumulator / screen hold the result afterwards
  void Tick(float deltaTime = 0.0f, int32_t frames = 1) {
    (void)deltaTime;
    prt_render_params p{};
    p.width = width_;
    p.height = height_;
    p.spp = frames * (AA ? 2 : 1);
    p.bounces = bounces;
    p.flags = Flags();
    p.render_mode = (int32_t)renderingMode;
    p.frame_index = frame_;
    p.seed = 0;
    const prt_postfx pf = camera.PostFx(isPostProcessed);
    check(prt_set_postfx(ctx_, &pf));
    check(prt_render(ctx_, &p, accumulator.data(), screen.data(), 0u, &stats_));
    if (stats_.stack_overflows)  // a dropped traversal stack group may have lost hits (prt_stats)
      throw Error(PRT_ERR_HIP, "traversal stack overflow: " + std::to_string(stats_.stack_overflows) +
                                        " node groups dropped");
    frame_ += (uint32_t)frames;
  }

  // Tick with the outputs in device memory (float4 average, 0x00RRGGBB) and no stats: no host wait.  With frames
  // in flight (SetFramesInFlight(n > 1), ABI 9) consecutive calls overlap on internal streams and a call's outputs
  // are complete in the context stream's order once n - 1 more calls are made, or after Finish(); the
  // accumulation stays in call order, so the images equal Tick()'s
  void TickDevice(float* avg_dev, uint32_t* rgb8_dev, int32_t frames = 1) {
    prt_render_params p{};
    p.width = width_;
    p.height = height_;
    p.spp = frames * (AA ? 2 : 1);
    p.bounces = bounces;
    p.flags = Flags();
    p.render_mode = (int32_t)renderingMode;
    p.frame_index = frame_;
    p.seed = 0;
    const prt_postfx pf = camera.PostFx(isPostProcessed);
    check(prt_set_postfx(ctx_, &pf));
    check(prt_render(ctx_, &p, avg_dev, rgb8_dev, PRT_OUT_DEVICE, nullptr));
    frame_ += (uint32_t)frames;
  }
  void SetFramesInFlight(int32_t n) { check(prt_set_frames_in_flight(ctx_, n)); }
  void Finish() { check(prt_finish(ctx_)); }  // the frames in flight joined into the context stream

  // Camera::HandleInput returned true: new screen plane, accumulator memset (Core/Renderer.cpp:147)
  // scene.models[index] was deformed (same topology): the device takes it, the model's BLAS is refitted in place and
  // the accumulation restarts in full (the accumulated frames, sample counts and distances show the old geometry)
  void ModelChanged(int32_t index) {
    scene.UpdateModel(ctx_, index);
    check(prt_reset_accumulation(ctx_, 1));
  }

  // scene.gameobjects moved (Scene::UpdateInstances): the instance BVH is refitted on the device and the accumulation
  // restarts in full.  InstancesMovedDevice takes the transforms from device memory instead (16 floats per game
  // object, 16-byte aligned, read in the context stream's order); scene.gameobjects then no longer says where the
  // objects are.  TlasCost() is the SAH cost of the instance BVH as it stands (prt_tlas_cost): it grows while the refit
  // follows the objects away from where the tree was built; scene.UploadInstances(ctx) builds a fresh tree on the host, InstancesRebuilt /
  // InstancesRebuiltDevice one on the device.  When to rebuild is the caller's decision.
  void InstancesMoved() {
    scene.UpdateInstances(ctx_);
    check(prt_reset_accumulation(ctx_, 1));
  }
  void InstancesMovedDevice(const float* transforms_dev) {
    check(prt_update_instances(ctx_, transforms_dev, (int32_t)scene.gameobjects.size(), PRT_IN_DEVICE));
    check(prt_reset_accumulation(ctx_, 1));
  }
  double TlasCost() const {
    double v = 0.0;
    check(prt_tlas_cost(ctx_, &v));
    return v;
  }
  // TlasCost() has grown: a fresh device build of the instance BVH (prt_rebuild_instances), over scene.gameobjects,
  // over transforms in device memory, or (InstancesRebuiltDevice(nullptr)) over the instances where they are -- also while
  // the transforms are device-resident.  Blocks until the builder is through; the accumulation restarts in full.
  void InstancesRebuilt(int32_t builder = PRT_BUILDER_GPU_PLOC) {
    scene.RebuildInstances(ctx_, builder);
    check(prt_reset_accumulation(ctx_, 1));
  }
  void InstancesRebuiltDevice(const float* transforms_dev, int32_t builder = PRT_BUILDER_GPU_PLOC) {
    check(prt_rebuild_instances(ctx_, transforms_dev, (int32_t)scene.gameobjects.size(), transforms_dev ? PRT_IN_DEVICE : 0u,
                                builder));
    check(prt_reset_accumulation(ctx_, 1));
  }

  // The SAH cost of model index's BLAS as it stands (prt_blas_cost): it grows while ModelChanged / SkinModel refit
  // the tree away from the pose it was built for.  RebuildModel(index) rebuilds it over scene.models[index] as it is
  // now; RebuildSkinnedModel(index) over the pose of the last SkinModel.  When to rebuild is the caller's decision.
  double BlasCost(int32_t index) const {
    double v = 0.0;
    check(prt_blas_cost(ctx_, index, &v));
    return v;
  }
  void RebuildModel(int32_t index, int32_t builder = PRT_BUILDER_GPU_PLOC) {
    scene.RebuildModel(ctx_, index, builder);
    check(prt_reset_accumulation(ctx_, 1));
  }
  void RebuildSkinnedModel(int32_t index, int32_t builder = PRT_BUILDER_GPU_PLOC) {
    check(prt_rebuild_mesh(ctx_, index, nullptr, 0u, builder));
    check(prt_reset_accumulation(ctx_, 1));
  }

  // scene.models[index] is bound to `skin` (Scene::SetSkin); SkinModel(index, matrices, joints) then poses it: joints
  // row-major 3 x 4 matrices from host memory, skinned and refitted on the device (prt_skin_mesh), and the
  // accumulation restarts in full as after ModelChanged.  The scene's Model keeps its bind-pose arrays.
  void SetSkin(int32_t index, Skin skin) { scene.SetSkin(ctx_, index, std::move(skin)); }
  void SkinModel(int32_t index, const float* matrices, int32_t joints) {
    check(prt_skin_mesh(ctx_, index, matrices, joints, 0u));
    check(prt_reset_accumulation(ctx_, 1));
  }

  void CameraMoved() {
    const prt_camera c = camera.Plane();
    check(prt_set_camera(ctx_, &c));
    check(prt_reset_accumulation(ctx_, 0));
  }

  // checkpoint of a long progressive render: the accumulation blob (prt_save_accumulation) and the frame counter
  // the RNG stream continues from; Resume(blob, frame) before the next Tick continues bit for bit
  std::vector<uint8_t> Checkpoint(uint32_t* frame) const {
    uint64_t n = 0;
    check(prt_accumulation_bytes(ctx_, &n));
    std::vector<uint8_t> blob(n);
    if (n) check(prt_save_accumulation(ctx_, blob.data(), n));
    if (frame) *frame = frame_;
    return blob;
  }
  void Resume(const std::vector<uint8_t>& blob, uint32_t frame) {
    check(prt_load_accumulation(ctx_, blob.data(), blob.size()));
    frame_ = frame;
  }

  // rays traced since construction (or the last reset): the reference's ImGui ray counter (Core/Renderer.cpp:467-474)
  void RayTotals(uint64_t* segments, uint64_t* shadow_rays, bool reset = false) const {
    check(prt_ray_totals(ctx_, segments, shadow_rays, reset ? 1 : 0));
  }
  // path-1 primary rays traced for reuse / taken from the kept records so far (prt_primary_rays; host counters)
  void PrimaryRays(uint64_t* traced, uint64_t* reused, bool reset = false) const {
    check(prt_primary_rays(ctx_, traced, reused, reset ? 1 : 0));
  }
  // shadow rays answered from the kept light visibility of the primary hits so far (prt_shadow_reuse; waits)
  uint64_t ShadowReuse(bool reset = false) const {
    uint64_t reused = 0;
    check(prt_shadow_reuse(ctx_, &reused, reset ? 1 : 0));
    return reused;
  }
  // work items whose primary hit was shaded from the kept surface values so far (prt_surface_reuse; host counter)
  uint64_t SurfaceReuse(bool reset = false) const {
    uint64_t reused = 0;
    check(prt_surface_reuse(ctx_, &reused, reset ? 1 : 0));
    return reused;
  }
  // shadow rays counted instead of traced because their contribution is zero so far (prt_shadow_dead; waits)
  uint64_t ShadowDead(bool reset = false) const {
    uint64_t dead = 0;
    check(prt_shadow_dead(ctx_, &dead, reset ? 1 : 0));
    return dead;
  }

  // First-hit feature buffers of the scene and camera at pixel centres (prt_render_aov): albedo = base colour
  // (w = 1; miss 0), normal_depth = the shading normal as Trace uses it with the hit distance in w (miss
  // 0,0,0,1e30); float4 x W*H each.  The accumulation and the ray totals stay as they are.
  void Aov(std::vector<float>& albedo, std::vector<float>& normal_depth) {
    albedo.assign(4 * (size_t)width_ * height_, 0.0f);
    normal_depth.assign(4 * (size_t)width_ * height_, 0.0f);
    const prt_postfx pf = camera.PostFx(isPostProcessed);  // the primary rays follow Tick's (Panini)
    check(prt_set_postfx(ctx_, &pf));
    check(prt_render_aov(ctx_, width_, height_, NORMALMAPPED ? PRT_FLAG_NORMALMAP : 0u, albedo.data(),
                         normal_depth.data(), 0u));
  }
  static prt_denoise_params DenoiseDefaults() {
    prt_denoise_params p{};
    check(prt_denoise_defaults(&p));
    return p;
  }
  // The current average (accumulator) filtered by the edge-avoiding a-trous denoiser with fresh AOVs (prt_denoise):
  // average gets the float4 image, screen8 its 0x00RRGGBB pixels (no screen pass).  accumulator, screen and the
  // accumulation stay as Tick() left them, so it can be called after any Tick.
  void Denoise(std::vector<float>& average, std::vector<uint32_t>& screen8,
               const prt_denoise_params& params = DenoiseDefaults()) {
    std::vector<float> albedo, normal_depth;
    Aov(albedo, normal_depth);
    average.assign(accumulator.size(), 0.0f);
    screen8.assign(screen.size(), 0u);
    check(prt_denoise(ctx_, &params, width_, height_, accumulator.data(), albedo.data(), normal_depth.data(),
                      average.data(), screen8.data(), 0u));
  }

  static prt_reproject_params ReprojectDefaults() {
    prt_reproject_params p{};
    check(prt_reproject_defaults(&p));
    return p;
  }
  // One Tick() that stands alone (the accumulation is reset in full first, and the camera handed over, so a moved
  // camera needs no CameraMoved()), reprojected onto the history this renderer keeps: the previous call's output,
  // AOVs and camera (prt_reproject).  history gets the float4 image with the history length in w, screen8 its
  // 0x00RRGGBB pixels (no screen pass); accumulator and screen are as Tick() left them.  The first call or
  // ResetTemporal() starts a new history.  Throws with isPostProcessed: Panini primary rays are not described by
  // the camera.
  void TickTemporal(std::vector<float>& history, std::vector<uint32_t>& screen8,
                    const prt_reproject_params& params = ReprojectDefaults()) {
    if (isPostProcessed)
      throw Error(PRT_ERR_INVALID_ARGUMENT,
                  "temporal reprojection is defined for the plane projection only (isPostProcessed is set)");
    const prt_camera cam = camera.Plane();
    check(prt_set_camera(ctx_, &cam));
    check(prt_reset_accumulation(ctx_, 1));
    Tick();
    std::vector<float> albedo, normal_depth;
    Aov(albedo, normal_depth);
    std::vector<float> out(accumulator.size(), 0.0f);
    screen8.assign(screen.size(), 0u);
    const bool have = !hist_.empty();
    check(prt_reproject(ctx_, &params, width_, height_, &cam, accumulator.data(), normal_depth.data(),
                        have ? &hist_cam_ : nullptr, have ? hist_.data() : nullptr, have ? hist_nd_.data() : nullptr,
                        out.data(), screen8.data(), 0u));
    hist_ = out;
    hist_nd_.swap(normal_depth);
    hist_ids_.clear();  // (a following TickTemporalMotion() starts a new history)
    hist_mom_.clear();  // (and so does a following TickTemporalVariance())
    hist_cam_ = cam;
    history.swap(out);
  }
  // TickTemporal() that follows moving instances (prt_reproject_motion): scene.gameobjects is handed to the context
  // first (Scene::UploadInstances), the first hits' instance ids are rendered with the AOVs (prt_render_aov_ids), the
  // previous ids and transforms are kept with the history, and the motion matrices come from prt_instance_motion.  A
  // changed instance count starts a new history, and so does a call that follows a plain TickTemporal().
  void TickTemporalMotion(std::vector<float>& history, std::vector<uint32_t>& screen8,
                          const prt_reproject_params& params = ReprojectDefaults()) {
    if (isPostProcessed)
      throw Error(PRT_ERR_INVALID_ARGUMENT,
                  "temporal reprojection is defined for the plane projection only (isPostProcessed is set)");
    scene.UploadInstances(ctx_);
    const prt_camera cam = camera.Plane();
    check(prt_set_camera(ctx_, &cam));
    check(prt_reset_accumulation(ctx_, 1));
    Tick();
    const size_t n = (size_t)width_ * height_;
    std::vector<float> normal_depth(4 * n, 0.0f), out(4 * n, 0.0f), xf;
    std::vector<uint32_t> ids(n, 0u);
    check(prt_render_aov_ids(ctx_, width_, height_, NORMALMAPPED ? PRT_FLAG_NORMALMAP : 0u, nullptr,
                             normal_depth.data(), ids.data(), 0u));
    for (const GameObject& g : scene.gameobjects) xf.insert(xf.end(), g.transform.begin(), g.transform.end());
    screen8.assign(n, 0u);
    const int32_t count = (int32_t)scene.gameobjects.size();
    if (hist_.empty() || hist_ids_.empty() || !hist_mom_.empty() || hist_xf_.size() != xf.size() || count == 0) {
      check(prt_reproject_motion(ctx_, &params, width_, height_, &cam, accumulator.data(), normal_depth.data(),
                                 ids.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, out.data(),
                                 screen8.data(), 0u));
    } else {
      std::vector<float> motion(12 * (size_t)count);
      check(prt_instance_motion(xf.data(), hist_xf_.data(), count, motion.data()));
      check(prt_reproject_motion(ctx_, &params, width_, height_, &cam, accumulator.data(), normal_depth.data(),
                                 ids.data(), &hist_cam_, hist_.data(), hist_nd_.data(), hist_ids_.data(),
                                 motion.data(), count, out.data(), screen8.data(), 0u));
    }
    hist_ = out;
    hist_nd_.swap(normal_depth);
    hist_ids_.swap(ids);
    hist_xf_.swap(xf);
    hist_mom_.clear();  // (a following TickTemporalVariance() starts a new history)
    hist_cam_ = cam;
    history.swap(out);
  }
  static prt_temporal_params TemporalDefaults() {
    prt_temporal_params p{};
    check(prt_temporal_defaults(&p));
    return p;
  }
  static prt_denoise_variance_params DenoiseVarianceDefaults() {
    prt_denoise_variance_params p{};
    check(prt_denoise_variance_defaults(&p));
    return p;
  }
  // TickTemporalMotion() with the luminance moments carried along (prt_reproject_moments) and the result filtered by
  // the variance-guided a-trous filter (prt_denoise_variance): filtered gets the filtered float4 image, screen8 its
  // 0x00RRGGBB pixels, history the unfiltered reprojection output.  The unfiltered output and its moments are the
  // next call's history (the filtered image is not fed back).  A changed instance count, ResetTemporal() or a
  // preceding TickTemporal() / TickTemporalMotion() starts a new history.
  // deform = true follows the models given to TrackModel() as ModelChanged() deforms them: the AOVs come from
  // prt_render_aov_deform, the pass is prt_reproject_deform with the kept previous transforms, and every tracked model
  // is snapshotted again after the pass (prt_snapshot_mesh).
  void TickTemporalVariance(std::vector<float>& filtered, std::vector<uint32_t>& screen8, std::vector<float>& history,
                            const prt_temporal_params& params = TemporalDefaults(),
                            const prt_denoise_variance_params& filter = DenoiseVarianceDefaults(),
                            bool deform = false) {
    if (isPostProcessed)
      throw Error(PRT_ERR_INVALID_ARGUMENT,
                  "temporal reprojection is defined for the plane projection only (isPostProcessed is set)");
    scene.UploadInstances(ctx_);
    const prt_camera cam = camera.Plane();
    check(prt_set_camera(ctx_, &cam));
    check(prt_reset_accumulation(ctx_, 1));
    Tick();
    const size_t n = (size_t)width_ * height_;
    std::vector<float> albedo(4 * n, 0.0f), normal_depth(4 * n, 0.0f), out(4 * n, 0.0f), mom(4 * n, 0.0f), xf;
    std::vector<float> offset(deform ? 4 * n : 0, 0.0f);
    std::vector<uint32_t> ids(n, 0u);
    if (deform)
      check(prt_render_aov_deform(ctx_, width_, height_, NORMALMAPPED ? PRT_FLAG_NORMALMAP : 0u, albedo.data(),
                                  normal_depth.data(), ids.data(), offset.data(), 0u));
    else
      check(prt_render_aov_ids(ctx_, width_, height_, NORMALMAPPED ? PRT_FLAG_NORMALMAP : 0u, albedo.data(),
                               normal_depth.data(), ids.data(), 0u));
    for (const GameObject& g : scene.gameobjects) xf.insert(xf.end(), g.transform.begin(), g.transform.end());
    const int32_t count = (int32_t)scene.gameobjects.size();
    if (hist_.empty() || hist_ids_.empty() || hist_mom_.empty() || hist_xf_.size() != xf.size() || count == 0) {
      check(prt_reproject_moments(ctx_, &params, width_, height_, &cam, accumulator.data(), normal_depth.data(),
                                  ids.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, out.data(),
                                  mom.data(), nullptr, 0u));
    } else {
      std::vector<float> motion(12 * (size_t)count);
      check(prt_instance_motion(xf.data(), hist_xf_.data(), count, motion.data()));
      if (deform)
        check(prt_reproject_deform(ctx_, &params, width_, height_, &cam, accumulator.data(), normal_depth.data(),
                                   ids.data(), &hist_cam_, hist_.data(), hist_nd_.data(), hist_ids_.data(),
                                   motion.data(), count, hist_mom_.data(), offset.data(), hist_xf_.data(), out.data(),
                                   mom.data(), nullptr, 0u));
      else
        check(prt_reproject_moments(ctx_, &params, width_, height_, &cam, accumulator.data(), normal_depth.data(),
                                    ids.data(), &hist_cam_, hist_.data(), hist_nd_.data(), hist_ids_.data(),
                                    motion.data(), count, hist_mom_.data(), out.data(), mom.data(), nullptr, 0u));
    }
    filtered.assign(4 * n, 0.0f);
    screen8.assign(n, 0u);
    check(prt_denoise_variance(ctx_, &filter, width_, height_, out.data(), mom.data(), albedo.data(),
                               normal_depth.data(), filtered.data(), nullptr, screen8.data(), 0u));
    if (deform)
      for (int32_t index : tracked_) check(prt_snapshot_mesh(ctx_, index));
    hist_ = out;
    hist_nd_.swap(normal_depth);
    hist_ids_.swap(ids);
    hist_xf_.swap(xf);
    hist_mom_.swap(mom);
    hist_cam_ = cam;
    history.swap(out);
  }
  // scene.models[index] deforms (ModelChanged every frame): its present positions are snapshotted now
  // (prt_snapshot_mesh), and TickTemporalVariance(deform = true) renews the snapshot after every pass
  void TrackModel(int32_t index) {
    check(prt_snapshot_mesh(ctx_, index));
    if (std::find(tracked_.begin(), tracked_.end(), index) == tracked_.end()) tracked_.push_back(index);
  }
  // the next TickTemporal() / TickTemporalMotion() / TickTemporalVariance() starts a new history
  void ResetTemporal() {
    hist_.clear();
    hist_ids_.clear();
    hist_mom_.clear();
  }

  uint32_t Flags() const {
    return (AA ? PRT_FLAG_AA : 0u) | (accumulates ? PRT_FLAG_ACCUMULATE : 0u) | (GAMMACORRECTED ? PRT_FLAG_GAMMA : 0u) |
           (NORMALMAPPED ? PRT_FLAG_NORMALMAP : 0u) | (SKYBOX ? PRT_FLAG_SKYBOX : 0u) | (LIGHTED ? PRT_FLAG_LIGHTED : 0u) |
           (isStochastic ? PRT_FLAG_STOCHASTIC : 0u);
  }
  const prt_stats& LastStats() const { return stats_; }
  prt_ctx* Context() const { return ctx_; }
  int32_t Width() const { return width_; }
  int32_t Height() const { return height_; }

 private:
  prt_ctx* ctx_ = nullptr;
  int32_t width_, height_;
  uint32_t frame_ = 0;
  prt_stats stats_{};
  std::vector<float> hist_, hist_nd_;  // TickTemporal's history: previous output, previous normal_depth (empty: none)
  prt_camera hist_cam_{};              // ... and the camera they were made with
  std::vector<uint32_t> hist_ids_;     // TickTemporalMotion's: the previous instance ids (empty: no such history)
  std::vector<float> hist_xf_;         // ... and the previous instance transforms (16 floats each)
  std::vector<float> hist_mom_;        // TickTemporalVariance's: the previous moments (empty: no such history)
  std::vector<int32_t> tracked_;       // TrackModel's models
};

}  // namespace prt
