/*
 * prt.h -- C ABI of the MI355X-native path-tracing hot path.
 *
 * Drop-in boundary for the reference's per-pixel hot path (Iancic/Physically-Based-Ray-Tracer):
 * a Renderer::Tick shim replaces Core/Renderer.cpp:43-141 with prt_render(),
 * after handing over the data the hot path reads without copying:
 *
 *   prt_set_textures   <- Model::{albedo,normal,metalness,emission}Texture (template/surface.h:49-94)
 *   prt_set_meshes     <- Model fat-triangle arrays (Core/Model.h:36-44, Core/Model.cpp:25-119)
 *   prt_set_instances  <- Scene::blases[i].transform + gameobjects[i]->modelIndex (Core/Scene.cpp:220-223,
 *                         Core/tiny_bvh.h:1243-1256)
 *   prt_set_lights     <- Renderer point-light SoA (Core/Renderer.h:80-88), directionalLights[0], spotlights[0]
 *   prt_set_sky        <- Camera::skyPixels (Core/Camera.cpp:9)
 *   prt_set_camera     <- Camera::camPos/topLeft/topRight/bottomLeft/right/up/ahead (Core/Camera.cpp:29-36)
 *   prt_set_postfx     <- Renderer::isPostProcessed + Camera post-process members (Core/Camera.h:11-31)
 *   prt_render         <- the OpenMP pixel loop + Renderer::Trace (Core/Renderer.cpp:43-141,150-406)
 *
 * Conventions: plain pointers and sizes, no C++ types; every call returns PRT_OK (0) or a negative
 * prt_status; prt_last_error() gives the message for the calling thread.  No exceptions cross the ABI.
 * One host thread per context.  All scene arrays are copied to device memory (HBM) during the call;
 * the caller may free them afterwards.  A HIP device must be present: there is no CPU fallback.
 * Ordering: prt_set_textures / prt_set_meshes / prt_set_sky first wait for the frames queued on the
 * context's stream (they overwrite resident buffers); prt_set_instances / prt_set_instance_materials are
 * stream-ordered (a frame queued before the call renders the old instances); the remaining setters are
 * read at the next prt_render.
 */
#ifndef PRT_H
#define PRT_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRT_ABI_VERSION 10

typedef enum {
    PRT_OK = 0,
    PRT_ERR_INVALID_ARGUMENT = -1,
    PRT_ERR_NO_DEVICE = -2,
    PRT_ERR_HIP = -3,
    PRT_ERR_OUT_OF_MEMORY = -4,
    PRT_ERR_NOT_READY = -5,     /* scene/camera incomplete */
    PRT_ERR_UNSUPPORTED = -6
} prt_status;

/* Render flags: the public Renderer bools, Core/Renderer.h:33,48 */
#define PRT_FLAG_AA          (1u << 0)
#define PRT_FLAG_ACCUMULATE  (1u << 1)
#define PRT_FLAG_GAMMA       (1u << 2)
#define PRT_FLAG_NORMALMAP   (1u << 3)
#define PRT_FLAG_SKYBOX      (1u << 4)
#define PRT_FLAG_LIGHTED     (1u << 5)
#define PRT_FLAG_STOCHASTIC  (1u << 6)
/* the reference's defaults (Core/Renderer.h:33,48) */
#define PRT_FLAGS_DEFAULT    (0x7Fu)

/* Renderer::RENDER_STATES, Core/Renderer.h:37-46 */
typedef enum {
    PRT_MODE_BRDF = 0, PRT_MODE_BASECOLOR = 1, PRT_MODE_GEOMETRYNORMAL = 2, PRT_MODE_SHADINGNORMAL = 3,
    PRT_MODE_METAL = 4, PRT_MODE_ROUGHNESS = 5, PRT_MODE_EMISSIVE = 6
} prt_render_mode;

typedef struct prt_ctx prt_ctx;

typedef struct {
    int32_t device;      /* HIP device ordinal (one process per GPU) */
    uint32_t flags;      /* reserved, 0 */
} prt_device_desc;

/* one packed 0x00RRGGBB texture, exactly Surface::pixels (template/surface.cpp:47-66) */
typedef struct {
    int32_t width, height;
    const uint32_t* pixels;
} prt_texture;

/* one Model (Core/Model.h:36-44).  T = tri_count, V = vertex_count.
 * fixed_uvs may hold any float, also where the host never sees them (PRT_IN_DEVICE).  Texel addressing is one total
 * function of the interpolated uv, per component, with n the ALBEDO map's width or height and x = uv * (float)n
 * (one float multiply):
 *     !(fabsf(x) < 2147483648.0f)  ->  0                       NaN, +-inf, |x| >= 2^31
 *     otherwise  r = (int)x % n;  if (r < 0) r += n;  ->  r    truncation toward zero, then a wrap into [0, n)
 * and every map is read at texel column + row * w, always inside [0, w * h).  For x > -1 this is the reference's
 * (int)x % n (Core/Scene.cpp:82-83,163-164) bit for bit: values >= 1 repeat the texture.  The reference itself
 * indexes outside the texture for x <= -1 and is undefined where the cast is; here a negative uv repeats the
 * texture as well.  Truncation, not floor: -1 < x < 0 addresses texel 0, as it does in the reference (the tiny
 * negative uv that w = 1 - u - v rounding can give on a triangle's edge), so texel 0 is two texels wide around
 * uv = 0 and the tiling is not translation-invariant across 0: texel k < 0 covers (k - 1, k], not [k, k + 1). */
typedef struct {
    int32_t tri_count;
    int32_t vertex_count;
    const float* triangles;      /* float4 x 3T : Model::triangles (fat, w ignored)            */
    const float* fixed_normals;  /* float4 x 3T : Model::fixedNormals                          */
    const float* fixed_uvs;      /* float2 x 3T : Model::fixedTextureCoords                    */
    const int32_t* indices;      /* int x 3T    : Model::indices                               */
    const float* vertices;       /* float3 x V  : Model::vertices                              */
    const float* face_normals;   /* float3 x T  : Model::faceNormals                           */
    int32_t albedo_tex;          /* required (Core/Scene.cpp:160 dereferences it)              */
    int32_t normal_tex;          /* -1 = none */
    int32_t metalness_tex;       /* -1 = none (G = roughness, B = metalness, Scene.cpp:175-181) */
    int32_t emission_tex;        /* -1 = none */
} prt_mesh;

/* lights as the hot path reads them (Core/Renderer.cpp:216-310) */
typedef struct {
    float point_pos[4][3];   /* posX/posY/posZ SoA of the 4 SIMD point lights */
    float point_color[4][3];
    float dir_pos[3], dir_color[3];                  /* directionalLights[0]->transform */
    float spot_pos[3], spot_color[3], spot_rot[3];   /* spotlights[0]->transform        */
} prt_lights;

/* Instance material kinds (prt_set_instance_materials).  The reference's Scene::GetMaterialBRDF has a
 * dielectric and a perfect-mirror branch gated on `modelIndex == -1`, which never holds (Core/Scene.cpp:
 * 193-205, "Instead of -1 place model index"); here the caller names the instances that take them.
 * DIELECTRIC takes Renderer::Trace's glass branch (Core/Renderer.cpp:331-372: reflection + refraction
 * rays, Schlick-weighted, depth first); MIRROR forces metalness 1 / roughness 0 (the :376 fast path). */
#define PRT_MAT_TEXTURED   0
#define PRT_MAT_DIELECTRIC 1
#define PRT_MAT_MIRROR     2

/* One emitting parallelogram corner + a*edge_u + b*edge_v (a, b in [0,1]) -- an extension: the reference's
 * AreaLight (Core/AreaLight.h) is never sampled by Trace.  Radiance on the side of cross(edge_u, edge_v)
 * (both sides when two_sided); sampled by next-event estimation at every lit hit and reached by BRDF rays,
 * combined with the power heuristic.  At a path's last segment the light sample is unweighted:
 * no BRDF ray follows there, so light sampling is the only strategy.  The BRDF strategy's integrand is the
 * reference's indirect weights (evalIndirectCombinedBRDF: (1, 1, 1) for the specular lobe), not evalCombinedBRDF,
 * so with more than one bounce the light's term is not the integral of evalCombinedBRDF over the light. */
typedef struct {
    float corner[3], edge_u[3], edge_v[3];
    float radiance[3];
    int32_t two_sided;
} prt_area_light;

/* Camera screen plane and basis (Core/Camera.cpp:29-36, 113-139; Core/Camera.h:15-17).  right / up /
 * ahead are only read by the Panini projection (post-processing on); prt_camera_look_at fills all. */
typedef struct {
    float pos[3];
    float top_left[3], top_right[3], bottom_left[3];
    float right[3], up[3], ahead[3];
} prt_camera;

typedef struct {
    int32_t width, height;
    int32_t spp;            /* camera paths per pixel in this call; with AA one reference frame = 2 paths */
    int32_t bounces;        /* Renderer::bounces (closest-hit segments per path), 0..16 */
    uint32_t flags;         /* PRT_FLAG_* */
    int32_t render_mode;    /* prt_render_mode */
    uint32_t frame_index;   /* first reference frame of this call (RNG stream) */
    uint32_t seed;          /* added to the per-pixel seed base */
} prt_render_params;

typedef struct {
    uint64_t segments;      /* closest-hit queries (TLAS intersections) */
    uint64_t shadow_rays;   /* any-hit queries (IsOccluded) */
    uint64_t paths;         /* camera paths traced */
    double   ms;            /* device time of the render (HIP events) */
    double   ms_trace;      /* device time of the path-tracing kernel(s) only */
    double   ms_closest;    /* device time of the traversal launches (closest + shadow rays together), summed */
    double   ms_anyhit;     /* reserved (0): shadow rays are traced inside the merged traversal launches */
    int32_t  pipeline;      /* 2 = the merged-trace wavefront (prt_wave2.hip); 3 = the same with each pass's paths
                               resolved in one launch at its end (prt_defer.hip) */
    int32_t  iterations;    /* traversal launches per call */
    int32_t  batches;       /* 1 */
    int32_t  ranks;         /* shards whose rays these stats count (1 unless a local group summed its members) */
    uint64_t stack_overflows; /* traversal stack overflows since the context was created: a BVH node group that
                                 found no free stack level (the host sizes the stacks from the BVH depth, so any
                                 non-zero count is a builder / sizing bug; the results may have lost hits) */
} prt_stats;

/* closest-hit record, tinybvh::Intersection (Core/tiny_bvh.h:545-567) minus user data */
typedef struct {
    float t, u, v;
    uint32_t prim, inst;
} prt_hit;

/* ---- context ---- */
int prt_abi_version(void);
const char* prt_last_error(void);
int prt_device_count(int32_t* count);
int prt_create(const prt_device_desc* desc, prt_ctx** out);
int prt_destroy(prt_ctx* ctx);
/* run subsequent work on an external hipStream_t (e.g. torch's current stream); NULL = ctx-owned stream */
int prt_set_stream(prt_ctx* ctx, void* hip_stream);
/* Frames in flight (ABI 9; the reference's Renderer::Tick renders one frame per call, Core/Renderer.cpp:43-141).
 * n = 1 (default): a prt_render call's work is complete in the context stream's order when the call returns.
 * n = 2..8 (ABI 10; 2..4 in ABI 9): a prt_render with device outputs (or a prt_render_tiles) and no stats enqueues its frame on one of n
 * internal streams, forked from the context stream, so its wavefront chain overlaps those of the previous n - 1
 * calls; the accumulation (and a sharded frame's gather and untile) still run in call order, so the results are
 * bit-identical to n = 1.  A call's outputs are complete in the context stream's order once n - 1 more render
 * calls have been enqueued, or after prt_finish.  prt_set_instances / prt_set_instance_materials (ABI 10) do not
 * join them: the instance state has n + 1 device copies and an update writes the next one once the frames that
 * read it are done (a stream wait).  Every other entry point (and a render with host outputs or stats) joins the
 * frames in flight first.  Local shard groups: n = 1 only (PRT_ERR_UNSUPPORTED). */
int prt_set_frames_in_flight(prt_ctx* ctx, int32_t n);
/* the context stream waits for every frame in flight (no host wait) */
int prt_finish(prt_ctx* ctx);

/* ---- scene (Scene / Model / Camera state) ---- */
int prt_set_textures(prt_ctx* ctx, const prt_texture* textures, int32_t count);
int prt_set_meshes(prt_ctx* ctx, const prt_mesh* meshes, int32_t count);
/* In-place mesh update with a BLAS refit (additive in ABI 10).  Mesh mesh_index of the last
 * prt_set_meshes takes the arrays of *mesh; its BLAS keeps its topology (the nodes, their slots, the order of the
 * triangle records) and its boxes are refitted bottom-up on the device.  Afterwards every query and render returns,
 * bit for bit, what a fresh context returns after prt_set_meshes with that mesh replaced by *mesh, whatever builder
 * made the tree.  tri_count, vertex_count and the four texture ids must equal the mesh's current ones
 * (PRT_ERR_INVALID_ARGUMENT otherwise, and nothing changes); all six arrays are required.
 * in_flags = 0: the arrays are host memory; indices is range-checked on the host (nothing changes on failure); the
 * arrays go through a pinned buffer of the context.  On a local group or RCCL context they apply to every member.
 * in_flags = PRT_IN_DEVICE: all six arrays are device memory on the context's device (after a skinning kernel, for
 * example; triangles 16-byte aligned), read in the context stream's order.  The kernels check every index against
 * vertex_count: one out of range reads vertex 0 in its place (never out of range) and the call returns
 * PRT_ERR_INVALID_ARGUMENT; THE MESH IS THEN IN A TRAVERSABLE BUT UNSPECIFIED STATE until the next successful
 * prt_update_mesh of it or prt_set_meshes.
 * The call waits on the host once, for 28 bytes (the mesh's new box and that flag), after its own kernels.  On a
 * local group: PRT_ERR_UNSUPPORTED.
 * Ordering: the call joins the frames in flight and enqueues its work on the context stream: frames enqueued
 * before it see the old geometry, frames enqueued after it (on any in-flight stream) the new one.  It neither
 * drains the context nor reallocates: its scratch is sized at the first update after a prt_set_meshes (that one
 * update also reads the mesh's nodes back once, to order them by tree level) and kept.  The instance boxes and the
 * instance BVH follow at the next frame, as after prt_set_instances; kept primary hits and light visibility go
 * stale.  No scene: PRT_ERR_NOT_READY.  A NaN coordinate is ignored by the boxes, as the builders ignore it. */
#define PRT_IN_DEVICE (1u << 0)
int prt_update_mesh(prt_ctx* ctx, int32_t mesh_index, const prt_mesh* mesh, uint32_t in_flags);
/* (additive in ABI 10; DESIGN.md "Deforming meshes") Keeps mesh mesh_index's present object-space corner positions as
 * its previous positions: nine floats per primitive in prim order, vertices[indices[3p + k]] for k = 0..2, as the last
 * prt_set_meshes or prt_update_mesh of the mesh left them.  prt_render_aov_deform measures against them.  A copy from
 * device memory to device memory by a kernel on the context stream: frames and updates enqueued before the call are
 * what it sees.  The storage (36 bytes per primitive) is per mesh, allocated at that mesh's first snapshot and kept: a
 * mesh never snapshotted costs nothing, the first snapshot of a mesh allocates and waits for the context stream once,
 * every later one neither allocates nor waits on the host.  A second snapshot overwrites the first; prt_update_mesh
 * never touches a snapshot; prt_set_meshes discards all of them.  On a local group or RCCL context it applies to every
 * member, as the setters do.  The call joins the frames in flight.
 * NULL context or an index out of range: PRT_ERR_INVALID_ARGUMENT.  No meshes: PRT_ERR_NOT_READY. */
int prt_snapshot_mesh(prt_ctx* ctx, int32_t mesh_index);
/* Linear-blend skinning inside the boundary (additive in ABI 10; DESIGN.md 8 "Skinning"; the definition, operation by
 * operation: csrc/prt_skin.h).  prt_set_mesh_skin binds a mesh's bind pose once; prt_skin_mesh takes the frame's joint
 * matrices, skins the vertices and normals, derives the arrays prt_update_mesh takes and refits the BLAS, all on the
 * device.  With w the four weights and j the four joints of vertex v, M the row-major 3 x 4 joint matrices (a joint's
 * world matrix times its inverse bind matrix, in the mesh's object space), every operation one f32 rounding in the
 * order written:
 *   B[r][c] = ((w0*M[j0][r][c] + w1*M[j1][r][c]) + w2*M[j2][r][c]) + w3*M[j3][r][c]
 *   P'_r = ((B[r][0]*P.x + B[r][1]*P.y) + B[r][2]*P.z) + B[r][3]     n_r = (B[r][0]*N.x + B[r][1]*N.y) + B[r][2]*N.z
 *   N' = n * (1.0f / sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z)), (0, 1, 0) if any component is not finite
 *   triangles[3p + k] = (P'[i_k], 0), fixed_normals[3p + k] = (N'[i_k], 0), vertices = P' (i_k = indices[3p + k]),
 *   face_normals[p] = normalize(cross(P'[i_1] - P'[i_0], P'[i_2] - P'[i_0])), (0, 0, 0) if not finite;
 *   fixed_uvs, the texture ids stay.
 * The weights are used as given (never renormalised; a weight of 0 still names a joint that must be in range).  The
 * normal goes through B's 3 x 3 part itself: exact for rotations and uniform scales, approximate otherwise (the choice
 * prt_reproject_motion makes for its normals).
 * The contract: after prt_skin_mesh every query, render, AOV, prt_read_blas and prt_read_blas_tris returns, bit for
 * bit, what the same context returns after prt_update_mesh with the six arrays derived as above, whatever builder
 * made the tree. */
typedef struct {
    int32_t vertex_count, tri_count;   /* must equal the mesh's */
    int32_t joint_count;               /* 1..65536 */
    const float*    positions;         /* float3 x V, bind pose */
    const float*    normals;           /* float3 x V */
    const int32_t*  indices;           /* int x 3T, the mesh's own */
    const uint16_t* joints;            /* 4 x V */
    const float*    weights;           /* 4 x V */
} prt_skin;
/* Binds *skin (host arrays) to mesh mesh_index, replacing an earlier binding; skin = NULL removes it.  The counts are
 * checked against the mesh, every index against vertex_count and every joint against joint_count, on the host:
 * PRT_ERR_INVALID_ARGUMENT, and nothing changes.  The call joins the frames in flight, waits for the context stream,
 * may allocate, and uploads into storage the context keeps per mesh.  Resident bytes per bound mesh:
 * 80 V + 60 T + 48 J (the binding 48 V + 12 T, the matrices 48 J, the scratch of the skinned vertices and fat
 * triangles 32 V + 48 T), each array rounded up to 256 bytes.  prt_set_meshes discards every binding; prt_update_mesh
 * leaves them alone.  On a local group or RCCL context it applies to every member.
 * NULL context or an index out of range: PRT_ERR_INVALID_ARGUMENT.  No meshes: PRT_ERR_NOT_READY. */
int prt_set_mesh_skin(prt_ctx* ctx, int32_t mesh_index, const prt_skin* skin);
/* Skins mesh mesh_index with joint_matrices (12 floats per joint, row-major 3 x 4) and refits its BLAS in place.
 * in_flags = 0: host memory, copied before the call returns and uploaded in the context stream's order.
 * in_flags = PRT_IN_DEVICE: device memory on the context's device, 16-byte aligned, read in the context stream's
 * order; on a local group PRT_ERR_UNSUPPORTED.  The matrices are not checked for finiteness: a NaN coordinate is
 * ignored by the boxes, as in prt_update_mesh.
 * Ordering, frames in flight and what goes stale are prt_update_mesh's: the call joins the frames in flight and
 * enqueues on the context stream; kept primary hits and light visibility go stale; the instance boxes and the instance
 * BVH follow at the next frame.  The call waits on the host once, for the mesh's new root box, after its own kernels;
 * after the first call on a binding nothing is allocated.
 * No binding on the mesh: PRT_ERR_NOT_READY.  joint_count different from the binding's, NULL matrices, unknown
 * flags, a bad index: PRT_ERR_INVALID_ARGUMENT. */
int prt_skin_mesh(prt_ctx* ctx, int32_t mesh_index, const float* joint_matrices, int32_t joint_count, uint32_t in_flags);
/* The SAH cost of mesh mesh_index's BLAS as it stands on the device (additive in ABI 10; DESIGN.md 8 "Rebuild"; the
 * definition: csrc/prt_blas_cost.h): over all its nodes, the decoded box area of every interior slot plus that of
 * every leaf slot times its triangle count, divided by the area of the box around the root node's occupied slots; 0
 * when that area is 0.  Areas are dx*dy + dy*dz + dz*dx of the boxes the traversal decodes, in f64; unoccupied slots
 * contribute nothing.  A refit keeps a tree's topology, so the cost of a mesh that prt_update_mesh / prt_skin_mesh
 * carried far from the pose its tree was built for grows; the caller compares it with the cost after the build (or
 * after the last prt_rebuild_mesh) and decides when to rebuild: the library has no policy of its own.
 * Two kernels on the context stream, no atomics: two calls on the same tree return the same bits.  The call joins
 * the frames in flight and waits on the host once, for the 8 bytes of the result; its scratch (one f64 per 256 nodes)
 * is allocated at the first call and kept.  On a local group or RCCL context it runs on the calling member.
 * NULL context, NULL cost or an index out of range: PRT_ERR_INVALID_ARGUMENT.  No meshes: PRT_ERR_NOT_READY. */
int prt_blas_cost(prt_ctx* ctx, int32_t mesh_index, double* cost);
/* prt_update_mesh with a fresh device build in place of the refit (additive in ABI 10; DESIGN.md 8 "Rebuild").
 * mesh != NULL: the arguments, the checks, the PRT_IN_DEVICE rule, the bad-index rule and the behaviour on a local
 * group or RCCL context are prt_update_mesh's.  mesh = NULL: the geometry is the fat triangles the mesh's skin binding
 * holds from its last prt_skin_mesh (no binding, or no prt_skin_mesh on it yet: PRT_ERR_NOT_READY).
 * builder: PRT_BUILDER_GPU_LBVH or PRT_BUILDER_GPU_PLOC (with PRT_TRBVH as at prt_set_meshes); the host builders
 * return PRT_ERR_UNSUPPORTED, any other value PRT_ERR_INVALID_ARGUMENT.  prt_scene_info.builder keeps reporting the
 * last prt_set_meshes; blas_nodes, blas_leaves and max_depth report the live trees.
 * The contract: afterwards every query, render and AOV returns, bit for bit, what a fresh context returns after
 * prt_set_meshes with that mesh replaced (hits do not depend on the builder); prt_read_blas / prt_read_blas_tris
 * return the new tree, the one a fresh context's build of the mesh alone with the same builder makes; the other
 * meshes' nodes and records are untouched.
 * The tree is built into scratch the context keeps (128 bytes per triangle of the largest mesh, sized at the first
 * rebuild after a prt_set_meshes) and committed only after the build succeeded: a failed build -- or a tree deeper
 * than 64 levels, PRT_ERR_UNSUPPORTED -- leaves the scene as it was.  A tree with at most as many nodes as the mesh's
 * region of the node array holds (what prt_set_meshes gave it) is committed in place, without draining or
 * allocating; a larger one moves the mesh's nodes to the end of a regrown node array (that region's size becomes the
 * mesh's), which drains the context and reallocates once.  A spatial-split mesh's surplus records go unused.
 * Ordering: the call joins the frames in flight and blocks the host while the builder synchronises (once per tree
 * level); frames enqueued before it see the old tree, frames enqueued after it the new one.  Snapshots and skin
 * bindings are kept; the next prt_update_mesh / prt_skin_mesh of the mesh reads the new nodes back once, as after
 * prt_set_meshes; kept primary hits and light visibility go stale; the instance boxes and the instance BVH follow at
 * the next frame. */
int prt_rebuild_mesh(prt_ctx* ctx, int32_t mesh_index, const prt_mesh* mesh, uint32_t in_flags, int32_t builder);
/* transforms: 16*count floats, row-major BLASInstance::transform; mesh_index: count.  Above 64 instances the rays
 * walk an instance BVH, rebuilt for every call as the reference's per-frame BVH::Build (a host SAH build): on the
 * calling thread when the instance count changes, otherwise on the context's worker thread, the context stream
 * waiting for that build before its upload (the caller neither builds nor waits) */
int prt_set_instances(prt_ctx* ctx, const float* transforms, const uint32_t* mesh_index, int32_t count);
int prt_set_lights(prt_ctx* ctx, const prt_lights* lights);
/* kinds: one PRT_MAT_* per instance (count = the instance count), or count 0 = all textured.  Reset by
 * prt_set_instances with a different instance count.  Dielectric instances need bounces <= 4 with AA (5 without): the depth-first path tree
 * has up to 2^bounces - 1 segments per path. */
int prt_set_instance_materials(prt_ctx* ctx, const int32_t* kinds, int32_t count);
/* New transforms for the instances of the last prt_set_instances (additive in ABI 10; DESIGN.md 8 "Instance updates:
 * the TLAS refit"; the definition: csrc/prt_tlas_refit.h): count row-major 4x4 matrices, laid out as prt_set_instances
 * takes them.  The mesh indices and material kinds stay; count must equal the current instance count.
 * The contract: afterwards every query, render and AOV returns, bit for bit, what a fresh context returns after
 * prt_set_instances with these transforms and the same mesh indices (and the same prt_set_instance_materials): hits do
 * not depend on the tree.  prt_stats.stack_overflows stays 0: the tree keeps its depth.
 * The instance BVH (above 64 instances, or with PRT_TLAS=1; below that only the records change) is refitted, not
 * rebuilt: the nodes, their slots, imask, meta, child_base, tri_base and the instance-slot table stay; leaf slot s of
 * node j gets the box of instance slot[8j + s], an interior slot its child node's uninflated box, and every node is
 * re-encoded bottom-up on the device, one launch per tree level.  A refit with the transforms the tree was built for
 * reproduces the built bytes; updating to T' and back to T is byte-identical as well.  When to pay for a fresh SAH
 * tree is the caller's decision: prt_tlas_cost measures the tree as it stands; prt_rebuild_instances (on the device)
 * and prt_set_instances (on the host) are the rebuilds.
 * in_flags = 0: host memory, copied before the call returns and uploaded in the context stream's order.  On a local
 * group or RCCL context it applies to every member.
 * in_flags = PRT_IN_DEVICE: device memory on the context's device, 16-byte aligned, read by one kernel in the context
 * stream's order into storage of the library's own: nothing rereads the caller's memory after that kernel.  On a
 * local group: PRT_ERR_UNSUPPORTED.  DEVICE-RESIDENT TRANSFORMS ARE A STATE that lasts until the next
 * prt_set_instances or host-memory prt_update_instances: in it prt_set_instance_materials and the refresh that
 * follows prt_update_mesh / prt_skin_mesh / prt_rebuild_mesh rebuild the records on the device from the transforms
 * kept there, under the new kinds and mesh boxes, and refit the tree; the library holds no host copy of them.
 * Ordering is prt_set_instances': the call does not join the frames in flight; it writes the next copy of the
 * instance state once the context stream has waited for the frames that read that copy; frames enqueued before the
 * call see the old instances, frames enqueued after it the new ones; kept primary hits and light visibility go
 * stale.  The call never waits on the GPU, builds nothing on the host and gives the worker thread nothing.  The
 * first call after a prt_set_instances waits (on the host only) until the worker has finished the builds queued
 * before it, takes that tree's topology and uploads its level order; after that first call nothing is allocated.
 * Transforms are not checked for finiteness: a non-finite one gives its instance the record prt_set_instances would,
 * and the node boxes ignore a NaN coordinate, as the BLAS refit does.
 * NULL context, NULL transforms, unknown flag bits, count different from the instance count, misaligned device
 * memory: PRT_ERR_INVALID_ARGUMENT.  No meshes or no instances yet: PRT_ERR_NOT_READY.  A worker build that failed
 * earlier is reported as prt_set_instances reports it.  Nothing changes in any of these cases. */
int prt_update_instances(prt_ctx* ctx, const float* transforms, int32_t count, uint32_t in_flags);
/* prt_update_instances with a fresh device build of the instance BVH in place of the refit (additive in ABI 10;
 * DESIGN.md 8 "Instance rebuild"; the definitions: csrc/prt_tlas_build.h).  It stands to prt_update_instances as
 * prt_rebuild_mesh stands to prt_update_mesh: the way to pay for a fresh tree when prt_tlas_cost has grown, also while
 * the transforms are device-resident and the library holds no host copy for prt_set_instances.
 * transforms != NULL: the arguments, the PRT_IN_DEVICE rule, the alignment rule, the local-group rule and the
 * resulting host / device-resident state are prt_update_instances'.  transforms = NULL: the instances stay where they
 * are -- in the device-resident state the transforms kept on the device are used, otherwise the host's; count must
 * still equal the instance count and in_flags must be 0.
 * builder: PRT_BUILDER_GPU_LBVH or PRT_BUILDER_GPU_PLOC (treelet passes: the builders' defaults, PRT_TRBVH, as at
 * prt_rebuild_mesh); the host builders return PRT_ERR_UNSUPPORTED (prt_set_instances is their rebuild), any other
 * value PRT_ERR_INVALID_ARGUMENT.  On the linear list (at most 64 instances without PRT_TLAS=1) the call is exactly
 * prt_update_instances, with transforms = NULL a no-op that returns PRT_OK; builder is still validated.
 * The contract: afterwards every query, render and AOV returns, bit for bit, what a fresh context returns after
 * prt_set_instances with these transforms and the same mesh indices and material kinds: hits do not depend on the
 * tree.  prt_stats.stack_overflows stays 0.  prt_read_tlas returns a tree in the host build's form: every instance in
 * exactly one leaf slot, with count 1; tri_base = 8j in node j; 0xFFFFFFFF in the slot table wherever a slot is no
 * leaf slot; interior children consecutive from child_base, with larger indices than their parent; each level's
 * nodes contiguous.  The node bytes are what the refit of prt_update_instances (csrc/prt_tlas_refit.h refit_tlas8)
 * makes of the same topology over the same instance boxes: the device collapse encodes as the refit does.  The tree is
 * the same from host memory, device memory and NULL for the same transforms and builder, and two rebuilds of the same
 * state with the same builder give the same bytes: the builder's collapse hands out node positions by atomic
 * counters, and the commit puts every level into its canonical order (the children of a level's nodes in those
 * nodes' order, each node's in slot order).
 * Afterwards a prt_update_instances refits the new topology and a prt_set_instances behaves as before;
 * prt_scene_info.tlas_rebuilds and tlas_async, which count worker builds, do not move.
 * Failure: the tree is built into scratch the context keeps (176 bytes per instance: 48 of builder input, 80 of
 * nodes, 48 of records; sized at the first rebuild of an instance count, and only that call may allocate) and
 * committed to the next copy of the instance state only after the build succeeded.  A failed build returns
 * PRT_ERR_HIP; a tree that with the deepest BLAS would exceed 64 levels returns PRT_ERR_UNSUPPORTED; in both cases
 * the live instances, tree and host / device-resident state are as before.  A tree deeper than the levels the
 * traversal stacks were sized for (prt_scene_info.tlas_depth) raises that figure to its depth: the stacks are sized
 * at every launch, and a deeper stack can cost an occupancy step.
 * Ordering: like prt_update_instances the call does not join the frames in flight and writes the next copy of the
 * instance state once the context stream has waited for the frames that read it; frames enqueued before the call see
 * the old instances, frames enqueued after it the new tree.  Unlike prt_update_instances it blocks the host: the
 * builder synchronises the context stream once per PLOC iteration and once per tree level, so the call also waits
 * for the work queued on that stream before it (on an RCCL context with the bounded wait).
 * Transforms are not checked for finiteness: with a non-finite one the call either builds a traversable tree or
 * returns an error with nothing changed; which of the two is outside the contract.
 * NULL context, count different from the instance count, unknown flag bits, flags without transforms, misaligned
 * device memory: PRT_ERR_INVALID_ARGUMENT.  No meshes or no instances yet: PRT_ERR_NOT_READY.  Device transforms on a
 * local group: PRT_ERR_UNSUPPORTED.  A worker build that failed earlier is reported as prt_update_instances reports
 * it.  Nothing changes in any of these cases.  On a local group or RCCL context a host-memory or NULL call applies
 * to every member. */
int prt_rebuild_instances(prt_ctx* ctx, const float* transforms, int32_t count, uint32_t in_flags, int32_t builder);
/* prt_blas_cost's measure (csrc/prt_blas_cost.h) of the instance BVH as it stands on the device; a leaf slot counts
 * one instance.  0 when the rays walk the linear list.  The same two kernels, no atomics: two calls return the same
 * bits.  The call joins the frames in flight and waits on the host once, for the 8 bytes of the result.  The library
 * has no rebuild policy: compare the cost after a prt_set_instances (a fresh SAH tree) with the cost after N refits.
 * NULL context or NULL cost: PRT_ERR_INVALID_ARGUMENT.  No meshes or no instances: PRT_ERR_NOT_READY. */
int prt_tlas_cost(prt_ctx* ctx, double* cost);
/* prt_read_blas's counterpart for the instance BVH, for tests and tools: the current tree's Node8 records (80 bytes
 * each, node 0 the root; csrc/bvh_build.h) into nodes and the 8 instance-slot words per node (0xFFFFFFFF where a slot
 * is no leaf slot) into slots, complete on return.  *nodes_needed / *slots_needed (each may be NULL) get the sizes in
 * bytes; nodes == NULL or slots == NULL reports only the sizes; a buffer that is too small returns
 * PRT_ERR_INVALID_ARGUMENT.  With the linear list both sizes are 0.  Joins the frames in flight and waits for the
 * context stream. */
int prt_read_tlas(prt_ctx* ctx, void* nodes, uint64_t node_bytes, uint32_t* slots, uint64_t slot_bytes,
                  uint64_t* nodes_needed, uint64_t* slots_needed);
/* count 0 (none) or 1 */
int prt_set_area_lights(prt_ctx* ctx, const prt_area_light* lights, int32_t count);
/* float RGB equirect, w*h*3; NULL/0 = no sky (misses shade 0 even with PRT_FLAG_SKYBOX) */
int prt_set_sky(prt_ctx* ctx, const float* rgb, int32_t width, int32_t height);
int prt_set_camera(prt_ctx* ctx, const prt_camera* cam);
/* Camera::Camera basis from position/target and aspect (Core/Camera.cpp:29-36) */
int prt_camera_look_at(const float pos[3], const float target[3], float aspect, prt_camera* out);

/* Post-processing (Renderer::isPostProcessed, Core/Renderer.h:48): Panini primary rays
 * (Camera::GetPrimaryRay/Panini, Core/Camera.cpp:81-139) and the screen pass of Core/Renderer.cpp:107-133
 * (chromatic aberration from the accumulator, vignette, colour grading).  avg_rgba stays the plain
 * average; rgb8 gets the post-processed pixel. */
typedef struct {
    int32_t enabled;            /* Renderer::isPostProcessed (default false) */
    int32_t aberration;         /* Camera::abberationIntensity, pixels */
    float fov;                  /* Camera::fov (Camera::Panini uses it as radians, :86) */
    float distortion;           /* Camera::distortion */
    float vignette_intensity;   /* Camera::vignetteIntensity */
    float vignette_radius;      /* Camera::vignetteRadius (the pow exponent) */
    float color_grading[4];     /* Camera::colorGrading */
} prt_postfx;
/* preset 0: the Camera member defaults (Core/Camera.h:12,23,27; DEBUGMODE build), 1: the GAME preset P1
 * (Core/Camera.cpp:18-23, vignetteRadius keeps its default: the constructor self-assigns it).
 * enabled is set to 1. */
int prt_postfx_preset(int32_t preset, prt_postfx* out);
int prt_set_postfx(prt_ctx* ctx, const prt_postfx* pfx);

/* ---- rendering (Renderer::Tick) ----
 * Traces params.spp camera paths per pixel as spp/2 (AA) or spp reference frames and folds each
 * frame into the persistent accumulation state exactly as Core/Renderer.cpp:81-104 does.
 * Outputs (either may be NULL): avg_rgba = float4 W*H average, rgb8 = 0x00RRGGBB W*H.
 * They are host pointers unless PRT_OUT_DEVICE is set in out_flags (then device pointers). */
#define PRT_OUT_DEVICE (1u << 0)
int prt_render(prt_ctx* ctx, const prt_render_params* params, float* avg_rgba, uint32_t* rgb8,
               uint32_t out_flags, prt_stats* stats);
/* Reset the accumulation state: memset of the accumulator (Core/Renderer.cpp:147) and, with
 * full != 0, also samplesPerPixel/distances (fresh Renderer). */
int prt_reset_accumulation(prt_ctx* ctx, int32_t full);
/* Running ray totals (ABI 7): closest-hit segments and shadow rays of every render since the context was created
 * or last reset, counted on the device at the end of each render (the figure behind the reference's ImGui ray
 * counter, Core/Renderer.cpp:467-474) so a frame loop need not pass prt_stats, which waits for each frame.  Waits for
 * the frames queued on the context's stream (a local group: on every member's, summed); reset != 0 zeroes the totals
 * after reading them. */
int prt_ray_totals(prt_ctx* ctx, uint64_t* segments, uint64_t* shadow_rays, int32_t reset);
/* Primary-hit reuse counters (additive within ABI 10).  Path 1 of a pixel starts at the pixel centre, so its
 * primary ray is the same in every reference frame while camera, resolution, tile map, geometry and instances stay
 * put; renders without extensions in render mode 0 trace it once per such state and reuse its hit (bit-identical
 * images; PRT_PRIMARY_REUSE=0 in the environment traces every item's ray every frame).  traced: path-1 primary rays
 * the calls so far handed to a traversal launch for reuse (one per pixel of the call's tile map); reused: those
 * whose hit was taken from the kept records instead.  Both stay 0 where the reuse does not apply.  Host bookkeeping
 * of the calls enqueued so far: no wait (a local group: summed over its members); reset != 0 zeroes them after
 * reading.  A reused primary segment is still a segment of its path: prt_ray_totals and prt_stats count it. */
int prt_primary_rays(prt_ctx* ctx, uint64_t* traced, uint64_t* reused, int32_t reset);
/* Shadow-ray reuse counter (additive within ABI 10).  The next-event shadow rays of a pixel's fixed path-1 primary
 * hit start at that hit and end at a light, so their answers repeat while the primary hits (above) and the positions
 * of the point, directional and spot lights stay put.  Calls that reuse the primary hits record each answer the first
 * time a frame traces it and skip the ray afterwards (bit-identical images; PRT_SHADOW_REUSE=0 in the environment
 * switches only this off, PRT_PRIMARY_REUSE=0 both).  A call that traces the primary hits anew neither reads nor
 * fills the record, so the skipping starts with the third call of a static view; new light positions clear the record
 * but keep the primary hits, colours and materials keep both.  reused: the shadow rays answered from the record so
 * far, counted on the device; waits for the frames queued on the context's stream like prt_ray_totals (a local group:
 * summed over its members); reset != 0 zeroes it after reading.  A skipped shadow ray is still a shadow ray of its
 * path: prt_ray_totals and prt_stats count it. */
int prt_shadow_reuse(prt_ctx* ctx, uint64_t* reused, int32_t reset);
/* Primary-surface reuse counter (additive within ABI 10).  What the shading of a pixel's fixed path-1 primary hit
 * reads before any random draw -- the shading normal, the material, the hit point, or the sky radiance of a miss --
 * repeats while the primary hits (above), the textures, the sky, the instance materials and the call's
 * PRT_FLAG_NORMALMAP and PRT_FLAG_SKYBOX bits stay put.  In the plain wavefront pipeline (render mode 0, no area
 * light or dielectrics, not the merged small-call form) the first call that reuses the primary hits keeps those values
 * per pixel and later calls shade from them (bit-identical images; PRT_SURFACE_REUSE=0 in the environment switches
 * only this off, PRT_SHADOW_REUSE=0 and PRT_PRIMARY_REUSE=0 switch it off too; PRT_INIT_FOLD=0 keeps the wave-init
 * launch in front of a pass that shades from the kept values).  Lights are no part of it.  reused:
 * the work items (pixels x reference frames) shaded from the kept values by the calls so far; host bookkeeping like
 * prt_primary_rays, no wait (a local group: summed over its members); reset != 0 zeroes it after reading. */
int prt_surface_reuse(prt_ctx* ctx, uint64_t* reused, int32_t reset);
/* Dead shadow-ray counter (additive within ABI 10).  A next-event shadow ray is dead when the factor its visibility
 * answer is multiplied by is exactly zero: PRT_FLAG_LIGHTED is off, or every channel of its unoccluded contribution
 * compares equal to zero (the light is behind the shading normal, the hit point is outside the spot's cone, the
 * light is black), or the one BRDF value all the item's rays are multiplied by is zero in every channel (the shading
 * normal faces away from the viewer or from the light the BRDF is evaluated for) while their contributions are
 * bounded.  Renders count such rays of the point, directional and spot lights instead of tracing them
 * (bit-identical images; PRT_DEAD_SHADOW in the environment is a level: 0 traces them all, 1 leaves the BRDF rule
 * out, unset or anything else applies both; the debug render modes cast no shadow rays, and an area light's own ray
 * is traced as ever).  Rays under the light-visibility record
 * (prt_shadow_reuse) are asked, learned and counted there as before.  dead: the shadow rays skipped this way so
 * far, counted on the device; waits like prt_shadow_reuse (a local group: summed over its members); reset != 0
 * zeroes it after reading.  A dead shadow ray is still a shadow ray of its path: prt_ray_totals and prt_stats count
 * it. */
int prt_shadow_dead(prt_ctx* ctx, uint64_t* dead, int32_t reset);

/* ---- checkpoint / resume of the progressive accumulation (the reference keeps it in memory only) ----
 * The accumulation state Renderer holds between Ticks (Core/Renderer.h:61-63: accumulator, samplesPerPixel,
 * distances) as one opaque blob with a header recording the image and shard geometry it belongs to.
 * prt_accumulation_bytes: the blob size (0 before the first render).  prt_save_accumulation: copies the state
 * out (waits for the frames queued on the context's stream).  prt_load_accumulation: restores it into a context
 * of the same shard geometry; the next prt_render with the same image size continues bit-identically (the caller
 * restores its frame_index too: the RNG stream is keyed by it).  A mismatched or truncated blob:
 * PRT_ERR_INVALID_ARGUMENT; a local group (prt_create_group): PRT_ERR_UNSUPPORTED (one blob per rank's context
 * with RCCL). */
int prt_accumulation_bytes(prt_ctx* ctx, uint64_t* bytes);
int prt_save_accumulation(prt_ctx* ctx, void* blob, uint64_t bytes);
int prt_load_accumulation(prt_ctx* ctx, const void* blob, uint64_t bytes);

/* ---- multi-GPU inside the boundary ----
 * A sharded context renders only its rank's pixel tiles (tile_size x tile_size, numbered row-major, dealt
 * round-robin: rank r owns tiles r, r + world, ...), and prt_render gathers the per-rank tile buffers on
 * rank 0 once per frame, replacing the reference's single-process OpenMP row loop (Core/Renderer.cpp:43).
 * Rank 0's outputs then hold the whole frame; the other ranks' outputs are not written (may be NULL).
 * Stats count the calling rank's rays (a local group sums its members, stats.ranks = world).
 * Post-processing shards except the chromatic aberration (neighbours' accumulators): PRT_ERR_UNSUPPORTED.
 *
 * One process per GPU over RCCL (xGMI): rank 0 makes an id, the caller carries its bytes to the other
 * ranks over any host channel (torch.distributed, MPI, a file), every rank joins with its own context.
 * The context owns the communicator; RCCL is loaded on first use (the copy the process already holds). */
#define PRT_SHARD_ID_BYTES 128
int prt_shard_unique_id(uint8_t id[PRT_SHARD_ID_BYTES]);
int prt_shard_init_rccl(prt_ctx* ctx, const uint8_t id[PRT_SHARD_ID_BYTES], int32_t rank, int32_t world,
                        int32_t tile_size);
/* ... or an existing communicator (ncclComm_t, not owned: the caller destroys it after prt_destroy) */
int prt_shard_attach_rccl(prt_ctx* ctx, void* nccl_comm, int32_t tile_size);
/* One process, several devices (prt_create with a device list).  The group context is member 0;
 * every setter applies to all members, prt_render renders all shards concurrently (one stream per member)
 * and gathers them on member 0 with device-to-device copies.  A device may repeat (several shards on one
 * GPU: how the decomposition is tested on a one-GPU box). */
int prt_create_group(const prt_device_desc* devices, int32_t count, int32_t tile_size, prt_ctx** out);
typedef struct {
    int32_t rank, world, tile_size;
    int32_t transport;      /* 0 = none (whole frame), 1 = RCCL, 2 = local group */
} prt_shard_info;
int prt_get_shard_info(prt_ctx* ctx, prt_shard_info* info);

/* ---- pixel-tile sharding with a caller-side transport (the building blocks of the above) ----
 * The image is cut into tile_size x tile_size tiles numbered in row-major order; rank r renders
 * tiles r, r+world, r+2*world, ...  into a compact float4 buffer laid out
 * [local_tile][tile_size*tile_size] (pixels outside the image are written as 0).
 * prt_tile_buffer_pixels() gives the element count (per rank, equal on all ranks: the max). */
int prt_tile_buffer_pixels(int32_t width, int32_t height, int32_t tile_size, int32_t world, int64_t* pixels);
/* host-only: image pixel index (y*width + x) of every element of rank's tile buffer, -1 where the tile
 * overhangs the image; pixel_of_slot holds prt_tile_buffer_pixels() entries.  No device needed. */
int prt_tile_pixel_map(int32_t width, int32_t height, int32_t tile_size, int32_t rank, int32_t world,
                       int32_t* pixel_of_slot);
int prt_render_tiles(prt_ctx* ctx, const prt_render_params* params, int32_t tile_size, int32_t rank,
                     int32_t world, float* tiles_rgba_device, prt_stats* stats);
/* rank-0 side: gathered [world][tile_buffer_pixels] float4 device buffer -> W*H avg_rgba + rgb8 (device).
 * With post-processing the vignette / grading apply to rgb8; chromatic aberration needs the neighbours'
 * accumulators, which stay on their ranks: PRT_ERR_UNSUPPORTED there. */
int prt_untile(prt_ctx* ctx, const float* gathered_device, int32_t width, int32_t height, int32_t tile_size,
               int32_t world, float* avg_rgba_device, uint32_t* rgb8_device);

/* ---- geometry-only queries (the traversal kernels on their own) ---- */
/* primary-ray closest hits for every pixel (config C2): out = W*H prt_hit (host or device per out_flags) */
int prt_trace_primary(prt_ctx* ctx, int32_t width, int32_t height, prt_hit* hits, uint32_t out_flags,
                      prt_stats* stats);
/* arbitrary rays: origins/dirs float3 x n (dirs normalised like the tinybvh::Ray ctor), tmax n (NULL = 1e30).
 * prt_intersect: the closest hit with 0 < t < tmax (strict, as tinybvh's t < ray.hit.t: a triangle at exactly tmax
 * is no hit, in whatever instance); among hits of equal t the smaller instance wins, then the larger prim.  A miss
 * is the record t = tmax, u = v = 0, prim = inst = 0.
 * prt_occluded: 1 when any triangle is hit with 0 < t < tmax (strict as well), else 0. */
int prt_intersect(prt_ctx* ctx, int32_t n, const float* origins, const float* dirs, const float* tmax,
                  prt_hit* hits);
int prt_occluded(prt_ctx* ctx, int32_t n, const float* origins, const float* dirs, const float* tmax,
                 int32_t* occluded);

/* ---- ray queries on caller arrays, in stream order (ABI 10, additive; DESIGN.md "Ray queries") ----
 * Both calls first join the frames in flight, run on the context stream (prt_set_stream) and mark their read of the
 * instance state as a frame does: a later prt_update_instances, prt_rebuild_instances or prt_set_instances waits for
 * them in stream order.  They touch neither the accumulation state nor the ray totals.  io_flags = 0: every pointer is
 * host memory and the results are complete on return.  io_flags = PRT_OUT_DEVICE: every pointer is device memory on
 * the context's device, 4-byte aligned, read and written only by the call's own kernels in the context stream's order;
 * the call never waits on the host and, after the first call on a scene with at least this n, allocates nothing.  On a
 * sharded or group context they run on the calling member over the whole scene.
 * Errors: NULL context, n < 0, n > 1 << 28, missing arrays or unknown io_flags bits: PRT_ERR_INVALID_ARGUMENT; no
 * scene: PRT_ERR_NOT_READY; n = 0: PRT_OK, nothing enqueued. */

/* (ABI 10, additive) n rays on the persistent traversal kernels: origins / dirs float3 x n, tmax n floats or NULL
 * (1e30 each).  hits[i]: the closest hit; occluded[i]: the any-hit answer; either may be NULL (both NULL:
 * PRT_ERR_INVALID_ARGUMENT), both given are answered in one launch.  For a traversed ray hits[i] is bit for bit
 * prt_intersect's record for that ray and tmax, occluded[i] prt_occluded's answer.
 * A ray is never traversed when an origin or direction component is not finite, the direction has zero length (its
 * float32 normalisation is not finite) or tmax is NaN or <= 0: it gets the miss record with t = tmax as given (or
 * 1e30) and occluded = 0.  BVH deeper than 64 levels: PRT_ERR_UNSUPPORTED. */
int prt_query_rays(prt_ctx* ctx, int32_t n, const float* origins, const float* dirs, const float* tmax,
                   prt_hit* hits, int32_t* occluded, uint32_t io_flags);
/* (ABI 10, additive) The shading inputs at n hit records, by the kernels' own hit-attribute code; traces nothing.
 * Record i is a hit iff hits[i].t < (tmax ? tmax[i] : 1e30f): pass the tmax the query ran under (the miss record alone
 * is ambiguous under a tmax).  A record that names no instance or primitive of the scene counts as a miss.  flags:
 * only PRT_FLAG_NORMALMAP is read.  Every output may be NULL:
 *   albedo_rgba     float4 x n: prt_render_aov's albedo_rgba; miss: 0,0,0,0
 *   normal_depth    float4 x n: prt_render_aov's normal_depth (w = hits[i].t); miss: 0,0,0,1e30
 *   geometry_normal float4 x n: xyz = the geometry normal as Trace uses it (Core/Scene.cpp:47-58), w = 1; miss: 0,0,0,0
 *   material        float x 8n: MaterialProperties in prt_brdf_probe's order -- base rgb, metalness, emissive rgb,
 *                   roughness; miss: eight zeros */
int prt_query_surface(prt_ctx* ctx, int32_t n, const prt_hit* hits, const float* tmax, uint32_t flags,
                      float* albedo_rgba, float* normal_depth, float* geometry_normal, float* material,
                      uint32_t io_flags);

/* ---- first-hit feature buffers and the denoiser they guide (ABI 10, additive; DESIGN.md "Denoiser") ----
 * Both calls first join the frames in flight and run on the context stream; with device pointers they do not wait
 * on the host.  Their scratch buffers belong to the context.  On a sharded or group context they run over the whole
 * image on the calling (member 0) device, with no collective. */

/* (ABI 10, additive) First-hit feature buffers of the current scene and camera at pixel centres (the unjittered
 * path-1 primary ray, Panini when post-processing is on).  Any output may be NULL; host pointers unless PRT_OUT_DEVICE.
 *   albedo_rgba  float4 W*H: rgb = MaterialProperties::baseColor as PRT_MODE_BASECOLOR shows it, w = 1; miss: 0,0,0,0
 *   normal_depth float4 W*H: xyz = the shading normal exactly as Trace uses it (NOT normalised in the smooth
 *                branch, Core/Scene.cpp:134-136), w = primary hit t; miss: 0,0,0,1e30
 * flags: only PRT_FLAG_NORMALMAP is read.  Does not touch the accumulation state or the ray totals.
 * No scene or camera: PRT_ERR_NOT_READY. */
int prt_render_aov(prt_ctx* ctx, int32_t width, int32_t height, uint32_t flags,
                   float* albedo_rgba, float* normal_depth, uint32_t out_flags);

/* (ABI 10, additive) Out of range (PRT_ERR_INVALID_ARGUMENT): iterations, normal_power, a negative or non-finite
 * sigma, sigma_color or sigma_depth 0. */
typedef struct {
    int32_t iterations;     /* 1..8, step 2^i in iteration i                       default 5    */
    int32_t normal_power;   /* log2 of the normal exponent, 0..7 (3 -> dot^8)      default 3    */
    float sigma_color;      /* halves every iteration                              default 4.0  */
    float sigma_depth;      /* relative depth change per pixel of tap distance     default 0.1  */
    float sigma_albedo;     /* 0 = albedo not used as a guide                      default 0.25 */
} prt_denoise_params;
/* (ABI 10, additive) host only, no context */
int prt_denoise_defaults(prt_denoise_params* out);

/* (ABI 10, additive) Edge-avoiding a-trous filter of a W*H float4 image (prt_render's avg_rgba) guided by
 * prt_render_aov's buffers.  out_rgba (w copied from the input) and out_rgb8 (RGBF32_to_RGB8 of out, no screen pass)
 * may each be NULL, not both; out_rgba may be color_rgba itself.  albedo_rgba may be NULL when sigma_albedo is 0.
 * All pointers host, or all device with PRT_OUT_DEVICE. */
int prt_denoise(prt_ctx* ctx, const prt_denoise_params* params, int32_t width, int32_t height, const float* color_rgba,
                const float* albedo_rgba, const float* normal_depth, float* out_rgba, uint32_t* out_rgb8,
                uint32_t out_flags);

/* (ABI 10, additive) With PRT_OUT_TIMED in out_flags, prt_render_aov and prt_denoise record HIP events around their
 * passes; prt_denoise_timings waits for the context stream and returns the device times in ms of the last timed
 * calls: ms[0] the AOV pass (primary hits + attributes), ms[1] the denoiser's prep pass, ms[2 + i] filter iteration i.
 * count = 1..PRT_DENOISE_TIMINGS; entries that did not run are 0. */
#define PRT_OUT_TIMED (1u << 1)
#define PRT_DENOISE_TIMINGS 10
int prt_denoise_timings(prt_ctx* ctx, float* ms, int32_t count);

/* ---- temporal reprojection of the frame history under camera motion (ABI 10, additive; DESIGN.md "Temporal
 * reprojection") ----
 * (ABI 10, additive) Out of range (PRT_ERR_INVALID_ARGUMENT): a negative or non-finite depth_tol, a normal_min outside
 * [-1, 1] or non-finite, a max_history that is non-finite or below 1. */
typedef struct {
    float depth_tol;     /* relative depth difference a history tap may have      default 0.05 */
    float normal_min;    /* least dot of the unit normals of pixel and tap        default 0.9  */
    float max_history;   /* cap of the history length, >= 1                       default 16   */
} prt_reproject_params;
/* (ABI 10, additive) host only, no context */
int prt_reproject_defaults(prt_reproject_params* out);

/* (ABI 10, additive) One stateless pass: the first hit of every pixel of this view is projected into the previous
 * view, the previous output is gathered there with bilinear weights from the taps whose depth and unit normal agree
 * (depth_tol, normal_min) and whose history length is >= 1, and this frame is blended in with weight 1 / length,
 * length = min(gathered length + 1, max_history).  A miss, a point behind or off the previous screen, or taps of
 * total weight <= 1/64 start over: out = (color.rgb, 1).
 *   color_rgba            this frame's image (prt_render's avg_rgba; its w is ignored)
 *   normal_depth          this view's prt_render_aov buffer
 *   camera                this view's camera
 *   prev_camera           the previous view's camera
 *   history_rgba          a previous out_rgba: rgb = the history, w = its length.  A raw avg_rgba (w = 0) is rejected
 *                         tap by tap and so behaves as no history
 *   history_normal_depth  the previous view's prt_render_aov buffer
 * The three prev / history arguments are all NULL (a history starts: out = (color.rgb, 1)) or all given; a mix is
 * PRT_ERR_INVALID_ARGUMENT.  out_rgba (w = the new history length) and out_rgb8 (RGBF32_to_RGB8 of out, no screen
 * pass) may each be NULL, not both.  out_rgba may be color_rgba; it must not be history_rgba or
 * history_normal_depth (neighbouring pixels are gathered): PRT_ERR_INVALID_ARGUMENT.
 * All image pointers host, or all device with PRT_OUT_DEVICE; the cameras are always host structs.  Like prt_denoise
 * the call joins the frames in flight, runs on the context stream, does not wait on the host with device pointers,
 * stages host images through context buffers, touches neither the accumulation state nor the ray totals, and on a
 * sharded or group context runs over the whole image on member 0's device.
 * Defined for the plane projection only: with Panini primary rays (post-processing on) the cameras do not describe
 * the rays, and this call cannot know -- the caller must not use it then (the Renderer mirrors refuse).  Only the
 * camera moves here: a moving instance's pixels are rejected by the depth and normal tests, or ghost.
 * prt_reproject_motion below follows the instances too. */
int prt_reproject(prt_ctx* ctx, const prt_reproject_params* params, int32_t width, int32_t height,
                  const prt_camera* camera, const float* color_rgba, const float* normal_depth,
                  const prt_camera* prev_camera, const float* history_rgba, const float* history_normal_depth,
                  float* out_rgba, uint32_t* out_rgb8, uint32_t out_flags);

/* ---- moving instances in the temporal reprojection (ABI 10, additive; DESIGN.md "Moving instances") ----
 * The frame loop: prt_set_instances -> prt_render -> prt_render_aov_ids -> prt_instance_motion ->
 * prt_reproject_motion -> prt_denoise. */

/* (ABI 10, additive) prt_render_aov with one more output, from the same single primary-hit pass:
 *   instance  uint32 W*H: the index of the first hit's instance, as prt_trace_primary reports it in prt_hit.inst;
 *             a miss: 0xFFFFFFFF
 * Everything else is prt_render_aov's contract: joins the frames in flight, runs on the context stream, any output
 * may be NULL, host pointers unless PRT_OUT_DEVICE, PRT_OUT_TIMED times the whole pass (ms[0] of
 * prt_denoise_timings). */
int prt_render_aov_ids(prt_ctx* ctx, int32_t width, int32_t height, uint32_t flags,
                       float* albedo_rgba, float* normal_depth, uint32_t* instance, uint32_t out_flags);

/* (ABI 10, additive) host only, no context.  Per instance the motion matrix A = prev * inverse(cur), which carries a
 * world-space point of this frame to where that point of the instance was in the previous frame.  transforms and
 * prev_transforms are count row-major 4x4 matrices as prt_set_instances takes them, read as affine (the last row is
 * ignored); motion receives count row-major 3x4 matrices (12 floats each), computed in double and rounded once.
 * An instance whose 16 floats are bytewise equal in both arrays gets the exact identity (1,0,0,0, 0,1,0,0, 0,0,1,0).
 * So does one whose current transform is non-finite or has determinant 0: such an instance covers no pixel, so its
 * matrix is never read for a hit.  count 0 is allowed; a NULL array with count > 0 or a negative count is
 * PRT_ERR_INVALID_ARGUMENT. */
int prt_instance_motion(const float* transforms, const float* prev_transforms, int32_t count, float* motion);

/* (ABI 10, additive) prt_reproject with the instances' motion taken into account.  With i = instance[p] and
 * A = motion[i], the pixel's world-space hit X is carried back to X' = A * (X, 1) before it is projected into the
 * previous view (the previous depth compared with the taps is |X' - prev pos|), the pixel's normal for the tap test
 * is unit(A3x3 * N), and with history_instance given a tap q is kept only if history_instance[q] == i as well.
 * A hit pixel with i >= count starts over and no matrix is read for it.  Everything else -- the operations, their
 * order, the taps, the start-over rules, the outputs -- is prt_reproject's definition.  With identity matrices and
 * history_instance NULL the output equals prt_reproject's bit for bit.
 * The normal is transformed by A's 3x3 part itself, which is exact for rotations and uniform scales (what a physics
 * engine produces) and approximate under non-uniform scale, where the inverse transpose would be needed.
 *   instance              this view's prt_render_aov_ids buffer (required when there is a history)
 *   history_instance      the previous view's, or NULL: taps are not compared by instance
 *   motion, count         count 3x4 matrices (prt_instance_motion, or the caller's own): always a host array like the
 *                         cameras, copied before the call returns and uploaded in the context stream's order
 * Either prev_camera, history_rgba, history_normal_depth, history_instance and motion are all NULL and count is 0 (a
 * history starts: out = (color.rgb, 1)), or prev_camera, history_rgba, history_normal_depth and motion are all given
 * with count > 0 (history_instance stays optional); anything else is PRT_ERR_INVALID_ARGUMENT, and so is an out_rgba
 * that is history_rgba or history_normal_depth, or an out_rgb8 that is history_instance.  out_rgba may be color_rgba.
 * Image pointers all host, or all device with PRT_OUT_DEVICE (then the call does not wait on the host).  What
 * prt_reproject says about frames in flight, sharded contexts, side effects and Panini holds here too.
 * Not tracked: lighting that changes because an object moved (its shadow on a static surface lags by up to
 * max_history frames; prt_reproject_moments' clamp_k below shortens that).  Deforming meshes are followed by
 * prt_reproject_deform below. */
int prt_reproject_motion(prt_ctx* ctx, const prt_reproject_params* params, int32_t width, int32_t height,
                         const prt_camera* camera, const float* color_rgba, const float* normal_depth,
                         const uint32_t* instance, const prt_camera* prev_camera, const float* history_rgba,
                         const float* history_normal_depth, const uint32_t* history_instance, const float* motion,
                         int32_t count, float* out_rgba, uint32_t* out_rgb8, uint32_t out_flags);

/* ---- luminance moments and the variance-guided filter (ABI 10, additive; DESIGN.md "Variance guidance") ----
 * The frame loop: prt_set_instances -> prt_render -> prt_render_aov_ids -> prt_instance_motion ->
 * prt_reproject_moments -> prt_denoise_variance; out_rgba and out_moments (not the filtered image) are the next
 * frame's history. */
typedef struct {
  float depth_tol, normal_min, max_history; /* as prt_reproject_params: same defaults (0.05, 0.9, 16), same ranges */
  float clamp_k;      /* 0 = no clamp (default); > 0: the gathered history is clamped per channel to
                         mean +- clamp_k * sigma of this frame's 3x3 neighbourhood; finite, >= 0 */
  float min_temporal; /* history length from which the variance comes from the moments; finite, >= 1, default 4 */
} prt_temporal_params;

/* host only, no context */
int prt_temporal_defaults(prt_temporal_params* out);

/* (ABI 10, additive) prt_reproject_motion that also carries the first two moments of the luminance
 * L(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z with the history and estimates its variance.
 *   moments images   float4 per pixel: x = first moment, y = second moment, z = the variance estimate
 *                    prt_denoise_variance reads, w = 0
 * A pixel with history (k_reproject_motion's rules decide, with the same taps q, weights wb, sum ws, length len and
 * a = 1 / len): hm1 = (sum wb * M_q.x) / ws and hm2 likewise over the kept taps in the colour gather's order; with
 * clamp_k > 0 the gathered colour h is clamped per channel to [mu - k sigma, mu + k sigma], where over the in-image
 * pixels of the 3x3 neighbourhood of p in color_rgba (row-major, n of them) mu = (sum c) / n and
 * sigma = sqrt(max((sum c * c) / n - mu * mu, 0)); then the colour blends as in prt_reproject_motion,
 * m1 = hm1 + a * (L - hm1), m2 = hm2 + a * (L * L - hm2).  A pixel that starts over (no history given, a miss, an id
 * >= count, behind or off the previous screen, ws <= 1/64) has out = (color.rgb, 1), m1 = L, m2 = L * L, len = 1.
 * The variance: 0 for a miss; max(m2 - m1 * m1, 0) when len >= min_temporal; otherwise the spatial estimate
 * max(s2 / n - mu * mu, 0) * (min_temporal / len) with s1 = sum L_q, s2 = sum L_q * L_q, mu = s1 / n over the pixels q
 * of the 5x5 window of p (row-major, inside the image) that are hits (normal_depth.w < 1e30) with
 * instance[q] == instance[p].
 * With clamp_k == 0 out_rgba and out_rgb8 equal prt_reproject_motion's bit for bit.
 * Arguments as prt_reproject_motion, except:
 *   instance         always required (the 5x5 window compares ids even when a history starts)
 *   history_moments  the previous call's out_moments: given with prev_camera, history_rgba, history_normal_depth and
 *                    motion (count > 0), or NULL with all of them (history_instance stays optional)
 *   out_moments      required; must not be history_moments
 *   out_rgba         must not be color_rgba: unlike prt_reproject_motion this pass reads the neighbours of color_rgba
 *                    (the clamp's 3x3 and the variance's 5x5 window), which another thread may already have overwritten
 * Anything else is PRT_ERR_INVALID_ARGUMENT.  Host / device pointers, frames in flight, the stream, sharded contexts,
 * side effects and Panini: as prt_reproject_motion. */
int prt_reproject_moments(prt_ctx* ctx, const prt_temporal_params* params, int32_t width, int32_t height,
                          const prt_camera* camera, const float* color_rgba, const float* normal_depth,
                          const uint32_t* instance, const prt_camera* prev_camera, const float* history_rgba,
                          const float* history_normal_depth, const uint32_t* history_instance, const float* motion,
                          int32_t count, const float* history_moments, float* out_rgba, float* out_moments,
                          uint32_t* out_rgb8, uint32_t out_flags);

typedef struct {
  int32_t iterations, normal_power;             /* as prt_denoise_params: 1..8, 0..7 */
  float sigma_color, sigma_depth, sigma_albedo; /* as prt_denoise_params; sigma_color is in standard deviations here */
  float color_decay;    /* sigma_color is multiplied by this after every iteration; > 0, finite; default 1
                           (0.5 is prt_denoise's schedule) */
  float variance_floor; /* > 0, finite; default 1e-6 */
} prt_denoise_variance_params;

/* host only, no context: iterations 5, normal_power 3, sigma_color 2, sigma_depth 0.1, sigma_albedo 0.25,
 * color_decay 1, variance_floor 1e-6 */
int prt_denoise_variance_defaults(prt_denoise_variance_params* out);

/* (ABI 10, additive) prt_denoise with the colour weight scaled by the variance of `moments` (its z; x, y and w are not
 * read).  Iteration i has step 2^i, I_0 = color, V_0 = moments.z; the taps, their order, the B3 weights, the centre
 * weight, the normal, depth and albedo weights and the miss pass-through are prt_denoise's.  Per hit pixel p:
 *   Vp = max(G / g, variance_floor) with G = sum g_q * V_i(q), g = sum g_q over the hits of the 3x3 neighbourhood of
 *   p inside the image (row-major; g_q = 1/16 corner, 1/8 edge, 1/4 centre)
 *   wc = 1 / (1 + c2 / (sc_i * sc_i * Vp)), sc_0 = sigma_color, sc_{i+1} = sc_i * color_decay (host, float)
 *   V_{i+1}(p) = (sum w * w * V_i(q)) / ((sum w) * (sum w)) over the kept taps; a miss keeps its V
 * out_rgba.w is copied from color_rgba; out_variance (float W*H, may be NULL) receives the last V.  out_rgba may be
 * color_rgba.  With moments.z == 1 everywhere, variance_floor <= 1, color_decay 0.5 and iterations 1 the colour output
 * is prt_denoise's bit for bit.  albedo_rgba may be NULL when sigma_albedo == 0.  Host / device pointers,
 * PRT_OUT_TIMED (ms[1] prep, ms[2 + i] iteration i of prt_denoise_timings), frames in flight and sharded contexts: as
 * prt_denoise. */
int prt_denoise_variance(prt_ctx* ctx, const prt_denoise_variance_params* params, int32_t width, int32_t height,
                         const float* color_rgba, const float* moments, const float* albedo_rgba,
                         const float* normal_depth, float* out_rgba, float* out_variance, uint32_t* out_rgb8,
                         uint32_t out_flags);

/* ---- deforming meshes in the temporal reprojection (ABI 10, additive; DESIGN.md "Deforming meshes") ----
 * The frame loop: prt_update_mesh -> prt_set_instances -> prt_render -> prt_render_aov_deform -> prt_instance_motion ->
 * prt_reproject_deform -> prt_denoise_variance -> prt_snapshot_mesh.  The snapshot at the end makes this frame's
 * geometry the next frame's previous geometry; a mesh that is not updated in the following frame then has offset 0
 * (INTEGRATION.md). */

/* (ABI 10, additive) prt_render_aov_ids with one more output, from the same single primary-hit pass:
 *   offset  float4 W*H.  For a hit pixel whose instance's mesh has a snapshot (prt_snapshot_mesh), with (prim, u, v)
 *           as prt_trace_primary reports them, c_k the mesh's current corners of prim and q_k the snapshotted ones
 *           (k = 0..2): d_k = q_k - c_k per component, w0 = (1 - u) - v,
 *           offset.xyz = (w0 * d_0 + u * d_1) + v * d_2 per component, offset.w = 1; every operation a correctly
 *           rounded f32, no contraction.  A miss, or a mesh without a snapshot: (0, 0, 0, 0).
 * The offset is in the mesh's object space: the displacement from where the surface point is now to where it was at
 * the snapshot.  A snapshot that equals the current positions gives exactly (0, 0, 0, 1).
 * Everything else is prt_render_aov_ids' contract: every output may be NULL, host pointers unless PRT_OUT_DEVICE,
 * PRT_OUT_TIMED times the whole pass including the offset (ms[0] of prt_denoise_timings), no effect on the
 * accumulation or the ray totals; the other three outputs equal prt_render_aov_ids' bit for bit. */
int prt_render_aov_deform(prt_ctx* ctx, int32_t width, int32_t height, uint32_t flags, float* albedo_rgba,
                          float* normal_depth, uint32_t* instance, float* offset, uint32_t out_flags);

/* (ABI 10, additive) prt_reproject_moments whose carried-back point follows the deformation.  The definition is
 * prt_reproject_moments' word for word with one change.  With i = instance[p], A = motion[i], L the upper-left 3x3 of
 * prev_transforms[i], delta = offset[p].xyz and X the pixel's world-space hit, row r of the point carried back is
 *   offset[p].w != 0:  X'_r = row4(A_r, X) + ((L_r.x * delta.x + L_r.y * delta.y) + L_r.z * delta.z)
 *   offset[p].w == 0:  X'_r = row4(A_r, X), as in prt_reproject_moments
 * where row4(A_r, X) = ((A_r.x * X.x + A_r.y * X.y) + A_r.z * X.z) + A_r.w.  Since A = T_prev * inverse(T_cur), X' is
 * T_prev applied to the object-space point at its previous position.  Everything after X' is unchanged: the
 * projection, the previous depth, the taps, the id test, the moments, the clamp, the spatial variance and the
 * start-over rules.
 * The normal used for the tap test stays unit(A3x3 * N): previous normals are not kept, so a deformation that turns
 * the surface by more than acos(normal_min) between two frames loses that pixel's history.
 *   offset           this view's prt_render_aov_deform buffer: an image pointer under the same host / device rule as
 *                    the others; must not be an output
 *   prev_transforms  always a host array: count row-major 4x4 matrices, the previous frame's prt_set_instances input
 *                    (what prt_instance_motion took as prev_transforms).  Only the upper-left 3x3 is read.  Copied
 *                    before the call returns and uploaded in the context stream's order with motion.
 * offset and prev_transforms are both NULL or both given, and given only together with a history; anything else is
 * PRT_ERR_INVALID_ARGUMENT.  Every other rule is prt_reproject_moments'.  With both NULL every output equals
 * prt_reproject_moments' bit for bit; so it does with an offset buffer whose xyz are all +0 and finite transforms
 * (a + 0 = a for every a but -0). */
int prt_reproject_deform(prt_ctx* ctx, const prt_temporal_params* params, int32_t width, int32_t height,
                         const prt_camera* camera, const float* color_rgba, const float* normal_depth,
                         const uint32_t* instance, const prt_camera* prev_camera, const float* history_rgba,
                         const float* history_normal_depth, const uint32_t* history_instance, const float* motion,
                         int32_t count, const float* history_moments, const float* offset,
                         const float* prev_transforms, float* out_rgba, float* out_moments, uint32_t* out_rgb8,
                         uint32_t out_flags);

/* ---- shading-function probe (ABI 10): the device's own BRDF functions (the ones the shading kernels inline) on
 * n host records, for known-answer tests of the BRDF restatement (Core/BRDF.cpp).  Record k: in[24 k ..], out[8 k ..].
 *   EVAL         BRDF::evalCombinedBRDF (:439-452)     in N[0..2] L[3..5] V[6..8] material[9..16]    out rgb[0..2]
 *   PROBABILITY  BRDF::getBrdfProbability (:504-526)   in N, V, material                          out p[0]
 *   INDIRECT     BRDF::evalIndirectCombinedBRDF (:454-502, weight in = 1)  in N, V, material, u[17..18],
 *                type[19] (1 diffuse, 2 specular)      out ok[0] dir[1..3] weight[4..6]
 *   GGX_D        ggxD (:218-222)                       in alphaSquared[0] NdotH[1]                out D[0]
 *   SMITH_G2     Smith_G2 height-correlated, divided by the denominator (:189-208)
 *                                                      in alphaSquared[0] NdotL[1] NdotV[2]       out G2[0]
 *   FRESNEL      evalFresnel Schlick (:84-87)          in f0[0..2] f90[3] NdotS[4]                out F[0..2]
 *   SHADOWED_F90 shadowedF90 (:100-104)                in F0[0..2]                                out f90[0]
 *   VNDF         sampleGGXVNDF (:224-269)              in Ve[0..2] alphaX[3] alphaY[4] u[5..6]    out H[0..2]
 *   TEXEL        the texel addressing of prt_mesh.fixed_uvs (Core/Scene.cpp:79-85,160-165) with a w x h albedo
 *                                                      in uv[0..1] w[2] h[3]                      out iu[0] iv[1]
 *                w and h are integers in 1..16384 held in floats, anything else is PRT_ERR_INVALID_ARGUMENT; iu and
 *                iv are the texel's column and row (index = iu + iv * w) as floats.
 * material = base rgb, metalness, emissive rgb, roughness (MaterialProperties, Core/BRDF.h:165-176). */
#define PRT_PROBE_EVAL 0
#define PRT_PROBE_PROBABILITY 1
#define PRT_PROBE_INDIRECT 2
#define PRT_PROBE_GGX_D 3
#define PRT_PROBE_SMITH_G2 4
#define PRT_PROBE_FRESNEL 5
#define PRT_PROBE_SHADOWED_F90 6
#define PRT_PROBE_VNDF 7
#define PRT_PROBE_TEXEL 8
int prt_brdf_probe(prt_ctx* ctx, int32_t op, int32_t n, const float* in, float* out);

/* ---- BLAS builder (the reference builds on the CPU, Core/tiny_bvh.h:1968-2284,3706-3781)
 * HOST_SAH (default): binned SAH binary tree + SAH-optimal 8-wide collapse on the host.
 * GPU_LBVH: Morton-code LBVH (Karras 2012) + treelet restructuring + SAH-optimal 8-wide collapse on the device,
 * Node8 layout only.
 * Applies to the next prt_set_meshes.  Hits do not depend on the builder (order-independent hit rule). */
#define PRT_BUILDER_HOST_SAH 0
#define PRT_BUILDER_GPU_LBVH 1
#define PRT_BUILDER_HOST_SBVH 2  /* spatial splits (BVH::BuildHQ, Core/tiny_bvh.h:1968-2284) + SAH-optimal collapse */
#define PRT_BUILDER_GPU_PLOC 3   /* device PLOC clustering + SAH-optimal collapse */
int prt_set_bvh_builder(prt_ctx* ctx, int32_t builder);

/* ---- introspection ---- */
typedef struct {
    int64_t blas_nodes;     /* device BVH nodes over all meshes */
    int64_t blas_leaves;
    int64_t device_bytes;   /* BVH + triangle + shading arrays resident in HBM */
    int32_t max_depth;
    int32_t triangles;
    double  build_ms;       /* wall time of the last prt_set_meshes (BLAS builds + uploads) */
    int32_t builder;        /* PRT_BUILDER_* used by the last prt_set_meshes */
    int32_t tlas_depth;     /* levels of the instance BVH the rays walk (0: instances tested as a linear list) */
    int32_t tlas_rebuilds;  /* rebuilds of the instance BVH since the instance count last changed: one per
                               prt_set_instances */
    int32_t tlas_async;     /* (ABI 10) of those, built on the context's worker thread in stream order (every update
                               after the one that set the instance count) */
    int32_t tlas_median;    /* (ABI 10) of the worker's builds, balanced median-split trees: the SAH tree was deeper
                               than the traversal stacks were sized for at the instance count's first build */
    float   tlas_build_ms;     /* (ABI 10) wall time of the worker's last build (instance boxes + build + collapse) */
    float   tlas_build_cpu_ms; /* (ABI 10) its thread CPU time */
} prt_scene_info;
int prt_get_scene_info(prt_ctx* ctx, prt_scene_info* info);
/* (additive in ABI 10) The Node8 records of mesh mesh_index's BLAS (80 bytes each, node 0 = the root), for tests and
 * tools: waits for the context stream and copies them to host memory, child_base and tri_base made relative to the
 * mesh (the copy does not depend on where the mesh sits in the concatenated arrays).  *needed (optional) receives
 * the byte count; nodes == NULL only reports it; bytes < *needed: PRT_ERR_INVALID_ARGUMENT. */
int prt_read_blas(prt_ctx* ctx, int32_t mesh_index, void* nodes, uint64_t bytes, uint64_t* needed);
/* (additive in ABI 10) The TriMT leaf records of mesh mesh_index's BLAS (48 bytes each: v0[3], prim, e1[3], 0, e2[3],
 * 0, in leaf order, record i being what a node's tri_base + offset i names once tri_base is mesh-relative as
 * prt_read_blas returns it), for tests and tools: waits for the context stream and copies them to host memory.  prim
 * is the mesh-local primitive index, as the builders write it.  There is one record per reference: the mesh's
 * triangle count, or more under PRT_BUILDER_HOST_SBVH (a triangle cut by spatial splits sits in several leaves).
 * *needed, tris == NULL and bytes < *needed as for prt_read_blas. */
int prt_read_blas_tris(prt_ctx* ctx, int32_t mesh_index, void* tris, uint64_t bytes, uint64_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* PRT_H */
