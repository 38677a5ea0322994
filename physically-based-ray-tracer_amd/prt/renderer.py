"""Host-side mirror of the reference's Renderer / Scene / Camera API surface (Core/Renderer.h:12-112,
Core/Scene.h:12-80, Core/Camera.h:198-231), driving the MI355X hot path through the C ABI (include/prt.h).

The reference's hot loop (Renderer::Tick's OpenMP pixel loop + Renderer::Trace) becomes one
prt_render() call per Tick; everything Trace reads (models, BLAS instances, lights, sky, camera
basis) is handed over once and stays resident in HBM.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import check

F32 = np.float32


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    """The address of a host array; a raw device pointer, None or a ctypes argument as it is."""
    return a.ctypes.data if isinstance(a, np.ndarray) else a


def _images(n, device_out, timed=False, f32=(), u32=(), outs=()):
    """The images of an image-space call (AOVs, denoisers, reprojections) and its out-flags: (f32 inputs, u32 inputs,
    outputs, flags).  Host mode: the inputs (arrays or None) as contiguous [n,4] float32 / [n] uint32 arrays, and a
    fresh zeroed output per (given, columns, dtype) of `outs`: [n,4] for 4 columns, [n] for 1, None for 0.
    device_out: every image is a raw device pointer and stays as given.  _ptr() makes either the call's argument."""
    of = (_lib.OUT_DEVICE if device_out else 0) | (_lib.OUT_TIMED if timed else 0)
    if device_out:
        return list(f32), list(u32), [o[0] for o in outs], of
    f32 = [_f32(a).reshape(n, 4) if a is not None else None for a in f32]
    u32 = [np.ascontiguousarray(a, np.uint32).reshape(n) if a is not None else None for a in u32]
    return f32, u32, [np.zeros((n, 4) if k == 4 else n, dt) if k else None for _, k, dt in outs], of


@dataclass
class LightTransform:
    """LightTransform (Core/LightTransform.cpp:4-23): position, color, rotation."""
    position: np.ndarray
    color: np.ndarray
    rotation: np.ndarray = field(default_factory=lambda: np.zeros(3, F32))


class Camera:
    """Camera (Core/Camera.cpp:6-37,113-139): screen plane at 2*ahead, height 2, width 2*aspect."""

    def __init__(self, camPos, camTarget, aspect):
        self.camPos = _f32(camPos)
        self.camTarget = _f32(camTarget)
        self.aspect = np.float32(aspect)
        # post-process members (Core/Camera.h:12,23,27), read when Renderer.isPostProcessed is set
        self.colorGrading = np.ones(4, F32)
        self.fov, self.distortion, self.vignetteIntensity, self.vignetteRadius = 40.0, 40.0, 20.0, 0.3
        self.abberationIntensity = 0
        self.update()

    def postfx(self, enabled=True):
        pf = _lib.PostFx()
        pf.enabled = 1 if enabled else 0
        pf.aberration = int(self.abberationIntensity)
        pf.fov, pf.distortion = float(self.fov), float(self.distortion)
        pf.vignette_intensity, pf.vignette_radius = float(self.vignetteIntensity), float(self.vignetteRadius)
        for i in range(4):
            pf.color_grading[i] = float(self.colorGrading[i])
        return pf

    def update(self):
        L = _lib.load()
        cd = _lib.CameraDesc()
        check(L.prt_camera_look_at(self.camPos.ctypes.data, self.camTarget.ctypes.data, C.c_float(self.aspect),
                                   C.byref(cd)))
        self.desc = cd
        self.topLeft = np.array(cd.top_left[:], F32)
        self.topRight = np.array(cd.top_right[:], F32)
        self.bottomLeft = np.array(cd.bottom_left[:], F32)
        self.right = np.array(cd.right[:], F32)
        self.up = np.array(cd.up[:], F32)
        self.ahead = np.array(cd.ahead[:], F32)


def postfx_preset(preset=0, **overrides):
    """prt_postfx with Renderer::isPostProcessed on: preset 0 = the Camera member defaults, 1 = the GAME
    preset P1 (Core/Camera.cpp:18-23); keyword overrides set single fields (color_grading: 4 floats)."""
    pf = _lib.PostFx()
    check(_lib.load().prt_postfx_preset(preset, C.byref(pf)))
    for k, v in overrides.items():
        if k == "color_grading":
            for i in range(4):
                pf.color_grading[i] = float(v[i])
        else:
            setattr(pf, k, v)
    return pf


def denoise_defaults(**overrides):
    """prt_denoise_params at the library's defaults (prt_denoise_defaults); keyword overrides set single fields
    (iterations, normal_power, sigma_color, sigma_depth, sigma_albedo)."""
    dp = _lib.DenoiseParams()
    check(_lib.load().prt_denoise_defaults(C.byref(dp)))
    for k, v in overrides.items():
        if k not in dict(dp._fields_):
            raise TypeError(f"prt_denoise_params has no field {k!r}")
        setattr(dp, k, v)
    return dp


def reproject_defaults(**overrides):
    """prt_reproject_params at the library's defaults (prt_reproject_defaults); keyword overrides set single fields
    (depth_tol, normal_min, max_history)."""
    rp = _lib.ReprojectParams()
    check(_lib.load().prt_reproject_defaults(C.byref(rp)))
    for k, v in overrides.items():
        if k not in dict(rp._fields_):
            raise TypeError(f"prt_reproject_params has no field {k!r}")
        setattr(rp, k, v)
    return rp


def temporal_defaults(**overrides):
    """prt_temporal_params at the library's defaults (prt_temporal_defaults); keyword overrides set single fields
    (depth_tol, normal_min, max_history, clamp_k, min_temporal)."""
    tp = _lib.TemporalParams()
    check(_lib.load().prt_temporal_defaults(C.byref(tp)))
    for k, v in overrides.items():
        if k not in dict(tp._fields_):
            raise TypeError(f"prt_temporal_params has no field {k!r}")
        setattr(tp, k, v)
    return tp


def denoise_variance_defaults(**overrides):
    """prt_denoise_variance_params at the library's defaults (prt_denoise_variance_defaults); keyword overrides set
    single fields (iterations, normal_power, sigma_color, sigma_depth, sigma_albedo, color_decay, variance_floor)."""
    dp = _lib.DenoiseVarianceParams()
    check(_lib.load().prt_denoise_variance_defaults(C.byref(dp)))
    for k, v in overrides.items():
        if k not in dict(dp._fields_):
            raise TypeError(f"prt_denoise_variance_params has no field {k!r}")
        setattr(dp, k, v)
    return dp


def _camera_desc(cam):
    """A Camera or a _lib.CameraDesc -> a copy of the prt_camera struct (the caller may go on moving its camera)."""
    cd = _lib.CameraDesc()
    C.memmove(C.byref(cd), C.byref(cam.desc if hasattr(cam, "desc") else cam), C.sizeof(cd))
    return cd


def instance_motion(transforms, prev_transforms):
    """prt_instance_motion: the [count, 12] float32 motion matrices prev * inverse(cur) of two sets of row-major 4x4
    instance transforms (anything that reshapes to [count, 16]); host only, no context."""
    cur, prev = _f32(transforms).reshape(-1, 16), _f32(prev_transforms).reshape(-1, 16)
    if cur.shape != prev.shape:
        raise ValueError("instance_motion: the two sets of transforms differ in count")
    out = np.zeros((len(cur), 12), F32)
    check(_lib.load().prt_instance_motion(cur.ctypes.data, prev.ctypes.data, len(cur), out.ctypes.data))
    return out


PANINI_REPROJECT = "temporal reprojection is defined for the plane projection only (isPostProcessed is set)"


class Scene:
    """Scene (Core/Scene.h): models, BLAS instances (gameobject -> modelIndex + transform), lights, sky."""

    def __init__(self):
        self.models = []          # scenes.Mesh (Model fat-triangle arrays)
        self.textures = []        # (h, w) uint32 0x00RRGGBB
        self.blases = []          # (modelIndex, 4x4 row-major transform)
        self.pointLights = [LightTransform(np.zeros(3, F32), np.zeros(3, F32)) for _ in range(4)]
        self.directionalLights = []
        self.spotlights = []
        self.sky = None           # (h, w, 3) float32
        self.materials = None     # per-blas material kind (_lib.MAT_*), None = all textured (Scene.cpp:193-205)
        self.areaLights = []      # at most one dict(corner, edge_u, edge_v, radiance, two_sided) (AreaLight.h)
        self.skins = {}           # model index -> scenes.Skin (set_skin)
        self.poses = {}           # model index -> [joints, 12] float32, the last skin_model (None: the bind pose)

    @classmethod
    def from_data(cls, sd):
        s = cls()
        s.models = list(sd.meshes)
        s.textures = list(sd.textures)
        s.blases = [(m, np.asarray(T, F32)) for m, T in sd.instances]
        lt = sd.lights
        s.pointLights = [LightTransform(_f32(lt.point_pos[i]), _f32(lt.point_col[i])) for i in range(4)]
        s.directionalLights = [LightTransform(_f32(lt.dir_pos), _f32(lt.dir_col))]
        s.spotlights = [LightTransform(_f32(lt.spot_pos), _f32(lt.spot_col), _f32(lt.spot_rot))]
        s.sky = sd.sky
        s.materials = list(sd.materials) if sd.materials is not None else None
        s.areaLights = [dict(sd.area_light)] if sd.area_light is not None else []
        return s

    @property
    def tri_count(self):
        return sum(self.models[m].tri_count for m, _ in self.blases)

    def update_model(self, index, mesh):
        """Model `index` takes `mesh` (a scenes.Mesh of the same topology); hand it to a context with
        Context.update_mesh(index, mesh), or use Renderer.UpdateModel, which does both."""
        old = self.models[index]
        if mesh.tri_count != old.tri_count or np.asarray(mesh.vertices).size != np.asarray(old.vertices).size:
            raise ValueError("update_model: the triangle and vertex counts must stay (set_scene for a new topology)")
        self.models[index] = mesh
        self.poses.pop(index, None)

    def set_skin(self, index, skin):
        """Model `index` is skinned from now on (`skin`: a scenes.Skin of the model's vertex count; None removes it).
        Context.set_scene binds every skin; hand a later one to a context with Context.set_mesh_skin(index, skin), or
        use Renderer.SetSkin, which does both."""
        self.poses.pop(index, None)
        if skin is None:
            self.skins.pop(index, None)
            return
        if np.asarray(skin.positions).size != np.asarray(self.models[index].vertices).size:
            raise ValueError("set_skin: the skin's vertex count differs from the model's")
        self.skins[index] = skin

    def skin_model(self, index, matrices):
        """Model `index` takes the pose `matrices` ([joints, 12] or [joints, 3, 4] float32, row-major 3 x 4): the scene
        keeps it, so that a later Context.set_scene poses the model again; hand it to a context with
        Context.skin_mesh(index, matrices), or use Renderer.SkinModel, which does both.  models[index] keeps its bind
        pose arrays."""
        skin = self.skins.get(index)
        if skin is None:
            raise ValueError("skin_model: the model has no skin (set_skin)")
        M = _f32(matrices).reshape(-1, 12).copy()
        if len(M) != skin.joint_count:
            raise ValueError("skin_model: the matrix count differs from the skin's joint_count")
        self.poses[index] = M


class Context:
    """One prt_ctx on one HIP device (one process per GPU)."""

    def __init__(self, device: int = 0, group=None, tile: int = 32):
        """group: a list of device ordinals -> one context over several GPUs of this process
        (prt_create_group: pixel tiles rendered concurrently, gathered on the first device); a device may
        repeat, which runs several shards on one GPU."""
        L = _lib.load()
        n = C.c_int32(0)
        check(L.prt_device_count(C.byref(n)))
        if n.value <= 0:
            raise _lib.PrtError("no HIP device visible (the product path has no CPU fallback)")
        h = C.c_void_p()
        if group is None:
            check(L.prt_create(C.byref(_lib.DeviceDesc(device, 0)), C.byref(h)))
        else:
            devs = (_lib.DeviceDesc * len(group))(*[_lib.DeviceDesc(int(d), 0) for d in group])
            check(L.prt_create_group(devs, len(group), tile, C.byref(h)))
            device = int(group[0])
        self.L = L
        self.h = h
        self.device = device

    # -- multi-GPU inside the boundary (include/prt.h, prt_shard_*)
    @staticmethod
    def shard_unique_id() -> bytes:
        """A fresh RCCL id (rank 0 makes it, the caller carries the bytes to the other ranks)."""
        buf = (C.c_uint8 * _lib.SHARD_ID_BYTES)()
        check(_lib.load().prt_shard_unique_id(buf))
        return bytes(buf)

    def shard_rccl(self, uid: bytes, rank: int, world: int, tile: int = 32):
        """Join the RCCL communicator of `uid` as `rank` of `world`: prt_render then renders this rank's
        pixel tiles and gathers the frame on rank 0 (one ncclGather per frame, on the context stream)."""
        if len(uid) != _lib.SHARD_ID_BYTES:
            raise ValueError("RCCL id must be %d bytes" % _lib.SHARD_ID_BYTES)
        buf = (C.c_uint8 * _lib.SHARD_ID_BYTES).from_buffer_copy(uid)
        check(self.L.prt_shard_init_rccl(self.h, buf, rank, world, tile))

    def shard_info(self):
        si = _lib.ShardInfo()
        check(self.L.prt_get_shard_info(self.h, C.byref(si)))
        return si

    def close(self):
        if self.h:
            self.L.prt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- scene upload
    def set_scene(self, scene: Scene):
        L = self.L
        keep = []
        texs = (_lib.Texture * max(1, len(scene.textures)))()
        for i, t in enumerate(scene.textures):
            t = np.ascontiguousarray(t, np.uint32)
            keep.append(t)
            texs[i] = _lib.Texture(t.shape[1], t.shape[0], t.ctypes.data)
        check(L.prt_set_textures(self.h, texs, len(scene.textures)))
        ms = (_lib.Mesh * len(scene.models))()
        for i, m in enumerate(scene.models):
            arrs = [_f32(m.triangles), _f32(m.fixed_normals), _f32(m.fixed_uvs),
                    np.ascontiguousarray(m.indices, np.int32), _f32(m.vertices), _f32(m.face_normals)]
            keep.extend(arrs)
            ms[i] = _lib.Mesh(m.tri_count, m.vertices.size // 3, *[a.ctypes.data for a in arrs], m.albedo, m.normal,
                              m.metalness, m.emission)
        check(L.prt_set_meshes(self.h, ms, len(scene.models)))
        for i, skin in getattr(scene, "skins", {}).items():  # (prt_set_meshes discarded the bindings)
            self.set_mesh_skin(i, skin)
            pose = getattr(scene, "poses", {}).get(i)
            if pose is not None:
                self.skin_mesh(i, pose)
        xf = _f32(np.stack([T for _, T in scene.blases]).reshape(-1))
        mi = np.ascontiguousarray([m for m, _ in scene.blases], np.uint32)
        check(L.prt_set_instances(self.h, xf.ctypes.data, mi.ctypes.data, len(scene.blases)))
        self._ninst = len(scene.blases)
        self.set_materials(scene.materials)
        self.set_area_light(scene.areaLights[0] if scene.areaLights else None)
        lt = _lib.Lights()
        for i in range(4):
            lt.point_pos[i][:] = [float(v) for v in scene.pointLights[i].position]
            lt.point_color[i][:] = [float(v) for v in scene.pointLights[i].color]
        d, s = scene.directionalLights[0], scene.spotlights[0]
        lt.dir_pos[:] = [float(v) for v in d.position]
        lt.dir_color[:] = [float(v) for v in d.color]
        lt.spot_pos[:] = [float(v) for v in s.position]
        lt.spot_color[:] = [float(v) for v in s.color]
        lt.spot_rot[:] = [float(v) for v in s.rotation]
        check(L.prt_set_lights(self.h, C.byref(lt)))
        if scene.sky is not None:
            sky = _f32(scene.sky)
            check(L.prt_set_sky(self.h, sky.ctypes.data, sky.shape[1], sky.shape[0]))
        else:
            check(L.prt_set_sky(self.h, None, 0, 0))

    def set_lights(self, lt):
        """The point, directional and spot lights alone (prt_set_lights) from a scenes.Lights; set_scene sets them
        with the rest of the scene."""
        l = _lib.Lights()
        for i in range(4):
            l.point_pos[i][:] = [float(v) for v in lt.point_pos[i]]
            l.point_color[i][:] = [float(v) for v in lt.point_col[i]]
        l.dir_pos[:] = [float(v) for v in lt.dir_pos]
        l.dir_color[:] = [float(v) for v in lt.dir_col]
        l.spot_pos[:] = [float(v) for v in lt.spot_pos]
        l.spot_color[:] = [float(v) for v in lt.spot_col]
        l.spot_rot[:] = [float(v) for v in lt.spot_rot]
        check(self.L.prt_set_lights(self.h, C.byref(l)))

    def set_instances(self, blases):
        """Per-frame instance update (physics moved the game objects, Core/Renderer.cpp:33-41): the transforms
        go to the device and are refit there in stream order, so frames already queued keep the old ones."""
        xf = _f32(np.stack([T for _, T in blases]).reshape(-1))
        mi = np.ascontiguousarray([m for m, _ in blases], np.uint32)
        check(self.L.prt_set_instances(self.h, xf.ctypes.data, mi.ctypes.data, len(blases)))
        self._ninst = len(blases)

    def update_instances(self, transforms, device=False):
        """prt_update_instances: the instances of the last set_instances / set_scene take new transforms; mesh indices
        and material kinds stay, and the instance BVH is refitted on the device (no host build, no wait for the GPU).
        `transforms`: a float32 array of shape (n, 4, 4) or (16 n,), row-major; with device=True a contiguous float32
        torch tensor of 16 n elements on this context's device, or a raw device pointer as (pointer, n), read by one
        kernel in the context stream's order.  Device transforms stay on the device: until the next set_instances or
        host update the context holds no host copy of them.  tlas_cost() tells when set_instances (a fresh SAH tree)
        is worth its build."""
        if device:
            if hasattr(transforms, "data_ptr"):
                if not transforms.is_cuda or not transforms.is_contiguous() or str(transforms.dtype) != "torch.float32" \
                        or transforms.numel() % 16:
                    raise ValueError("update_instances: transforms must be a contiguous torch.float32 tensor of 16 per "
                                     "instance on the device")
                ptr, n = transforms.data_ptr(), transforms.numel() // 16
            else:
                ptr, n = transforms
            check(self.L.prt_update_instances(self.h, int(ptr), int(n), _lib.IN_DEVICE))
            return
        xf = _f32(transforms).reshape(-1)
        if xf.size % 16:
            raise ValueError("update_instances: 16 floats per instance")
        check(self.L.prt_update_instances(self.h, xf.ctypes.data, xf.size // 16, 0))

    def rebuild_instances(self, transforms=None, builder=_lib.BUILDER_GPU_PLOC, device=False):
        """prt_rebuild_instances: update_instances with a fresh device build of the instance BVH in place of the refit
        (builder: _lib.BUILDER_GPU_LBVH or BUILDER_GPU_PLOC).  `transforms` as update_instances takes them -- a float32
        array, or a torch tensor on this context's device (taken as device memory, with or without device=True), or
        (pointer, n) with device=True; None: the instances stay where they are and only the tree is rebuilt, from the
        transforms the context holds (on the device, after a device update).  Blocks until the builder is through."""
        if transforms is None:
            check(self.L.prt_rebuild_instances(self.h, None, getattr(self, "_ninst", 0), 0, int(builder)))
            return
        if device or hasattr(transforms, "data_ptr"):
            if hasattr(transforms, "data_ptr"):
                if not transforms.is_cuda or not transforms.is_contiguous() or str(transforms.dtype) != "torch.float32" \
                        or transforms.numel() % 16:
                    raise ValueError("rebuild_instances: transforms must be a contiguous torch.float32 tensor of 16 per "
                                     "instance on the device")
                ptr, n = transforms.data_ptr(), transforms.numel() // 16
            else:
                ptr, n = transforms
            check(self.L.prt_rebuild_instances(self.h, int(ptr), int(n), _lib.IN_DEVICE, int(builder)))
            return
        xf = _f32(transforms).reshape(-1)
        if xf.size % 16:
            raise ValueError("rebuild_instances: 16 floats per instance")
        check(self.L.prt_rebuild_instances(self.h, xf.ctypes.data, xf.size // 16, 0, int(builder)))

    def tlas_cost(self):
        """prt_tlas_cost: the SAH cost of the instance BVH as it stands on the device (prt_blas_cost's measure, a leaf
        slot counting one instance; 0.0 on the linear list).  It grows as update_instances carries the instances away
        from where the tree was built and falls back after set_instances."""
        v = C.c_double()
        check(self.L.prt_tlas_cost(self.h, C.byref(v)))
        return v.value

    def read_tlas(self):
        """prt_read_tlas: the instance BVH's Node8 records as a uint8 array [nodes, 80] and its instance-slot table as a
        uint32 array [nodes, 8] (0xFFFFFFFF where a slot is no leaf slot); both empty on the linear list.  Introspection
        for tests and tools; waits for the context stream."""
        nb, sb = C.c_uint64(), C.c_uint64()
        check(self.L.prt_read_tlas(self.h, None, 0, None, 0, C.byref(nb), C.byref(sb)))
        nodes, slots = np.zeros(nb.value, np.uint8), np.zeros(sb.value // 4, np.uint32)
        if nb.value:
            check(self.L.prt_read_tlas(self.h, nodes.ctypes.data, nb.value, slots.ctypes.data, sb.value, None, None))
        return nodes.reshape(-1, 80), slots.reshape(-1, 8)

    def update_mesh(self, index, mesh, device=False):
        """prt_update_mesh: mesh `index` of the last set_scene takes `mesh`'s arrays and its BLAS is refitted in place
        (same triangle and vertex counts, same texture ids; the tree keeps its topology).  `mesh` is a scenes.Mesh of
        host arrays, or with device=True anything with the same six attributes holding torch tensors on this
        context's device (float32, indices int32, contiguous) or raw device pointers (ints; then tri_count and
        vertex_count attributes are required): the arrays are read in the context stream's order, the call waits for
        28 bytes, and an index out of range raises (the mesh is then traversable but unspecified until the next
        update)."""
        m, keep = self._mesh_arg(mesh, device, "update_mesh")
        check(self.L.prt_update_mesh(self.h, int(index), C.byref(m), _lib.IN_DEVICE if device else 0))
        del keep

    @staticmethod
    def _mesh_arg(mesh, device, who):
        """The prt_mesh of update_mesh / rebuild_mesh and the arrays it points into (kept alive by the caller)."""
        names = ("triangles", "fixed_normals", "fixed_uvs", "indices", "vertices", "face_normals")
        arrs = [getattr(mesh, n) for n in names]
        if not device:
            arrs = [np.ascontiguousarray(a, np.int32 if n == "indices" else np.float32) for n, a in zip(names, arrs)]
            ptrs = [a.ctypes.data for a in arrs]
            tri_count, verts = arrs[3].size // 3, arrs[4].size // 3
        else:
            ptrs = []
            for n, a in zip(names, arrs):
                if hasattr(a, "data_ptr"):
                    want = "torch.int32" if n == "indices" else "torch.float32"
                    if not a.is_cuda or not a.is_contiguous() or str(a.dtype) != want:
                        raise ValueError(f"{who}: {n} must be a contiguous {want} tensor on the device")
                    ptrs.append(a.data_ptr())
                else:
                    ptrs.append(int(a))
            tri_count = getattr(mesh, "tri_count", None)
            verts = getattr(mesh, "vertex_count", None)
            if tri_count is None:
                tri_count = arrs[3].numel() // 3
            if verts is None:
                verts = arrs[4].numel() // 3
        return _lib.Mesh(int(tri_count), int(verts), *ptrs, mesh.albedo, mesh.normal, mesh.metalness, mesh.emission), arrs

    def rebuild_mesh(self, index, mesh=None, device=False, builder=_lib.BUILDER_GPU_PLOC):
        """prt_rebuild_mesh: update_mesh with a fresh device build (builder: _lib.BUILDER_GPU_LBVH or BUILDER_GPU_PLOC)
        in place of the refit.  `mesh` and `device` are update_mesh's; mesh=None rebuilds over the fat triangles the
        mesh's skin binding holds from its last skin_mesh.  Blocks while the builder synchronises; a tree that outgrows
        the mesh's node region drains the context once.  Decide when from blas_cost()."""
        if mesh is None:
            check(self.L.prt_rebuild_mesh(self.h, int(index), None, 0, int(builder)))
            return
        m, keep = self._mesh_arg(mesh, device, "rebuild_mesh")
        check(self.L.prt_rebuild_mesh(self.h, int(index), C.byref(m), _lib.IN_DEVICE if device else 0, int(builder)))
        del keep

    def blas_cost(self, index):
        """prt_blas_cost: the SAH cost of mesh `index`'s BLAS as it stands on the device (a float; the same tree gives
        the same bits).  It grows as update_mesh / skin_mesh carry the mesh away from the pose its tree was built for
        and falls back after rebuild_mesh."""
        v = C.c_double()
        check(self.L.prt_blas_cost(self.h, int(index), C.byref(v)))
        return v.value

    def set_mesh_skin(self, index, skin):
        """prt_set_mesh_skin: binds `skin` (a scenes.Skin; None removes the binding) to mesh `index` of the last
        set_scene.  Checked on the host against the mesh (counts, every index, every joint); waits for the context
        stream and may allocate."""
        if skin is None:
            check(self.L.prt_set_mesh_skin(self.h, int(index), None))
            return
        P, N = _f32(skin.positions).reshape(-1), _f32(skin.normals).reshape(-1)
        idx = np.ascontiguousarray(skin.indices, np.int32).reshape(-1)
        J = np.ascontiguousarray(skin.joints, np.uint16).reshape(-1)
        Wt = _f32(skin.weights).reshape(-1)
        V = P.size // 3
        if N.size != P.size or J.size != 4 * V or Wt.size != 4 * V:
            raise ValueError("set_mesh_skin: positions, normals, joints and weights differ in vertex count")
        s = _lib.Skin(V, idx.size // 3, int(skin.joint_count), P.ctypes.data, N.ctypes.data, idx.ctypes.data,
                      J.ctypes.data, Wt.ctypes.data)
        check(self.L.prt_set_mesh_skin(self.h, int(index), C.byref(s)))

    def skin_mesh(self, index, matrices, device=False):
        """prt_skin_mesh: mesh `index` (bound by set_mesh_skin) is skinned with `matrices` and its BLAS refitted in
        place, on the device.  `matrices`: [joints, 12] (or [joints, 3, 4]) float32 row-major 3 x 4, a host array; with
        device=True a contiguous float32 torch tensor on this context's device, read in the context stream's order.
        The call waits for the mesh's new root box."""
        if device:
            if not hasattr(matrices, "data_ptr") or not matrices.is_cuda or not matrices.is_contiguous() or \
                    str(matrices.dtype) != "torch.float32" or matrices.numel() % 12:
                raise ValueError("skin_mesh: matrices must be a contiguous torch.float32 tensor of 12 per joint on the device")
            check(self.L.prt_skin_mesh(self.h, int(index), matrices.data_ptr(), matrices.numel() // 12, _lib.IN_DEVICE))
            return
        M = _f32(matrices).reshape(-1)
        if M.size % 12:
            raise ValueError("skin_mesh: 12 floats per joint")
        check(self.L.prt_skin_mesh(self.h, int(index), M.ctypes.data, M.size // 12, 0))

    def snapshot_mesh(self, index):
        """prt_snapshot_mesh: mesh `index`'s present corner positions become its previous positions, which
        render_aov_deform() measures against (a device copy on the context stream; a mesh's first snapshot allocates,
        later ones neither allocate nor wait)."""
        check(self.L.prt_snapshot_mesh(self.h, int(index)))

    def read_blas(self, index):
        """prt_read_blas: mesh `index`'s Node8 records as a uint8 array [nodes, 80], child_base / tri_base relative to
        the mesh (introspection for tests and tools; waits for the context stream)."""
        n = C.c_uint64()
        check(self.L.prt_read_blas(self.h, int(index), None, 0, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        check(self.L.prt_read_blas(self.h, int(index), buf.ctypes.data, n.value, None))
        return buf.reshape(-1, 80)

    def read_blas_tris(self, index):
        """prt_read_blas_tris: mesh `index`'s TriMT leaf records as a uint8 array [records, 48] in leaf order, prim
        mesh-local (one record per reference: more than the triangle count only under BUILDER_HOST_SBVH)."""
        n = C.c_uint64()
        check(self.L.prt_read_blas_tris(self.h, int(index), None, 0, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        check(self.L.prt_read_blas_tris(self.h, int(index), buf.ctypes.data, n.value, None))
        return buf.reshape(-1, 48)

    def set_materials(self, kinds=None):
        """Per-instance material kinds (_lib.MAT_TEXTURED / MAT_DIELECTRIC / MAT_MIRROR), None = all textured."""
        if kinds is None:
            check(self.L.prt_set_instance_materials(self.h, None, 0))
            return
        k = np.ascontiguousarray(kinds, np.int32)
        check(self.L.prt_set_instance_materials(self.h, k.ctypes.data, len(k)))

    def set_area_light(self, al=None):
        """One area light (dict: corner, edge_u, edge_v, radiance, two_sided) or None."""
        if al is None:
            check(self.L.prt_set_area_lights(self.h, None, 0))
            return
        a = _lib.AreaLight()
        a.corner[:] = [float(v) for v in al["corner"]]
        a.edge_u[:] = [float(v) for v in al["edge_u"]]
        a.edge_v[:] = [float(v) for v in al["edge_v"]]
        a.radiance[:] = [float(v) for v in al["radiance"]]
        a.two_sided = 1 if al.get("two_sided", False) else 0
        check(self.L.prt_set_area_lights(self.h, C.byref(a), 1))

    def set_camera(self, cam: Camera):
        check(self.L.prt_set_camera(self.h, C.byref(cam.desc)))

    def set_postfx(self, pf=None):
        """Post-processing on (a prt_postfx, see postfx_preset) or off (None)."""
        if pf is None:
            pf = _lib.PostFx()
        check(self.L.prt_set_postfx(self.h, C.byref(pf)))

    def set_bvh_builder(self, builder):
        """BLAS builder for the next set_scene: _lib.BUILDER_HOST_SAH (default), _lib.BUILDER_GPU_LBVH,
        _lib.BUILDER_HOST_SBVH (spatial splits) or _lib.BUILDER_GPU_PLOC."""
        check(self.L.prt_set_bvh_builder(self.h, builder))

    def scene_info(self):
        si = _lib.SceneInfo()
        check(self.L.prt_get_scene_info(self.h, C.byref(si)))
        return si

    # -- rendering
    def render(self, width, height, spp, bounces, flags=_lib.FLAGS_DEFAULT, mode=0, frame_index=0, seed=0,
               avg=None, rgb8=None, device_out=False, stats=True):
        p = _lib.RenderParams(width, height, spp, bounces, flags, mode, frame_index, seed)
        st = _lib.Stats() if stats else None
        if not device_out:
            if avg is None:
                avg = np.zeros((height * width, 4), F32)
            if rgb8 is None:
                rgb8 = np.zeros(height * width, np.uint32)
            pa, pr = avg.ctypes.data, rgb8.ctypes.data
        else:
            pa, pr = avg, rgb8  # raw device pointers (ints) or None
        check(self.L.prt_render(self.h, C.byref(p), pa, pr, _lib.OUT_DEVICE if device_out else 0,
                                C.byref(st) if st is not None else None))
        return avg, rgb8, _checked(st)

    def reset_accumulation(self, full=True):
        check(self.L.prt_reset_accumulation(self.h, 1 if full else 0))

    def ray_totals(self, reset=False):
        """(segments, shadow_rays) of every render since creation or the last reset, counted on the device
        (prt_ray_totals): a frame loop can count rays without stats=True, which waits for each frame."""
        seg, sh = C.c_uint64(), C.c_uint64()
        check(self.L.prt_ray_totals(self.h, C.byref(seg), C.byref(sh), 1 if reset else 0))
        return int(seg.value), int(sh.value)

    def primary_rays(self, reset=False):
        """(traced, reused): path-1 primary rays the calls so far traced for reuse (one per pixel of the call's
        tile map, once per camera / tile map / scene / instance state and wavefront state) and those whose hit was
        taken from the kept records instead (prt_primary_rays).  Host counters, no wait; both stay 0 where the
        reuse does not apply (extensions, debug render modes, PRT_PRIMARY_REUSE=0)."""
        tr, re_ = C.c_uint64(), C.c_uint64()
        check(self.L.prt_primary_rays(self.h, C.byref(tr), C.byref(re_), 1 if reset else 0))
        return int(tr.value), int(re_.value)

    def shadow_reuse(self, reset=False):
        """Shadow rays of path-1 primary hits that the calls so far answered from the kept light visibility instead
        of tracing them (prt_shadow_reuse).  Counted on the device: waits for the queued frames, like ray_totals.
        0 where primary-hit reuse does not apply, with PRT_SHADOW_REUSE=0, and in the first two calls of a view (the
        first traces the primary hits, the second learns)."""
        n = C.c_uint64()
        check(self.L.prt_shadow_reuse(self.h, C.byref(n), 1 if reset else 0))
        return int(n.value)

    def surface_reuse(self, reset=False):
        """Work items (pixels x reference frames) whose path-1 primary hit the calls so far shaded from the kept
        surface values -- normal, material, hit point, or a miss's sky radiance -- instead of gathering them again
        (prt_surface_reuse).  A host counter, no wait.  0 outside the plain pipeline, with PRT_SURFACE_REUSE=0,
        PRT_SHADOW_REUSE=0 or PRT_PRIMARY_REUSE=0, and in the first two calls of a view (the first traces the primary
        hits, the second fills the record)."""
        n = C.c_uint64()
        check(self.L.prt_surface_reuse(self.h, C.byref(n), 1 if reset else 0))
        return int(n.value)

    def shadow_dead(self, reset=False):
        """Shadow rays the calls so far counted instead of tracing because their contribution is exactly zero: the
        light behind the shading normal, the hit outside the spot's cone, a black light, PRT_FLAG_LIGHTED off
        (prt_shadow_dead).  Counted on the device: waits for the queued frames, like ray_totals.  0 in the debug
        render modes and with PRT_DEAD_SHADOW=0; an area light's own ray is never counted; rays under the light-visibility record count in
        shadow_reuse() instead."""
        n = C.c_uint64()
        check(self.L.prt_shadow_dead(self.h, C.byref(n), 1 if reset else 0))
        return int(n.value)

    def save_accumulation(self) -> bytes:
        """The accumulation state (accumulator, samplesPerPixel, distances) as an opaque blob
        (prt_save_accumulation); b"" before the first render."""
        n = C.c_uint64()
        check(self.L.prt_accumulation_bytes(self.h, C.byref(n)))
        if n.value == 0:
            return b""
        buf = (C.c_uint8 * n.value)()
        check(self.L.prt_save_accumulation(self.h, buf, n.value))
        return bytes(buf)

    def load_accumulation(self, blob: bytes):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        check(self.L.prt_load_accumulation(self.h, buf, len(blob)))

    def trace_primary(self, width, height):
        hits = np.zeros(width * height, dtype=[("t", F32), ("u", F32), ("v", F32), ("prim", np.uint32),
                                               ("inst", np.uint32)])
        st = _lib.Stats()
        check(self.L.prt_trace_primary(self.h, width, height, hits.ctypes.data, 0, C.byref(st)))
        return hits, _checked(st)

    # -- first-hit feature buffers and the denoiser they guide (include/prt.h prt_render_aov / prt_denoise)
    def render_aov(self, width, height, flags=_lib.FLAG_NORMALMAP, device_out=False, albedo=None, normal_depth=None,
                   timed=False):
        """(albedo[n,4], normal_depth[n,4]) of the first hit at pixel centres: base colour (w = 1; miss 0) and the
        shading normal as Trace uses it with the hit distance in w (miss 0,0,0,1e30).  The accumulation and the ray
        totals stay as they are.  device_out: albedo / normal_depth are raw device pointers (either may be None)."""
        _, _, (albedo, normal_depth), of = _images(width * height, device_out, timed,
                                                   outs=((albedo, 4, F32), (normal_depth, 4, F32)))
        check(self.L.prt_render_aov(self.h, width, height, flags, _ptr(albedo), _ptr(normal_depth), of))
        return albedo, normal_depth

    def denoise(self, color, albedo, normal_depth, width, height, params=None, device_out=False, out=None, rgb8=None,
                timed=False):
        """Edge-avoiding a-trous filter of `color` (float4 per pixel, render()'s avg) guided by render_aov()'s
        buffers; returns (out[n,4], rgb8[n]).  device_out: every image is a raw device pointer, out / rgb8 are
        where the results go (either may be None; out may be the same pointer as color) and no host wait happens."""
        dp = params if params is not None else denoise_defaults()
        ins, _, (out, rgb8), of = _images(width * height, device_out, timed, (color, albedo, normal_depth),
                                          outs=((out, 4, F32), (rgb8, 1, np.uint32)))
        check(self.L.prt_denoise(self.h, C.byref(dp), width, height, *map(_ptr, ins + [out, rgb8]), of))
        return out, rgb8

    def denoise_timings(self):
        """Device ms of the last timed=True calls: [AOV pass, denoiser prep, filter iteration 0, 1, ...]."""
        ms = (C.c_float * _lib.DENOISE_TIMINGS)()
        check(self.L.prt_denoise_timings(self.h, ms, _lib.DENOISE_TIMINGS))
        return [float(v) for v in ms]

    # -- temporal reprojection of the frame history (include/prt.h prt_reproject)
    def reproject(self, color, normal_depth, camera, history=None, history_normal_depth=None, prev_camera=None, *,
                  width, height, params=None, device_out=False, out=None, rgb8=None):
        """`color` (render()'s avg of this frame) blended into the previous output `history` (rgb, w = history
        length) reprojected from `prev_camera`'s view onto `camera`'s, guided by both views' render_aov()
        normal_depth; returns (out[n,4], rgb8[n]), out's w the new history length.  history, history_normal_depth and
        prev_camera are all None (a history starts) or all given.  Cameras: Camera or _lib.CameraDesc.  device_out:
        every image is a raw device pointer, out / rgb8 are where the results go (either may be None; out may be
        color, not a history buffer) and no host wait happens.  Plane projection only (no post-processing)."""
        rp = params if params is not None else reproject_defaults()
        cam = _camera_desc(camera)
        prev = C.byref(_camera_desc(prev_camera)) if prev_camera is not None else None
        (c, g, h, hg), _, (out, rgb8), of = _images(
            width * height, device_out, False, (color, normal_depth, history, history_normal_depth),
            outs=((out, 4, F32), (rgb8, 1, np.uint32)))
        check(self.L.prt_reproject(self.h, C.byref(rp), width, height, C.byref(cam),
                                   *map(_ptr, (c, g, prev, h, hg, out, rgb8)), of))
        return out, rgb8

    # -- moving instances in the reprojection (include/prt.h prt_render_aov_ids / prt_reproject_motion)
    def render_aov_ids(self, width, height, flags=_lib.FLAG_NORMALMAP, device_out=False, albedo=None,
                       normal_depth=None, instance=None, timed=False):
        """render_aov() with the first hit's instance index per pixel (uint32, a miss 0xFFFFFFFF) from the same
        primary-hit pass: (albedo[n,4], normal_depth[n,4], instance[n]).  device_out: the three are raw device
        pointers (any may be None)."""
        _, _, outs, of = _images(width * height, device_out, timed,
                                 outs=((albedo, 4, F32), (normal_depth, 4, F32), (instance, 1, np.uint32)))
        check(self.L.prt_render_aov_ids(self.h, width, height, flags, *map(_ptr, outs), of))
        return tuple(outs)

    def reproject_motion(self, color, normal_depth, instance, camera, history=None, history_normal_depth=None,
                         prev_camera=None, history_instance=None, motion=None, *, width, height, params=None,
                         device_out=False, out=None, rgb8=None):
        """reproject() that follows moving instances: `instance` / `history_instance` are both views'
        render_aov_ids() ids and `motion` the [count, 12] matrices of instance_motion() (always a host array).
        history, history_normal_depth, prev_camera and motion are all None (a history starts) or all given;
        history_instance is optional (None: taps are not compared by instance).  Returns (out[n,4], rgb8[n])."""
        rp = params if params is not None else reproject_defaults()
        cam = _camera_desc(camera)
        prev = C.byref(_camera_desc(prev_camera)) if prev_camera is not None else None
        mo = _f32(motion).reshape(-1, 12) if motion is not None else None
        (c, g, h, hg), (i, hi), (out, rgb8), of = _images(
            width * height, device_out, False, (color, normal_depth, history, history_normal_depth),
            (instance, history_instance), ((out, 4, F32), (rgb8, 1, np.uint32)))
        check(self.L.prt_reproject_motion(
            self.h, C.byref(rp), width, height, C.byref(cam),
            *map(_ptr, (c, g, i, prev, h, hg, hi, mo, 0 if mo is None else len(mo), out, rgb8)), of))
        return out, rgb8

    # -- luminance moments and the variance-guided filter (include/prt.h prt_reproject_moments / prt_denoise_variance)
    def reproject_moments(self, color, normal_depth, instance, camera, history=None, history_normal_depth=None,
                          prev_camera=None, history_instance=None, motion=None, history_moments=None, *, width,
                          height, params=None, device_out=False, out=None, moments=None, rgb8=None):
        """reproject_motion() that carries the luminance moments with the history: `history_moments` is the previous
        call's moments output and belongs to the all-or-nothing history group; `instance` is always required; `out`
        must not be `color`.  Returns (out[n,4], moments[n,4], rgb8[n]); moments is (m1, m2, variance, 0)."""
        tp = params if params is not None else temporal_defaults()
        cam = _camera_desc(camera)
        prev = C.byref(_camera_desc(prev_camera)) if prev_camera is not None else None
        mo = _f32(motion).reshape(-1, 12) if motion is not None else None
        (c, g, h, hg, hm), (i, hi), (out, moments, rgb8), of = _images(
            width * height, device_out, False, (color, normal_depth, history, history_normal_depth, history_moments),
            (instance, history_instance), ((out, 4, F32), (moments, 4, F32), (rgb8, 1, np.uint32)))
        check(self.L.prt_reproject_moments(
            self.h, C.byref(tp), width, height, C.byref(cam),
            *map(_ptr, (c, g, i, prev, h, hg, hi, mo, 0 if mo is None else len(mo), hm, out, moments, rgb8)), of))
        return out, moments, rgb8

    def denoise_variance(self, color, moments, albedo, normal_depth, width, height, params=None, device_out=False,
                         out=None, variance=None, rgb8=None, timed=False, want_variance=True):
        """denoise() whose colour weight is scaled by the variance in `moments` (reproject_moments()' output); returns
        (out[n,4], variance[n] or None, rgb8[n]).  device_out: every image is a raw device pointer, out / variance /
        rgb8 are where the results go (out or rgb8 and variance may be None; out may be the same pointer as color)."""
        dp = params if params is not None else denoise_variance_defaults()
        ins, _, outs, of = _images(
            width * height, device_out, timed, (color, moments, albedo, normal_depth),
            outs=((out, 4, F32), (variance, 1 if want_variance else 0, F32), (rgb8, 1, np.uint32)))
        check(self.L.prt_denoise_variance(self.h, C.byref(dp), width, height, *map(_ptr, ins + outs), of))
        return tuple(outs)

    # -- deforming meshes in the reprojection (include/prt.h prt_render_aov_deform / prt_reproject_deform)
    def render_aov_deform(self, width, height, flags=_lib.FLAG_NORMALMAP, device_out=False, albedo=None,
                          normal_depth=None, instance=None, offset=None, timed=False):
        """render_aov_ids() with the first hit's object-space displacement to where its surface point was at the
        mesh's snapshot_mesh() (xyz, w = 1; a miss or a mesh without a snapshot: zeros), from the same primary-hit
        pass: (albedo[n,4], normal_depth[n,4], instance[n], offset[n,4]).  device_out: the four are raw device
        pointers (any may be None)."""
        _, _, outs, of = _images(width * height, device_out, timed,
                                 outs=((albedo, 4, F32), (normal_depth, 4, F32), (instance, 1, np.uint32),
                                       (offset, 4, F32)))
        check(self.L.prt_render_aov_deform(self.h, width, height, flags, *map(_ptr, outs), of))
        return tuple(outs)

    def reproject_deform(self, color, normal_depth, instance, camera, history=None, history_normal_depth=None,
                         prev_camera=None, history_instance=None, motion=None, history_moments=None, offset=None,
                         prev_transforms=None, *, width, height, params=None, device_out=False, out=None, moments=None,
                         rgb8=None):
        """reproject_moments() that follows deforming meshes: `offset` is this view's render_aov_deform() buffer and
        `prev_transforms` the previous frame's instance transforms ([count, 16], always a host array, what
        instance_motion() took); both None or both given, and given only with a history.  Returns (out[n,4],
        moments[n,4], rgb8[n])."""
        tp = params if params is not None else temporal_defaults()
        cam = _camera_desc(camera)
        prev = C.byref(_camera_desc(prev_camera)) if prev_camera is not None else None
        mo = _f32(motion).reshape(-1, 12) if motion is not None else None
        pxf = _f32(prev_transforms).reshape(-1, 16) if prev_transforms is not None else None
        if mo is not None and pxf is not None and len(pxf) != len(mo):
            raise ValueError("reproject_deform: motion and prev_transforms differ in count")
        (c, g, h, hg, hm, off), (i, hi), (out, moments, rgb8), of = _images(
            width * height, device_out, False,
            (color, normal_depth, history, history_normal_depth, history_moments, offset),
            (instance, history_instance), ((out, 4, F32), (moments, 4, F32), (rgb8, 1, np.uint32)))
        check(self.L.prt_reproject_deform(
            self.h, C.byref(tp), width, height, C.byref(cam),
            *map(_ptr, (c, g, i, prev, h, hg, hi, mo, 0 if mo is None else len(mo), hm, off, pxf, out, moments,
                        rgb8)), of))
        return out, moments, rgb8

    def intersect(self, O, D, tmax=None):
        O, D = _f32(O), _f32(D)
        n = O.shape[0]
        tm = _f32(tmax) if tmax is not None else None
        hits = np.zeros(n, dtype=[("t", F32), ("u", F32), ("v", F32), ("prim", np.uint32), ("inst", np.uint32)])
        check(self.L.prt_intersect(self.h, n, O.ctypes.data, D.ctypes.data,
                                   tm.ctypes.data if tm is not None else None, hits.ctypes.data))
        return hits

    def occluded(self, O, D, tmax):
        O, D, tm = _f32(O), _f32(D), _f32(tmax)
        occ = np.zeros(O.shape[0], np.int32)
        check(self.L.prt_occluded(self.h, O.shape[0], O.ctypes.data, D.ctypes.data, tm.ctypes.data, occ.ctypes.data))
        return occ

    # -- ray queries on caller arrays, in stream order (include/prt.h prt_query_rays / prt_query_surface)
    def _query_tensor(self, t, what, per, n=None):
        """A contiguous float32 CUDA tensor of `per` floats per ray on this context's device (as update_instances
        validates its transforms); returns its ray count."""
        if str(t.dtype) != "torch.float32" or not t.is_cuda \
                or not t.is_contiguous() or t.device.index != self.device or t.numel() % per \
                or (n is not None and t.numel() != per * n):
            raise ValueError(f"{what} must be a contiguous torch.float32 tensor of {per} per ray on cuda:{self.device}")
        return t.numel() // per

    def query_rays(self, origins, dirs, tmax=None, *, closest=True, any_hit=False):
        """prt_query_rays: n arbitrary rays on the persistent traversal kernels; returns (hits, occluded), None for
        the answer not asked for.  numpy arrays go through the host path and come back as numpy, complete on return
        (hits in intersect()'s dtype).  Contiguous float32 CUDA tensors on this context's device are read in place in
        the context stream's order, with no host wait: hits is an [n, 5] float32 tensor (t, u, v, then prim and inst,
        which hits[:, 3:].view(torch.int32) reads), occluded an int32 tensor.  tmax None: 1e30 for every ray.  A ray
        with a non-finite component, a zero direction or a tmax that is NaN or <= 0 is not traversed: a miss."""
        if not closest and not any_hit:
            raise ValueError("query_rays: closest or any_hit")
        if hasattr(origins, "data_ptr"):
            import torch
            n = self._query_tensor(origins, "query_rays: origins", 3)
            self._query_tensor(dirs, "query_rays: dirs", 3, n)
            if tmax is not None:
                self._query_tensor(tmax, "query_rays: tmax", 1, n)
            hits = torch.empty((n, 5), dtype=torch.float32, device=origins.device) if closest else None
            occ = torch.empty(n, dtype=torch.int32, device=origins.device) if any_hit else None
            if n:  # (an empty tensor has no address to hand over, and an empty batch enqueues nothing)
                check(self.L.prt_query_rays(self.h, n, origins.data_ptr(), dirs.data_ptr(),
                                            tmax.data_ptr() if tmax is not None else None,
                                            hits.data_ptr() if closest else None,
                                            occ.data_ptr() if any_hit else None, _lib.OUT_DEVICE))
            return hits, occ
        O, D = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = O.shape[0]
        if D.shape[0] != n:
            raise ValueError("query_rays: one direction per origin")
        tm = _f32(tmax).reshape(-1) if tmax is not None else None
        if tm is not None and tm.size != n:
            raise ValueError("query_rays: one tmax per ray")
        hits = np.zeros(n, dtype=[("t", F32), ("u", F32), ("v", F32), ("prim", np.uint32),
                                  ("inst", np.uint32)]) if closest else None
        occ = np.zeros(n, np.int32) if any_hit else None
        check(self.L.prt_query_rays(self.h, n, O.ctypes.data, D.ctypes.data, _ptr(tm), _ptr(hits), _ptr(occ), 0))
        return hits, occ

    def query_surface(self, hits, tmax=None, normalmap=True, *, albedo=True, normal_depth=True, geometry_normal=True,
                      material=True):
        """prt_query_surface: the shading inputs at query_rays' hit records, as a dict of the outputs asked for:
        albedo [n, 4] and normal_depth [n, 4] as render_aov defines them, geometry_normal [n, 4] (w = 1) and material
        [n, 8] (base rgb, metalness, emissive rgb, roughness); misses get zeros (normal_depth 0, 0, 0, 1e30).  Pass the
        tmax the query ran under: record i is a hit iff its t < tmax[i].  hits: intersect()'s numpy records (host
        path, numpy out) or query_rays' [n, 5] tensor (device path, tensors out, no host wait)."""
        want = [k for k, on in (("albedo", albedo), ("normal_depth", normal_depth),
                                ("geometry_normal", geometry_normal), ("material", material)) if on]
        width = {"albedo": 4, "normal_depth": 4, "geometry_normal": 4, "material": 8}
        fl = _lib.FLAG_NORMALMAP if normalmap else 0
        if hasattr(hits, "data_ptr"):
            import torch
            n = self._query_tensor(hits, "query_surface: hits", 5)
            if tmax is not None:
                self._query_tensor(tmax, "query_surface: tmax", 1, n)
            out = {k: torch.empty((n, width[k]), dtype=torch.float32, device=hits.device) for k in want}
            if n:
                ptrs = [out[k].data_ptr() if k in out else None for k in width]
                check(self.L.prt_query_surface(self.h, n, hits.data_ptr(), tmax.data_ptr() if tmax is not None else None,
                                               fl, *ptrs, _lib.OUT_DEVICE))
            return out
        rec = np.ascontiguousarray(hits)
        if rec.dtype.itemsize != 20:
            raise ValueError("query_surface: hits must be intersect()'s records (20 bytes each)")
        n = rec.shape[0]
        tm = _f32(tmax).reshape(-1) if tmax is not None else None
        if tm is not None and tm.size != n:
            raise ValueError("query_surface: one tmax per record")
        out = {k: np.zeros((n, width[k]), F32) for k in want}
        ptrs = [_ptr(out[k]) if k in out else None for k in width]
        check(self.L.prt_query_surface(self.h, n, rec.ctypes.data, _ptr(tm), fl, *ptrs, 0))
        return out

    def brdf_probe(self, op, records):
        """prt_brdf_probe: the device BRDF functions on n records (float32 [n, 24] in, [n, 8] out; include/prt.h)."""
        rec = np.ascontiguousarray(records, np.float32).reshape(-1, 24)
        out = np.zeros((rec.shape[0], 8), np.float32)
        check(self.L.prt_brdf_probe(self.h, int(op), rec.shape[0], rec.ctypes.data, out.ctypes.data))
        return out

    def tile_buffer_pixels(self, width, height, tile, world):
        n = C.c_int64(0)
        check(self.L.prt_tile_buffer_pixels(width, height, tile, world, C.byref(n)))
        return n.value

    def render_tiles(self, width, height, spp, bounces, tile, rank, world, tiles_dev_ptr, flags=_lib.FLAGS_DEFAULT,
                     mode=0, frame_index=0, seed=0, stats=False):
        p = _lib.RenderParams(width, height, spp, bounces, flags, mode, frame_index, seed)
        st = _lib.Stats() if stats else None
        check(self.L.prt_render_tiles(self.h, C.byref(p), tile, rank, world, tiles_dev_ptr,
                                      C.byref(st) if st is not None else None))
        return _checked(st)

    def untile(self, gathered_dev_ptr, width, height, tile, world, avg_dev_ptr, rgb8_dev_ptr):
        check(self.L.prt_untile(self.h, gathered_dev_ptr, width, height, tile, world, avg_dev_ptr, rgb8_dev_ptr))

    def set_stream(self, stream_ptr):
        check(self.L.prt_set_stream(self.h, stream_ptr))

    def set_frames_in_flight(self, n):
        """prt_set_frames_in_flight: with n = 2 a render with device outputs overlaps the previous one; its outputs
        are complete in the context stream's order once the next render is enqueued or finish() was called."""
        check(self.L.prt_set_frames_in_flight(self.h, int(n)))

    def finish(self):
        """prt_finish: the context stream waits for every frame in flight."""
        check(self.L.prt_finish(self.h))


def _checked(st):
    """Stats of a call whose context has dropped a traversal stack group (prt_stats.stack_overflows) raise:
    such a render may have lost hits, and the host sizes the stacks so that it cannot happen."""
    if st is not None and st.stack_overflows:
        raise _lib.PrtError(f"traversal stack overflow: {st.stack_overflows} node groups dropped")
    return st


class Renderer:
    """Renderer (Core/Renderer.h:12-112): public flags + Tick().  Tick() renders one reference frame
    (two camera paths per pixel with AA) and folds it into the progressive accumulator; screen holds
    the packed 0x00RRGGBB pixels, average the float average (Core/Renderer.cpp:22-148)."""

    RENDER_STATES = dict(BRDF=0, BASECOLOR=1, GEOMETRYNORMAL=2, SHADINGNORMAL=3, METAL=4, ROUGHNESS=5, EMMISIVE=6)

    def __init__(self, scene: Scene, camera: Camera, width: int, height: int, device: int = 0):
        self.accumulates = True
        self.bounces = 2
        self.renderingMode = 0
        self.LIGHTED = self.GAMMACORRECTED = self.NORMALMAPPED = self.SKYBOX = self.AA = self.isStochastic = True
        self.isPostProcessed = False
        self.width, self.height = width, height
        self.scene, self.camera = scene, camera
        self.ctx = Context(device)
        self.frame = 0
        self.seed = 0
        self.screen = np.zeros(width * height, np.uint32)
        self.average = np.zeros((width * height, 4), F32)
        self.last_stats = None
        # TickTemporal's history: (width, height, out, normal_depth, camera[, ids, transforms[, moments]])
        self._temporal = None
        self._tracked = []  # TrackModel: the models whose snapshot TickTemporalVariance(deform=True) renews
        self.Init()

    def Init(self):
        self.ctx.set_scene(self.scene)
        self.ctx.set_camera(self.camera)

    def flags(self):
        f = 0
        for bit, on in ((_lib.FLAG_AA, self.AA), (_lib.FLAG_ACCUMULATE, self.accumulates),
                        (_lib.FLAG_GAMMA, self.GAMMACORRECTED), (_lib.FLAG_NORMALMAP, self.NORMALMAPPED),
                        (_lib.FLAG_SKYBOX, self.SKYBOX), (_lib.FLAG_LIGHTED, self.LIGHTED),
                        (_lib.FLAG_STOCHASTIC, self.isStochastic)):
            if on:
                f |= bit
        return f

    def Tick(self, deltaTime: float = 0.0, frames: int = 1):
        spp = frames * (2 if self.AA else 1)
        self.ctx.set_postfx(self.camera.postfx(self.isPostProcessed))
        _, _, st = self.ctx.render(self.width, self.height, spp, self.bounces, self.flags(), self.renderingMode,
                                   self.frame, self.seed, avg=self.average, rgb8=self.screen)
        self.frame += frames
        self.last_stats = st
        return st

    def Denoise(self, params=None):
        """The current average filtered by the a-trous denoiser with fresh first-hit AOVs of the scene and camera:
        returns (average, screen) of the denoised image.  self.average, self.screen and the accumulation stay as
        Tick() left them, so progressive rendering continues undisturbed."""
        flags = _lib.FLAG_NORMALMAP if self.NORMALMAPPED else 0
        self.ctx.set_postfx(self.camera.postfx(self.isPostProcessed))  # the AOV primary rays follow Tick's (Panini)
        alb, nd = self.ctx.render_aov(self.width, self.height, flags)
        return self.ctx.denoise(self.average, alb, nd, self.width, self.height, params)

    def TickTemporal(self, params=None, motion=False):
        """One Tick() that stands alone (the accumulation is reset in full first, and the camera handed over, so a
        moved camera needs no CameraMoved()), reprojected onto the history this renderer keeps: the previous call's
        output, AOVs and camera.  Returns (history, screen): float4 with the history length in w, and its 0x00RRGGBB
        pixels (no screen pass).  self.average and self.screen are as Tick() left them.  The first call, a changed
        image size or ResetTemporal() starts a new history.  Raises with isPostProcessed: Panini primary rays are
        not described by the camera.
        motion=True follows moving instances: scene.blases is handed to the context first (set_instances), the
        instance ids are rendered with the AOVs, the previous ids and transforms are kept with the history, and the
        pass is reproject_motion with the matrices of instance_motion; a changed instance count starts a new history,
        and so does a call that follows one with motion=False (which kept no ids)."""
        if self.isPostProcessed:
            raise ValueError(PANINI_REPROJECT)
        W, H = self.width, self.height
        if motion:
            return self._tick_temporal_motion(params, W, H)
        self.ctx.set_camera(self.camera)
        self.ctx.reset_accumulation(full=True)
        self.Tick()
        _, nd = self.ctx.render_aov(W, H, _lib.FLAG_NORMALMAP if self.NORMALMAPPED else 0)
        cam = _camera_desc(self.camera)
        t = self._temporal
        if t is not None and t[:2] != (W, H):
            t = None
        hist, hist_nd, prev = t[2:5] if t is not None else (None, None, None)
        out, rgb8 = self.ctx.reproject(self.average, nd, cam, hist, hist_nd, prev, width=W, height=H, params=params)
        self._temporal = (W, H, out, nd, cam)
        return out, rgb8

    def _tick_temporal_motion(self, params, W, H):
        self.ctx.set_instances(self.scene.blases)
        self.ctx.set_camera(self.camera)
        self.ctx.reset_accumulation(full=True)
        self.Tick()
        _, nd, ids = self.ctx.render_aov_ids(W, H, _lib.FLAG_NORMALMAP if self.NORMALMAPPED else 0)
        cam = _camera_desc(self.camera)
        xf = _f32(np.stack([T for _, T in self.scene.blases])).reshape(-1, 16).copy()
        t = self._temporal
        if t is not None and (t[:2] != (W, H) or len(t) != 7 or len(t[6]) != len(xf)):
            t = None
        if t is None:
            out, rgb8 = self.ctx.reproject_motion(self.average, nd, ids, cam, width=W, height=H, params=params)
        else:
            hist, hist_nd, prev, hist_ids, prev_xf = t[2:]
            out, rgb8 = self.ctx.reproject_motion(self.average, nd, ids, cam, hist, hist_nd, prev, hist_ids,
                                                  instance_motion(xf, prev_xf), width=W, height=H, params=params)
        self._temporal = (W, H, out, nd, cam, ids, xf)
        return out, rgb8

    def TrackModel(self, index):
        """Model `index` deforms (UpdateModel every frame): its present positions are snapshotted now
        (Context.snapshot_mesh) and TickTemporalVariance(deform=True) renews the snapshot after every pass, so each
        frame's reprojection measures the deformation since the previous frame."""
        self.ctx.snapshot_mesh(index)
        if index not in self._tracked:
            self._tracked.append(index)

    def TickTemporalVariance(self, params=None, filter_params=None, deform=False):
        """TickTemporal(motion=True) with the luminance moments carried along (reproject_moments, `params`:
        temporal_defaults()) and the result filtered by denoise_variance (`filter_params`:
        denoise_variance_defaults()).  Returns (filtered, screen, history): the filtered float4 image, its 0x00RRGGBB
        pixels and the unfiltered reprojection output.  The unfiltered output and its moments are the next call's
        history (the filtered image is not fed back).  A changed image size or instance count, ResetTemporal() or a
        preceding TickTemporal() starts a new history.
        deform=True follows the models given to TrackModel() as UpdateModel() deforms them: the AOVs come from
        render_aov_deform, the pass is reproject_deform with the kept previous transforms, and every tracked model is
        snapshotted again after the pass."""
        if self.isPostProcessed:
            raise ValueError(PANINI_REPROJECT)
        W, H = self.width, self.height
        if deform:
            return self._tick_temporal_deform(params, filter_params, W, H)
        self.ctx.set_instances(self.scene.blases)
        self.ctx.set_camera(self.camera)
        self.ctx.reset_accumulation(full=True)
        self.Tick()
        alb, nd, ids = self.ctx.render_aov_ids(W, H, _lib.FLAG_NORMALMAP if self.NORMALMAPPED else 0)
        cam = _camera_desc(self.camera)
        xf = _f32(np.stack([T for _, T in self.scene.blases])).reshape(-1, 16).copy()
        t = self._temporal
        if t is not None and (t[:2] != (W, H) or len(t) != 8 or len(t[6]) != len(xf)):
            t = None
        if t is None:
            out, mom, _ = self.ctx.reproject_moments(self.average, nd, ids, cam, width=W, height=H, params=params)
        else:
            hist, hist_nd, prev, hist_ids, prev_xf, hist_mom = t[2:]
            out, mom, _ = self.ctx.reproject_moments(self.average, nd, ids, cam, hist, hist_nd, prev, hist_ids,
                                                     instance_motion(xf, prev_xf), hist_mom, width=W, height=H,
                                                     params=params)
        self._temporal = (W, H, out, nd, cam, ids, xf, mom)
        filtered, _, rgb8 = self.ctx.denoise_variance(out, mom, alb, nd, W, H, filter_params, want_variance=False)
        return filtered, rgb8, out

    def _tick_temporal_deform(self, params, filter_params, W, H):
        self.ctx.set_instances(self.scene.blases)
        self.ctx.set_camera(self.camera)
        self.ctx.reset_accumulation(full=True)
        self.Tick()
        alb, nd, ids, off = self.ctx.render_aov_deform(W, H, _lib.FLAG_NORMALMAP if self.NORMALMAPPED else 0)
        cam = _camera_desc(self.camera)
        xf = _f32(np.stack([T for _, T in self.scene.blases])).reshape(-1, 16).copy()
        t = self._temporal
        if t is not None and (t[:2] != (W, H) or len(t) != 8 or len(t[6]) != len(xf)):
            t = None
        if t is None:
            out, mom, _ = self.ctx.reproject_deform(self.average, nd, ids, cam, width=W, height=H, params=params)
        else:
            hist, hist_nd, prev, hist_ids, prev_xf, hist_mom = t[2:]
            out, mom, _ = self.ctx.reproject_deform(self.average, nd, ids, cam, hist, hist_nd, prev, hist_ids,
                                                    instance_motion(xf, prev_xf), hist_mom, off, prev_xf, width=W,
                                                    height=H, params=params)
        self._temporal = (W, H, out, nd, cam, ids, xf, mom)
        filtered, _, rgb8 = self.ctx.denoise_variance(out, mom, alb, nd, W, H, filter_params, want_variance=False)
        for index in self._tracked:
            self.ctx.snapshot_mesh(index)
        return filtered, rgb8, out

    def ResetTemporal(self):
        """The next TickTemporal() / TickTemporalVariance() starts a new history."""
        self._temporal = None

    def Capture(self, path):
        """Renderer::Capture (Core/Renderer.cpp:437-465): the screen as a PNG (the reference names it by time)."""
        from .ingest import capture_png
        capture_png(path, self.screen, self.width, self.height)

    def SaveCheckpoint(self, path):
        """Checkpoint of a long progressive render: the accumulation state plus the frame counter and
        seed the RNG stream continues from, as an .npz of plain arrays (load with allow_pickle=False)."""
        blob = np.frombuffer(self.ctx.save_accumulation(), np.uint8)
        # through a file handle: np.savez(<str>) would append ".npz" to a path without it, and LoadCheckpoint(path)
        # would then look for a file that does not exist
        with open(path, "wb") as f:
            np.savez(f, accumulation=blob, frame=np.int64(self.frame), seed=np.int64(self.seed),
                     size=np.array([self.width, self.height], np.int64))

    def LoadCheckpoint(self, path):
        """Resume from SaveCheckpoint: the next Tick continues the same frame sequence bit for bit."""
        with open(path, "rb") as f:
            z = dict(np.load(f, allow_pickle=False))
        if tuple(int(v) for v in z["size"]) != (self.width, self.height):
            raise ValueError("checkpoint of another image size")
        self.ctx.load_accumulation(z["accumulation"].tobytes())
        self.frame, self.seed = int(z["frame"]), int(z["seed"])

    def UpdateModel(self, index, mesh):
        """scene.models[index] deformed into `mesh` (same topology): the scene takes it and the context refits the
        model's BLAS in place (prt_update_mesh; a frame loop: UpdateModel, then scene.blases / TickTemporal(motion=
        True) or Tick).  The accumulation is reset in full: the accumulated frames, their sample counts and distances
        show the old geometry."""
        self.scene.update_model(index, mesh)
        self.ctx.update_mesh(index, mesh)
        self.ctx.reset_accumulation(full=True)

    def UpdateInstances(self, transforms, device=False):
        """scene.blases moved to `transforms` (one 4x4 per instance, the models stay): the context takes them and refits
        its instance BVH on the device (prt_update_instances), where Tick-time set_instances would rebuild it on the
        host.  Host transforms ((n, 4, 4) float32) also replace those in scene.blases; with device=True (a torch
        tensor on the context's device) the scene's host copy is left as it is and is stale until the next host
        update -- TickTemporal(motion=True), which hands scene.blases to the context, wants a host copy.  The
        accumulation is reset in full, as by UpdateModel.  TlasCost() tells when a set_instances pays."""
        if not device:
            T = _f32(transforms).reshape(-1, 4, 4)
            if len(T) != len(self.scene.blases):
                raise ValueError("UpdateInstances: one transform per instance")
            self.scene.blases = [(m, T[i].copy()) for i, (m, _) in enumerate(self.scene.blases)]
        self.ctx.update_instances(transforms, device=device)
        self.ctx.reset_accumulation(full=True)

    def TlasCost(self):
        """The SAH cost of the instance BVH as it stands (prt_tlas_cost)."""
        return self.ctx.tlas_cost()

    def RebuildInstances(self, transforms=None, builder=_lib.BUILDER_GPU_PLOC, device=False):
        """UpdateInstances with a fresh device build of the instance BVH in place of the refit (prt_rebuild_instances);
        transforms=None rebuilds over the instances where they are, device-resident transforms included.  TlasCost()
        tells when it pays: the library has no policy."""
        if transforms is not None and not device and not hasattr(transforms, "data_ptr"):
            T = _f32(transforms).reshape(-1, 4, 4)
            if len(T) != len(self.scene.blases):
                raise ValueError("RebuildInstances: one transform per instance")
            self.scene.blases = [(m, T[i].copy()) for i, (m, _) in enumerate(self.scene.blases)]
        self.ctx.rebuild_instances(transforms, builder=builder, device=device)
        self.ctx.reset_accumulation(full=True)

    def RebuildModel(self, index, mesh=None, builder=_lib.BUILDER_GPU_PLOC):
        """UpdateModel with a fresh device build of the model's BLAS in place of the refit (prt_rebuild_mesh); mesh=None
        rebuilds over the pose of the last SkinModel.  BlasCost(index) tells when it pays: the library has no policy."""
        if mesh is not None:
            self.scene.update_model(index, mesh)
        self.ctx.rebuild_mesh(index, mesh, builder=builder)
        self.ctx.reset_accumulation(full=True)

    def BlasCost(self, index):
        """The SAH cost of model index's BLAS as it stands (prt_blas_cost)."""
        return self.ctx.blas_cost(index)

    def SetSkin(self, index, skin):
        """scene.models[index] is skinned from now on (a scenes.Skin; None removes it): the scene keeps the skin and the
        context binds it (prt_set_mesh_skin).  SkinModel then poses the model."""
        self.scene.set_skin(index, skin)
        self.ctx.set_mesh_skin(index, skin)

    def SkinModel(self, index, matrices):
        """scene.models[index] takes the pose `matrices` ([joints, 12] float32, row-major 3 x 4): the scene keeps the
        pose and the context skins the model and refits its BLAS on the device (prt_skin_mesh; a frame loop:
        SkinModel, then scene.blases / TickTemporal(motion=True) or Tick).  The accumulation is reset in full, as by
        UpdateModel."""
        self.scene.skin_model(index, matrices)
        self.ctx.skin_mesh(index, matrices)
        self.ctx.reset_accumulation(full=True)

    def CameraMoved(self):
        """Camera::HandleInput returned true: memset of the accumulator only (Core/Renderer.cpp:147)."""
        self.ctx.set_camera(self.camera)
        self.ctx.reset_accumulation(full=False)
