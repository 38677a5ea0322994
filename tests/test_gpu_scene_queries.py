"""Device scene queries against the independent reference tests/scene_ref.py: primary rays, the skybox lookup,
materials, geometry and shading normals, and the point / directional / spot light block of a one-bounce path.

Every other GPU render test compares libprt.so with oracle/prt_oracle.c, a restatement against a restatement; here
the expected values come from scene_ref, written from the reference's source lines alone.  Two tiers (scene_ref's
docstring): bit identity for the float32 restatements, rtol = atol = scene_ref.CLOSED_TOL for the float64 closed
forms.  tests/test_scene_ref.py runs the same checks (the check_* functions below) against the oracle on the CPU.

The scenes are built here.  In `attr`, `sky` and `lit` every vertex UV is >= 0, where texel addressing is the
reference's own.  Negative, huge and boundary UVs, which include/prt.h (prt_mesh.fixed_uvs) defines beyond the
reference, are `uv_scene`'s; tests/test_gpu_texel.py feeds them to the device and tests/test_texel_ref.py to the oracle.
"""
import functools
import types

import numpy as np
import pytest

import scene_ref as R
from prt import _lib, scenes

F = np.float32
NORMALMAP, SKYBOX, LIGHTED, STOCHASTIC = _lib.FLAG_NORMALMAP, _lib.FLAG_SKYBOX, _lib.FLAG_LIGHTED, _lib.FLAG_STOCHASTIC
TOL = R.CLOSED_TOL
LIT_W, LIT_H = 96, 72  # the image of the `lit` scenes
MARGIN = 1e-3          # scene units (about 1): hit points this close to a discrete boundary are not tested
PANINI = {0: types.SimpleNamespace(fov=40.0, distortion=40.0),    # Camera member defaults (Core/Camera.h:23)
          1: types.SimpleNamespace(fov=90.0, distortion=2.0)}     # the GAME preset P1 (Core/Camera.h:20)


# ------------------------------------------------------------------------------------------------ scenes
def _mesh(P, N, UV, **tex):
    """P, N: (T,3,3), UV: (T,3,2) per corner -> the reference's Model arrays with one vertex per corner."""
    T = P.shape[0]
    verts = P.reshape(-1, 3).astype(F)
    tri4 = np.zeros((3 * T, 4), F)
    tri4[:, :3] = verts
    n4 = np.zeros((3 * T, 4), F)
    n4[:, :3] = N.reshape(-1, 3)
    fn = R.normalize(R.cross(verts[1::3] - verts[0::3], verts[2::3] - verts[0::3]))       # Core/Model.cpp:100-110
    return scenes.Mesh(tri4.reshape(-1), n4.reshape(-1), UV.reshape(-1).astype(F), np.arange(3 * T, dtype=np.int32),
                       verts.reshape(-1).copy(), fn.reshape(-1).astype(F), **tex)


def _patch(rng, nx, nz, size):
    """2 * nx * nz triangles over [-size, size]^2: a jittered lattice with random heights, every triangle with its
    own corner normals (non-unit, different per corner) and its own corner UVs in [0.05, 1.95]."""
    X, Z = np.meshgrid(np.linspace(-size, size, nx + 1), np.linspace(-size, size, nz + 1), indexing="ij")
    cx, cz = 2 * size / nx, 2 * size / nz
    X[1:-1, :] += rng.uniform(-0.3, 0.3, X[1:-1, :].shape) * cx
    Z[:, 1:-1] += rng.uniform(-0.3, 0.3, Z[:, 1:-1].shape) * cz
    Y = rng.uniform(-0.25, 0.25, X.shape)
    V = np.stack([X, Y, Z], -1)
    P = []
    for a in range(nx):
        for b in range(nz):
            v00, v01, v10, v11 = V[a, b], V[a, b + 1], V[a + 1, b], V[a + 1, b + 1]
            P += [[v00, v01, v10], [v10, v01, v11]] if rng.random() < 0.5 else [[v00, v01, v11], [v00, v11, v10]]
    P = np.array(P)
    T = P.shape[0]
    N = np.array([0.0, 1.0, 0.0]) + rng.uniform(-0.5, 0.5, (T, 3, 3))
    N *= rng.uniform(0.5, 2.0, (T, 3, 1)) / np.linalg.norm(N, axis=-1, keepdims=True)
    UV = np.zeros((T, 3, 2))
    for t in range(T):
        while True:   # a tangent frame needs a UV triangle of some area (Scene.cpp:99-100 divides by it)
            uv = rng.uniform(0.05, 1.95, (3, 2))
            d1, d2 = uv[1] - uv[0], uv[2] - uv[0]
            if abs(d1[0] * d2[1] - d1[1] * d2[0]) > 0.2:
                break
        UV[t] = uv
    return P, N, UV


def _trs(t, ry, rx, s):
    cy, sy, cx, sx = np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    M = np.eye(4)
    M[:3, :3] = (Ry @ Rx) @ np.diag(s)
    M[:3, 3] = t
    return M.astype(F)


def _no_lights():
    z = np.zeros(3, F)
    return scenes.Lights(np.zeros((4, 3), F), np.zeros((4, 3), F), z.copy(), z.copy(), z.copy(), z.copy(),
                         np.array([0, 1, 0], F))


@functools.lru_cache(None)
def attr_scene():
    """Scene `attr`: mesh 0 (16 triangles) carries an 8x4 albedo, a 16x4 normal map, a 4x8 metalness map and an 8x4
    emission map of random texels -- the normal and metalness maps' dimensions differ from the albedo's, whose width
    and height the reference indexes every map with; each has >= 32 texels, so that index stays inside.  Mesh 1
    (4 triangles) has a 5x3 albedo only.  Instances: mesh 0 as it is, mesh 1 translated, mesh 0 rotated and
    non-uniformly scaled (ratio 3.2)."""
    rng = np.random.default_rng(20240611)
    tex = [rng.integers(0, 1 << 24, shape, dtype=np.uint32) for shape in ((4, 8), (4, 16), (8, 4), (4, 8), (3, 5))]
    m0 = _mesh(*_patch(rng, 4, 2, 1.0), albedo=0, normal=1, metalness=2, emission=3)
    m1 = _mesh(*_patch(rng, 2, 1, 0.9), albedo=4)
    inst = [(0, np.eye(4, dtype=F)), (1, _trs((2.1, 0.3, 0.5), 0.0, 0.0, (1.0, 1.0, 1.0))),
            (0, _trs((-2.2, 0.2, 0.3), 0.6, 0.3, (1.6, 0.5, 0.8)))]
    return scenes.SceneData([m0, m1], tex, inst, _no_lights(), None, np.array([0.1, 3.2, -4.2], F),
                            np.array([0.0, 0.0, 0.0], F), "attr")


# The constant UVs of `uv_scene`, by class (include/prt.h prt_mesh.fixed_uvs: any float is defined).  "boundary":
# multiples of 1/8 or 1/4, texel boundaries of an 8x4 albedo, where the interpolation's rounding decides the side;
# "huge": finite values whose product with the size passes 2^24 (the texel is the rounding's), reaches 2^31 exactly
# (2^28 * 8), exceeds it, or overflows to infinity (3.4e38 * 8).
UV_CLASSES = (
    ("negative", (-0.3, -0.55, -1.7, -2.25, -0.05, -3.9, -0.999, -1.001, -7.4, -0.51, -1e-8, -0.125001)),
    ("minus_one", (-1.0, -1.0)),
    ("ge_2", (2.0, 2.6, 3.125, 17.3, 2.0000002, 255.9)),
    ("boundary", (0.125, 0.25, 0.5, 0.75, -0.125, -0.25, 1.0, -2.0, 0.375, -0.5, -0.75, 1.5, 0.0, -0.0, -1.25, 2.25)),
    ("huge", (1e9, 2.6e8, -2.6e8, -3e9, 3.4e38, -3.4e38, 16777216.0, -16777216.0, 268435456.0, -268435456.0, 5.3e8,
              1e20)),
)
UV_VARYING = 12   # further triangles of `uv_scene` whose UVs vary across the triangle, class "straddle"


def uv_triangle_classes():
    """(class of u, class of v) of every triangle of `uv_scene`'s mesh; triangle i's constant UV is
    (value[i], value[(7 i + 3) % n]) of UV_CLASSES flattened."""
    flat = [(name, x) for name, xs in UV_CLASSES for x in xs]
    n = len(flat)
    const = [(flat[i], flat[(7 * i + 3) % n]) for i in range(n)]
    return ([(a[0], b[0]) for a, b in const] + [("straddle", "straddle")] * UV_VARYING,
            np.array([(a[1], b[1]) for a, b in const], F))


@functools.lru_cache(None)
def uv_scene(shift=0):
    """Scene `uv`: one mesh of 60 small triangles in a 10 x 6 grid facing the camera, about 25 pixels each at 96x72,
    under an 8x4 albedo, a 16x4 normal map, a 4x8 metalness map and an 8x4 emission map whose texels are distinct
    within each map (in the metalness map the roughness and the metalness bytes are each distinct), so a wrong texel
    shows in every mode.  48 triangles carry one UV at all three corners (UV_CLASSES); 12 carry UVs that vary across
    the triangle around 0 and around -1 in each component, with a UV triangle of some area, so the normal-mapped
    branch is finite there.  One identity instance, a directional and a point light on the camera's side.
    shift != 0: the same scene with triangle i carrying triangle (i + shift)'s UVs."""
    rng = np.random.default_rng(20240917)
    classes, const = uv_triangle_classes()
    T = len(classes)
    assert T == 60 and const.shape == (48, 2)
    tex = [rng.choice(1 << 24, 32, replace=False).astype(np.uint32).reshape(4, 8),
           rng.choice(1 << 24, 64, replace=False).astype(np.uint32).reshape(4, 16),
           ((rng.choice(256, 32, replace=False) << 8) | rng.choice(256, 32, replace=False)).astype(np.uint32).reshape(8, 4),
           rng.choice(1 << 24, 32, replace=False).astype(np.uint32).reshape(4, 8)]
    P = np.zeros((T, 3, 3))
    for t in range(T):
        x0, y0 = -3.0 + 0.6 * (t % 10), -1.8 + 0.6 * (t // 10)
        P[t] = [[x0 + 0.04, y0 + 0.05, 0.0], [x0 + 0.56, y0 + 0.08, 0.0], [x0 + 0.27, y0 + 0.57, 0.0]]
    P[:, :, 2] = rng.uniform(-0.1, 0.1, (T, 3))
    N = np.array([0.0, 0.0, -1.0]) + rng.uniform(-0.4, 0.4, (T, 3, 3))
    N *= rng.uniform(0.5, 2.0, (T, 3, 1)) / np.linalg.norm(N, axis=-1, keepdims=True)
    UV = np.zeros((T, 3, 2), F)
    UV[:48] = const[:, None, :]
    for t in range(48, T):
        centre = np.array([(0.0, -1.0)[(t >> 0) & 1], (0.0, -1.0)[(t >> 1) & 1]])
        while True:
            uv = centre + rng.uniform(-0.45, 0.45, (3, 2))
            d1, d2 = uv[1] - uv[0], uv[2] - uv[0]
            if abs(d1[0] * d2[1] - d1[1] * d2[0]) > 0.1 and (uv.min(0) < centre).all() and (uv.max(0) > centre).all():
                break
        UV[t] = uv
    UV = np.roll(UV, -shift, 0)
    mesh = _mesh(P, N, UV, albedo=0, normal=1, metalness=2, emission=3)
    far, black = [0.0, 60.0, 0.0], [0.0, 0.0, 0.0]
    lights = scenes.Lights(np.array([[0.5, 0.3, -2.0], far, far, far], F), np.array([[4.0, 3.0, 2.0], black, black, black], F),
                           np.array([10.0, 20.0, -40.0], F), np.array([3.0, 2.5, 2.0], F),
                           np.array([0.0, 3.0, 0.0], F), np.array(black, F), np.array([0.0, 1.0, 0.0], F))
    return scenes.SceneData([mesh], tex, [(0, np.eye(4, dtype=F))], lights, None, np.array([0.0, 0.0, -5.0], F),
                            np.array([0.0, 0.0, 0.0], F), "uv" if not shift else "uv-shift%d" % shift)


@functools.lru_cache(None)
def sky_scene(camera):
    """Mesh 1 of `attr` under a 37x19 random sky.  camera "seam" looks along -x, so the atan2 = +-pi seam of the
    lookup's u crosses the image; "up" is pitched up about 50 degrees, so the first sky rows are in view (the pole
    itself stays outside the image)."""
    a = attr_scene()
    sky = np.random.default_rng(7).uniform(0.0, 4.0, (19, 37, 3)).astype(F)
    pos, tgt = {"seam": ((3.0, 0.8, 0.25), (-1.0, 0.5, 0.1)), "up": ((1.5, -2.0, -2.0), (0.9, 0.4, -0.6))}[camera]
    return scenes.SceneData([a.meshes[1]], [a.textures[4]] * 5, [(0, np.eye(4, dtype=F))], _no_lights(), sky,
                            np.array(pos, F), np.array(tgt, F), "sky-" + camera)


def _quad(cx, y, cz, half, **tex):
    c = np.array([[cx - half, y, cz - half], [cx - half, y, cz + half], [cx + half, y, cz - half],
                  [cx + half, y, cz + half]])
    P = np.array([[c[0], c[1], c[2]], [c[2], c[1], c[3]]])              # (v00, v01, v10): +y face normals
    UV = np.array([[[0.1, 0.1], [0.1, 0.9], [0.9, 0.1]], [[0.9, 0.1], [0.1, 0.9], [0.9, 0.9]]])
    return _mesh(P, np.tile(np.array([0.0, 1.0, 0.0]), (2, 3, 1)), UV, **tex)


@functools.lru_cache(None)
def lit_scene(variant="classes"):
    """Scene `lit`: a 6x6 floor quad at y = 0 with a 1x1 albedo and a 1x1 metalness / roughness map (roughness 0.4,
    metalness 0.8 over a saturated albedo), plus one occluder quad that shares the maps; every instance is the
    identity.
    "classes": four point lights of distinct colours, a directional light and a spot light above the origin whose
      cone edge (factor 0.9, radius 3 tan(acos 0.9) = 1.45) crosses the floor; the occluder's directional shadow
      falls inside the cone, apart from its spot shadow, so no pixel is dark for two classes at once.  The four
      point-class candidates share the summed contribution and differ in the BRDF's light direction alone: F0
      differs strongly between the channels (metalness 0.8, albedo 0xF88030), so two directions that agree in one
      channel disagree in another, and the lights and the camera are placed without symmetry; the lights are bright
      enough that the differences clear 100 times the tolerance (check_candidates_distinct).
    "above": only point light 0 shines, 2 above the floor, with the quad 1 above IT: floor points whose ray through
      the light reaches the quad are in shadow in the reference, whose shadow ray runs to tmax = d^2 - EPSILON
      (Renderer.cpp:257): it reaches the quad at 1.5 d < d^2 - EPSILON since d >= 2.
    "below": only point light 1 shines, 0.5 above the floor, with the quad at 0.35 between: the floor under it is
      lit in the reference because tmax = 0.25 - EPSILON ends the ray before the quad.
    Both are the opposite of the physical answer, which tmax = d - EPSILON would give."""
    tex = [np.array([[0xF88030]], np.uint32), np.array([[0x0066CC]], np.uint32)]
    floor = _quad(0.0, 0.0, 0.0, 3.0, albedo=0, metalness=1)
    far = [0.0, 60.0, 0.0]
    black = [0.0, 0.0, 0.0]
    if variant == "classes":
        occ = _quad(0.8, 0.8, -0.6, 0.3, albedo=0, metalness=1)
        lights = scenes.Lights(
            np.array([[-2.0, 2.2, -1.0], [1.8, 2.6, 1.4], [-1.2, 3.0, 2.0], [1.0, 1.4, -2.2]], F),
            np.array([[90.0, 18.0, 12.0], [12.0, 75.0, 18.0], [15.0, 21.0, 90.0], [60.0, 60.0, 9.0]], F),
            np.array([30.0, 40.0, -20.0], F), np.array([15.0, 14.0, 12.0], F),
            np.array([0.0, 3.0, 0.0], F), np.array([60.0, 30.0, 80.0], F), np.array([0.0, 1.0, 0.0], F))
        cam = ((0.7, 3.5, -5.5), (0.0, 0.0, 0.0))
    elif variant == "above":
        occ = _quad(0.5, 3.0, 0.3, 0.25, albedo=0, metalness=1)
        lights = scenes.Lights(np.array([[0.5, 2.0, 0.3], far, far, far], F), np.array([[4.0, 3.0, 2.0], black, black, black], F),
                               np.array([30.0, 40.0, -20.0], F), np.array(black, F),
                               np.array([0.0, 3.0, 0.0], F), np.array(black, F), np.array([0.0, 1.0, 0.0], F))
        cam = ((0.0, 2.6, -4.0), (0.5, 0.0, 0.3))
    elif variant == "below":
        occ = _quad(-0.4, 0.35, 0.2, 0.1, albedo=0, metalness=1)
        lights = scenes.Lights(np.array([far, [-0.4, 0.5, 0.2], far, far], F), np.array([black, [2.0, 3.0, 4.0], black, black], F),
                               np.array([30.0, 40.0, -20.0], F), np.array(black, F),
                               np.array([0.0, 3.0, 0.0], F), np.array(black, F), np.array([0.0, 1.0, 0.0], F))
        cam = ((-0.4, 1.6, -2.0), (-0.4, 0.0, 0.2))
    else:
        raise ValueError(variant)
    eye = np.eye(4, dtype=F)
    return scenes.SceneData([floor, occ], tex, [(0, eye), (1, eye.copy())], lights, None, np.array(cam[0], F),
                            np.array(cam[1], F), "lit-" + variant)


# ------------------------------------------------------------------------------------------------ shared checks
# A `view` is one implementation under test loaded with one scene at one image size: view.hits() -> the primary hit
# records (t, u, v, prim, inst), view.render(flags, mode) -> [n, 3] float32 of one spp = 1, bounces = 1 frame.
def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got, F), np.ascontiguousarray(exp, F)
    bad = np.flatnonzero((bits(got) != bits(exp)).reshape(got.shape[0], -1).any(-1))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:3]], exp[bad[:3]])


def camera_rays(sd, W, H, postfx=None):
    """(O, D) of every pixel: scene_ref's singly-normalised primary directions."""
    cam = R.camera(sd.cam_pos, sd.cam_target, F(W) / F(H))
    ys, xs = np.mgrid[0:H, 0:W]
    D = R.primary_rays(cam, W, H, xs.reshape(-1), ys.reshape(-1), postfx)
    return np.repeat(cam["pos"][None], W * H, 0), D


def check_primary(traced, intersected):
    """Test 1: intersect() of scene_ref's rays returns trace_primary()'s records bit for bit, at every pixel; both
    hand the direction to the same tinybvh::Ray constructor restatement.  Returns the hit mask."""
    for k in ("t", "u", "v"):
        assert np.array_equal(bits(traced[k]), bits(intersected[k])), k
    hit = traced["t"] < R.BVH_FAR
    assert np.array_equal(hit, intersected["t"] < R.BVH_FAR)           # the miss pattern
    assert hit.sum() > 100 and (~hit).sum() > 100
    for k in ("prim", "inst"):
        assert np.array_equal(traced[k][hit], intersected[k][hit]), k
    return hit


def check_sky(view, sd, W, H):
    """Test 2: every miss pixel of a SKYBOX-only frame equals sample_sky bit for bit.  Returns the u0 columns."""
    h = view.hits()
    miss = ~(h["t"] < R.BVH_FAR)
    assert miss.mean() > 0.5
    _, D = camera_rays(sd, W, H)
    D = R.ray_ctor_dir(D)[miss]
    assert_bits(view.render(SKYBOX, 0)[miss], R.sample_sky(sd.sky, D), "sky")
    taps = R.sky_taps(D, sd.sky.shape[1], sd.sky.shape[0])
    return taps[2], taps[3]


def _inst_pixels(sd, h, inst):
    sel = np.flatnonzero((h["t"] < R.BVH_FAR) & (h["inst"] == inst))
    mesh = sd.meshes[sd.instances[inst][0]]
    return sel, mesh, h["prim"][sel], h["u"][sel], h["v"][sel]


def _normal_close(got, exp, what):
    """Closed-form tier for normals: TOL relative to the vector's length."""
    err = np.abs(got.astype(np.float64) - exp).max(-1) / np.linalg.norm(exp, axis=-1)
    assert err.max() <= TOL, (what, err.max())
    return float(err.max())


def _close(got, exp, what):
    err = np.abs(got.astype(np.float64) - exp) / (1.0 + np.abs(exp))
    assert err.max() <= TOL, (what, err.max())
    return float(err.max())


def check_attributes(view, sd, insts, exact, aov=None):
    """Tests 3 and 4: the debug modes 1..6 (and, with `aov` = {flags: (albedo, normal_depth)}, the AOV images) at
    the pixels that hit `insts`, against material / shading_normal / geometry_normal evaluated at the primary hit
    records.  exact: everything bit for bit, the normal matrix being exact; else the normals against the float64
    normal matrix within TOL of their length, the texel-derived values still bit for bit.  Returns the coverage the
    tests assert on and the largest normal deviation seen."""
    h = view.hits()
    cov = dict(mapped=0, smooth=0, uv_ge_1=0, own_dims_differ=0, worst=0.0)
    img = {(fl, mode): view.render(fl, mode) for fl in (0, NORMALMAP) for mode in range(1, 7)}
    for inst in insts:
        sel, mesh, prim, u, v = _inst_pixels(sd, h, inst)
        assert sel.size > 200, (inst, sel.size)
        nm = R.normal_matrix(sd.instances[inst][1])
        if exact:
            nm = nm.astype(F)
            assert np.array_equal(nm[:3, :3], np.eye(3, dtype=F))
        m = R.material(mesh, sd.textures, prim, u, v)
        uv = R.hit_uv(mesh, prim, u, v)
        cov["uv_ge_1"] += int((uv >= 1).any(-1).sum())
        for t in (mesh.normal, mesh.metalness):
            if t >= 0:
                own = R.texel_index(uv, sd.textures[t].shape[1], sd.textures[t].shape[0])
                cov["own_dims_differ"] += int((own != m["texel"]).sum())
        g = R.geometry_normal(mesh, nm, prim)
        for fl in (0, NORMALMAP):
            n = R.shading_normal(mesh, sd.textures, nm, prim, u, v, bool(fl & NORMALMAP))
            cov["mapped" if (mesh.normal >= 0 and fl) else "smooth"] += sel.size
            what = (sd.name, inst, fl)
            assert_bits(img[fl, 1][sel], m["base"], what + ("mode 1",))
            for mode, key in ((4, "metalness"), (5, "roughness")):
                assert_bits(img[fl, mode][sel], np.repeat(m[key][:, None], 3, 1), what + (mode,))
            assert_bits(img[fl, 6][sel], m["emissive"], what + ("mode 6",))
            if exact:
                assert_bits(img[fl, 2][sel], (g + F(1)) * F(0.5), what + ("mode 2",))     # Renderer.cpp:185,188
                assert_bits(img[fl, 3][sel], (n + F(1)) * F(0.5), what + ("mode 3",))
            else:
                cov["worst"] = max(cov["worst"], _close(img[fl, 2][sel], (g + 1.0) * 0.5, what + ("mode 2",)),
                                   _close(img[fl, 3][sel], (n + 1.0) * 0.5, what + ("mode 3",)))
            if aov is not None:
                albedo, nd = aov[fl]
                assert_bits(albedo[sel, :3], m["base"], what + ("aov albedo",))
                assert_bits(nd[sel, 3], h["t"][sel], what + ("aov depth",))
                if exact:
                    assert_bits(nd[sel, :3], n, what + ("aov normal",))
                else:
                    cov["worst"] = max(cov["worst"], _normal_close(nd[sel, :3], n, what + ("aov normal",)))
    return cov


def assert_attr_coverage(cov):
    assert cov["mapped"] > 0 and cov["smooth"] > 0          # both shading-normal branches
    assert cov["uv_ge_1"] > 0                               # a uv that wraps
    assert cov["own_dims_differ"] > 0                       # a texel the map's own dimensions would place elsewhere


def world_triangles(sd):
    out = []
    for mi, T in sd.instances:
        P = np.asarray(sd.meshes[mi].triangles, np.float64).reshape(-1, 4)[:, :3]
        T = np.asarray(T, np.float64)
        out.append((P @ T[:3, :3].T + T[:3, 3]).reshape(-1, 3, 3))
    return np.concatenate(out), np.cumsum([0] + [len(o) for o in out])


def _outcomes(I, lights, tris):
    """Every discrete decision of the light block at hit points I: which triangle each shadow ray meets, and the
    spot's cone test."""
    return np.concatenate([R.shadow_hits(I, lights, tris).reshape(I.shape[0], -1),
                           (R.spot_factor(I, lights) > 0.9)[:, None]], 1)


class LightRef:
    """The closed form of one `lit` scene at the primary hits `h` (computed once per view, shared by the tests):
    hit mask, tested mask, direct_light's candidates, the visibility under the reference's and under the physical
    shadow range."""

    def __init__(self, sd, W, H, h):
        self.sd = sd
        self.hit = h["t"] < R.BVH_FAR
        sel = np.flatnonzero(self.hit)
        O, D = camera_rays(sd, W, H)
        D = R.ray_ctor_dir(D)[sel].astype(np.float64)
        I = O[sel].astype(np.float64) + h["t"][sel].astype(np.float64)[:, None] * D      # tiny_bvh.h:586
        tris, first = world_triangles(sd)
        tri = tris[first[h["inst"][sel]] + h["prim"][sel]]
        N = np.zeros((sel.size, 3), F)
        mat = {k: np.zeros((sel.size,) + s, F) for k, s in (("base", (3,)), ("metalness", ()), ("roughness", ()),
                                                            ("emissive", (3,)))}
        for inst, (mi, T) in enumerate(sd.instances):
            k = h["inst"][sel] == inst
            mesh = sd.meshes[mi]
            nm = R.normal_matrix(T).astype(F)
            N[k] = R.shading_normal(mesh, sd.textures, nm, h["prim"][sel][k], h["u"][sel][k], h["v"][sel][k], False)
            m = R.material(mesh, sd.textures, h["prim"][sel][k], h["u"][sel][k], h["v"][sel][k])
            for key in mat:
                mat[key][k] = m[key]
        # not tested: hit points within MARGIN of an edge of their triangle ...
        edge = np.full(sel.size, np.inf)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            A, B = tri[:, a], tri[:, b]
            s = np.clip(np.sum((I - A) * (B - A), -1) / np.sum((B - A) ** 2, -1), 0.0, 1.0)
            edge = np.minimum(edge, np.linalg.norm(I - (A + s[:, None] * (B - A)), axis=-1))
        ok = edge > MARGIN
        # ... or of a shadow boundary of any light (an occluder's edge or inner diagonal grazed by the shadow ray,
        # the end of the shadow range) or of the spot's cone edge: a discrete outcome changes among eight points
        # on a circle around the hit point in its triangle's plane.  A straight boundary closer than
        # r cos(22.5 deg) crosses the octagon; r = 1.1 MARGIN makes that MARGIN.
        e1 = tri[:, 1] - tri[:, 0]
        e1 /= np.linalg.norm(e1, axis=-1, keepdims=True)
        nrm = np.cross(e1, tri[:, 2] - tri[:, 0])
        e2 = np.cross(nrm / np.linalg.norm(nrm, axis=-1, keepdims=True), e1)
        centre = _outcomes(I, sd.lights, tris)
        for a in np.arange(8) * (np.pi / 4):
            probe = I + 1.1 * MARGIN * (np.cos(a) * e1 + np.sin(a) * e2)
            ok &= (_outcomes(probe, sd.lights, tris) == centre).all(-1)
        self.sel, self.I, self.ok = sel, I, ok
        self.visible = R.visibility(I, sd.lights, tris)
        self.physical = R.visibility(I, sd.lights, tris, physical=True)
        self.inside = R.spot_factor(I, sd.lights) > 0.9
        self.cand = R.direct_light(I, N, -D, mat, sd.lights, self.visible)
        self.six = np.concatenate([self.cand["point"], self.cand["dir"][None], self.cand["spot"][None]])  # (6,n,3)

    def matches(self, got):
        """bool (6, n): candidate j matches the pixel in every channel within rtol = atol = TOL."""
        return (np.abs(got[self.sel].astype(np.float64)[None] - self.six) <= TOL + TOL * np.abs(self.six)).all(-1)

    def worst(self, got, exp):
        return float((np.abs(got[self.sel].astype(np.float64) - exp) / (1.0 + np.abs(exp)))[self.ok].max())


def check_exclusion_cap(ref):
    """At most 10 % of the hit pixels are left out."""
    assert ref.sel.size > 500
    assert (~ref.ok).mean() <= 0.10, (~ref.ok).mean()


def check_candidates_distinct(ref):
    """At every tested pixel the six candidates differ pairwise by more than 100 times the tolerance in some channel."""
    for a in range(6):
        for b in range(a + 1, 6):
            x, y = ref.six[a][ref.ok], ref.six[b][ref.ok]
            far = (np.abs(x - y) > 100 * (TOL + TOL * np.maximum(np.abs(x), np.abs(y)))).any(-1)
            assert far.all(), (a, b, int((~far).sum()), x[~far][:2], y[~far][:2])


def check_plain_light(view, ref):
    """Test 5: LIGHTED only -- every tested pixel is emissive + brdf * colour * cos * visible (Renderer.cpp:312-326)."""
    got = view.render(LIGHTED, 0)
    exp = ref.cand["plain"]
    assert ref.ok.sum() > 500
    assert ((~ref.visible[:, 4]) & ref.ok).sum() > 10 and (ref.visible[:, 4] & ref.ok).sum() > 10   # shadow and light
    worst = ref.worst(got, exp)
    assert worst <= TOL, worst
    return worst


def check_light_classes(view, ref):
    """Test 6: LIGHTED | STOCHASTIC -- every tested pixel matches exactly one of direct_light's six candidates, each
    outcome occurs, and the classes' shares lie within 4 sigma of 0.3 / 0.5 / 0.2."""
    got = view.render(LIGHTED | STOCHASTIC, 0)
    m = ref.matches(got)[:, ref.ok]
    n = m.shape[1]
    count = m.sum(0)
    assert (count == 1).all(), (int((count == 0).sum()), int((count > 1).sum()), n)
    assert m.any(1).all(), m.sum(1)                                      # each of the six outcomes
    assert (ref.inside & ref.ok).any() and (~ref.inside & ref.ok).any()  # both sides of the cone edge
    for share, p in ((m[:4].sum() / n, 0.3), (m[4].sum() / n, 0.5), (m[5].sum() / n, 0.2)):
        assert abs(share - p) <= 4 * np.sqrt(p * (1 - p) / n), (share, p, n)
    which = ref.matches(got).argmax(0)
    return ref.worst(got, ref.six[which, np.arange(which.size)])


def check_shadow_range(view, ref, light, lit_in_reference):
    """Test 7: the pixels where the reference's shadow range (tmax = d^2 - EPSILON) and the physical one
    (d - EPSILON) disagree about point light `light`, the only light that shines.  Every tested pixel matches a
    candidate; in that region the reference's answer holds: dark, or lit for the point class' share of the pixels."""
    region = ref.ok & (ref.visible[:, light] == lit_in_reference) & (ref.physical[:, light] != lit_in_reference)
    n = int(region.sum())
    assert n >= 30, n
    got = view.render(LIGHTED | STOCHASTIC, 0)
    assert ref.matches(got)[:, ref.ok].any(0).all()
    bright = np.abs(got[ref.sel][region]).max(-1) > 1e-3
    if not lit_in_reference:
        assert not bright.any(), int(bright.sum())
    else:
        assert (ref.six[:4, region].max(-1) > 0.05).all()   # the lit value is far from dark for every whichLight
        assert abs(bright.mean() - 0.3) <= 4 * np.sqrt(0.3 * 0.7 / n), (bright.mean(), n)
    return n


# ------------------------------------------------------------------------------------------------ the device
pytestmark = pytest.mark.gpu


class GpuView:
    """One scene at one image size on the shared context; whichever view is used puts its scene back first."""
    _loaded = None

    def __init__(self, ctx, sd, W, H):
        self.ctx, self.sd, self.W, self.H = ctx, sd, W, H
        self._hits = None

    def load(self):
        if GpuView._loaded is not self:
            from helpers import gpu_scene
            self.ctx.set_postfx(None)
            gpu_scene(self.ctx, self.sd, self.W, self.H)
            GpuView._loaded = self
        return self.ctx

    def hits(self):
        if self._hits is None:
            self._hits = self.load().trace_primary(self.W, self.H)[0]
        return self._hits

    def render(self, flags, mode):
        ctx = self.load()
        ctx.reset_accumulation(full=True)
        return ctx.render(self.W, self.H, 1, 1, flags, mode)[0][:, :3].copy()


@pytest.mark.parametrize("preset", [None, 0, 1])
def test_primary_rays(gpu_ctx, preset):
    """prt_trace_primary's rays are scene_ref.primary_rays: plane projection, and Panini at both presets.
    prt_trace_primary and prt_intersect both build their ray with make_ray (prt_traverse.h), the restatement of the
    tinybvh::Ray constructor, so the singly-normalised direction goes in."""
    import prt
    sd, W, H = attr_scene(), 97, 61
    view = GpuView(gpu_ctx, sd, W, H)
    view.load()
    try:
        if preset is not None:
            pf = prt.postfx_preset(preset)
            assert (pf.fov, pf.distortion) == (PANINI[preset].fov, PANINI[preset].distortion)
            gpu_ctx.set_postfx(pf)
        O, D = camera_rays(sd, W, H, PANINI[preset] if preset is not None else None)
        check_primary(view.hits(), gpu_ctx.intersect(O, D))
    finally:
        gpu_ctx.set_postfx(None)
        GpuView._loaded = None


def test_map_needs_the_albedo_texel_count_not_its_width(gpu_ctx):
    """Every map is read at a flat index below the albedo's texel count (Scene.cpp:79-85,160-165): `attr`'s 4x8
    metalness map under its 8x4 albedo loads (the reference renders it); a map of fewer texels is refused, since
    that index would run past its end."""
    import dataclasses
    import prt
    sd = attr_scene()
    GpuView(gpu_ctx, sd, 16, 12).load()
    short = list(sd.textures)
    short[2] = short[2][:7]                     # 4 x 7 = 28 texels < 32
    try:
        with pytest.raises(prt._lib.PrtError):
            gpu_ctx.set_scene(prt.Scene.from_data(dataclasses.replace(sd, textures=short)))
    finally:
        GpuView._loaded = None


def test_sky(gpu_ctx):
    cols = []
    for camera in ("seam", "up"):
        sd = sky_scene(camera)
        cols.append(check_sky(GpuView(gpu_ctx, sd, 61, 47), sd, 61, 47))
    assert (cols[0][0] == 36).any() and (cols[0][0] == 0).any()      # both columns at the seam
    assert (cols[1][1] <= 1).any()                                   # small v


@pytest.fixture(scope="module")
def attr_view(gpu_ctx):
    sd, W, H = attr_scene(), 128, 96
    view = GpuView(gpu_ctx, sd, W, H)
    h = view.hits()
    hit = h["t"] < R.BVH_FAR
    aov = {}
    for fl in (0, NORMALMAP):
        albedo, nd, ids = gpu_ctx.render_aov_ids(W, H, fl)
        assert np.array_equal(ids[hit], h["inst"][hit]) and (ids[~hit] == 0xFFFFFFFF).all()
        aov[fl] = (albedo, nd)
    return view, aov


def test_material_and_normals_exact(attr_view):
    view, aov = attr_view
    assert_attr_coverage(check_attributes(view, view.sd, (0, 1), True, aov))


def test_normals_general_transform(attr_view):
    view, aov = attr_view
    cov = check_attributes(view, view.sd, (2,), False, aov)
    print("largest normal deviation (mode images: / (1 + |x|); AOV: / length):", cov["worst"])


@pytest.fixture(scope="module")
def lit_classes(gpu_ctx):
    sd = lit_scene("classes")
    view = GpuView(gpu_ctx, sd, LIT_W, LIT_H)
    return view, LightRef(sd, LIT_W, LIT_H, view.hits())


def test_plain_directional_light(lit_classes):
    view, ref = lit_classes
    check_exclusion_cap(ref)
    print("largest deviation / (1 + |x|):", check_plain_light(view, ref))


def test_stochastic_light_classes(lit_classes):
    view, ref = lit_classes
    check_candidates_distinct(ref)
    print("largest deviation / (1 + |x|):", check_light_classes(view, ref))


@pytest.mark.parametrize("variant,light,lit", [("above", 0, False), ("below", 1, True)])
def test_point_shadow_range_is_squared_distance(gpu_ctx, variant, light, lit):
    sd = lit_scene(variant)
    view = GpuView(gpu_ctx, sd, LIT_W, LIT_H)
    ref = LightRef(sd, LIT_W, LIT_H, view.hits())
    check_exclusion_cap(ref)
    check_shadow_range(view, ref, light, lit)
