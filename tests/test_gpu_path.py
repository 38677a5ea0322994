"""Multi-bounce paths on the device against the independent float64 path reference tests/path_ref.py.
tests/test_path_ref.py runs the same checks (the check_* functions below) against the oracle on the CPU, and proves
the reference itself.

Everything a path does after its first hit -- the lobe pick and throughput / p, throughput * weight, shading at depth
>= 1 (emission, direct light with the shadow ray and V = -D of a bounced ray, scaled by the throughput), the sky on an
indirect miss, the depth cap, the result + Trace(..) * throughput unwinding, MIS at a vertex that is neither first nor
last, a dielectric tree whose children hit shaded surfaces -- was checked only between libprt.so and
oracle/prt_oracle.c, two restatements by one author.  Here the expected values are path_ref's.

Scenes, all 16 x 12 with test_gpu_estimator's SEED, CHUNK and FLAGS (no AA, no gamma; the skybox flag where there is a
sky), built from its floor_scene / _flat_quad / sky_ramp and test_gpu_scene_queries._mesh:
  sky-floor         the floor under sky_ramp(), dark lights, the three MATERIALS; bounces 2 and 3 (the floor is planar:
                    the same expectation at both)
  corner            a (0.5, 1) floor, an upright wall at z = 2 facing the camera with its own 1 x 1 maps (another
                    albedo, roughness 0.5 / metalness 0.5, an emission texel) and a small quad at y = 1.4 that shadows
                    part of the floor and of the wall from the directional light (no camera ray meets it; bounced rays
                    meet either face); sky_ramp(); bounces 2, 3, 4 without the stochastic flag, bounces 3 with it and
                    with the four point lights and the spot light lit
  corner-area       the corner with a (1, 0) floor, no emission map, dark reference lights and the `big` light of
                    test_gpu_estimator over the floor; bounces 3: MIS at depth 0 and 1, an unweighted last segment at
                    depth 2, BRDF rays from the wall reaching the light; and bounces 1, where the first hit is the
                    last segment (the planted slip of a weighted last segment shows there, see test_path_ref.py)
  corner-turned     the corner (plain and stochastic lights) with instances, camera and lights under one rigid motion
                    G, a rotation about a generic axis and a translation; mesh k is authored rotated by Q_k^-1 and
                    instanced with G Q_k, so every instance has its own rotation and no world normal is axis-aligned
                    (path_ref carries rectangles under rigid transforms); bounces 3 with and without the stochastic
                    flag.  The sky does not turn and the camera's up stays (0, 1, 0): another scene, not another view
  glass-over-floor  a DIELECTRIC quad over part of the floor, whose emission texel is lit, under sky_ramp(), seen from
                    steeply above (GLASS_CAM); bounces 3 and 4: the refracted child shades the floor, whose bounce
                    meets the glass's back face
  mirror-corner     floor and wall MIRROR (exact, see check_mirror_corner)
The non-extension scenes take the deferred-resolve pipeline and the primary-surface record, the area-light and glass
scenes the extension kernels.

Statistical cases.  n = 4096 device frames (N_FRAMES_OF: more where the power condition needs it), M = 4 n reference
paths per tested pixel.  Tested pixels: those whose primary ray passes further than MARGIN from every outline and
meets a rectangle first (not the shadowing quad); at least 60 per scene and 20 per class (floor, wall, glass), thinned
to TESTED_CAP per class to bound the reference's time.  Bounds, fixed before any run, sigma being the REFERENCE's
sample standard deviation of one path:
  per pixel and channel  |mean_dev - mean_ref| <= 6 sigma sqrt(1 / n + 1 / M)
  per channel, summed    |sum mean_dev - sum mean_ref| <= 6 sqrt(sum sigma^2 (1 / n + 1 / M))
test_path_ref.py asserts from the reference alone that every summed bound is below 10 % of the summed expectation.

A pixel whose reference sigma is 0 (a shadowed pixel at bounces 1) must equal the reference exactly.
The largest z (deviation over sigma sqrt(1 / n + 1 / M); the bound is 6) seen on the oracle, whose frames the device
reproduces bit for bit (test_device_equals_oracle), and the reference's run time are recorded in
tests/test_path_ref.py; on an MI355X every case printed the oracle's sums and z to the last digit, largest pixel 3.05
(corner-area, bounces 3), largest sum 2.17 (corner-turned-plain; 1.95 on sky-floor (0.5, 0.5)), 1 to 2.3 s per test.
"""
import functools

import numpy as np
import pytest

import estimator_ref as E
import path_ref as P
import scene_ref as R
import test_gpu_estimator as Q
import test_gpu_scene_queries as SQ
from prt import _lib, scenes

F = np.float32
W, H = Q.W, Q.H
N_FRAMES = 4096
N_FRAMES_OF = {}           # (scene, bounces) -> frames, where 4096 miss the 10 % power condition
REF_FACTOR = 4             # M = REF_FACTOR * n reference paths per tested pixel
REF_SEED = 20251021
MARGIN = Q.MARGIN
TESTED_CAP = 30            # tested pixels per class (every class keeps at least 20, every scene at least 60)
WALL_Z, WALL_H = 2.0, 3.0
BLOCKER = (-0.6, 1.4, 1.0, 0.8)
DIR_POS, DIR_COL = (-4.0, 5.0, -3.0), (24.0, 20.0, 16.0)
GLASS = (0.0, 0.8, -0.2, 0.9)      # cx, y, cz, half
# steep enough that every camera ray enters the glass inside asin(1 / 1.46) = 43.2 degrees of its normal (at most 37
# degrees, at the far corners): beyond that refract() returns the zero direction and the child shades nothing
GLASS_CAM = ((0.0, 4.0, -1.5), (0.0, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------ scenes
def _upright_quad(x0, x1, y0, y1, z, **tex):
    """A quad in the plane z = const whose face and vertex normals point to -z, towards the camera."""
    c = np.array([[x0, y0, z], [x0, y1, z], [x1, y0, z], [x1, y1, z]])
    Pp = np.array([[c[0], c[1], c[2]], [c[2], c[1], c[3]]])
    return SQ._mesh(Pp, np.tile(np.array([0.0, 0.0, -1.0]), (2, 3, 1)), np.full((2, 3, 2), 0.5), **tex)


def _lights(stochastic):
    lg = Q._dark_lights()
    lg.dir_pos[:], lg.dir_col[:] = DIR_POS, DIR_COL
    if stochastic:      # every class contributes: the point lights in front of the wall, the spot above the floor
        lg.point_pos[:] = [[-2.0, 2.2, -1.0], [1.8, 2.6, 1.4], [-1.2, 3.0, 1.0], [1.0, 1.4, -2.2]]
        lg.point_col[:] = [[3.0, 0.6, 0.4], [0.4, 2.5, 0.6], [0.5, 0.7, 3.0], [2.0, 2.0, 0.3]]
        lg.spot_pos[:], lg.spot_col[:], lg.spot_rot[:] = (0.0, 5.0, 0.5), (50.0, 25.0, 60.0), (0.0, 1.0, 0.0)
    return lg


def corner_scene(variant):
    """variant: "plain" / "stochastic" (the lights differ), "area", "mirror"."""
    r8, m8 = (255, 0) if variant == "area" else (128, 255)
    tex = [np.array([[0x00C0B0A0]], np.uint32), np.array([[(r8 << 8) | m8]], np.uint32),
           np.array([[0x004080D0]], np.uint32), np.array([[(128 << 8) | 128]], np.uint32),
           np.array([[0x00302010]], np.uint32)]
    emission = {} if variant in ("area", "mirror") else dict(emission=4)
    meshes = [Q._flat_quad(0.0, 0.0, 0.0, Q.HALF, albedo=0, metalness=1),
              _upright_quad(-Q.HALF, Q.HALF, 0.0, WALL_H, WALL_Z, albedo=2, metalness=3, **emission)]
    kinds = None
    if variant == "mirror":
        kinds = [_lib.MAT_MIRROR, _lib.MAT_MIRROR]
    else:
        meshes.append(Q._flat_quad(*BLOCKER, albedo=0, metalness=1))
    lights = Q._dark_lights() if variant in ("area", "mirror") else _lights(variant == "stochastic")
    light = None
    if variant == "area":
        light = Q.LIGHTS["big"]
    inst = [(k, np.eye(4, dtype=F)) for k in range(len(meshes))]
    return scenes.SceneData(meshes, tex, inst, lights, Q.sky_ramp(), np.array(Q.CAM_POS, F), np.array(Q.CAM_TARGET, F),
                            "corner-" + variant, materials=kinds, area_light=light)


def _rotation(axis, angle):
    """Rodrigues' rotation about `axis` by `angle`, float64 3 x 3."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


# the rigid motion G of `corner-turned` (a rotation about a generic axis, then a translation) and, per mesh, the
# rotation Q^-1 it is authored under: instance k is G Q_k, a different transform for each
TURN_G = (_rotation((1.0, 2.0, 3.0), 0.55), np.array([0.3, -0.2, 0.4]))
TURN_Q = [_rotation((2.0, -1.0, 0.5), 0.4), _rotation((-1.0, 1.0, 2.0), -0.7), _rotation((0.5, 3.0, -1.0), 1.1)]


def corner_turned_scene(variant):
    """corner_scene("plain" / "stochastic") with the whole world -- instances, camera, lights -- under the rigid motion
    TURN_G (the sky stays where it is: another scene, not the corner seen from elsewhere).  Mesh k is authored rotated
    by Q_k^-1 (vertices and normals) and instanced with G Q_k, so every instance carries a different rotation, no
    world normal is axis-aligned, and a hit at any depth needs its instance's normal matrix."""
    sd = corner_scene(variant)
    G, g = TURN_G
    meshes, inst = [], []
    for k, m in enumerate(sd.meshes):
        Qi = TURN_Q[k].T
        Pp = np.asarray(m.vertices, np.float64).reshape(2, 3, 3) @ Qi.T
        Nn = np.asarray(m.fixed_normals, np.float64).reshape(-1, 4)[:, :3].reshape(2, 3, 3) @ Qi.T
        tex = {key: getattr(m, key) for key in ("albedo", "metalness", "emission") if getattr(m, key) >= 0}
        meshes.append(SQ._mesh(Pp, Nn, np.asarray(m.fixed_uvs, np.float64).reshape(2, 3, 2), **tex))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = G @ TURN_Q[k], g
        inst.append((k, T.astype(F)))

    def move(p):
        return (np.asarray(p, np.float64) @ G.T + g).astype(F)

    lg = sd.lights
    lights = scenes.Lights(move(lg.point_pos), lg.point_col.copy(), move(lg.dir_pos), lg.dir_col.copy(),
                           move(lg.spot_pos), lg.spot_col.copy(), (np.asarray(lg.spot_rot, np.float64) @ G.T).astype(F))
    return scenes.SceneData(meshes, sd.textures, inst, lights, sd.sky, move(sd.cam_pos), move(sd.cam_target),
                            "corner-turned-" + variant)


def glass_over_floor_scene():
    tex = [np.array([[0x00C0B0A0]], np.uint32), np.array([[(128 << 8) | 128]], np.uint32),
           np.array([[0x00203040]], np.uint32)]
    meshes = [Q._flat_quad(0.0, 0.0, 0.0, Q.HALF, albedo=0, metalness=1, emission=2), Q._flat_quad(*GLASS, albedo=0)]
    inst = [(k, np.eye(4, dtype=F)) for k in range(2)]
    return scenes.SceneData(meshes, tex, inst, Q._dark_lights(), Q.sky_ramp(), np.array(GLASS_CAM[0], F),
                            np.array(GLASS_CAM[1], F), "glass-over-floor",
                            materials=[_lib.MAT_TEXTURED, _lib.MAT_DIELECTRIC])


# scene name -> (scene, class name of each rectangle or None, the bounce counts tested)
@functools.lru_cache(None)
def scene_table():
    t = {}
    for rough, metal in Q.MATERIALS:
        t[f"sky-floor-{rough}-{metal}"] = (Q.floor_scene(rough, metal, None, sky=Q.sky_ramp(),
                                                         name=f"sky-floor-{rough}-{metal}"), ["floor"], (2, 3))
    t["corner-plain"] = (corner_scene("plain"), ["floor", "wall", None], (2, 3, 4))
    t["corner-stochastic"] = (corner_scene("stochastic"), ["floor", "wall", None], (3,))
    t["corner-area"] = (corner_scene("area"), ["floor", "wall", None], (1, 3))
    t["corner-turned-plain"] = (corner_turned_scene("plain"), ["floor", "wall", None], (3,))
    t["corner-turned-stochastic"] = (corner_turned_scene("stochastic"), ["floor", "wall", None], (3,))
    t["glass-over-floor"] = (glass_over_floor_scene(), ["floor", "glass"], (3, 4))
    return t


STAT_CASES = [(name, b) for name, b in
              [(f"sky-floor-{r}-{m}", b) for r, m in Q.MATERIALS for b in (2, 3)]
              + [("corner-plain", 2), ("corner-plain", 3), ("corner-plain", 4), ("corner-stochastic", 3),
                 ("corner-area", 1), ("corner-area", 3), ("glass-over-floor", 3), ("glass-over-floor", 4),
                 ("corner-turned-plain", 3), ("corner-turned-stochastic", 3)]]


def scene_flags(name):
    """test_gpu_estimator's flags for the scene (FLAGS carries the stochastic bit), without it for corner-plain and
    corner-turned-plain."""
    f = Q.scene_flags(scene_table()[name][0]) if name in scene_table() else Q.scene_flags(corner_scene("mirror"))
    return f & ~_lib.FLAG_STOCHASTIC if name in ("corner-plain", "corner-turned-plain") else f


@functools.lru_cache(None)
def ref_scene(name):
    sd = scene_table()[name][0]
    return P.Scene(sd, stochastic=bool(scene_flags(name) & _lib.FLAG_STOCHASTIC), skybox=True)


@functools.lru_cache(None)
def chosen_pixels(name):
    """(pixel indices, class name per pixel) from the reference's geometry alone."""
    _, classes, _ = scene_table()[name]
    idx, edge = ref_scene(name).classify(W, H, MARGIN)
    cap = max(TESTED_CAP, -(-60 // sum(c is not None for c in classes)))
    px, cls = [], []
    for k, c in enumerate(classes):
        if c is None:
            continue
        mine = np.flatnonzero((idx == k) & ~edge)
        assert mine.size >= 20, (name, c, mine.size)
        if mine.size > cap:             # thin evenly over the image
            mine = mine[np.round(np.linspace(0, mine.size - 1, cap)).astype(int)]
        px.append(mine)
        cls += [c] * mine.size
    px = np.concatenate(px)
    assert px.size >= 60, (name, px.size)
    return px, np.array(cls)


class PathRef:
    """The reference of one statistical case at its tested pixels, computed once per process."""

    def __init__(self, name, bounces, slip=None):
        import time
        self.name, self.bounces = name, bounces
        self.n = N_FRAMES_OF.get((name, bounces), N_FRAMES)
        self.M = REF_FACTOR * self.n
        self.sel, self.cls = chosen_pixels(name)
        t0 = time.perf_counter()
        self.mean, self.sigma = ref_scene(name).estimate(self.sel, W, H, bounces, self.M, REF_SEED, slip=slip)
        self.seconds = time.perf_counter() - t0
        self.se = self.sigma * np.sqrt(1.0 / self.n + 1.0 / self.M)
        self.sum_bound = 6.0 * np.sqrt((self.se ** 2).sum(0))


@functools.lru_cache(None)
def path_ref(name, bounces, slip=None):
    return PathRef(name, bounces, slip)


# ------------------------------------------------------------------------------------------------ shared checks
# A `view` is test_gpu_estimator's: view.mean(bounces, n), view.frames(bounces, k) of one scene at 16 x 12.
def z_scores(ref, mean):
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.abs(mean[ref.sel] - ref.mean)
        zp = np.where(ref.se > 0, dev / np.where(ref.se > 0, ref.se, 1.0), np.where(dev > 0, np.inf, 0.0))
    zs = np.abs(mean[ref.sel].sum(0) - ref.mean.sum(0)) / (ref.sum_bound / 6.0)
    return zp, zs


def check_path(view, ref):
    mean = view.mean(ref.bounces, ref.n)
    zp, zs = z_scores(ref, mean)
    got, exp = mean[ref.sel].sum(0), ref.mean.sum(0)
    print(f"{ref.name} bounces {ref.bounces}: pixels {ref.sel.size}, sum {got.round(3)} expected {exp.round(3)}, "
          f"largest z pixel {zp.max():.2f} sum {zs.max():.2f}")
    assert ref.sel.size >= 60 and all((ref.cls == c).sum() >= 20 for c in set(ref.cls))
    assert (zs <= 6.0).all(), (ref.name, ref.bounces, "sum", got, exp, zs)
    assert (zp <= 6.0).all(), (ref.name, ref.bounces, "pixel", float(zp.max()), int((zp > 6.0).sum()))
    return float(zp.max()), float(zs.max())


def mirror_paths():
    """Per pixel of mirror-corner, from geometry alone: `twice` -- two reflections (floor and wall, either order),
    every hit further than MARGIN from an outline, and the twice-reflected ray leaves the scene; `once_more` -- the
    first reflection meets the other mirror; and the twice-reflected direction."""
    s = P.Scene(corner_scene("mirror"))
    O, D = s.primary(W, H)
    n = len(O)
    ok = np.ones(n, bool)
    hits = []
    for _ in range(2):
        t, idx = s.closest(O, D)
        edge = np.zeros(n, bool)
        for r in s.rects:
            edge |= r.hit(O, D, MARGIN)[1]
        ok &= ~edge
        hits.append(idx)
        Nn = np.stack([s.rects[max(k, 0)].N for k in idx])
        I = O + np.where(np.isfinite(t), t, 0.0)[:, None] * D
        D = D - 2.0 * E._dot(D, Nn)[:, None] * Nn
        O = I + D * P.EPS
    t, idx = s.closest(O, D)
    edge = np.zeros(n, bool)
    for r in s.rects:
        edge |= r.hit(O, D, MARGIN)[1]
    two = (hits[0] >= 0) & (hits[1] >= 0) & (hits[0] != hits[1])
    return two & ok & ~edge & (idx == -1), two & ok, D


def check_mirror_corner(view):
    """Floor and wall MIRROR under the sky ramp, every light dark.  bounces 3: a pixel whose two reflections leave the
    scene equals the sky in the twice-reflected direction; bounces 2: a pixel whose first reflection meets the other
    mirror is exactly 0 (its second hit is the path's last segment: emission and light, both 0, and no ray follows).

    Tolerance, derived as test_gpu_estimator.check_glass derives its own: off two plane mirrors the direction depends
    on the camera ray and the two normals alone; each reflection is a float32 closed form within scene_ref.CLOSED_TOL
    of the float64 one, so the direction turns by at most 2 CLOSED_TOL, which moves the lookup by at most
    2 CLOSED_TOL (w / (2 pi r) + h / pi) texels (r the direction's horizontal length), and the bilinear lookup of the
    ramp by at most that times the ramp's largest texel step; with the lookup's own relative error
        tol = CLOSED_TOL (|expected| + 2 step shift)  per channel."""
    sd = view.sd
    twice, once_more, D2 = mirror_paths()
    assert twice.sum() >= 20 and once_more.sum() >= 20, (twice.sum(), once_more.sum())
    Dn = R.ray_ctor_dir(D2.astype(F))
    exp = R.sample_sky(sd.sky, Dn).astype(np.float64)
    r = np.sqrt(Dn[:, 0].astype(np.float64) ** 2 + Dn[:, 2].astype(np.float64) ** 2)
    h, w = sd.sky.shape[:2]
    shift = w / (2 * np.pi * np.maximum(r, 1e-300)) + h / np.pi
    sky = sd.sky.astype(np.float64)
    step = max(np.abs(np.diff(sky, axis=0)).max(), np.abs(np.diff(sky, axis=1)).max())
    tol = R.CLOSED_TOL * (np.abs(exp) + 2.0 * step * shift[:, None])
    assert (R.sky_taps(Dn, w, h)[2][twice] < w - 1).all() and (r[twice] > 0.1).all()     # no tap at the ramp's seam
    got = view.frames(3, 1)[0].astype(np.float64)
    err = np.abs(got - exp)
    worst = float((err[twice] / tol[twice]).max())
    assert (err[twice] <= tol[twice]).all(), (worst, got[twice][:3], exp[twice][:3])
    assert (exp[twice].min(0) > 0.1).all()
    capped = view.frames(2, 1)[0]
    assert Q._same(capped[once_more], 0.0), capped[once_more]
    return worst


def exact_scenes():
    """(name, scene, flags, bounce counts) of every scene of this file, for the device = oracle comparison."""
    out = [(name, sd, scene_flags(name), bs) for name, (sd, _, bs) in scene_table().items()]
    out.append(("mirror-corner", corner_scene("mirror"), scene_flags("mirror-corner"), (2, 3)))
    return out


# ------------------------------------------------------------------------------------------------ the device
pytestmark = pytest.mark.gpu


class GpuView(Q.GpuView):
    """test_gpu_estimator's view of the shared context, rendering with the case's own flags."""

    def __init__(self, ctx, sd, flags):
        super().__init__(ctx, sd)
        self.flags = flags

    def frames(self, bounces, k, frame_index=0):
        ctx = self.load()
        ctx.reset_accumulation(full=True)
        avg, rgb8, st = ctx.render(W, H, k, bounces, self.flags, 0, frame_index, Q.SEED)
        self.pipeline = int(st.pipeline)
        return avg[:, :3].copy(), rgb8.copy(), int(st.segments), int(st.shadow_rays)


@pytest.fixture(autouse=True)
def _forget_view():
    yield
    Q.GpuView._loaded = None


@pytest.mark.parametrize("name,bounces", STAT_CASES)
def test_path_expectation(gpu_ctx, name, bounces):
    check_path(GpuView(gpu_ctx, scene_table()[name][0], scene_flags(name)), path_ref(name, bounces))


def test_mirror_corner(gpu_ctx):
    print("largest error / tolerance:", check_mirror_corner(GpuView(gpu_ctx, corner_scene("mirror"),
                                                                    scene_flags("mirror-corner"))))


def test_device_equals_oracle(gpu_ctx, oracle_mod):
    """Every scene of this file at every tested bounce count, 2 frames: image, RGB8 and ray counts bit for bit; the
    scenes without an area light or a dielectric (mirror-corner among them) run the deferred-resolve chain
    (prt_stats.pipeline 3), the area-light and glass scenes the per-iteration one with the extension kernels (2)."""
    for name, sd, flags, bs in exact_scenes():
        extensions = sd.area_light is not None or _lib.MAT_DIELECTRIC in (sd.materials or [])
        view = GpuView(gpu_ctx, sd, flags)
        osc = oracle_mod.OracleScene(sd, W, H)
        for bounces in bs:
            a_o, r_o, _, s_o = osc.render(W, H, spp=2, bounces=bounces, flags=flags, seed=Q.SEED)
            a_g, r_g, seg, sh = view.frames(bounces, 2)
            assert np.array_equal(SQ.bits(a_o[:, :3]), SQ.bits(a_g)), (name, bounces)
            assert np.array_equal(r_o, r_g), (name, bounces)
            assert (int(s_o.segments), int(s_o.shadow_rays)) == (seg, sh), (name, bounces)
            assert view.pipeline == (2 if extensions else 3), (name, bounces, view.pipeline)
