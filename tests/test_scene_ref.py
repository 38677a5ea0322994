"""tests/scene_ref.py proven on the CPU: hand-computed known answers that need no scene, then the checks of
tests/test_gpu_scene_queries.py run against the oracle (oracle/prt_oracle.c) on that module's scenes -- the exact
tier bit for bit, the closed-form tier within scene_ref.CLOSED_TOL.

A disagreement is either a slip in scene_ref or a slip that the oracle shares with the device code; the reference
lines cited in scene_ref decide which.  What was found:
  - no shared slip: the oracle (and the device) agree with scene_ref on both tiers; the one disagreement on the way
    was scene_ref's own known answer for the camera's up vector, whose z is -0 (cross(right, ahead), Camera.cpp:32);
  - prt_set_meshes refused `attr`'s 4x8 metalness map under an 8x4 albedo for being narrower than the albedo, though
    the reference reads every map at a flat index below the albedo's texel count (Scene.cpp:160-186) and renders it;
    the texel-count condition alone keeps that index inside the map, and is what the library now asks for.

Each of these changes to the restatement fails the named tests here (tried on copies of prt_oracle.c):
  a map indexed with its own dimensions   material_and_normals_exact, normals_general_transform
  u = x / W                               primary_rays (all three), sky
  the smooth normal normalised            material_and_normals_exact, normals_general_transform
  T and B swapped                         material_and_normals_exact, normals_general_transform
  point-light tmax = d - EPSILON          point_shadow_range (both)
  point-light falloff 1 / d^2             point_shadow_range (both), stochastic_light_classes
  spot class divided by 0.5               stochastic_light_classes
`factor > 0.9f` in place of `(double)factor > 0.9` fails nothing because it changes nothing: 0.9f = 0.89999998 lies
below 0.9 and the next float, 0.90000004, above it, so no float separates the two comparisons."""
import types

import numpy as np
import pytest

import scene_ref as R
import test_gpu_scene_queries as Q

F = np.float32


def f(x):
    return F(x)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(Q.bits(a), Q.bits(b))
    return np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ known answers
def _sky_vectors():
    """The lookup's addressing at the seam and at the pole, on a 37 x 19 sky whose texel (row, col) holds
    (col, row, 100 col + row): a value read anywhere names the tap it came from."""
    W, H = 37, 19
    rows, cols = np.mgrid[0:H, 0:W]
    sky = np.stack([cols, rows, 100 * cols + rows], -1).astype(F)
    out = []
    # D = (-1, 0, +0): atan2(+0, -1) = +pi, u = 0.5 + pi / (2 pi) = 1, uTex = 37, u0 = 37 % 37 = 0, u1 = 1, and
    # du = uTex - u0 = 37: computed from the WRAPPED u0, the lookup extrapolates 37 texels to the right.
    # v = acos(0) / pi: float(pi / 2) / float(pi) = 0.5 exactly (the float nearest pi / 2 is half the one nearest pi),
    # vTex = 9.5, v0 = 9, v1 = 10, dv = 0.5.  Row 9.5 of channel 0 (col): 0 + 37 * (1 - 0) = 37; channel 1 (row): 9.5
    t = R.sky_taps(np.array([-1.0, 0.0, 0.0], F), W, H)
    out += [(t[0], f(1.0)), (t[2], 0), (t[4], 1), (t[6], f(37.0)), (t[1], f(0.5)), (t[3], 9), (t[5], 10), (t[7], f(0.5))]
    c = R.sample_sky(sky, np.array([-1.0, 0.0, 0.0], F))
    out += [(c[0], f(37.0)), (c[1], f(9.5)), (c[2], f(3709.5))]
    # D = (-1, 0, -0): atan2(-0, -1) = -pi, u = 0, u0 = 0, u1 = 1, du = 0: texel column 0 itself
    t = R.sky_taps(np.array([-1.0, 0.0, -0.0], F), W, H)
    out += [(t[0], f(0.0)), (t[2], 0), (t[4], 1), (t[6], f(0.0))]
    c = R.sample_sky(sky, np.array([-1.0, 0.0, -0.0], F))
    out += [(c[0], f(0.0)), (c[1], f(9.5)), (c[2], f(9.5))]
    # just before the seam u1 wraps: z slightly positive, x = -1: u a little under 1, u0 = 36, u1 = (36 + 1) % 37 = 0
    t = R.sky_taps(np.array([-1.0, 0.0, 0.001], F), W, H)
    out += [(t[2], 36), (t[4], 0)]
    # D = (0, 1, 0): v = acos(1) / pi = 0, v0 = 0, v1 = 1, dv = 0; atan2(0, 0) = 0, u = 0.5, uTex = 18.5, u0 = 18,
    # du = 0.5: row 0 between columns 18 and 19
    t = R.sky_taps(np.array([0.0, 1.0, 0.0], F), W, H)
    out += [(t[1], f(0.0)), (t[3], 0), (t[5], 1), (t[7], f(0.0)), (t[0], f(0.5)), (t[2], 18), (t[4], 19), (t[6], f(0.5))]
    c = R.sample_sky(sky, np.array([0.0, 1.0, 0.0], F))
    out += [(c[0], f(18.5)), (c[1], f(0.0)), (c[2], f(1850.0))]
    return out


def _texel_vectors():
    out = []
    s = f(1) / f(255)
    # srgb_to_linear: the linear branch up to and including 0.04045f, the power branch from the next float on
    lo = f(0.04045)
    nxt = np.nextafter(lo, f(1))
    out += [(R.srgb_to_linear(f(0.0)), f(0.0)), (R.srgb_to_linear(lo), lo / f(12.92)), (R.srgb_to_linear(f(1.0)), f(1.0)),
            (R.srgb_to_linear(nxt), f(float((nxt + f(0.055)) / f(1.055)) ** float(f(2.4))))]
    # the branches meet without a jump: within 1e-7 of each other at the threshold
    out += [(abs(float(R.srgb_to_linear(nxt)) - float(R.srgb_to_linear(lo))) < 1e-7, True)]
    # 0x8080FF: 128 * (2 / 255) - 1 twice, 255 * (2 / 255) - 1
    n = R.normal_from_texel(np.uint32(0x8080FF))
    two = f(2) / f(255)
    out += [(n[0], f(128) * two - f(1)), (n[1], f(128) * two - f(1)), (n[2], f(255) * two - f(1)),
            (abs(float(n[0]) - 1 / 255) < 1e-7, True), (abs(float(n[2]) - 1.0) < 1e-7, True)]
    c = R.color_from_texel(np.uint32(0xFF8000))
    out += [(c[0], f(255) * s), (c[1], f(128) * s), (c[2], f(0.0))]
    out += [(R.extract_channel(R.GREEN, np.uint32(0x12345678)), f(0x56) * s),
            (R.extract_channel(R.BLUE, np.uint32(0x12345678)), f(0x78) * s),
            (R.extract_channel(R.RED, np.uint32(0x12345678)), f(0x34) * s),
            (R.extract_channel(R.ALPHA, np.uint32(0x12345678)), f(0x12) * s)]
    # texel index with an 8 x 4 albedo: uv = 1 exactly wraps to texel 0; uv in [1, 2) wraps once
    out += [(R.texel_index(np.array([1.0, 1.0], F), 8, 4), 0),
            (R.texel_index(np.array([0.0, 0.0], F), 8, 4), 0),
            (R.texel_index(np.array([0.999, 0.999], F), 8, 4), 7 + 3 * 8),
            (R.texel_index(np.array([1.5, 0.3], F), 8, 4), 4 + 1 * 8),          # (int)12 % 8 = 4, (int)1.2 = 1
            (R.texel_index(np.array([0.3, 1.75], F), 8, 4), 2 + 3 * 8),         # (int)2.4 = 2, (int)7 % 4 = 3
            (R.texel_index(np.array([1.99, 1.99], F), 8, 4), 7 + 3 * 8)]
    return out


def _camera_vectors():
    """A camera at the origin looking down +z with aspect 2: ahead = (0,0,1), right = cross(ahead, up) = (-1,0,0),
    up = (0,1,0); the screen plane is z = 2, x from +2 (left) to -2, y from +1 (top) to -1.  W = 97, H = 61."""
    W, H = 97, 61
    cam = R.camera([0, 0, 0], [0, 0, 5], 2.0)
    out = [(cam["ahead"], np.array([0, 0, 1], F)), (cam["right"], np.array([-1, 0, 0], F)),
           (cam["up"], np.array([0, 1, -0.0], F)),       # z = right.x * ahead.y - right.y * ahead.x = -0 - 0
           (cam["tl"], np.array([2, 1, 2], F)),
           (cam["tr"], np.array([-2, 1, 2], F)), (cam["bl"], np.array([2, -1, 2], F))]
    # pixel (0, 0): P = topLeft = (2, 1, 2), |P| = 3 exactly: the direction is P * (1 / 3)
    d = R.primary_rays(cam, W, H, np.array([0.0], F), np.array([0.0], F))[0]
    third = f(1) / f(3)
    out += [(d, np.array([f(2) * third, third, f(2) * third], F))]
    # pixel (96, 60): u = 96 * (1 / 97) in float32 -- NOT 96 / 97 -- and v = 60 * (1 / 61)
    u, v = f(96) * (f(1) / f(97)), f(60) * (f(1) / f(61))
    P = np.array([f(2) + u * f(-4), f(1) + v * f(-2), f(2)], F)
    inv = f(1) / np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
    d = R.primary_rays(cam, W, H, np.array([96.0], F), np.array([60.0], F))[0]
    out += [(d, P * inv), (bool(u != f(96) / f(97) or v != f(60) / f(61)), True)]
    # the constructor's second normalisation: a unit axis stays, a zero vector stays zero, (3, 0, 4) becomes / 5
    out += [(R.ray_ctor_dir(np.array([0, 0, 1], F)), np.array([0, 0, 1], F)),
            (R.ray_ctor_dir(np.array([0, 0, 0], F)), np.array([0, 0, 0], F)),
            (R.ray_ctor_dir(np.array([3, 0, 4], F)), np.array([3, 0, 4], F) * (f(1) / f(5)))]
    return out


def vectors():
    return _sky_vectors() + _texel_vectors() + _camera_vectors()


def test_vector_count():
    assert len(vectors()) >= 40


def test_known_answers():
    bad = [(i, got, exp) for i, (got, exp) in enumerate(vectors()) if not same(got, exp)]
    assert not bad, bad


def test_x_over_w_differs_from_x_times_reciprocal():
    """At W = 97 the two ways of computing u differ for some pixel, so the 97-wide images can tell them apart."""
    xs = np.arange(97, dtype=F)
    assert (xs * (f(1) / f(97)) != xs / f(97)).any()


def test_normal_matrix():
    assert np.array_equal(R.normal_matrix(np.eye(4)), np.eye(4))
    T = np.eye(4, dtype=F)
    T[:3, 3] = (2.5, 0.3, 0.5)
    assert np.array_equal(R.normal_matrix(T)[:3, :3], np.eye(3))
    S = np.diag([2.0, 0.5, 4.0, 1.0])
    assert np.allclose(R.normal_matrix(S), np.diag([0.5, 2.0, 0.25, 1.0]), rtol=1e-15)


def test_direct_light_by_hand():
    """One white Lambert-like point on the floor under a single point light straight above at height 2: d = 2,
    cos = 1, falloff 1 / d = 0.5, so the point class gives brdf * colour * 0.5 / 0.3, whichever light is picked for
    the BRDF's direction when all four sit in the same place."""
    from test_brdf_vectors import eval_brdf
    lights = types.SimpleNamespace(point_pos=np.tile([0.0, 2.0, 0.0], (4, 1)), point_col=np.array([[1.0, 2.0, 3.0]] + [[0, 0, 0]] * 3),
                                   dir_pos=np.array([0.0, 4.0, 0.0]), dir_col=np.array([1.0, 1.0, 1.0]),
                                   spot_pos=np.array([0.0, 3.0, 0.0]), spot_col=np.array([9.0, 9.0, 9.0]),
                                   spot_rot=np.array([0.0, 1.0, 0.0]))
    I, N, V = np.zeros((1, 3)), np.array([[0.0, 1.0, 0.0]]), np.array([[0.0, 0.6, 0.8]])
    mat = dict(base=np.array([[0.5, 0.5, 0.5]]), metalness=np.array([0.0]), roughness=np.array([1.0]),
               emissive=np.array([[0.1, 0.0, 0.0]]))
    b = np.array(eval_brdf(N[0], [0.0, 1.0, 0.0], V[0], (0.5, 0.5, 0.5), 0.0, 1.0))
    vis = np.ones((1, 6), bool)
    out = R.direct_light(I, N, V, mat, lights, vis)
    p3 = float(F(0.3))
    for k in range(4):
        assert np.allclose(out["point"][k][0], [0.1, 0, 0] + b * np.array([1.0, 2.0, 3.0]) * 0.5 / p3, rtol=1e-12)
    assert np.allclose(out["plain"][0], [0.1, 0, 0] + b, rtol=1e-12)
    assert np.allclose(out["dir"][0], [0.1, 0, 0] + b / 0.5, rtol=1e-12)
    assert np.allclose(out["spot"][0], [0.1, 0, 0] + b * 9.0 / 9.0 / float(F(0.2)), rtol=1e-12)   # 1 / d^2 = 1 / 9
    vis[0, 5] = False
    assert np.allclose(R.direct_light(I, N, V, mat, lights, vis)["spot"][0], [0.1, 0, 0])
    # visibility: a triangle 1 above the point hides every light; the point lights' range is d^2 - eps = 3.99
    tri = np.array([[[-1.0, 1.0, -1.0], [3.0, 1.0, -1.0], [-1.0, 1.0, 3.0]]])
    assert not R.visibility(I, lights, tri).any()
    tri[:, :, 1] = 3.5   # above every light but the directional: physically nothing but that one is hidden ...
    assert R.visibility(I, lights, tri, physical=True).tolist() == [[True] * 4 + [False, True]]
    assert R.visibility(I, lights, tri).tolist() == [[False] * 4 + [False, True]]   # ... the point lights' rays reach it


# ------------------------------------------------------------------------------------------------ the oracle
class OracleView:
    def __init__(self, oracle_mod, sd, W, H):
        self.o, self.sd, self.W, self.H = oracle_mod, sd, W, H
        self.osc = oracle_mod.OracleScene(sd, W, H)
        self._hits = None

    def hits(self):
        if self._hits is None:
            self._hits = dict(zip(("t", "u", "v", "prim", "inst"), self.osc.primary_hits(self.W, self.H)))
        return self._hits

    def render(self, flags, mode):
        return self.osc.render(self.W, self.H, spp=1, bounces=1, flags=flags, mode=mode)[0][:, :3].copy()


@pytest.mark.parametrize("preset", [None, 0, 1])
def test_oracle_primary_rays(oracle_mod, preset):
    sd, W, H = Q.attr_scene(), 97, 61
    view = OracleView(oracle_mod, sd, W, H)
    if preset is not None:
        view.osc.set_postfx(True, fov=Q.PANINI[preset].fov, distortion=Q.PANINI[preset].distortion)
    O, D = Q.camera_rays(sd, W, H, Q.PANINI[preset] if preset is not None else None)
    got = dict(zip(("t", "u", "v", "prim", "inst"), view.osc.intersect(O, D)))
    Q.check_primary(view.hits(), got)


def test_oracle_sky(oracle_mod):
    cols = []
    for camera in ("seam", "up"):
        sd = Q.sky_scene(camera)
        cols.append(Q.check_sky(OracleView(oracle_mod, sd, 61, 47), sd, 61, 47))
    assert (cols[0][0] == 36).any() and (cols[0][0] == 0).any()
    assert (cols[1][1] <= 1).any()


@pytest.fixture(scope="module")
def attr_view(oracle_mod):
    return OracleView(oracle_mod, Q.attr_scene(), 128, 96)


def test_oracle_material_and_normals_exact(attr_view):
    Q.assert_attr_coverage(Q.check_attributes(attr_view, attr_view.sd, (0, 1), True))


def test_oracle_normals_general_transform(attr_view):
    Q.check_attributes(attr_view, attr_view.sd, (2,), False)


@pytest.fixture(scope="module")
def lit_classes(oracle_mod):
    sd = Q.lit_scene("classes")
    view = OracleView(oracle_mod, sd, Q.LIT_W, Q.LIT_H)
    return view, Q.LightRef(sd, Q.LIT_W, Q.LIT_H, view.hits())


def test_reference_alone(lit_classes):
    """What the closed form asserts about itself: the exclusion cap and the candidates' distance."""
    _, ref = lit_classes
    Q.check_exclusion_cap(ref)
    Q.check_candidates_distinct(ref)


def test_oracle_plain_directional_light(lit_classes):
    Q.check_plain_light(*lit_classes)


def test_oracle_stochastic_light_classes(lit_classes):
    Q.check_light_classes(*lit_classes)


@pytest.mark.parametrize("variant,light,lit", [("above", 0, False), ("below", 1, True)])
def test_oracle_point_shadow_range(oracle_mod, variant, light, lit):
    sd = Q.lit_scene(variant)
    view = OracleView(oracle_mod, sd, Q.LIT_W, Q.LIT_H)
    ref = Q.LightRef(sd, Q.LIT_W, Q.LIT_H, view.hits())
    Q.check_exclusion_cap(ref)
    Q.check_shadow_range(view, ref, light, lit)
