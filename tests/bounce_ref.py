"""Independent float64 reference for what a path does at its SECOND hit when the first one is a mirror or a glass
pane over textured, normal-mapped, transformed instances, and for the depth cap of a path between two facing mirrors.
TEST INFRASTRUCTURE ONLY.

Composed from tests/scene_ref.py (camera rays, material, shading_normal, normal_matrix, visibility, direct_light),
tests/estimator_ref.py (glass, glass_combine) and tests/path_ref.py (the rectangles of the hall); this module imports
neither `oracle` nor `prt`, and finds every hit by a float64 Moeller-Trumbore brute force over the world-space
triangles, which shares nothing with the traversal of either restatement.  Scenes are scenes.SceneData-shaped objects.

Part 1, `Bounce`: bounces = 2, no AA, no sky, the stochastic flag cleared, so a pixel is deterministic:
  1. the camera ray is scene_ref's; its first hit is the brute force's;
  2. a MIRROR first hit (metalness 1, roughness 0, emission never set: Core/Scene.cpp:199-204) gathers its own
     direct_light term and sends D' = D - 2 (D.N) N from I + D' EPSILON with weight (1, 1, 1)
     (Core/Renderer.cpp:376,396-404); a DIELECTRIC first hit drops what it gathered and blends its two children,
     estimator_ref.glass / glass_combine (Core/Renderer.cpp:331-372);
  3. a child's hit (instance, primitive, u, v, t) is the brute force's again, and being the path's last segment it
     returns emission + the plain directional term (Core/Renderer.cpp:196,312-329) evaluated with the material and
     the shading normal of THAT instance (float64 normal matrix), the hit point I2, V2 = -D' and the visibility over
     every world triangle, the mirror or the pane included; a child that leaves the scene returns 0.

Tolerance (no free factor).  An implementation forms the child's direction, the hit point and the shading normal in
float32; each errs by at most scene_ref.CLOSED_TOL relative to its own scale (1 for the direction; the diagonal of
the scene's bounding box for the hit point, which is origin + t * direction with t up to that diagonal; the normal's
own length -- the non-exact tier of tests/test_gpu_scene_queries.py).  The closed form evaluated on exact inputs errs
by CLOSED_TOL |expected|.  To first order the inputs' errors add up to sum_inputs sum_axes |d expected / d input_axis|
* CLOSED_TOL * scale, which is taken by finite differences: the last segment re-evaluated with that input displaced
by CLOSED_TOL of its scale along each axis in turn, everything discrete (primitive, texel, visibility) held fixed:
    tol = CLOSED_TOL |expected| + sum_children weight * sum_{input, axis} |value(displaced) - value|
(the mirror's own term joins the sum with its hit point and its normal displaced; its V is the camera ray's).
A pixel whose tol exceeds 0.1 |expected| in some channel sits on a specular peak and is not tested; nor is a lit hit
on the flat top of a narrow lobe, where a first-order difference sees nothing and float32 cancellation alone passes
CLOSED_TOL (B_MIN below).

Not tested either, all decided here: a first or a child's hit within EDGE (barycentric) of a triangle's edge, or whose
ray meets another triangle first once every triangle is grown by EDGE (an outline in front); a child's miss that
turns into a hit under that growth; a child's hit whose UV lies within TEXEL_EDGE of a texel boundary of the albedo's
grid; a lit hit one of whose shadow rays, or whose spot test, changes its outcome among eight points MARGIN around it
in its triangle's plane (test_gpu_scene_queries.LightRef's octagon); glass pixels with |k_refract| < K_MARGIN.

Part 2, `Hall`: two facing delta mirrors; the number k of mirror hits before the ray leaves decides, with `bounces`,
whether the sky arrives (k + 1 <= bounces) and how many floor emissions are gathered (those among the first
min(k, bounces) hits), folded bottom-up in float32 as result + Trace(..) * (1, 1, 1) unwinds.

`slip=` plants one named defect (SLIPS, HALL_SLIPS) to show that a comparison against this reference can see it.
"""
import numpy as np

import estimator_ref as E
import path_ref as P
import scene_ref as R

F = np.float32
EPS = float(R.EPSILON)
TOL = R.CLOSED_TOL
EDGE = 0.02          # barycentric
TEXEL_EDGE = 1e-3    # in UV
MARGIN = 1e-3        # scene units, test_gpu_scene_queries.MARGIN
K_MARGIN = 1e-3      # test_gpu_estimator.K_MARGIN
PEAK = 0.1           # tol > PEAK |expected|: a specular peak
# The GGX denominator b = (a2 - 1) nh^2 + 1 (Core/BRDF.cpp:218-222) is formed in float32 from terms of magnitude 1 in
# three roundings, so it carries an absolute error of up to 3 * 2^-24 and D = a2 / (pi b^2) a relative one of
# 2 * 3 * 2^-24 / b, which passes CLOSED_TOL where b < B_MIN: the flat top of a narrow lobe (b = a2 >= 1e-5 where
# nh = 1, which a non-unit shading normal's clamp reaches over whole regions).  A first-order difference is blind
# there -- the top is flat -- so lit hits with b < B_MIN are the specular peak's pixels too, and are not tested.
B_MIN = 6 * 2.0 ** -24 / TOL
MAT_TEXTURED, MAT_DIELECTRIC, MAT_MIRROR = 0, 1, 2      # include/prt.h PRT_MAT_*

SLIPS = ("normalmap_only_at_first_hit", "identity_normal_matrix_at_depth_1", "first_hit_instance_at_depth_1",
         "uv_swapped", "texel_at_own_map_dims", "v_is_camera_ray", "smooth_normal_normalised",
         "shadow_from_first_hit_point", "glass_children_swapped")
HALL_SLIPS = ("cap_one_early", "cap_one_late")


# ------------------------------------------------------------------------------------------------ geometry
def world_triangles(sd):
    """(triangles (k,3,3) float64 in world space, first triangle of each instance (+ the total))."""
    out = []
    for mi, T in sd.instances:
        Pp = np.asarray(sd.meshes[mi].triangles, np.float64).reshape(-1, 4)[:, :3]
        T = np.asarray(T, np.float64)
        out.append((Pp @ T[:3, :3].T + T[:3, 3]).reshape(-1, 3, 3))
    return np.concatenate(out), np.cumsum([0] + [len(o) for o in out])


def closest(O, D, tris, grow=0.0):
    """float64 Moeller-Trumbore of rays (n,3) against triangles (k,3,3): (triangle or -1, t, u, v) of the nearest hit
    with t > 0; u runs along v1 - v0 and v along v2 - v0 (the convention of scene_ref.hit_uv).  grow: the barycentric
    amount by which every triangle is enlarged."""
    O_, D_ = O[:, None, :], D[:, None, :]
    v0, e1, e2 = tris[None, :, 0], (tris[:, 1] - tris[:, 0])[None], (tris[:, 2] - tris[:, 0])[None]
    p = np.cross(D_, e2)
    det = np.sum(e1 * p, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = O_ - v0
        u = np.sum(s * p, -1) * inv
        q = np.cross(s, e1)
        v = np.sum(D_ * q, -1) * inv
        t = np.sum(e2 * q, -1) * inv
        ok = (np.abs(det) > 1e-300) & (u >= -grow) & (v >= -grow) & (u + v <= 1 + grow) & (t > 0)
    t = np.where(ok, t, np.inf)
    k = t.argmin(1)
    rows = np.arange(len(O))
    hit = np.isfinite(t[rows, k])
    return np.where(hit, k, -1), t[rows, k], np.where(hit, u[rows, k], 0.0), np.where(hit, v[rows, k], 0.0)


def _outcomes(I, lights, tris):
    """Every discrete decision of the light block at the points I (test_gpu_scene_queries._outcomes)."""
    return np.concatenate([R.shadow_hits(I, lights, tris).reshape(I.shape[0], -1),
                           (R.spot_factor(I, lights) > 0.9)[:, None]], 1)


def _outline_near(I, tri, lights, tris):
    """bool: a discrete outcome of the light block changes among eight points 1.1 MARGIN around I in its triangle's
    plane (a straight boundary closer than MARGIN crosses that octagon)."""
    e1 = tri[:, 1] - tri[:, 0]
    e1 = e1 / np.linalg.norm(e1, axis=-1, keepdims=True)
    nrm = np.cross(e1, tri[:, 2] - tri[:, 0])
    e2 = np.cross(nrm / np.linalg.norm(nrm, axis=-1, keepdims=True), e1)
    centre = _outcomes(I, lights, tris)
    near = np.zeros(len(I), bool)
    for a in np.arange(8) * (np.pi / 4):
        probe = I + 1.1 * MARGIN * (np.cos(a) * e1 + np.sin(a) * e2)
        near |= (_outcomes(probe, lights, tris) != centre).any(-1)
    return near


def _pixels(textures, index):
    return np.asarray(textures[index], np.uint32).reshape(-1)


def _material_own_dims(mesh, textures, prim, u, v):
    """The slip texel_at_own_map_dims: scene_ref.material with every map addressed by its OWN width and height."""
    uv = R.hit_uv(mesh, prim, u, v)

    def px(t):
        return R.texel_index(uv, np.asarray(textures[t]).shape[1], np.asarray(textures[t]).shape[0])

    n = uv.shape[0]
    base = R.srgb_to_linear(R.color_from_texel(_pixels(textures, mesh.albedo)[px(mesh.albedo)]))
    metal, rough, emis = np.zeros(n, F), np.zeros(n, F), np.zeros((n, 3), F)
    if mesh.metalness >= 0:
        c = _pixels(textures, mesh.metalness)[px(mesh.metalness)]
        rough, metal = R.extract_channel(R.GREEN, c), R.extract_channel(R.BLUE, c)
    if mesh.emission >= 0:
        emis = R.color_from_texel(_pixels(textures, mesh.emission)[px(mesh.emission)])
    return dict(base=base, metalness=metal, roughness=rough, emissive=emis, texel=px(mesh.albedo))


# ------------------------------------------------------------------------------------------------ part 1
class Bounce:
    """The reference of one scene under one setting at every pixel (n = W * H):
      first      bool: the camera ray meets the specular instance (the only MIRROR or DIELECTRIC one) first
      expected   (n,3) float64;  tol (n,3);  tested (n,) bool
      exact      the scene is the mirror with every light dark: expected is the child's emission texel, to the bit
      reach      (n,) the instance the main child (the mirror's ray, the pane's refracted ray) meets, -1 none
      lit, shadowed   (n,) bool: the main child's hit sees the directional light in front of its normal / is occluded
      cover      counts over the tested main-child hits: mapped, smooth, uv_ge_1, own_dims_differ, scaled
      excluded   name -> (n,) bool, why a pixel with `first` is not tested
    normalmap: the NORMALMAP flag; lit: the LIGHTED block is evaluated (else every light is taken as dark)."""

    def __init__(self, sd, W, H, normalmap, lit, slip=None, with_tol=True):
        assert slip is None or slip in SLIPS
        self.sd, self.W, self.H, self.normalmap, self.is_lit, self.slip = sd, W, H, normalmap, lit, slip
        kinds = list(sd.materials)
        spec = [k for k, m in enumerate(kinds) if m != MAT_TEXTURED]
        assert len(spec) == 1
        self.spec, self.kind = spec[0], kinds[spec[0]]
        self.tris, self.first_tri = world_triangles(sd)
        self.inst_of_tri = np.repeat(np.arange(len(sd.instances)), np.diff(self.first_tri))
        box = self.tris.reshape(-1, 3)
        self.extent = float(np.linalg.norm(box.max(0) - box.min(0)))
        n = W * H
        cam = R.camera(sd.cam_pos, sd.cam_target, F(W) / F(H))
        ys, xs = np.mgrid[0:H, 0:W]
        D = R.ray_ctor_dir(R.primary_rays(cam, W, H, xs.reshape(-1), ys.reshape(-1))).astype(np.float64)
        O = np.repeat(cam["pos"].astype(np.float64)[None], n, 0)
        k1, t1, u1, v1 = closest(O, D, self.tris)
        kg = closest(O, D, self.tris, EDGE)[0]
        first = (k1 >= 0) & (self.inst_of_tri[np.maximum(k1, 0)] == self.spec)
        self.first = first
        sel = np.flatnonzero(first)
        self.sel = sel
        D, k1, t1, u1, v1 = D[sel], k1[sel], t1[sel], u1[sel], v1[sel]
        I1 = O[sel] + t1[:, None] * D
        prim1 = k1 - self.first_tri[self.spec]
        mesh1 = sd.meshes[sd.instances[self.spec][0]]
        nm1 = R.normal_matrix(sd.instances[self.spec][1])
        N1 = np.asarray(R.shading_normal(mesh1, sd.textures, nm1, prim1, u1.astype(F), v1.astype(F), normalmap),
                        np.float64)
        excl = dict(first_edge=(np.minimum(np.minimum(u1, v1), 1 - u1 - v1) <= EDGE) | (kg[sel] != k1))
        m = sel.size
        own, own_delta = np.zeros((m, 3)), np.zeros((m, 3))
        if self.kind == MAT_MIRROR:
            if lit:
                mat1 = dict(R.material(mesh1, sd.textures, prim1, u1.astype(F), v1.astype(F)))
                mat1.update(metalness=np.ones(m, F), roughness=np.zeros(m, F), emissive=np.zeros((m, 3), F))
                own, own_delta, flat = self._light(I1, N1, -D, mat1, R.visibility(I1, sd.lights, self.tris),
                                                   "IN" if with_tol and slip is None else "")
                excl["first_outline"] = _outline_near(I1, self.tris[k1], sd.lights, self.tris)
                excl["first_flat_top"] = flat
            D2 = D - 2.0 * E._dot(D, N1)[:, None] * N1
            children = [(I1 + D2 * EPS, P._unit0(D2), np.ones(m))]
            main = 0
        else:
            g = E.glass(D, N1)
            w_refl, w_refr = g["fres"], np.where(g["traced"], 1.0 - g["fres"], 0.0)
            children = [(I1 + N1 * EPS, P._unit0(g["R"]), w_refl), (I1 - N1 * EPS, P._unit0(g["T"]), w_refr)]
            if slip == "glass_children_swapped":
                children = [(children[0][0], children[0][1], w_refr), (children[1][0], children[1][1], w_refl)]
            excl["k_refract"] = np.abs(g["k_refract"]) < K_MARGIN
            main = 1
        expected, spread = own.copy(), own_delta
        for c, (Oc, Dc, wc) in enumerate(children):
            seg = self._segment(Oc, Dc, D, I1, with_tol)
            expected += wc[:, None] * seg["value"]
            spread += wc[:, None] * seg["delta"]
            for name, flag in seg["excluded"].items():
                excl[name] = excl.get(name, np.zeros(m, bool)) | flag
            if c == main:
                main_seg = seg
        tol = TOL * np.abs(expected) + spread
        excl["peak"] = (tol > PEAK * np.abs(expected)).any(-1)
        ok = ~np.any(list(excl.values()), 0)

        def full(a, fill):
            out = np.full((n,) + a.shape[1:], fill, a.dtype)
            out[sel] = a
            return out

        self.expected, self.tol, self.tested = full(expected, 0.0), full(tol, 0.0), full(ok, False)
        self.excluded = {k: full(v, False) for k, v in excl.items()}
        self.exact = self.kind == MAT_MIRROR and not lit
        self.reach = full(main_seg["inst"], -1)
        self.lit, self.shadowed = full(main_seg["lit"], False), full(main_seg["shadowed"], False)
        self.cover = {k: int((v & ok).sum()) for k, v in main_seg["cover"].items()}

    def _light(self, I, N, V, mat, vis, displace):
        """(emission + the plain directional term, the summed finite differences over the inputs named in `displace`
        -- I the hit point, N the shading normal, V the direction --, whether a lit hit lies on a lobe's flat top)."""
        lights = self.sd.lights

        def plain(I, N, V):
            return R.direct_light(I, N, V, mat, lights, vis)["plain"]

        value, delta = plain(I, N, V), np.zeros((len(I), 3))
        length = np.linalg.norm(N, axis=-1, keepdims=True)
        for ax in range(3):
            e = np.zeros(3)
            e[ax] = 1.0
            if "I" in displace:
                delta += np.abs(plain(I + TOL * self.extent * e, N, V) - value)
            if "N" in displace:
                delta += np.abs(plain(I, N + TOL * length * e, V) - value)
            if "V" in displace:
                delta += np.abs(plain(I, N, V + TOL * e) - value)
        L = R._unit(np.asarray(lights.dir_pos, np.float64) - I)[0]
        nh = np.clip(E._dot(N, E._unit(L + V)), 0.0, 1.0)
        a2 = np.maximum(1e-5, np.asarray(mat["roughness"], np.float64) ** 4)
        flat = vis[:, 4] & (E._dot(N, L) > 0) & (E._dot(N, V) > 0) & ((a2 - 1.0) * nh * nh + 1.0 < B_MIN)
        return value, delta, flat

    def _segment(self, O, D, D_cam, I_first, with_tol):
        """A child ray as the path's last segment: value (m,3) (0 on a miss), delta (m,3) the summed finite
        differences of the tolerance, the hit's instance (-1: none), the exclusions and the coverage flags."""
        sd, slip, m = self.sd, self.slip, len(O)
        k2, t2, u2, v2 = closest(O, D, self.tris)
        kg = closest(O, D, self.tris, EDGE)[0]
        hit = k2 >= 0
        inst = np.where(hit, self.inst_of_tri[np.maximum(k2, 0)], -1)
        prim = k2 - self.first_tri[np.maximum(inst, 0)]
        I2 = O + np.where(hit, t2, 0.0)[:, None] * D
        V = -(D_cam if slip == "v_is_camera_ray" else D)
        value, delta = np.zeros((m, 3)), np.zeros((m, 3))
        excl = dict(edge=(hit & (np.minimum(np.minimum(u2, v2), 1 - u2 - v2) <= EDGE)) | (kg != k2),
                    texel=np.zeros(m, bool), outline=np.zeros(m, bool), flat_top=np.zeros(m, bool))
        cover = {k: np.zeros(m, bool) for k in ("mapped", "smooth", "uv_ge_1", "own_dims_differ", "scaled")}
        lit_, shadowed = np.zeros(m, bool), np.zeros(m, bool)
        if slip == "uv_swapped":
            u2, v2 = v2, u2
        for i in range(len(sd.instances)):
            a = np.flatnonzero(inst == i)
            if not a.size:
                continue
            j, pr = i, prim[a]
            if slip == "first_hit_instance_at_depth_1":
                j = self.spec
                pr = pr % sd.meshes[sd.instances[j][0]].tri_count
            mesh = sd.meshes[sd.instances[j][0]]
            T = np.asarray(sd.instances[j][1], np.float64)
            nm = np.eye(4) if slip == "identity_normal_matrix_at_depth_1" else R.normal_matrix(T)
            mapped = self.normalmap and slip != "normalmap_only_at_first_hit"
            uf, vf = u2[a].astype(F), v2[a].astype(F)
            N = np.asarray(R.shading_normal(mesh, sd.textures, nm, pr, uf, vf, mapped), np.float64)
            is_mapped = mesh.normal >= 0 and mapped
            if slip == "smooth_normal_normalised" and not is_mapped:
                N = N / np.linalg.norm(N, axis=-1, keepdims=True)
            mat = (_material_own_dims if slip == "texel_at_own_map_dims" else R.material)(mesh, sd.textures, pr, uf, vf)
            # exclusions and coverage come from the true hit alone (they are only read when slip is None)
            uv = R.hit_uv(mesh, pr, uf, vf).astype(np.float64)
            alb = np.asarray(sd.textures[mesh.albedo])
            grid = np.array([alb.shape[1], alb.shape[0]], np.float64)
            excl["texel"][a] = (np.abs(uv * grid - np.rint(uv * grid)) / grid < TEXEL_EDGE).any(-1)
            cover["mapped" if is_mapped else "smooth"][a] = True
            cover["uv_ge_1"][a] = (uv >= 1).any(-1)
            for t in (mesh.normal, mesh.metalness):
                if t >= 0:
                    shape = np.asarray(sd.textures[t]).shape
                    cover["own_dims_differ"][a] |= R.texel_index(uv.astype(F), shape[1], shape[0]) != mat["texel"]
            sv = np.linalg.svd(T[:3, :3], compute_uv=False)
            cover["scaled"][a] = sv[0] / sv[-1] > 1.5
            if not self.is_lit:
                value[a] = mat["emissive"]
                continue
            Iv = I_first[a] if slip == "shadow_from_first_hit_point" else I2[a]
            vis = R.visibility(Iv, sd.lights, self.tris)
            excl["outline"][a] = _outline_near(I2[a], self.tris[k2[a]], sd.lights, self.tris)

            value[a], delta[a], excl["flat_top"][a] = self._light(I2[a], N, V[a], mat, vis,
                                                                  "INV" if with_tol and slip is None else "")
            L = R._unit(np.asarray(sd.lights.dir_pos, np.float64) - I2[a])[0]
            lit_[a] = vis[:, 4] & (E._dot(N, L) > 0)
            shadowed[a] = ~vis[:, 4]
        return dict(value=value, delta=delta, inst=inst, excluded=excl, cover=cover, lit=lit_, shadowed=shadowed)

    def differs(self, other, tested):
        """How many of the `tested` pixels another reference of the same case differs at: in its float32 bits for the
        exact case, by more than 100 tol in some channel otherwise."""
        if self.exact:
            d = (self.expected.astype(F).view(np.uint32) != other.expected.astype(F).view(np.uint32)).any(-1)
        else:
            d = (np.abs(self.expected - other.expected) > 100.0 * self.tol).any(-1)
        return int((d & tested).sum())


# ------------------------------------------------------------------------------------------------ part 2
class Hall:
    """Two facing delta mirrors (rectangles 0 = floor, which emits, and 1 = ceiling) under a sky.  Per pixel: k, the
    mirror hits before the ray leaves (counted up to `max_hits`); ok, no hit and no passage within `margin` of an
    outline; which of the hits are the floor's; the camera direction in float32."""

    def __init__(self, sd, W, H, margin, max_hits=24):
        s = P.Scene(sd, skybox=True)
        assert len(s.rects) == 2 and all(r.metal == 1.0 and r.rough == 0.0 for r in s.rects)
        assert abs(s.rects[0].N[1]) == 1.0 and s.rects[0].N[1] == -s.rects[1].N[1] and not s.rects[1].emis.any()
        O, D = s.primary(W, H)
        n = len(O)
        cam = R.camera(sd.cam_pos, sd.cam_target, F(W) / F(H))
        ys, xs = np.mgrid[0:H, 0:W]
        self.D32 = R.ray_ctor_dir(R.primary_rays(cam, W, H, xs.reshape(-1), ys.reshape(-1)))
        self.sd, self.emis = sd, s.rects[0].emis.astype(F)
        self.k = np.zeros(n, int)
        self.ok = np.ones(n, bool)
        self.floor = np.zeros((n, max_hits), bool)
        alive = np.ones(n, bool)
        for j in range(max_hits + 1):
            t, idx = s.closest(O, D)
            edge = np.zeros(n, bool)
            for r in s.rects:
                edge |= r.hit(O, D, margin)[1]
            self.ok &= ~(alive & edge)
            alive = alive & (idx >= 0)
            if j == max_hits:
                break
            self.floor[:, j] = alive & (idx == 0)
            self.k += alive
            Nn = np.stack([s.rects[max(i, 0)].N for i in idx])
            I = O + np.where(np.isfinite(t), t, 0.0)[:, None] * D
            D = np.where(alive[:, None], D - 2.0 * E._dot(D, Nn)[:, None] * Nn, D)
            O = np.where(alive[:, None], I + D * EPS, O)
        self.capped = alive          # still between the mirrors after max_hits: k is a lower bound
        self.max_hits = max_hits

    def expected(self, bounces, slip=None):
        """(expected (n,3) float32, sky_arrives (n,) bool, tol (n,3)) at `bounces`; the sky term's tolerance is
        test_gpu_path.check_mirror_corner's, the emission-only pixels are exact (tol 0)."""
        assert slip is None or slip in HALL_SLIPS
        b = bounces + {"cap_one_early": -1, "cap_one_late": 1}.get(slip, 0)
        assert b < self.max_hits
        sky_arrives = self.k + 1 <= b
        Dn = self.D32.copy()
        Dn[:, 1] = np.where(self.k % 2 == 1, -Dn[:, 1], Dn[:, 1])        # y flips at every hit: exact in float32
        Dn = R.ray_ctor_dir(Dn)
        sky = R.sample_sky(self.sd.sky, Dn)
        acc = np.where(sky_arrives[:, None], sky, F(0)).astype(F)
        for j in range(self.max_hits - 1, -1, -1):
            use = (j < np.minimum(self.k, b)) & self.floor[:, j]
            acc = np.where(use[:, None], self.emis[None, :] + acc, acc).astype(F)
        r = np.sqrt(Dn[:, 0].astype(np.float64) ** 2 + Dn[:, 2].astype(np.float64) ** 2)
        h, w = self.sd.sky.shape[:2]
        shift = w / (2 * np.pi * np.maximum(r, 1e-300)) + h / np.pi
        sk = self.sd.sky.astype(np.float64)
        step = max(np.abs(np.diff(sk, axis=0)).max(), np.abs(np.diff(sk, axis=1)).max())
        tol = R.CLOSED_TOL * (np.abs(acc.astype(np.float64)) + 2.0 * step * shift[:, None])
        self.seam_free = (R.sky_taps(Dn, w, h)[2] < w - 1) & (r > 0.1)
        return acc, sky_arrives, np.where(sky_arrives[:, None], tol, 0.0)
