"""Independent float64 Monte Carlo of the recursion of Renderer::Trace, for scenes of a few rectangles.  TEST
INFRASTRUCTURE ONLY.

Written from include/prt.h (the instance material kinds, prt_area_light), the DESIGN.md area-light paragraph and the
reference's Core/Renderer.cpp:150-406,522-550 -- not from csrc/ nor oracle/, and this module imports neither `oracle`
nor `prt`: a slip that the two restatements share disagrees with it.  Camera rays, the sky lookup, the material query
and the light constants come from tests/scene_ref.py; the BRDF closed forms, the samplers, the densities, the power
heuristic and the dielectric split from tests/estimator_ref.py.

What is restated here is only the order of Renderer::Trace (line numbers of Core/Renderer.cpp):
  :152      depth >= bounces returns 0
  :157-159  the closest hit; a miss returns the sky (0 without the skybox flag)
  :196      emission
  :198-326  the reference lights: the directional light alone, or with the stochastic flag one class drawn with
            probability 0.3 / 0.5 / 0.2 and divided by it (point lights: all four summed with a 1 / d falloff and a
            shadow ray that ends at d^2 - EPSILON, times the BRDF towards light (int)(u * 10) % 4; spot: 1 / d^2 inside
            the cone of cosine 0.9)
  prt.h     the area light's sample at every lit hit that is neither a mirror nor a dielectric: f Le w(pl, pb) / pl,
            unweighted at a path's last segment
  :329      depth == bounces - 1 returns what was gathered
  :331-372  a dielectric traces the reflection, then the refraction, and returns their Schlick blend ALONE: what the
            hit itself gathered is dropped
  :376      metalness 1 and roughness 0: the specular lobe without a draw
  :380-391  else the lobe pick u < p, throughput / p or / (1 - p)
  :396-404  the indirect sample and its weight ((1, 1, 1) for the specular lobe: sampleSpecularMicrofacet takes its
            weight by value); a weight of zero luminance ends the path; the bounced ray starts at I + dir * EPSILON
            and what it returns is multiplied by the throughput
A specular sample whose direction lies below the horizon is traced like any other (BRDF.cpp:498-499 is commented
out): it starts under the surface.  The area light is geometry for every closest-hit ray: a ray that reaches it before
any rectangle ends there with Le w on the emitting side(s) and 0 on the other, w = w(pb, pl) for a ray the lobe
sampling made (pb of the hit it left, pl = d^2 / (area cos_l) with d measured from that hit) and 1 for a camera ray, a
mirror's ray and a dielectric's children.  Shadow rays do not see the light.  Shading normals are the rectangles' own,
never flipped: a back-face hit is shaded with N.V < 0 exactly as the closed forms take it.

An instance transform may be rigid (Scene, Rect.carried): the rectangle and its normal are carried to the world, where
everything above happens.  Unit normals stay required: lobe_densities and the MIS weights assume them.

Random numbers are numpy's, so only the estimator's expectation and variance are comparable with an implementation,
never single frames.  `slip=` plants one named defect (SLIPS) to show that a comparison against this reference has the
power to see it.
"""
import numpy as np

import estimator_ref as E
import scene_ref as R

MAT_TEXTURED, MAT_DIELECTRIC, MAT_MIRROR = 0, 1, 2      # include/prt.h PRT_MAT_*
EPS = float(R.EPSILON)
_LUM = np.array([0.2126, 0.7152, 0.0722])                # luminance(), Core/BRDF.cpp

SLIPS = ("no_lobe_division", "direct_not_scaled_by_throughput", "indirect_miss_is_black",
         "emission_only_at_first_hit", "cap_one_early", "cap_one_late", "spec_below_horizon_ends_path",
         "last_segment_weighted_everywhere", "glass_children_swapped", "bounced_ray_not_transformed")


def _unit0(v):
    """The direction a tinybvh::Ray holds (scene_ref.ray_ctor_dir, in float64): the zero direction stays zero."""
    l = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where(l > 0, v / np.where(l > 0, l, 1.0), 0.0)


class Rect:
    """c + a eu + b ev (a, b in [0, 1]; eu, ev orthogonal) with one shading normal and one material."""

    def __init__(self, c, eu, ev, normal, mat, kind):
        self.c, self.eu, self.ev = (np.asarray(x, np.float64) for x in (c, eu, ev))
        self.plane = np.cross(self.eu, self.ev)
        self.N = np.asarray(normal, np.float64)
        self.kind = kind
        self.base = np.asarray(mat["base"], np.float64).reshape(3)
        self.metal = float(np.asarray(mat["metalness"]).reshape(()))
        self.rough = float(np.asarray(mat["roughness"]).reshape(()))
        self.emis = np.asarray(mat["emissive"], np.float64).reshape(3)
        if kind == MAT_MIRROR:                               # prt.h: MIRROR forces metalness 1 / roughness 0, and
            self.metal, self.rough = 1.0, 0.0                # Core/Scene.cpp:199-204 never sets a mirror's emission
            self.emis = np.zeros(3)
        self.N_object = self.N                               # the normal as authored, before carried()

    def carried(self, T):
        """This rectangle under the rigid instance transform T (4x4, row-major): c' = T c, eu' = R eu, ev' = R ev,
        N' = R N -- a rotation's normal matrix is the rotation."""
        T = np.asarray(T, np.float64)
        Rm = T[:3, :3]
        assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) and np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-6, T
        self.c, self.eu, self.ev = Rm @ self.c + T[:3, 3], Rm @ self.eu, Rm @ self.ev
        self.plane = np.cross(self.eu, self.ev)
        self.N = Rm @ self.N_object
        return self

    def hit(self, O, D, margin=None):
        """t (inf where none) of rays O, D with 0 < t; with `margin` also whether the plane point lies within that
        distance of the outline, on either side."""
        den = D @ self.plane
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(den != 0, ((self.c - O) @ self.plane) / np.where(den != 0, den, 1.0), np.inf)
        t = np.where(t > 0, t, np.inf)
        P = O + np.where(np.isfinite(t), t, 0.0)[:, None] * D - self.c
        a, b = (P @ self.eu) / (self.eu @ self.eu), (P @ self.ev) / (self.ev @ self.ev)
        inside = np.isfinite(t) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
        if margin is None:
            return np.where(inside, t, np.inf)
        ma, mb = margin / np.linalg.norm(self.eu), margin / np.linalg.norm(self.ev)
        grown = np.isfinite(t) & (a >= -ma) & (a <= 1 + ma) & (b >= -mb) & (b <= 1 + mb)
        shrunk = np.isfinite(t) & (a >= ma) & (a <= 1 - ma) & (b >= mb) & (b <= 1 - mb)
        return np.where(inside, t, np.inf), grown & ~shrunk


def _rect_of_mesh(mesh, textures, kind):
    """A two-triangle mesh (v00, v01, v10), (v10, v01, v11) with one normal and one texel -> Rect."""
    v = np.asarray(mesh.vertices, np.float64).reshape(-1, 3)
    assert v.shape[0] == 6 and np.array_equal(v[1], v[4]) and np.array_equal(v[2], v[3])
    c, eu, ev = v[0], v[1] - v[0], v[2] - v[0]
    # (a mesh authored pre-rotated holds float32 roundings of a rectangle's corners)
    scale = np.linalg.norm(eu) * np.linalg.norm(ev)
    assert np.allclose(v[5], c + eu + ev, atol=1e-6 * np.sqrt(scale)) and abs(eu @ ev) < 1e-6 * scale
    n = np.asarray(mesh.fixed_normals, np.float64).reshape(-1, 4)[:, :3]
    assert (n == n[0]).all() and np.isclose(np.linalg.norm(n[0]), 1.0)
    mat = R.material(mesh, textures, np.zeros(1, np.int64), np.full(1, 0.25, R.F), np.full(1, 0.25, R.F))
    return Rect(c, eu, ev, n[0], mat, kind)


class Scene:
    """The rectangles, lights, sky and area light of a scenes.SceneData-shaped object (one instance per mesh in order,
    each under a rigid transform: R^T R = I within 1e-6 and any translation; anything else asserts) under the flags
    `stochastic`, `skybox` and `lighted`."""

    def __init__(self, sd, stochastic=False, skybox=True, lighted=True):
        kinds = sd.materials if sd.materials is not None else [MAT_TEXTURED] * len(sd.instances)
        self.rects = []
        for k, (mi, T) in enumerate(sd.instances):
            self.rects.append(_rect_of_mesh(sd.meshes[mi], sd.textures, int(kinds[k])).carried(T))
        self.lights, self.sky, self.sd = sd.lights, sd.sky, sd
        self.stochastic, self.skybox, self.lighted = stochastic, skybox and sd.sky is not None, lighted
        self.light = None
        if sd.area_light is not None:
            c, eu, ev, n, Le, area, two = E.light_geometry(sd.area_light)
            z = np.zeros(3)
            self.light = dict(rect=Rect(c, eu, ev, n, dict(base=z, metalness=0.0, roughness=0.0, emissive=z), None),
                              n=n, Le=Le, area=area, two=two)

    # ---------------------------------------------------------------------------------------- geometry
    def primary(self, W, H):
        """Every pixel's camera ray (scene_ref, float32 as the reference makes it), as float64 origin and direction."""
        cam = R.camera(self.sd.cam_pos, self.sd.cam_target, R.F(W) / R.F(H))
        ys, xs = np.mgrid[0:H, 0:W]
        D = R.ray_ctor_dir(R.primary_rays(cam, W, H, xs.reshape(-1), ys.reshape(-1))).astype(np.float64)
        return np.repeat(cam["pos"].astype(np.float64)[None], W * H, 0), D

    def closest(self, O, D):
        """(t, index of the rectangle; -1 = none)."""
        t = np.full(len(O), np.inf)
        idx = np.full(len(O), -1)
        for k, r in enumerate(self.rects):
            tk = r.hit(O, D)
            nearer = tk < t
            t, idx = np.where(nearer, tk, t), np.where(nearer, k, idx)
        return t, idx

    def occluded(self, O, D, tmax):
        """Scene::IsOccluded: any rectangle with 0 < t < tmax."""
        occ = np.zeros(len(O), bool)
        for r in self.rects:
            occ |= r.hit(O, D) < tmax
        return occ

    def classify(self, W, H, margin):
        """Per pixel the first thing its camera ray meets (rectangle index, -1 nothing, -2 the area light) and whether
        the ray passes within `margin` of any outline."""
        O, D = self.primary(W, H)
        t, idx = self.closest(O, D)
        edge = np.zeros(len(O), bool)
        for r in self.rects:
            edge |= r.hit(O, D, margin)[1]
        if self.light is not None:
            tl, el = self.light["rect"].hit(O, D, margin)
            idx = np.where(tl < t, -2, idx)
            edge |= el
        return idx, edge

    # ---------------------------------------------------------------------------------------- the estimator
    def estimate(self, pixels, W, H, bounces, M, seed, slip=None, batch=1 << 19):
        """Mean and sample standard deviation (both (P, 3)) of one path's radiance at `pixels`, from M paths each."""
        assert slip is None or slip in SLIPS
        O, D = self.primary(W, H)
        pixels = np.asarray(pixels)
        run = _Run(self, bounces, np.random.default_rng(seed), slip)
        mean, sigma = np.zeros((pixels.size, 3)), np.zeros((pixels.size, 3))
        per = max(1, batch // M)
        for p0 in range(0, pixels.size, per):
            px = pixels[p0:p0 + per]
            acc = np.ones((px.size * M, 3)) if slip == "direct_not_scaled_by_throughput" else None
            rad = run.trace(np.repeat(O[px], M, 0), np.repeat(D[px], M, 0), 0, None, acc).reshape(px.size, M, 3)
            mean[p0:p0 + per] = rad.mean(1)
            sigma[p0:p0 + per] = rad.std(1, ddof=1)
        return mean, sigma


class _Run:
    def __init__(self, scene, bounces, rng, slip):
        self.s, self.rng, self.slip = scene, rng, slip
        self.bounces = bounces + {"cap_one_early": -1, "cap_one_late": 1}.get(slip, 0)

    # acc: the product of the throughputs above this ray, kept only for the slip that needs it
    def trace(self, O, D, depth, pb, acc):
        """Radiance (n, 3) of rays O, D at recursion depth `depth`.  pb: None, or per ray the density with which the
        lobe sampling of the hit it left made its direction (the area light's weight needs it)."""
        s, n = self.s, len(O)
        out = np.zeros((n, 3))
        if depth >= self.bounces or n == 0:                                        # :152
            return out
        D = _unit0(D)
        t, idx = s.closest(O, D)
        if s.light is not None:
            lt = s.light
            tl = lt["rect"].hit(O, D)
            first = tl < t
            cos_l = -(D @ lt["n"])
            emits = first & ((np.abs(cos_l) > 0) if lt["two"] else (cos_l > 0))
            w = np.ones(n)
            if pb is not None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    pl = (tl + EPS) ** 2 / (lt["area"] * np.abs(cos_l))
                w = np.where(emits, E.mis_power(pb, np.where(emits, pl, 1.0)), 0.0)
            out[emits] = lt["Le"] * w[emits, None]
            idx = np.where(first, -2, idx)
        miss = idx == -1
        if s.skybox and miss.any() and not (self.slip == "indirect_miss_is_black" and depth > 0):
            out[miss] = R.sample_sky(s.sky, D[miss].astype(R.F)).astype(np.float64)   # :159
        for k in range(len(s.rects)):
            sel = np.flatnonzero(idx == k)
            if sel.size:
                out[sel] = self.shade(s.rects[k], O[sel] + t[sel, None] * D[sel], D[sel], depth,
                                      None if acc is None else acc[sel])
        return out

    def brdf(self, r, N, L, V):
        n = len(L)
        return E.eval_brdf(N, L[:, None, :], V, np.broadcast_to(r.base, (n, 3)), np.full(n, r.metal),
                           np.full(n, r.rough))[:, 0, :]

    def pb(self, r, N, L, V, p):
        pd, ps = E.lobe_densities(N, L[:, None, :], V, np.full(len(L), r.rough))
        return p * ps[:, 0] + (1.0 - p) * pd[:, 0]

    def towards(self, I, pos):
        Lv = np.asarray(pos, np.float64) - I
        d = np.linalg.norm(Lv, axis=-1)
        return Lv / d[:, None], d

    def lit(self, I, L, tmax):
        return ~self.s.occluded(I + L * EPS, L, tmax)

    def reference_lights(self, r, I, N, V):
        """Renderer.cpp:198-326 for one hit each: the radiance the point / directional / spot block adds."""
        s, n = self.s, len(I)
        lg = s.lights
        out = np.zeros((n, 3))
        if not s.lighted:
            return out
        pick = np.ones(n, int)
        prob = 1.0
        if s.stochastic:
            u = self.rng.random(n)
            pick = np.where(u < float(R.P_POINT), 0, np.where(u < float(R.P_POINT) + float(R.P_DIR), 1, 2))   # :210-214
        a = np.flatnonzero(pick == 0)
        if a.size:                                                                              # :216-269
            contrib = np.zeros((a.size, 3))
            Ls = []
            for i in range(4):
                L, d = self.towards(I[a], np.asarray(lg.point_pos, np.float64).reshape(4, 3)[i])
                cosa = np.maximum(0.0, E._dot(N[a], L))
                vis = self.lit(I[a], L, d * d - EPS)                                          # :257, the squared distance
                col = np.asarray(lg.point_col, np.float64).reshape(4, 3)[i]
                contrib += np.where(vis[:, None], col * ((1.0 / d) * cosa)[:, None], 0.0)
                Ls.append(L)
            contrib /= float(R.P_POINT)
            which = (self.rng.random(a.size) * 10).astype(int) % 4                              # :267
            Lw = np.stack(Ls, 0)[which, np.arange(a.size)]
            out[a] = self.brdf(r, N[a], Lw, V[a]) * contrib
        a = np.flatnonzero(pick == 1)
        if a.size:                                                                              # :270-286, :312-326
            L, d = self.towards(I[a], lg.dir_pos)
            cosa = np.maximum(0.0, E._dot(N[a], L))
            vis = self.lit(I[a], L, d - EPS)
            prob = float(R.P_DIR) if s.stochastic else 1.0
            con = np.where(vis[:, None], np.asarray(lg.dir_col, np.float64) * cosa[:, None], 0.0) / prob
            out[a] = self.brdf(r, N[a], L, V[a]) * con
        a = np.flatnonzero(pick == 2)
        if a.size:                                                                              # :287-310
            L, d = self.towards(I[a], lg.spot_pos)
            cosa = np.maximum(0.0, E._dot(N[a], L))
            inside = (L @ np.asarray(lg.spot_rot, np.float64)) > 0.9
            vis = self.lit(I[a], L, d - EPS) & inside
            con = np.where(vis[:, None], np.asarray(lg.spot_col, np.float64) * ((1.0 / (d * d)) * cosa)[:, None], 0.0)
            out[a] = self.brdf(r, N[a], L, V[a]) * (con / float(R.P_SPOT))
        return out

    def area_sample(self, r, I, N, V, p, last):
        """prt.h prt_area_light: one uniform point of the light, f Le w(pl, pb) / pl, unweighted at a last segment."""
        lt = self.s.light
        n = len(I)
        ab = self.rng.random((n, 2))
        Y = lt["rect"].c + ab[:, :1] * lt["rect"].eu + ab[:, 1:] * lt["rect"].ev
        L, d = self.towards(I, Y)
        cos_l = -(L @ lt["n"])
        if lt["two"]:
            cos_l = np.abs(cos_l)
        seen = (cos_l > 0) & (E._dot(N, L) > 0)
        f = self.brdf(r, N, L, V)
        pl = d * d / (lt["area"] * np.where(seen, cos_l, 1.0))
        w = np.ones(n)
        if not last or self.slip == "last_segment_weighted_everywhere":
            w = E.mis_power(pl, self.pb(r, N, L, V, p))
        seen &= self.lit(I, L, d - EPS)
        return np.where(seen[:, None], f * lt["Le"] * (w / pl)[:, None], 0.0)

    def shade(self, r, I, D, depth, acc):
        s, n = self.s, len(I)
        V = -D
        N = np.broadcast_to(r.N_object if self.slip == "bounced_ray_not_transformed" and depth > 0 else r.N, (n, 3))
        base = np.broadcast_to(r.base, (n, 3))
        metal, rough = np.full(n, r.metal), np.full(n, r.rough)
        last = depth == self.bounces - 1
        delta = r.kind == MAT_MIRROR or (r.metal == 1.0 and r.rough == 0.0)
        result = np.zeros((n, 3))
        if not (self.slip == "emission_only_at_first_hit" and depth > 0):
            result = result + r.emis                                                           # :196
        direct = self.reference_lights(r, I, N, V)
        p = E.probability(N, V, base, metal)
        if s.light is not None and s.lighted and not delta and r.kind != MAT_DIELECTRIC:
            direct = direct + self.area_sample(r, I, N, V, p, last)
        if self.slip == "direct_not_scaled_by_throughput" and depth > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                direct = np.where(acc > 0, direct / np.where(acc > 0, acc, 1.0), 0.0)
        result = result + direct
        if last:                                                                               # :329
            return result
        if r.kind == MAT_DIELECTRIC:                                                           # :331-372
            g = E.glass(D, N)
            fres = g["fres"][:, None]
            refl = self.trace(I + N * EPS, g["R"], depth + 1, None, None if acc is None else acc * fres)
            refr = np.zeros((n, 3))
            tr = np.flatnonzero(g["traced"])
            refr[tr] = self.trace(I[tr] - N[tr] * EPS, g["T"][tr], depth + 1, None,
                                  None if acc is None else acc[tr] * (1.0 - fres[tr]))
            if self.slip == "glass_children_swapped":
                refl, refr = refr, refl
            return E.glass_combine(g, refl, refr)
        q = E.rotation_to_z(N)
        Vl = E.rotate(q, V)
        thr = np.ones((n, 3))
        if delta:                                                                              # :376
            spec = np.ones(n, bool)
        else:                                                                                  # :380-391
            spec = self.rng.random(n) < p
            if self.slip != "no_lobe_division":
                thr = thr / np.where(spec, p, 1.0 - p)[:, None]
        u = self.rng.random((n, 1, 2))                                                         # :396
        alpha = rough * rough
        if r.rough == 0.0:
            Hs = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (n, 3))                            # BRDF.cpp:356-359
        else:
            Hs = E.vndf(Vl, alpha, u)[:, 0, :]
        Ls = 2.0 * E._dot(Vl, Hs)[:, None] * Hs - Vl                                           # reflect(-Vlocal, H)
        Ld = E.sample_hemisphere(u[:, 0, :])
        wd = E.diffuse_weight(u, N, V, base, metal, rough)[:, 0, :]
        Ll = np.where(spec[:, None], Ls, Ld)
        weight = np.where(spec[:, None], 1.0, wd)
        alive = (weight @ _LUM) != 0.0                                                         # BRDF.cpp:493
        if self.slip == "spec_below_horizon_ends_path":
            alive &= ~(spec & (Ls[:, 2] <= 0.0))
        dirw = E._unit(E.rotate(q * np.array([-1.0, -1.0, -1.0, 1.0]), Ll))                    # BRDF.cpp:496
        thr = thr * weight                                                                     # :401
        a = np.flatnonzero(alive)
        if a.size:
            pb = None
            if s.light is not None and not delta:
                pb = self.pb(r, N[a], dirw[a], V[a], p[a])
            got = self.trace(I[a] + dirw[a] * EPS, dirw[a], depth + 1, pb, None if acc is None else acc[a] * thr[a])
            result[a] = result[a] + got * thr[a]                                               # :404
        return result
