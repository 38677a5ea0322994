"""The area-light estimator and the dielectric branch on the device, against the independent float64 reference
tests/estimator_ref.py.  tests/test_estimator_ref.py runs the same checks (the check_* functions below) against the
oracle on the CPU.

Every other test of these two extensions compares libprt.so with oracle/prt_oracle.c -- two restatements by one
author of code the reference never runs -- or asserts inequalities.  Here the expected values come from a quadrature of
the estimator's definition (statistical cases), from geometry alone (exact cases), and from the literal dielectric
split in float64 (glass).

The scene: one floor quad (y = 0, half-size 3, unit normals, every UV 0.5) under 1 x 1 maps, every reference light
black and far away, camera (0, 2.5, -4) -> (0, 0, 0.5), image 16 x 12, flags = default - AA - GAMMA - SKYBOX: one
centred path per pixel per frame, whose only radiance is the area light's.

Statistical cases.  n = 4096 frames of fixed seed (frame_index advances; 16384 for the big light over the (0.25, 1)
floor, see N_FRAMES_OF), rendered in chunks whose averages are summed in float64.  With `bounces` = 1 every hit is a path's last segment (estimator_ref.expected_direct, bounces_left = 0);
with `bounces` = 2 the first hit combines both strategies (bounces_left = 1): the floor is planar, so a BRDF ray
meets the light or nothing, and the second segment adds nothing else.  Bounds, fixed before any run:
  per pixel and channel  |mean - expectation| <= 6 se + allowance,  se = (sigma_nee + sigma_brdf) / sqrt(n) from
                         estimator_ref.second_moment (a bound on the sum's deviation whatever the correlation of the
                         two terms), allowance = |E_K - E_2K| of the quadrature (the expectation used is E_2K)
  per channel, summed    |sum mean - sum expectation| <= 6 sqrt(sum se^2) + sum allowance (pixels are independent)
6 standard errors is 2e-9 per pixel, two-sided; the seeds are fixed anyway.  estimator_ref's self-check asserts that
the summed bound is below 10 % of the summed expectation for every case, so a 10 % bias cannot pass.

Largest z = (|mean - expectation| - allowance) / se seen with the corrected estimator, on the oracle (the device's
frames are bit-identical, test_device_equals_oracle; `pytest -s` prints them), per (light, roughness, metalness), as
largest pixel / largest channel sum:
  bounces 1   big 1,0: 3.34 / 0.02    big .5,.5: 3.32 / 0.24    big .25,1: 2.69 / 0.08
              small 1,0: 3.24 / 0.09  small .5,.5: 3.27 / 0.94  small .25,1: 3.34 / 1.75
  bounces 2   big 1,0: 3.26 / 1.86    big .5,.5: 3.29 / 0.98    big .25,1: 2.65 / 0.71
              small 1,0: 3.24 / 0.39  small .5,.5: 3.27 / 0.91  small .25,1: 3.34 / 0.92
(the cases share their seeds, hence their light samples: the same pixel is the unluckiest in most of them).
Before the correction -- the light sample of a last segment still weighted by w(pl, pb) -- the bounces = 1 red sums of
the 91 tested pixels under the big light were 13.65 against 21.13 expected (1, 0), 13.71 against 28.78 (0.5, 0.5) and
3.54 against 31.40 (0.25, 1): z of the sums 94, 96 and 41, at 4096 frames each.  Under the small, far light pl
dwarfs pb, the weight was nearly 1, and the three cases stayed inside the bound before as after.
"""
import dataclasses
import functools

import numpy as np
import pytest

import estimator_ref as E
import scene_ref as R
import test_gpu_scene_queries as SQ
from prt import _lib, scenes

F = np.float32
W, H = 16, 12
FLAGS = _lib.FLAGS_DEFAULT & ~(_lib.FLAG_AA | _lib.FLAG_GAMMA | _lib.FLAG_SKYBOX)
SEED = 20250117
N_FRAMES = 4096
# under the big light the (0.25, 1) floor's last-segment sample has a standard error that would let a 13 % bias of the
# summed pixels pass at 4096 frames; 16384 frames bring the summed bound to 7 % (test_estimator_ref.py asserts < 10 %)
N_FRAMES_OF = {("big", 0.25, 1.0): 16384}
CHUNK = 256            # frames per render call: the float32 accumulator of one call sums at most 256 values
# cells per side of the light at the coarse level; the fine level doubles it ((big, 0.25, 1): the narrow lobe, and a
# standard error halved by four times the frames)
K_QUAD = {"big": 64, "small": 48, ("big", 0.25, 1.0): 80}
MARGIN = 0.02          # scene units: a primary or reflected ray this close to the light's outline is not tested
CAM_POS, CAM_TARGET = (0.0, 2.5, -4.0), (0.0, 0.0, 0.5)
HALF = 3.0

LIGHTS = {
    # emit downwards: cross(edge_u, edge_v) = (0, -1, 0) * area
    "big": scenes.ceiling_light(corner=(-1.0, 0.6, -1.0), edge_u=(2.0, 0.0, 0.0), edge_v=(0.0, 0.0, 2.0),
                                radiance=(4.0, 4.0, 4.0)),
    "small": scenes.ceiling_light(corner=(-0.2, 2.0, 0.3), edge_u=(0.4, 0.0, 0.0), edge_v=(0.0, 0.0, 0.4),
                                  radiance=(40.0, 40.0, 40.0)),
}
# a panel above the camera's height: no camera ray (they all point downwards) can cross it, so a scene's shadow-ray
# count with it and without it differ by the light's own rays alone
HIGH = dict(corner=(-1.5, 2.6, 0.0), radiance=(3.0, 2.0, 1.0))
MATERIALS = [(1.0, 0.0), (0.5, 0.5), (0.25, 1.0)]      # (roughness, metalness)
STAT_CASES = [(light, rough, metal) for light in LIGHTS for rough, metal in MATERIALS]


# ------------------------------------------------------------------------------------------------ scenes
def _dark_lights():
    """Every reference light black, and far from any hit point (a light AT a hit point would divide by zero)."""
    far = np.array([0.0, 60.0, 0.0], F)
    z = np.zeros(3, F)
    return scenes.Lights(np.tile(far, (4, 1)), np.zeros((4, 3), F), far.copy(), z.copy(), far.copy(), z.copy(),
                         np.array([0.0, 1.0, 0.0], F))


def _flat_quad(cx, y, cz, half, **tex):
    c = np.array([[cx - half, y, cz - half], [cx - half, y, cz + half], [cx + half, y, cz - half],
                  [cx + half, y, cz + half]])
    P = np.array([[c[0], c[1], c[2]], [c[2], c[1], c[3]]])              # (v00, v01, v10): +y face normals
    return SQ._mesh(P, np.tile(np.array([0.0, 1.0, 0.0]), (2, 3, 1)), np.full((2, 3, 2), 0.5), **tex)


def floor_scene(rough=1.0, metal=0.0, light=None, kind=_lib.MAT_TEXTURED, blocker=None, floor_y=0.0, sky=None,
                cam=(CAM_POS, CAM_TARGET), name="floor"):
    """The floor under 1 x 1 maps (albedo 0x00C0B0A0, metalness texel (rough8 << 8) | metal8) with the area light
    `light` (a dict, or None), the floor instance of material `kind`, and optionally a blocker quad (cx, y, cz, half)."""
    r8, m8 = int(round(rough * 255)), int(round(metal * 255))
    tex = [np.array([[0x00C0B0A0]], np.uint32), np.array([[(r8 << 8) | m8]], np.uint32)]
    meshes = [_flat_quad(0.0, floor_y, 0.0, HALF, albedo=0, metalness=1)]
    inst = [(0, np.eye(4, dtype=F))]
    kinds = [kind]
    if blocker is not None:
        meshes.append(_flat_quad(*blocker, albedo=0, metalness=1))
        inst.append((1, np.eye(4, dtype=F)))
        kinds.append(_lib.MAT_TEXTURED)
    return scenes.SceneData(meshes, tex, inst, _dark_lights(), sky, np.array(cam[0], F), np.array(cam[1], F), name,
                            materials=kinds if kind != _lib.MAT_TEXTURED else None, area_light=light)


def sky_ramp(w=64, h=32):
    """A smooth ramp, linear in u and in v and distinct per channel; no texel repeats along a row or a column."""
    v, u = np.mgrid[0:h, 0:w]
    u, v = u / (w - 1.0), v / (h - 1.0)
    return np.stack([0.5 + 2.0 * u + 0.5 * v, 3.0 - 1.5 * u + 1.0 * v, 0.25 + 0.75 * u + 2.0 * v], -1).astype(F)


# ------------------------------------------------------------------------------------------------ geometry of a view
def _rect_hit(O, D, c, eu, ev, margin=0.0):
    """float64 rays against the parallelogram c + a eu + b ev: (t, inside, near_edge); t = inf where parallel.
    inside: a, b within [0, 1]; near_edge: within `margin` (scene units) of the outline, on either side."""
    n = np.cross(eu, ev)
    den = D @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den != 0, ((c - O) @ n) / den, np.inf)
    t = np.where(t > 0, t, np.inf)
    Pp = O + np.where(np.isfinite(t), t, 0.0)[:, None] * D - c
    a, b = (Pp @ eu) / (eu @ eu), (Pp @ ev) / (ev @ ev)          # the edges used here are orthogonal
    ma, mb = margin / np.linalg.norm(eu), margin / np.linalg.norm(ev)
    fin = np.isfinite(t)
    inside = fin & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
    grown = fin & (a >= -ma) & (a <= 1 + ma) & (b >= -mb) & (b <= 1 + mb)
    shrunk = fin & (a >= ma) & (a <= 1 - ma) & (b >= mb) & (b <= 1 - mb)
    return t, inside, grown & ~shrunk


class Geometry:
    """What scene_ref says about the primary rays of a floor scene: per pixel the float64 ray, whether it reaches the
    floor (and where), whether it reaches the area light first, and which pixels are too close to an outline."""

    def __init__(self, sd, margin=MARGIN):
        cam = R.camera(sd.cam_pos, sd.cam_target, F(W) / F(H))
        ys, xs = np.mgrid[0:H, 0:W]
        D32 = R.ray_ctor_dir(R.primary_rays(cam, W, H, xs.reshape(-1), ys.reshape(-1)))
        self.D32 = D32
        self.D = D32.astype(np.float64)
        self.O = np.repeat(cam["pos"].astype(np.float64)[None], W * H, 0)
        verts = np.asarray(sd.meshes[0].vertices, np.float64).reshape(-1, 3)
        self.floor_y = float(verts[0, 1])
        lo = np.array([-HALF, self.floor_y, -HALF])
        ex, ez = np.array([2 * HALF, 0.0, 0.0]), np.array([0.0, 0.0, 2 * HALF])
        self.t_floor, on_floor, floor_edge = _rect_hit(self.O, self.D, lo, ex, ez, margin)
        t_first = np.where(on_floor, self.t_floor, np.inf)
        self.blocked = np.zeros(W * H, bool)
        edge = floor_edge.copy()
        for mi in range(1, len(sd.meshes)):                     # a blocker quad: its pixels are not floor pixels
            v = np.asarray(sd.meshes[mi].vertices, np.float64).reshape(-1, 3)
            c0 = v.min(0)
            span = v.max(0) - c0
            tb, inb, eb = _rect_hit(self.O, self.D, c0, np.array([span[0], 0, 0]), np.array([0, 0, span[2]]), margin)
            self.blocked |= inb & (tb < t_first)
            edge |= eb
            t_first = np.where(inb, np.minimum(t_first, tb), t_first)
        self.light_first = np.zeros(W * H, bool)
        self.light_cos = np.zeros(W * H)
        if sd.area_light is not None:
            c, eu, ev, n, _, _, _ = E.light_geometry(sd.area_light)
            tl, inl, el = _rect_hit(self.O, self.D, c, eu, ev, margin)
            self.light_first = inl & (tl < t_first)
            self.light_cos = -(self.D @ n)                      # > 0: the camera sees the emitting side
            edge |= el
        self.edge = edge
        self.floor = on_floor & ~self.blocked & ~self.light_first & ~edge
        self.I = self.O + np.where(np.isfinite(self.t_floor), self.t_floor, 0.0)[:, None] * self.D   # tiny_bvh.h:586
        self.N = np.tile(np.array([0.0, 1.0, 0.0]), (W * H, 1))
        self.V = -self.D
        n_px = W * H
        self.mat = R.material(sd.meshes[0], sd.textures, np.zeros(n_px, np.int64), np.full(n_px, 0.25, F),
                              np.full(n_px, 0.25, F))


@functools.lru_cache(None)
def stat_scene(light, rough, metal):
    return floor_scene(rough, metal, LIGHTS[light], name=f"floor-{light}-{rough}-{metal}")


class StatRef:
    """The float64 reference of one statistical case at its tested pixels, computed once per process."""

    def __init__(self, light, rough, metal):
        sd = stat_scene(light, rough, metal)
        g = Geometry(sd)
        self.sel = np.flatnonzero(g.floor)
        mat = {k: g.mat[k][self.sel] for k in ("base", "metalness", "roughness")}
        args = (g.I[self.sel], g.N[self.sel], g.V[self.sel], mat, sd.area_light)
        K = K_QUAD.get((light, rough, metal), K_QUAD[light])
        self.n = N_FRAMES_OF.get((light, rough, metal), N_FRAMES)
        coarse, fine = E.quadrature(*args, K), E.quadrature(*args, 2 * K)
        self.exp, self.allow, self.se = {}, {}, {}
        for left in (0, 1):
            self.exp[left] = E.expected_direct(*args, left, q=fine)
            self.allow[left] = np.abs(self.exp[left] - E.expected_direct(*args, left, q=coarse))
            m = E.second_moment(*args, left, q=fine)
            assert np.allclose(m["nee_m1"] + m["brdf_m1"], self.exp[left], rtol=1e-12, atol=1e-300)
            self.se[left] = (m["sigma_nee"] + m["sigma_brdf"]) / np.sqrt(self.n)


@functools.lru_cache(None)
def stat_ref(light, rough, metal):
    return StatRef(light, rough, metal)


# ------------------------------------------------------------------------------------------------ shared checks
# A `view` is one implementation under test loaded with one scene at 16 x 12:
#   view.mean(bounces, n)      -> [n_pixels, 3] float64, the mean of n frames (chunk averages summed in float64)
#   view.frames(bounces, k)    -> (avg [n_pixels, 3] float32, rgb8, segments, shadow_rays) of one call of k frames
def z_scores(ref, left, mean):
    """(largest per-pixel z, per-channel z of the sums); z = (|deviation| - allowance) / standard error."""
    dev = np.abs(mean[ref.sel] - ref.exp[left])
    zp = (dev - ref.allow[left]) / ref.se[left]
    dsum = np.abs(mean[ref.sel].sum(0) - ref.exp[left].sum(0))
    zs = (dsum - ref.allow[left].sum(0)) / np.sqrt((ref.se[left] ** 2).sum(0))
    return zp, zs


def check_statistical(view, ref, bounces):
    left = 0 if bounces == 1 else 1
    mean = view.mean(bounces, ref.n)
    zp, zs = z_scores(ref, left, mean)
    got, exp = mean[ref.sel].sum(0), ref.exp[left].sum(0)
    print(f"{view.sd.name} bounces {bounces}: pixels {ref.sel.size}, sum {got.round(3)} expected {exp.round(3)}, "
          f"largest z pixel {zp.max():.2f} sum {zs.max():.2f}")
    assert ref.sel.size >= 60
    assert (zs <= 6.0).all(), (view.sd.name, bounces, "sum", got, exp, zs)
    assert (zp <= 6.0).all(), (view.sd.name, bounces, "pixel", float(zp.max()), int((zp > 6.0).sum()))
    return float(zp.max()), float(zs.max())


def _le(sd):
    return np.asarray(sd.area_light["radiance"], F)


def _same(got, exp):
    return np.array_equal(SQ.bits(got), SQ.bits(np.broadcast_to(np.asarray(exp, F), got.shape)))


def _area_shadow_rays(view, bounces):
    """The shadow rays the area light adds to a call: the count with it minus the count of the scene without it."""
    return view.frames(bounces, 1)[3] - view.without_light().frames(bounces, 1)[3]


def mirror_scene():
    high = scenes.ceiling_light(edge_u=(3.0, 0.0, 0.0), edge_v=(0.0, 0.0, 3.0), **HIGH)
    return floor_scene(light=high, kind=_lib.MAT_MIRROR, name="floor-mirror")


def check_mirror(view):
    """A MIRROR floor (metalness 1, roughness 0: the delta lobe) takes no light sample; its reflected ray returns
    exactly Le where it meets the light's emitting side and 0 where it misses, and no shadow ray is cast."""
    sd = view.sd
    g = Geometry(sd)
    c, eu, ev, n, _, _, _ = E.light_geometry(sd.area_light)
    Rd = g.D - 2.0 * g.D[:, 1:2] * g.N
    _, inl, el = _rect_hit(g.I + Rd * float(R.EPSILON), Rd, c, eu, ev, MARGIN)
    front = -(Rd @ n) > 0
    assert front[g.floor].all() and not g.light_first.any()
    hit, miss = g.floor & inl & ~el, g.floor & ~inl & ~el
    assert hit.sum() >= 5 and miss.sum() >= 20, (hit.sum(), miss.sum())
    avg, _, seg, _ = view.frames(2, 1)
    assert _same(avg[hit], _le(sd)), avg[hit]
    assert _same(avg[miss], 0.0), avg[miss]
    assert _area_shadow_rays(view, 2) == 0
    return int(hit.sum()), int(miss.sum())


def light_side_scene(two_sided):
    return floor_scene(light=dict(LIGHTS["big"], two_sided=two_sided), name=f"floor-back-{two_sided}")


def check_light_back(view, two_sided):
    """The camera looks down on the light's back: exactly 0 for the one-sided light, exactly Le for the two-sided one,
    and the path ends there whatever `bounces` allows (the lit floor beneath adds nothing)."""
    g = Geometry(view.sd)
    px = g.light_first & ~g.edge
    assert px.sum() >= 10 and (g.light_cos[px] < 0).all()
    for bounces in (1, 2, 3):
        avg = view.frames(bounces, 1)[0]
        assert _same(avg[px], _le(view.sd) if two_sided else 0.0), (bounces, avg[px])
    return int(px.sum())


def behind_scene(variant):
    """"below": the floor lies above the downward-emitting big light (N.L < 0 as well).  "up": the high panel hangs
    over the floor but emits upwards (edges swapped), so N.L > 0 and only the light's own cosine says no."""
    if variant == "below":
        return floor_scene(light=dict(LIGHTS["big"], corner=np.array([-1.0, -0.6, -1.0], F)), name="floor-behind-below")
    up = scenes.ceiling_light(edge_u=(0.0, 0.0, 3.0), edge_v=(3.0, 0.0, 0.0), **HIGH)
    return floor_scene(light=up, name="floor-behind-up")


def check_light_from_behind(view, variant):
    """A one-sided light that faces away from the floor adds nothing to it and casts no shadow ray."""
    g = Geometry(view.sd)
    _, _, _, n, _, _, _ = E.light_geometry(view.sd.area_light)
    assert g.floor.sum() >= 60 and not g.light_first.any()
    assert n[1] == (1.0 if variant == "up" else -1.0)
    for bounces in (1, 2):
        avg = view.frames(bounces, 1)[0]
        assert _same(avg, 0.0), (bounces, np.abs(avg).max())
        assert _area_shadow_rays(view, bounces) == 0
    return int(g.floor.sum())


BLOCKER = (0.0, 1.7, 1.0, 1.0)     # under a small light (x, z in [-0.2, 0.2] + (0, 1) at y = 2): from any floor point
                                   # the light's outline projects at most 0.2 + 0.15 * 4.2 = 0.83 from the centre


def blocked_scene():
    """The small light moved half a unit on, where no camera ray crosses it (the row that would passes in front)."""
    return floor_scene(light=dict(LIGHTS["small"], corner=np.array([-0.2, 2.0, 0.8], F)), blocker=BLOCKER,
                       name="floor-blocked")


def check_blocked(view):
    """A quad that hides the whole light from every floor point: every floor pixel is exactly 0 at bounces = 1, and
    the light still costs one shadow ray per lit hit (floor and blocker top alike: both face the light)."""
    g = Geometry(view.sd, margin=1e-4)     # counting hits: float32 decides alike 1e-4 from an outline (errors ~1e-6)
    c, eu, ev, _, _, _, _ = E.light_geometry(view.sd.area_light)
    bx, by, bz, bh = BLOCKER
    for corner in (c, c + eu, c + ev, c + eu + ev):             # the cover, from the floor's four corners
        for fx in (-HALF, HALF):
            for fz in (-HALF, HALF):
                o = np.array([fx, 0.0, fz])
                p = o + (corner - o) * (by / corner[1])
                assert abs(p[0] - bx) < bh - 0.05 and abs(p[2] - bz) < bh - 0.05
    assert g.floor.sum() >= 60 and g.blocked.sum() >= 1 and not g.light_first.any()
    assert not g.edge.any()     # no primary ray grazes an outline: the hit count below is the same in float32
    avg, _, seg, _ = view.frames(1, 1)
    assert _same(avg[g.floor], 0.0), np.abs(avg[g.floor]).max()
    hits = int((g.floor | g.blocked).sum())
    assert seg == W * H
    assert _area_shadow_rays(view, 1) == hits, (_area_shadow_rays(view, 1), hits)
    return hits


def seen_scene():
    """The big light turned over (edges swapped): the camera looks down on its emitting side."""
    up = scenes.ceiling_light(corner=(-1.0, 0.6, -1.0), edge_u=(0.0, 0.0, 2.0), edge_v=(2.0, 0.0, 0.0),
                              radiance=(3.0, 2.0, 1.0))
    return floor_scene(light=up, name="floor-seen")


def check_seen_directly(view):
    """A camera ray that reaches the light's emitting side first returns exactly Le (weight 1: no strategy sampled
    it), whatever `bounces` allows beyond; the floor, which the light faces away from, stays black."""
    g = Geometry(view.sd)
    px = g.light_first & ~g.edge
    assert px.sum() >= 10 and (g.light_cos[px] > 0).all() and g.floor.sum() >= 60
    for bounces in (1, 3):
        avg = view.frames(bounces, 1)[0]
        assert _same(avg[px], _le(view.sd)), (bounces, avg[px])
        assert _same(avg[g.floor], 0.0)
    return int(px.sum())


# ---- glass
GLASS_CAMS = {"front": (CAM_POS, CAM_TARGET), "below": ((0.3, -1.5, -2.5), (0.0, 0.0, 0.3))}
K_MARGIN = 1e-3     # |k| of refract() below this: the choice between the zero direction and a grazing one may flip


def glass_scene(camera):
    return floor_scene(kind=_lib.MAT_DIELECTRIC, sky=sky_ramp(), cam=GLASS_CAMS[camera], name="glass-" + camera)


def _sky_seen(sd, g, O, D):
    """The radiance a secondary ray (float64 origin O, direction D as the split hands it to the ray constructor) of the
    glass scene returns at the path's last segment: 0 where it meets the quad again (a dielectric's last segment is
    its emission, 0), else the sky in the ray's own, renormalised direction -- the zero direction stays zero, for
    which the lookup reads atan2(0, 0) = 0 and acos(0) = pi / 2: u = v = 0.5 (Camera.cpp:45-48).
    Also returns the tolerance's texel shift per unit of direction error (see check_glass)."""
    lo = np.array([-HALF, g.floor_y, -HALF])
    _, again, _ = _rect_hit(O, D, lo, np.array([2 * HALF, 0.0, 0.0]), np.array([0.0, 0.0, 2 * HALF]))
    Dn = R.ray_ctor_dir(D.astype(F))
    sky = R.sample_sky(sd.sky, Dn).astype(np.float64)
    r = np.sqrt(Dn[:, 0].astype(np.float64) ** 2 + Dn[:, 2].astype(np.float64) ** 2)
    h, w = sd.sky.shape[:2]
    with np.errstate(divide="ignore"):
        shift = np.where(r > 0, w / (2 * np.pi * np.where(r > 0, r, 1.0)) + h / np.pi, 0.0)
    taps = R.sky_taps(Dn, w, h)
    return np.where(again[:, None], 0.0, sky), np.where(again, 0.0, shift), again, taps


def check_glass(view, camera):
    """bounces = 2 on the DIELECTRIC quad under the sky ramp: every tested pixel equals
    fres sky(R) + (1 - fres) sky(T) with R, T, fres from estimator_ref.glass; bounces = 1 gives exactly 0.

    Tolerance, derived (not tuned): the device computes the split in float32, each quantity within
    scene_ref.CLOSED_TOL (relative) of the float64 one -- the bound scene_ref gives a float32 closed form of this
    length.  A direction off by CLOSED_TOL turns by at most that angle, which moves the lookup by at most
    CLOSED_TOL * (w / (2 pi r) + h / pi) texels (r = the direction's horizontal length: the azimuth's lever), and the
    bilinear lookup of the ramp then changes by at most that many times the ramp's largest texel-to-texel step.  With
    the relative error of fres and of the blend itself:
        tol = CLOSED_TOL * (|expected| + step * (fres shift_R + (1 - fres) shift_T))  per channel.
    Pixels whose refract() k lies within K_MARGIN of 0 are not tested (the zero direction against a grazing one)."""
    sd = view.sd
    g = Geometry(sd)
    px = np.flatnonzero(np.isfinite(g.t_floor) & (np.abs(g.I[:, 0]) < HALF - MARGIN) & (np.abs(g.I[:, 2]) < HALF - MARGIN))
    assert px.size >= 60
    I, D, N = g.I[px], g.D[px], g.N[px]
    s = E.glass(D, N)
    eps = float(R.EPSILON)
    refl, sh_r, again_r, taps_r = _sky_seen(sd, g, I + N * eps, s["R"])
    refr, sh_t, again_t, taps_t = _sky_seen(sd, g, I - N * eps, s["T"])
    exp = E.glass_combine(s, refl, refr)
    sky = sd.sky.astype(np.float64)
    step = max(np.abs(np.diff(sky, axis=0)).max(), np.abs(np.diff(sky, axis=1)).max())
    tol = R.CLOSED_TOL * (np.abs(exp) + step * (s["fres"] * sh_r + (1 - s["fres"]) * sh_t)[:, None])
    ok = np.abs(s["k_refract"]) > K_MARGIN
    w = sd.sky.shape[1]
    for taps, again in ((taps_r, again_r), (taps_t, again_t)):   # no tested lookup touches the ramp's seam
        assert (taps[2][~again] < w - 1).all()
    zero_dir = (s["k_refract"] < 0) & ok
    if camera == "front":       # entering rays: both the refracted direction and the zero direction occur
        assert (D[:, 1] < 0).all() and not again_r.any()
        assert zero_dir.sum() >= 10 and (~zero_dir & ok).sum() >= 10, (zero_dir.sum(), (~zero_dir & ok).sum())
        assert (exp[ok].min(0) > 0.1).all()
    else:                        # back-face hits: cosTheta clamps to 0, fres = 1, the reflection meets the quad again
        assert (D[:, 1] > 0).all() and again_r.all() and (s["fres"] == 1.0).all() and not zero_dir.any()
        assert (exp == 0).all()
    got = view.frames(2, 1)[0][px].astype(np.float64)
    err = np.abs(got - exp)
    assert (err[ok] <= tol[ok]).all(), (camera, float((err[ok] / np.maximum(tol[ok], 1e-300)).max()), got[ok][:3], exp[ok][:3])
    last = view.frames(1, 1)[0]
    assert _same(last[px], 0.0)
    return float((err[ok] / np.maximum(tol[ok], 1e-300)).max()) if camera == "front" else 0.0


def exact_scenes():
    """Every scene of this file, by name, for the device = oracle comparison."""
    out = {f"stat-{l}-{r}-{m}": stat_scene(l, r, m) for l, r, m in STAT_CASES}
    out.update({"mirror": mirror_scene(), "back-one": light_side_scene(False), "back-two": light_side_scene(True),
                "behind-below": behind_scene("below"), "behind-up": behind_scene("up"), "blocked": blocked_scene(), "seen": seen_scene(),
                "glass-front": glass_scene("front"), "glass-below": glass_scene("below")})
    return out


def scene_flags(sd):
    return FLAGS | (_lib.FLAG_SKYBOX if sd.sky is not None else 0)


# ------------------------------------------------------------------------------------------------ the device
pytestmark = pytest.mark.gpu


class GpuView:
    """One scene at 16 x 12 on the shared context; whichever view is used puts its scene back first."""
    _loaded = None

    def __init__(self, ctx, sd):
        self.ctx, self.sd = ctx, sd

    def load(self):
        if GpuView._loaded is not self:
            from helpers import gpu_scene
            self.ctx.set_postfx(None)
            gpu_scene(self.ctx, self.sd, W, H)
            GpuView._loaded = self
            SQ.GpuView._loaded = None       # the scene-query views share this context
        return self.ctx

    def without_light(self):
        return GpuView(self.ctx, dataclasses.replace(self.sd, area_light=None))

    def frames(self, bounces, k, frame_index=0):
        ctx = self.load()
        ctx.reset_accumulation(full=True)
        avg, rgb8, st = ctx.render(W, H, k, bounces, scene_flags(self.sd), 0, frame_index, SEED)
        return avg[:, :3].copy(), rgb8.copy(), int(st.segments), int(st.shadow_rays)

    def mean(self, bounces, n):
        total = np.zeros((W * H, 3), np.float64)
        for f0 in range(0, n, CHUNK):
            total += self.frames(bounces, CHUNK, f0)[0].astype(np.float64)
        return total / (n // CHUNK)


@pytest.fixture(autouse=True)
def _forget_view():
    yield
    GpuView._loaded = None


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("light,rough,metal", STAT_CASES)
def test_area_light_expectation(gpu_ctx, light, rough, metal, bounces):
    check_statistical(GpuView(gpu_ctx, stat_scene(light, rough, metal)), stat_ref(light, rough, metal), bounces)


def test_mirror_floor_returns_le_exactly(gpu_ctx):
    check_mirror(GpuView(gpu_ctx, mirror_scene()))


@pytest.mark.parametrize("two_sided", [False, True])
def test_light_back(gpu_ctx, two_sided):
    check_light_back(GpuView(gpu_ctx, light_side_scene(two_sided)), two_sided)


@pytest.mark.parametrize("variant", ["below", "up"])
def test_light_from_behind(gpu_ctx, variant):
    check_light_from_behind(GpuView(gpu_ctx, behind_scene(variant)), variant)


def test_fully_blocked_light(gpu_ctx):
    check_blocked(GpuView(gpu_ctx, blocked_scene()))


def test_light_seen_directly(gpu_ctx):
    check_seen_directly(GpuView(gpu_ctx, seen_scene()))


@pytest.mark.parametrize("camera", ["front", "below"])
def test_glass(gpu_ctx, camera):
    print("largest error / tolerance:", check_glass(GpuView(gpu_ctx, glass_scene(camera)), camera))


def test_device_equals_oracle(gpu_ctx, oracle_mod):
    """Every scene of this file at bounces 1 and 2, 2 frames: image, RGB8 and ray counts bit for bit."""
    for name, sd in exact_scenes().items():
        view = GpuView(gpu_ctx, sd)
        osc = oracle_mod.OracleScene(sd, W, H)
        for bounces in (1, 2):
            a_o, r_o, _, s_o = osc.render(W, H, spp=2, bounces=bounces, flags=scene_flags(sd), seed=SEED)
            a_g, r_g, seg, sh = view.frames(bounces, 2)
            assert np.array_equal(SQ.bits(a_o[:, :3]), SQ.bits(a_g)), (name, bounces)
            assert np.array_equal(r_o, r_g), (name, bounces)
            assert (int(s_o.segments), int(s_o.shadow_rays)) == (seg, sh), (name, bounces)
