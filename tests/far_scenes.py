"""Small geometry seen from far away, and geometry at large coordinates, generated (no fixture files): the scales at
which the Node8 child test fma(q, b, a), a = (p - O) * rD, b = 2^(e-127) * rD, loses the quantised byte q -- once a
node's extent is below about half an ulp of the ray's distance to it, all eight child slots decode to the same slab
interval, the unoccupied ones (inverted box 255 .. 0) included.  prt_node8.h: a visit hands on occupied slots only.

  ripple(s, c)        an 800-triangle patch of extent 2 s centred at c
  PLACEMENTS          (s, |c| / s, camera distance / s); `dagger`: the raw slab mask names unoccupied slots there
  placement_rays      4,000 rays from the far camera at random points of 1.15 x the footprint, 500 straight down
                      through grid vertices (signed-zero components), 499 along +x: 4,999, no multiple of 64
  telephoto           a camera at that distance whose window is 1.2 x the patch, around the patch
  field(n)            n translated instances of a 2-triangle quad in a 20 x 2 x 20 box (the instance BVH)
  blocker()           the patch lit by a point light 1e5 units away with a second patch 10 units in front of the light

Used by tests/test_traverse_scales.py (CPU: tests/cpp/trav_check.cpp) and tests/test_gpu_traverse_scales.py.
Importable without a GPU."""
import dataclasses

import numpy as np

import degenerate as dg

F32 = np.float32
VIEW = np.array([0.3, 0.8, -0.52])       # from the target towards the camera (length 1.0002)
CENTRE_DIR = np.array([0.6, 0.48, 0.64])  # unit: where an off-origin patch is centred
NQ = 20                                   # quads per side of the patch


@dataclasses.dataclass(frozen=True)
class Placement:
    s: float          # scale of the patch
    centre: float     # |c| / s
    dist: float       # camera distance / s
    dagger: bool      # the raw slab mask must name an unoccupied slot here

    @property
    def c(self):
        return self.s * self.centre * CENTRE_DIR

    @property
    def cam(self):
        return self.c + self.s * self.dist * VIEW


PLACEMENTS = {
    "A": Placement(1.0, 0.0, 3.0, False),
    "B": Placement(1.0, 0.0, 3e4, True),
    "C": Placement(1.0, 0.0, 1e5, True),
    "D": Placement(1.0, 1e3, 1e5, True),
    "E": Placement(1e3, 1e3, 1e5, True),
    "F": Placement(1.0, 0.0, 1e6, True),
}
POINT_DIST = 5.0  # placement P: eight triangles whose corners all equal the origin, seen from this far


def _grid():
    g = np.linspace(-1.0, 1.0, NQ + 1)
    x, z = np.meshgrid(g, g, indexing="ij")
    return np.stack([x, 0.3 * np.sin(3 * x) * np.cos(2 * z), z], -1)  # (21, 21, 3) float64


def ripple_tris(s=1.0, c=(0.0, 0.0, 0.0)):
    """(800, 3, 3) float32: a 20 x 20-quad height field over [-1, 1]^2 with y = 0.3 sin 3x cos 2z, every vertex
    (float32)(c + s * p) computed in float64."""
    P = (np.asarray(c, np.float64) + s * _grid()).astype(F32)
    a, b, cc, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t = np.stack([np.stack([a, b, cc], -2), np.stack([cc, b, d], -2)], 2)  # (20, 20, 2, 3, 3)
    return np.ascontiguousarray(t.reshape(-1, 3, 3))


def ripple(s=1.0, c=(0.0, 0.0, 0.0)):
    return dg.soup_mesh(ripple_tris(s, c))


def point_tris():
    return np.zeros((8, 3, 3), F32)


def placement_tris(name):
    if name == "P":
        return point_tris()
    p = PLACEMENTS[name]
    return ripple_tris(p.s, p.c)


def _signed_zero(k, bit):
    return np.where(k & bit, -0.0, 0.0)


def placement_rays(name, seed=7):
    """(O, D) float32, 4,999 rays: see the module docstring.  P: 4,000 rays from random points at distance 5 with
    D = -O (through the point, exactly), then the two axis-parallel families through and beside it."""
    rng = np.random.default_rng(seed)
    n = 4000
    if name == "P":
        s, c, dist = 1.0, np.zeros(3), POINT_DIST
        o = rng.normal(size=(n, 3))
        o = (dist * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(F32)
        fam_O, fam_D = [o], [-o]
        gv = np.zeros((NQ + 1, NQ + 1, 3), F32)
        gv[..., 0], gv[..., 2] = np.meshgrid(np.linspace(-1e-6, 1e-6, NQ + 1), np.linspace(-1e-6, 1e-6, NQ + 1), indexing="ij")
    else:
        p = PLACEMENTS[name]
        s, c, dist = p.s, p.c, p.dist
        tgt = c + s * 1.15 * np.stack([rng.uniform(-1, 1, n), np.zeros(n), rng.uniform(-1, 1, n)], 1)
        cam = np.broadcast_to(p.cam, (n, 3))
        fam_O, fam_D = [cam.astype(F32)], [(tgt - cam).astype(F32)]
        gv = (c + s * _grid()).astype(F32)  # the patch's own float32 vertices
    gv = gv.reshape(-1, 3)
    k = np.arange(500)
    v = gv[k % gv.shape[0]]
    fam_O.append(np.stack([v[:, 0], np.full(500, c[1] + s * dist), v[:, 2]], 1).astype(F32))
    fam_D.append(np.stack([_signed_zero(k, 1), np.full(500, -1.0), _signed_zero(k, 2)], 1).astype(F32))
    k = np.arange(499)
    y = c[1] + s * np.linspace(-0.35, 0.35, 499)
    z = c[2] + s * ((k * 0.6180339887) % 1.0 * 2.0 - 1.0)
    fam_O.append(np.stack([np.full(499, c[0] - s * dist), y, z], 1).astype(F32))
    fam_D.append(np.stack([np.ones(499), _signed_zero(k, 1), _signed_zero(k, 2)], 1).astype(F32))
    O, D = np.concatenate(fam_O), np.concatenate(fam_D)
    assert O.shape[0] == 4999 and O.shape[0] % 64 != 0
    return np.ascontiguousarray(O), np.ascontiguousarray(D)


SLICES = {"one": slice(4000, 4001), "s63": slice(10, 73), "s65": slice(4400, 4465)}


def scene_of(tris, name, cam_pos=(0.3, 3.0, -5.0), cam_target=(0.0, 0.0, 0.0)):
    """One identity instance of the triangles, with the lights, sky and textures of the degenerate scenes."""
    sd = dg._scene([dg.soup_mesh(tris)], [(0, dg._xf())], name, cam_pos=cam_pos)
    return dataclasses.replace(sd, cam_target=np.array(cam_target, F32))


def placement_scene(name):
    if name == "P":
        return scene_of(point_tris(), "far-P", cam_pos=POINT_DIST * VIEW / np.linalg.norm(VIEW))
    p = PLACEMENTS[name]
    return scene_of(placement_tris(name), "far-" + name, cam_pos=p.cam, cam_target=p.c)


def telephoto(target, half, cam):
    """{pos, top_left, top_right, bottom_left, right, up, ahead} float32: a camera at `cam` whose screen window is the
    square of half-side `half` around `target`, facing the camera -- the window sits at the geometry, so its corners
    keep their precision and every primary ray crosses the target's small nodes."""
    target, cam = np.asarray(target, np.float64), np.asarray(cam, np.float64)
    ahead = target - cam
    ahead /= np.linalg.norm(ahead)
    right = np.cross([0.0, 1.0, 0.0], ahead)
    right /= np.linalg.norm(right)
    up = np.cross(ahead, right)
    out = {"pos": cam, "top_left": target - half * right + half * up, "top_right": target + half * right + half * up,
           "bottom_left": target - half * right - half * up, "right": right, "up": up, "ahead": ahead}
    return {k: np.ascontiguousarray(v, F32) for k, v in out.items()}


def placement_telephoto(name):
    p = PLACEMENTS[name]
    return telephoto(p.c, 1.2 * p.s, p.cam)


FIELD_HALF = np.array([10.0, 1.0, 10.0])


def field_positions(n, seed=9):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)) * FIELD_HALF


def field(n, seed=9):
    """n instances of the 2-triangle quad scaled to 0.3, translation-only, in a 20 x 2 x 20 box."""
    tris = (dg.big_quad().astype(np.float64) * 0.3).astype(F32)
    inst = [(0, dg._xf(t=tuple(t))) for t in field_positions(n, seed)]
    return dg._scene([dg.soup_mesh(tris)], inst, f"far-field-{n}")


def field_boxes(n, seed=9):
    """(n, 6) float32 world boxes of field(n)'s instances, inflated by bvh_build.cpp's rule."""
    tris = (dg.big_quad().astype(np.float64) * 0.3).astype(F32).reshape(-1, 3)
    lo, hi = tris.min(0).astype(np.float64), tris.max(0).astype(np.float64)
    T = np.array([xf[:3, 3] for _, xf in field(n, seed).instances], np.float64)
    blo, bhi = (T + lo).astype(F32), (T + hi).astype(F32)
    pad = (np.maximum(np.abs(blo), np.abs(bhi)) * F32(1e-6) + F32(1e-7)).astype(F32)
    return np.ascontiguousarray(np.concatenate([blo - pad, bhi + pad], 1), F32)


FIELD_DISTS = (1e6, 1e7)  # both dagger


def field_rays(n, dist, seed=9, rays_seed=13):
    """4,999 rays at field(n): 4,000 from dist * VIEW at random points of the field's box, 500 straight down through
    instance centres from height dist, 499 along +x from dist away."""
    rng = np.random.default_rng(rays_seed)
    m = 4000
    tgt = rng.uniform(-1, 1, (m, 3)) * FIELD_HALF
    cam = np.broadcast_to(dist * VIEW, (m, 3))
    fam_O, fam_D = [cam.astype(F32)], [(tgt - cam).astype(F32)]
    T = np.array([xf[:3, 3] for _, xf in field(n, seed).instances], F32)
    k = np.arange(500)
    v = T[k % n]
    fam_O.append(np.stack([v[:, 0], np.full(500, dist), v[:, 2]], 1).astype(F32))
    fam_D.append(np.stack([_signed_zero(k, 1), np.full(500, -1.0), _signed_zero(k, 2)], 1).astype(F32))
    k = np.arange(499)
    v = T[k % n]
    fam_O.append(np.stack([np.full(499, -dist), v[:, 1], v[:, 2]], 1).astype(F32))
    fam_D.append(np.stack([np.ones(499), _signed_zero(k, 1), _signed_zero(k, 2)], 1).astype(F32))
    O, D = np.concatenate(fam_O), np.concatenate(fam_D)
    assert O.shape[0] % 64 != 0
    return np.ascontiguousarray(O), np.ascontiguousarray(D)


def field_telephoto(dist):
    return telephoto(np.zeros(3), 12.0, dist * VIEW)


LIGHT = 1e5 * VIEW


def blocker(with_far=True):
    """ripple(1, 0) lit by point light 0 moved to LIGHT (its colour scaled by the squared distance ratio, so what it
    adds is of the order of the other lights), and -- with_far -- a second instance of the patch 10 units in front of
    the light: every shadow ray towards that light runs 1e5 units and then crosses the far patch's small nodes."""
    sd = scene_of(ripple_tris(), "far-blocker" if with_far else "far-blocker-open", cam_pos=(0.2, 1.8, -2.2))
    lt = sd.lights
    pp, pc = np.array(lt.point_pos, F32), np.array(lt.point_col, F32)
    pc[0] = (pc[0].astype(np.float64) * (np.linalg.norm(LIGHT) / np.linalg.norm(pp[0].astype(np.float64))) ** 2).astype(F32)
    pp[0] = LIGHT.astype(F32)
    sd = dataclasses.replace(sd, lights=dataclasses.replace(lt, point_pos=pp, point_col=pc))
    if with_far:
        t = LIGHT - 10.0 * VIEW / np.linalg.norm(VIEW)
        sd = dataclasses.replace(sd, instances=list(sd.instances) + [(0, dg._xf(t=tuple(t)))])
    return sd
