"""Degenerate geometry and exact ties, generated (no fixture files): meshes with duplicate triangles, coincident
centroids, zero-area triangles, a zero-thickness box and fewer than eight triangles; scenes with coincident, mirrored
and non-uniformly scaled instances; rays with exact +0.0 / -0.0 direction components that pass exactly through shared
vertices and edges; and a numpy brute force that restates the hit rule on its own (prt_traverse.h: closest t, an
equal t to the smaller instance, then to the LARGER prim; a hit needs t < tmax).

Used by tests/test_degenerate_ref.py (oracle and host builders, CPU) and tests/test_gpu_degenerate.py (HIP traversal
and device builders).  Importable without a GPU."""
import dataclasses

import numpy as np

from prt import scenes

F32 = np.float32
FAR = F32(1e30)


def soup_mesh(tris):
    """A scenes.Mesh from a (T, 3, 3) float32 triangle array: unshared vertices, the constant vertex normal (0, 1, 0),
    face normals normalize(cross(e1, e2)) in float32 with the non-finite ones of zero-area triangles set to 0, the
    texture ids of scenes.config_heightfield.  The texture coordinates depend on the primitive index, so two
    coincident triangles shade differently and a frame shows which of them won a tie."""
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 3, 3)
    T = tris.shape[0]
    tri4 = np.zeros((3 * T, 4), F32)
    tri4[:, :3] = tris.reshape(-1, 3)
    n4 = np.zeros((3 * T, 4), F32)
    n4[:, 1] = 1.0
    p = np.arange(T, dtype=np.float64)
    a, b = (p * 0.6180339887) % 0.8, (p * 0.3819660113) % 0.8
    uv = np.stack([np.stack([a, b], 1), np.stack([a + 0.15, b], 1), np.stack([a, b + 0.15], 1)], 1).astype(F32)
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F32)
    d = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        fn = (c * (F32(1.0) / np.sqrt(d))[:, None]).astype(F32)
    fn[~np.isfinite(fn).all(axis=1)] = 0.0
    m = scenes.Mesh(tri4.reshape(-1).copy(), n4.reshape(-1).copy(), uv.reshape(-1).copy(),
                    np.arange(3 * T, dtype=np.int32), tris.reshape(-1).copy(), fn.reshape(-1).copy())
    m.albedo, m.normal, m.metalness, m.emission = 0, 1, 2, 3
    return m


def mesh_tris(m):
    """(T, 3, 3) float32 corners of a scenes.Mesh's fat triangles."""
    return np.asarray(m.triangles, F32).reshape(-1, 3, 4)[:, :, :3].copy()


def _heightfield_tris(nx, nz, extent):
    return mesh_tris(scenes.heightfield(nx, nz, extent))


def doubled():
    """A 12x10 heightfield of extent 2, included twice: every triangle has a coincident copy 240 prims above it."""
    h = _heightfield_tris(12, 10, 2.0)
    return np.concatenate([h, h])


def pile(n=40):
    """n identical triangles in the plane y = 1: one centroid, one box, one Morton code."""
    t = np.array([[-1.5, 1.0, -1.5], [-1.5, 1.0, 1.5], [1.5, 1.0, -1.5]], F32)
    return np.tile(t, (n, 1, 1))


def zero_area():
    """Three collinear points, three equal points, two equal points, around y = 2."""
    return np.array([[[-1.0, 2.0, 0.0], [0.0, 2.0, 0.0], [1.0, 2.0, 0.0]],
                     [[0.5, 2.0, 0.5], [0.5, 2.0, 0.5], [0.5, 2.0, 0.5]],
                     [[-0.5, 2.0, 1.0], [-0.5, 2.0, 1.0], [0.5, 2.0, -1.0]]], F32)


def lattice(n=8, y=-1.0):
    """n x n quads with integer coordinates in the plane y = const (a box of zero thickness; every intersection
    with an axis-parallel ray through a half-integer grid is computed exactly, so shared vertices tie 6 ways)."""
    ix, iz = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x0, z0 = (ix.reshape(-1) - n // 2).astype(F32), (iz.reshape(-1) - n // 2).astype(F32)
    yy = np.full_like(x0, y)
    P = lambda dx, dz: np.stack([x0 + dx, yy, z0 + dz], 1)
    t1 = np.stack([P(0, 0), P(0, 1), P(1, 0)], 1)
    t2 = np.stack([P(1, 0), P(0, 1), P(1, 1)], 1)
    return np.stack([t1, t2], 1).reshape(-1, 3, 3).astype(F32)


def degenerate_soup():
    """(tris, ranges): the concatenation of the pieces and the prim range of each as {name: (first, end)}."""
    parts = [("doubled", doubled()), ("pile", pile()), ("zero_area", zero_area()), ("lattice", lattice())]
    ranges, at = {}, 0
    for name, t in parts:
        ranges[name] = (at, at + t.shape[0])
        at += t.shape[0]
    return np.concatenate([t for _, t in parts]).astype(F32), ranges


def tiny_pieces():
    """Five pieces of a 6x5 heightfield (extent 2) of 1, 2, 7, 8 and 9 triangles: strips side by side along x."""
    h = _heightfield_tris(6, 5, 2.0)
    return [h[10 * k:10 * k + n].copy() for k, n in enumerate((1, 2, 7, 8, 9))]


def big_quad():
    """Two triangles covering [-2, 2]^2 (the 1x1 heightfield of extent 2)."""
    return _heightfield_tris(1, 1, 2.0)


def slivers(n=400, seed=2):
    """n long thin slivers at random angles across a square, every box spanning most of it (the triangles of
    tests/test_bvh_build.py::test_spatial_splits_duplicate_within_budget): the spatial-split builder cuts them, so its
    tree holds more records than triangles."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, np.pi, n)
    c = rng.uniform(-1, 1, (n, 2))
    d = np.stack([np.cos(a), np.sin(a)], 1)
    p0, p1 = c - 6 * d, c + 6 * d
    w = 0.01 * np.stack([-d[:, 1], d[:, 0]], 1)
    P = np.zeros((n, 3, 3), F32)
    P[:, 0, [0, 2]], P[:, 1, [0, 2]], P[:, 2, [0, 2]] = p0, p1, p1 + w
    P[:, :, 1] = rng.uniform(0, 0.05, n)[:, None]
    return P


def _scene(meshes, instances, name, cam_pos=(0.3, 3.0, -5.0)):
    base = scenes.config_small(4, 4)  # lights, sky, textures
    return dataclasses.replace(base, meshes=meshes, instances=instances, cam_pos=np.array(cam_pos, F32),
                               cam_target=np.zeros(3, F32), name=name)


def _xf(diag=(1.0, 1.0, 1.0), t=(0.0, 0.0, 0.0)):
    M = np.eye(4, dtype=F32)
    M[0, 0], M[1, 1], M[2, 2] = diag
    M[:3, 3] = t
    return M


def soup1():
    """The soup, one identity instance."""
    return _scene([soup_mesh(degenerate_soup()[0])], [(0, _xf())], "soup1")


def soup_identity(n):
    """The soup at n coincident identity instances (the brute force covers these)."""
    return _scene([soup_mesh(degenerate_soup()[0])], [(0, _xf()) for _ in range(n)], f"soup-identity-{n}")


def soup4():
    """The soup at four instances: two identity transforms (instance 1 coincides with instance 0 and must always
    lose), one mirrored (diag(-1, 1, 1), x + 0.5), one non-uniformly scaled (diag(2, 0.5, 1), y - 0.5)."""
    inst = [(0, _xf()), (0, _xf()), (0, _xf((-1.0, 1.0, 1.0), (0.5, 0.0, 0.0))),
            (0, _xf((2.0, 0.5, 1.0), (0.0, -0.5, 0.0)))]
    return _scene([soup_mesh(degenerate_soup()[0])], inst, "soup4")


def tiny():
    """Five meshes of 1, 2, 7, 8 and 9 triangles, one identity instance each."""
    ms = [soup_mesh(t) for t in tiny_pieces()]
    return _scene(ms, [(i, _xf()) for i in range(len(ms))], "tiny")


def coincident70():
    """70 coincident identity instances of a 2-triangle mesh: more than the linear instance list holds, so the
    instance BVH is walked; every hit ties 70 ways and must report instance 0."""
    return _scene([soup_mesh(big_quad())], [(0, _xf()) for _ in range(70)], "coincident70")


def edge_rays(seed=1):
    """(O, D, slices): random rays towards the soup; rays straight down (from y = 3) and straight up (from y = -3)
    through a 0.5-spaced grid over [-4, 4]^2, their zero direction components +0.0 or -0.0 in turn (the slab tests'
    safercp -> 1e30 branch; the grid passes exactly through heightfield and lattice vertices and edges); +x rays
    across the heightfield with two zero components.  The total is no multiple of 64.  slices: one ray, 63 and 65
    rays, taken from the axis-parallel families."""
    rng = np.random.default_rng(seed)
    n = 4000
    O = rng.uniform(-3, 3, (n, 3))
    O[:, 1] = rng.uniform(0.5, 4.0, n)
    tgt = rng.uniform(-2.5, 2.5, (n, 3))
    tgt[:, 1] = rng.uniform(-0.5, 0.5, n)
    fam_O, fam_D = [O.astype(F32)], [(tgt - O).astype(F32)]
    g = np.arange(-4.0, 4.25, 0.5)
    gx, gz = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    k = np.arange(gx.size)
    sx, sz = np.where(k & 1, -0.0, 0.0), np.where(k & 2, -0.0, 0.0)  # signed zeros
    for y0, dy in ((3.0, -1.0), (-3.0, 1.0)):
        fam_O.append(np.stack([gx, np.full_like(gx, y0), gz], 1).astype(F32))
        fam_D.append(np.stack([sx, np.full_like(gx, dy), sz], 1).astype(F32))
    zz, yy = [a.reshape(-1) for a in np.meshgrid(np.linspace(-2.0, 2.0, 21), np.linspace(-0.35, 0.35, 8),
                                                 indexing="ij")]
    k = np.arange(zz.size)
    fam_O.append(np.stack([np.full_like(zz, -3.0), yy, zz], 1).astype(F32))
    fam_D.append(np.stack([np.ones_like(zz), np.where(k & 1, -0.0, 0.0), np.where(k & 2, -0.0, 0.0)], 1).astype(F32))
    O, D = np.concatenate(fam_O), np.concatenate(fam_D)
    assert O.shape[0] % 64 != 0
    centre = n + gx.size // 2  # the down ray through the origin
    up = n + gx.size  # the first up ray
    slices = {"one": slice(centre, centre + 1), "s63": slice(n, n + 63), "s65": slice(up + 100, up + 165)}
    return O, D, slices


def brute_force(tris, O, D, n_identity_instances=1, tmax=None):
    """Every ray against every triangle, numpy float32: Moeller-Trumbore in mt_test's operation order (each +, -, *,
    / rounded once), then the hit rule stated directly -- the smallest t with 0 < t < tmax; among the triangles at
    that t the largest prim; n coincident identity instances all tie, so the instance is 0.  Returns (t, u, v, prim,
    inst, ties): the hit records (a miss is t = tmax, u = v = 0, prim = inst = 0) and, per ray, how many distinct
    triangles share the best t (0 on a miss).  Identity instances only: their instance-space rays are the world
    rays, exactly."""
    assert n_identity_instances >= 1
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 3, 3)
    O, D = np.ascontiguousarray(O, F32), np.ascontiguousarray(D, F32)
    R = O.shape[0]
    tm = np.full(R, FAR, F32) if tmax is None else np.ascontiguousarray(tmax, F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # tinybvh_normalize: D * (1 / sqrt(x^2 + y^2 + z^2))
        ln = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
        D = (D * np.where(ln == 0, F32(0), F32(1) / ln)[:, None]).astype(F32)
        v0, e1, e2 = tris[:, 0], (tris[:, 1] - tris[:, 0]).astype(F32), (tris[:, 2] - tris[:, 0]).astype(F32)
        Dx, Dy, Dz = (D[:, k, None] for k in range(3))
        Ox, Oy, Oz = (O[:, k, None] for k in range(3))
        e1x, e1y, e1z = (e1[None, :, k] for k in range(3))
        e2x, e2y, e2z = (e2[None, :, k] for k in range(3))
        hx = Dy * e2z - Dz * e2y
        hy = Dz * e2x - Dx * e2z
        hz = Dx * e2y - Dy * e2x
        sx, sy, sz = Ox - v0[None, :, 0], Oy - v0[None, :, 1], Oz - v0[None, :, 2]
        det = (e1x * hx + e1y * hy) + e1z * hz
        inv = F32(1) / det
        u = ((sx * hx + sy * hy) + sz * hz) * inv
        qx = sy * e1z - sz * e1y
        qy = sz * e1x - sx * e1z
        qz = sx * e1y - sy * e1x
        v = ((Dx * qx + Dy * qy) + Dz * qz) * inv
        t = ((e2x * qx + e2y * qy) + e2z * qz) * inv
        assert t.dtype == F32 and u.dtype == F32
        ok = ((det <= F32(-0.000001)) | (det >= F32(0.000001))) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1)
        ok &= (t > 0) & (t < tm[:, None])
    tt = np.where(ok, t, np.inf).astype(F32)
    best = tt.min(axis=1)
    hit = np.isfinite(best)
    at_best = ok & (tt == best[:, None])
    ties = at_best.sum(axis=1).astype(np.int32)
    prim = np.where(hit, tris.shape[0] - 1 - np.argmax(at_best[:, ::-1], axis=1), 0).astype(np.uint32)
    r = np.arange(R)
    out_t = np.where(hit, best, tm).astype(F32)
    out_u = np.where(hit, u[r, prim], F32(0)).astype(F32)
    out_v = np.where(hit, v[r, prim], F32(0)).astype(F32)
    return out_t, out_u, out_v, prim, np.zeros(R, np.uint32), ties


def brute_force_meshes(meshes_tris, O, D, tmax=None):
    """brute_force over several meshes at one identity instance each (instance i = mesh i): the closest t, an
    equal t to the smaller instance.  Returns (t, u, v, prim, inst)."""
    out = None
    for i, tris in enumerate(meshes_tris):
        t, u, v, prim, _, ties = brute_force(tris, O, D, 1, tmax)
        if out is None:
            out = [t, u, v, prim, np.zeros(t.shape[0], np.uint32)]
            hit_any = ties > 0
            continue
        better = (ties > 0) & (~hit_any | (t < out[0]))
        for k, a in enumerate((t, u, v, prim, np.full(t.shape[0], i, np.uint32))):
            out[k] = np.where(better, a, out[k])
        hit_any |= ties > 0
    return tuple(out)
