"""Deformed copies of a scenes.Mesh for the mesh-update tests (prt_update_mesh): the vertex positions move, the
topology (indices, texture coordinates, texture ids) stays, and everything derived from the positions is recomputed
consistently -- `triangles` and `vertices` from the new positions, `face_normals` as scenes._mesh_from_grid computes
them (normalize(cross(e1, e2)) in float32; a zero-area triangle's non-finite normal becomes 0), `fixed_normals` as
the normalised sum of the adjacent faces' cross products per vertex ((0, 1, 0) where that sum vanishes)."""
import dataclasses

import numpy as np

F32 = np.float32


def with_positions(mesh, P):
    """`mesh` with its vertices at P ((V, 3), any float type; rounded to float32 first)."""
    P = np.ascontiguousarray(P, F32).reshape(-1, 3)
    idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)
    assert P.shape[0] == np.asarray(mesh.vertices).size // 3
    T = idx.shape[0]
    tri4 = np.zeros((3 * T, 4), F32)
    tri4[:, :3] = P[idx.reshape(-1)]
    v0, v1, v2 = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
    e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        fn = (c * (F32(1.0) / np.sqrt(d.astype(F32)))[:, None]).astype(F32)
    fn[~np.isfinite(fn).all(axis=1)] = 0.0
    acc = np.zeros((P.shape[0], 3), np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c64 = np.cross(v1.astype(np.float64) - v0, v2.astype(np.float64) - v0)
        for k in range(3):
            np.add.at(acc, idx[:, k], c64)
        ln = np.linalg.norm(acc, axis=1)
        vn = acc / ln[:, None]
    vn[~(ln > 0) | ~np.isfinite(vn).all(axis=1)] = (0.0, 1.0, 0.0)
    n4 = np.zeros((3 * T, 4), F32)
    n4[:, :3] = vn.astype(F32)[idx.reshape(-1)]
    return dataclasses.replace(mesh, triangles=tri4.reshape(-1).copy(), fixed_normals=n4.reshape(-1).copy(),
                               fixed_uvs=np.array(mesh.fixed_uvs, F32, copy=True),
                               indices=np.array(mesh.indices, np.int32, copy=True), vertices=P.reshape(-1).copy(),
                               face_normals=fn.reshape(-1).copy())


def positions(mesh):
    return np.asarray(mesh.vertices, np.float64).reshape(-1, 3).copy()


def sine_twist(mesh, amp=1.0, twist=0.6, phase=0.0):
    """Every vertex displaced by a sine of amplitude `amp` (y by x and z, x by z), then turned about the vertical
    axis by `twist` radians per unit of distance from it: with amp of the order of the mesh's extent no box of the
    original tree still holds its triangles."""
    P = positions(mesh)
    x, y, z = P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy()
    y = y + amp * np.sin(1.3 * x + 0.7 * z + phase)
    x = x + 0.5 * amp * np.sin(0.9 * z + 2.0 * phase)
    a = twist * np.hypot(x, z)
    ca, sa = np.cos(a), np.sin(a)
    return with_positions(mesh, np.stack([ca * x - sa * z, y, sa * x + ca * z], 1))


def scaled(mesh, s):
    """Every vertex times s (about the origin): the mesh's extent changes by that factor."""
    return with_positions(mesh, positions(mesh) * float(s))


def travelling_sine(mesh, amp, t=0.0, k=2.0):
    """y displaced by amp * sin(k * (x + z) - t): the wave of scripts/mesh_update_time.py's tree-quality table."""
    P = positions(mesh)
    P[:, 1] += amp * np.sin(k * (P[:, 0] + P[:, 2]) - t)
    return with_positions(mesh, P)
