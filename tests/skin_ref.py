"""Linear-blend skinning of a scenes.Mesh in numpy: the definition of prt_skin_mesh (include/prt.h, csrc/prt_skin.h)
restated, every operation one float32 rounding in the order the header writes it.  Imports neither the library nor the
oracle.

  B[r][c] = ((w0*M[j0][r][c] + w1*M[j1][r][c]) + w2*M[j2][r][c]) + w3*M[j3][r][c]
  P'_r = ((B[r][0]*P.x + B[r][1]*P.y) + B[r][2]*P.z) + B[r][3]      n_r = (B[r][0]*N.x + B[r][1]*N.y) + B[r][2]*N.z
  N' = n * (1 / sqrt((n.x*n.x + n.y*n.y) + n.z*n.z)), (0, 1, 0) where not finite
  triangles / fixed_normals = (P' / N' of the corner, 0), vertices = P',
  face_normals = normalize(cross(P'[i1] - P'[i0], P'[i2] - P'[i0])), (0, 0, 0) where not finite; the rest stays."""
import dataclasses

import numpy as np

F32 = np.float32


def _normalize(n):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(F32)
        inv = (F32(1.0) / np.sqrt(d).astype(F32)).astype(F32)
        return (n * inv[:, None]).astype(F32)


def skin_vertices(positions, normals, joints, weights, matrices):
    """(P', N'), each (V, 3) float32."""
    P = np.ascontiguousarray(positions, F32).reshape(-1, 3)
    N = np.ascontiguousarray(normals, F32).reshape(-1, 3)
    j = np.asarray(joints, np.int64).reshape(-1, 4)
    w = np.ascontiguousarray(weights, F32).reshape(-1, 4)
    M = np.ascontiguousarray(matrices, F32).reshape(-1, 12)
    assert P.shape == N.shape and j.shape[0] == P.shape[0] == w.shape[0] and 0 <= j.min() and j.max() < M.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        B = (w[:, 0:1] * M[j[:, 0]]).astype(F32) + (w[:, 1:2] * M[j[:, 1]]).astype(F32)
        B = B.astype(F32) + (w[:, 2:3] * M[j[:, 2]]).astype(F32)
        B = (B.astype(F32) + (w[:, 3:4] * M[j[:, 3]]).astype(F32)).astype(F32).reshape(-1, 3, 4)
        Po = np.zeros_like(P)
        n = np.zeros_like(P)
        for r in range(3):
            b = B[:, r]
            Po[:, r] = ((b[:, 0] * P[:, 0] + b[:, 1] * P[:, 1]) + b[:, 2] * P[:, 2]) + b[:, 3]
            n[:, r] = (b[:, 0] * N[:, 0] + b[:, 1] * N[:, 1]) + b[:, 2] * N[:, 2]
    No = _normalize(n)
    No[~np.isfinite(No).all(axis=1)] = (0.0, 1.0, 0.0)
    return Po, No


def skin_mesh(mesh, skin, matrices):
    """`mesh` (a scenes.Mesh) posed by `matrices` ([joints, 12]) through `skin` (anything with positions, normals,
    joints, weights): a new scenes.Mesh with the six arrays prt_update_mesh takes."""
    Po, No = skin_vertices(skin.positions, skin.normals, skin.joints, skin.weights, matrices)
    idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)
    T = idx.shape[0]
    tri4 = np.zeros((3 * T, 4), F32)
    tri4[:, :3] = Po[idx.reshape(-1)]
    n4 = np.zeros((3 * T, 4), F32)
    n4[:, :3] = No[idx.reshape(-1)]
    v0, v1, v2 = Po[idx[:, 0]], Po[idx[:, 1]], Po[idx[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F32)
    fn = _normalize(c)
    fn[~np.isfinite(fn).all(axis=1)] = 0.0
    return dataclasses.replace(mesh, triangles=tri4.reshape(-1).copy(), fixed_normals=n4.reshape(-1).copy(),
                               fixed_uvs=np.array(mesh.fixed_uvs, F32, copy=True),
                               indices=np.array(mesh.indices, np.int32, copy=True), vertices=Po.reshape(-1).copy(),
                               face_normals=fn.reshape(-1).copy())


# ---- poses and weights the skinning tests share

def rigid(angle=0.0, axis=(0.0, 1.0, 0.0), translate=(0.0, 0.0, 0.0), scale=1.0, pivot=(0.0, 0.0, 0.0)):
    """One row-major 3 x 4 matrix (12 float32): a turn by `angle` about `axis` through `pivot`, times `scale`, then
    `translate` (computed in float64, rounded once)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)) * float(scale)
    pv = np.asarray(pivot, np.float64)
    t = pv - R @ pv + np.asarray(translate, np.float64)
    return np.concatenate([R, t[:, None]], 1).astype(F32).reshape(12)


def smooth_weights(positions, joint_count, used=None, seed=5, rigid_part=0.15):
    """Four joints and four weights per vertex, deterministic: `used` (default all) joints spread along x, each vertex
    bound to its four nearest with weights falling off with distance, summing to about 1 (float32).  With fewer than
    four joints the spare influences name joint 0 with weight 0.  The vertices in the lowest `rigid_part` of the x
    range follow the first used joint alone (weight 1): a pose that zeroes that joint's matrix collapses their
    triangles, and only theirs, to zero area."""
    P = np.asarray(positions, np.float64).reshape(-1, 3)
    used = np.arange(joint_count) if used is None else np.asarray(used)
    rng = np.random.default_rng(seed)
    lo, hi = P[:, 0].min(), P[:, 0].max()
    centres = lo + (hi - lo) * (np.arange(len(used)) + 0.5) / len(used)
    centres = centres + rng.uniform(-0.1, 0.1, len(used)) * (hi - lo) / len(used)
    d = np.abs(P[:, 0:1] - centres[None, :])
    k = min(4, len(used))
    near = np.argsort(d, axis=1, kind="stable")[:, :k]
    wt = 1.0 / (np.take_along_axis(d, near, 1) + 0.05 * (hi - lo))
    wt = wt / wt.sum(1, keepdims=True)
    j = np.zeros((P.shape[0], 4), np.uint16)
    w = np.zeros((P.shape[0], 4), F32)
    j[:, :k] = used[near]
    w[:, :k] = wt.astype(F32)
    stiff = P[:, 0] < lo + rigid_part * (hi - lo)
    j[stiff] = used[0]
    w[stiff] = (1.0, 0.0, 0.0, 0.0)
    return j, w


def pose(joint_count, seed, amount=1.0, used=None):
    """[joint_count, 12] float32: every used joint a small turn, scale and shift of its own (seeded), the rest the
    identity."""
    rng = np.random.default_rng(seed)
    M = np.tile(rigid(), (joint_count, 1))
    for j in (range(joint_count) if used is None else used):
        M[j] = rigid(angle=amount * rng.uniform(-0.5, 0.5), axis=rng.normal(size=3) + (0, 2, 0),
                     translate=amount * rng.uniform(-0.3, 0.3, 3), scale=1.0 + amount * rng.uniform(-0.1, 0.1))
    return M
