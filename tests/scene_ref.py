"""Independent numpy reference for the per-pixel scene queries of the reference renderer: primary rays
(Core/Camera.cpp:29-36,81-139), the skybox lookup (Core/Camera.cpp:43-74), texel addressing and decode
(Core/Scene.cpp:225-263), the material and normal queries (Core/Scene.cpp:47-218) and the light block of
Renderer::Trace (Core/Renderer.cpp:196-326).  TEST INFRASTRUCTURE ONLY.

Written from those source lines, not from the C restatement (oracle/prt_oracle.c) nor from the device code: this
module imports neither `oracle` nor `prt`, so a transcription slip that the two restatements share disagrees with
it.  (direct_light borrows the float64 closed form of Core/BRDF.cpp from tests/test_brdf_vectors.py, which is
independent of both as well; it is imported when direct_light is first called.)

Two tiers:

exact        float32 restatements that keep the reference's operation order.  Every intermediate is np.float32;
             + - * / sqrt are correctly rounded there as in C built with -ffp-contract=off -fno-fast-math; atan2,
             acos, pow, sin and cos are evaluated in float64 and rounded once, as the cr_* functions of prt_math.h
             do.  The restatements are expected to agree with these bit for bit.
closed form  float64 answers (normal_matrix, visibility, direct_light), compared within CLOSED_TOL.

Every function is vectorised over a leading "pixel" axis.
"""
import numpy as np

F = np.float32
PI = F(3.141592653589)   # Core/BRDF.h:27, the macro Camera.cpp and Renderer.cpp see
EPSILON = F(0.01)        # template/common.h:26
BVH_FAR = F(1e30)        # Core/tiny_bvh.h:131

# closed-form tier: the bound tests/test_brdf_vectors.py gives a float32 EVAL against its float64 closed form, plus
# 32 * 2^-24 for the at most 32 further float32 roundings of the normal matrix, the light factors and the division
# by the class probability; used as rtol = atol, per channel (normals: relative to the vector's length)
CLOSED_TOL = 2e-5 + 32 * 2.0 ** -24

P_POINT, P_DIR, P_SPOT = F(0.3), F(0.5), F(0.2)   # Core/Renderer.cpp:205-207


# ------------------------------------------------------------------------------------------------ float3 helpers
def dot3(a, b):
    """tmpl8math.h:495 / tiny_bvh.h:399: a.x * b.x + a.y * b.y + a.z * b.z, summed left to right."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    """tmpl8math.h:553."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize(v):
    """tmpl8math.h:139,517 (and glm::normalize): v * (1 / sqrt(dot(v, v)))."""
    inv = F(1) / np.sqrt(dot3(v, v))
    return v * inv[..., None]


def ray_ctor_dir(d):
    """The direction a tinybvh::Ray holds: tinybvh_normalize of the constructor's argument
    (Core/tiny_bvh.h:403-408,583): l = sqrt(x*x + y*y + z*z), d * (l == 0 ? 0 : 1 / l)."""
    d = np.asarray(d, F)
    l = np.sqrt(dot3(d, d))
    with np.errstate(divide="ignore"):
        rl = np.where(l == 0, F(0), F(1) / l).astype(F)
    return d * rl[..., None]


def transform_vector(v, T):
    """tinybvh_transform_vector (Core/tiny_bvh.h:418-422); T is a row-major 4x4 (or 3x3)."""
    T = np.asarray(T)
    return np.stack([(T[k, 0] * v[..., 0] + T[k, 1] * v[..., 1]) + T[k, 2] * v[..., 2] for k in range(3)], -1)


# ------------------------------------------------------------------------------------------------ camera
def camera(pos, target, aspect):
    """Camera::Camera's basis and screen plane (Core/Camera.cpp:29-36; tmpUp = (0, 1, 0), Camera.h:18)."""
    pos, target, aspect = np.asarray(pos, F), np.asarray(target, F), F(aspect)
    ahead = normalize(target - pos)
    right = normalize(cross(ahead, np.array([0, 1, 0], F)))
    up = normalize(cross(right, ahead))
    tl = pos + ahead * F(2) - aspect * right + up
    tr = pos + ahead * F(2) + aspect * right + up
    bl = pos + ahead * F(2) - aspect * right - up
    return dict(pos=pos, ahead=ahead, right=right, up=up, tl=tl, tr=tr, bl=bl)


def _cr(fn, *a):
    """A libm function evaluated in float64 on float32 arguments and rounded once."""
    return fn(*[np.asarray(x, F).astype(np.float64) for x in a]).astype(F)


def panini(ndc_x, ndc_y, fov, distortion):
    """Camera::Panini (Core/Camera.cpp:81-111)."""
    fov, d = F(fov), F(distortion)
    fo = PI / F(2) - fov * F(0.5)
    f = _cr(np.cos, fo) / _cr(np.sin, fo) * F(2)
    f2 = f * f
    d2 = d * d
    b = (np.sqrt(np.maximum(F(0), (d + d2) * (d + d2) * (f2 + f2 * f2))) - (d * f + f)) / (d2 + d2 * f2 - F(1))
    ndc_x, ndc_y = ndc_x * b, ndc_y * b
    h, v = ndc_x, ndc_y
    h2 = h * h
    k = h2 / ((d + F(1)) * (d + F(1)))
    k2 = k * k
    discr = np.maximum(F(0), k2 * d2 - (k + F(1)) * (k * d2 - F(1)))
    cos_phi = (-k * d + np.sqrt(discr)) / (k + F(1))
    S = (d + F(1)) / (d + cos_phi)
    tan_theta = v / S
    sin_phi = np.sqrt(np.maximum(F(0), F(1) - cos_phi * cos_phi))
    sin_phi = np.where(ndc_x < F(0), sin_phi * F(-1), sin_phi)
    s = F(1) / np.sqrt(F(1) + tan_theta * tan_theta)
    return np.stack([sin_phi, tan_theta, cos_phi], -1) * s[..., None]


def primary_rays(cam, W, H, xs, ys, postfx=None):
    """Camera::GetPrimaryRay (Core/Camera.cpp:113-139) for pixel coordinates xs, ys: the singly-normalised direction
    the reference hands to the tinybvh::Ray constructor (which normalises it once more, ray_ctor_dir).  `cam` is
    camera()'s dict; postfx is None (plane projection) or anything with .fov and .distortion (Panini, :124-135)."""
    xs, ys = np.asarray(xs, F), np.asarray(ys, F)
    u = xs * (F(1) / F(W))                                                                  # :116, not x / W
    v = ys * (F(1) / F(H))
    tl, tr, bl, pos = cam["tl"], cam["tr"], cam["bl"], cam["pos"]
    P = tl + u[..., None] * (tr - tl) + v[..., None] * (bl - tl)
    if postfx is None:
        return normalize(P - pos)
    ndc_x, ndc_y = (F(2) * u) - F(1), F(1) - (F(2) * v)
    pd = panini(ndc_x, ndc_y, postfx.fov, postfx.distortion)
    Pc = P - pos
    c = pd * np.sqrt(dot3(Pc, Pc))[..., None]                                               # :128
    world = cam["right"] * c[..., 0:1] + cam["up"] * c[..., 1:2] + cam["ahead"] * c[..., 2:3]
    return normalize(world)


# ------------------------------------------------------------------------------------------------ skybox
def sky_taps(D, sky_w, sky_h):
    """The addressing half of Camera::SampleSkybox (Core/Camera.cpp:45-57): (u, v, u0, v0, u1, v1, du, dv).  u0 is
    taken modulo the width BEFORE the + 1 of u1, and du is computed from the wrapped u0."""
    D = np.asarray(D, F)
    u = F(0.5) + _cr(np.arctan2, D[..., 2], D[..., 0]) / (F(2) * PI)
    v = _cr(np.arccos, D[..., 1]) / PI
    u_tex = u * F(sky_w)
    v_tex = v * F(sky_h)
    W, Hh = np.uint32(sky_w), np.uint32(sky_h)
    u0 = np.floor(u_tex).astype(np.uint32) % W
    v0 = np.floor(v_tex).astype(np.uint32) % Hh
    u1 = (u0 + np.uint32(1)) % W
    v1 = (v0 + np.uint32(1)) % Hh
    du = u_tex - u0.astype(F)
    dv = v_tex - v0.astype(F)
    return u, v, u0, v0, u1, v1, du, dv


def sample_sky(sky, D):
    """Camera::SampleSkybox (Core/Camera.cpp:43-74).  sky: (h, w, 3) float32; D: the ray's own direction, that is
    after the constructor's second normalisation."""
    sky = np.asarray(sky, F)
    h, w = sky.shape[:2]
    _, _, u0, v0, u1, v1, du, dv = sky_taps(D, w, h)
    c00, c01, c10, c11 = sky[v0, u0], sky[v0, u1], sky[v1, u0], sky[v1, u1]
    a = c00 + du[..., None] * (c01 - c00)
    b = c10 + du[..., None] * (c11 - c10)
    return a + dv[..., None] * (b - a)


# ------------------------------------------------------------------------------------------------ texels
# planted defects of texel_index (slip=), to show that a comparison against it can see a wrong rule
TEXEL_SLIPS = ("floor", "abs", "clamp", "no_negative_wrap", "wrap_v_with_w", "no_range_guard")
_INT_MIN, _INT_MAX = -(1 << 31), (1 << 31) - 1


def _texel_coord(c, n, slip, wrap_n=None):
    """One component of texel_index: the float32 array c times the size n, as an int64 array."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(c, F) * F(n)                              # one float32 multiply
        inside = np.abs(x) < F(2147483648.0)                     # False for NaN, +-inf, |x| >= 2^31
    whole = np.trunc(np.where(inside, x, F(0))).astype(np.int64)    # truncation toward zero
    if slip == "floor":
        whole = np.floor(np.where(inside, x, F(0))).astype(np.int64)
    if slip == "abs":
        whole = np.abs(whole)
    if slip == "no_range_guard":   # the cast as the device's conversion does it: NaN -> 0, the rest saturates
        sat = np.where(np.isnan(x), F(0), np.clip(x.astype(np.float64), _INT_MIN, _INT_MAX))
        whole = np.trunc(sat).astype(np.int64)
    if slip == "clamp":
        return np.clip(whole, 0, n - 1)
    if slip == "no_negative_wrap":   # C's %, which keeps the dividend's sign
        return np.fmod(whole, np.int64(n))
    return np.mod(whole, np.int64(n if wrap_n is None else wrap_n))   # numpy's mod of integers lies in [0, n)


def texel_index(uv, albedo_w, albedo_h, slip=None):
    """The texel every map of a mesh is read at, for any float32 uv: column + row * w with the ALBEDO texture's w and
    h, whichever map is then read (Scene.cpp:79-85,160-165).  Per component, with x = uv * n in float32: x is
    truncated toward zero and wrapped into [0, n); where x is NaN, infinite or |x| >= 2^31 the component is 0.  For
    x > -1 that is the reference's (int)x % n; the reference indexes outside the texture below that and is undefined
    where the cast is, and include/prt.h (prt_mesh.fixed_uvs) defines the rest as stated here.  int64 throughout, so
    nothing overflows.  slip: None, or one of TEXEL_SLIPS."""
    assert slip is None or slip in TEXEL_SLIPS
    uv = np.asarray(uv, F)
    iu = _texel_coord(uv[..., 0], albedo_w, slip)
    iv = _texel_coord(uv[..., 1], albedo_h, slip, albedo_w if slip == "wrap_v_with_w" else None)
    return iu + iv * albedo_w


def _chan(c, shift):
    return ((np.asarray(c, np.uint32) >> np.uint32(shift)) & np.uint32(0xFF)).astype(F)


def color_from_texel(c):
    """Scene::MakeColorFromTexel (Scene.cpp:225-229)."""
    s = F(1) / F(255)
    return np.stack([_chan(c, 16) * s, _chan(c, 8) * s, _chan(c, 0) * s], -1)


def normal_from_texel(c):
    """Scene::MakeNormalFromTexel (Scene.cpp:231-235)."""
    s = F(2) / F(255)
    return np.stack([_chan(c, 16) * s - F(1), _chan(c, 8) * s - F(1), _chan(c, 0) * s - F(1)], -1)


RED, GREEN, BLUE, ALPHA = 16, 8, 0, 24


def extract_channel(channel, c):
    """Scene::ExtractChannel (Scene.cpp:237-254); channel is RED, GREEN, BLUE or ALPHA."""
    return _chan(c, channel) * (F(1) / F(255))


def srgb_to_linear(c):
    """Scene::SrgbToLinear (Scene.cpp:256-263)."""
    c = np.asarray(c, F)
    hi = _cr(np.power, (c + F(0.055)) / F(1.055), np.broadcast_to(F(2.4), c.shape))
    return np.where(c <= F(0.04045), c / F(12.92), hi).astype(F)


# ------------------------------------------------------------------------------------------------ hit attributes
def _corner(a, prim, k, width, take):
    """Corner k of triangle `prim` in a flat per-corner array of `width` floats per corner."""
    return np.asarray(a, F).reshape(-1, width)[3 * np.asarray(prim, np.int64) + k, :take]


def hit_uv(mesh, prim, u, v):
    """v * uv[V2] + u * uv[V1] + w * uv[V0] with w = 1 - u - v (Scene.cpp:64-66,75-77,148-158)."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    w = F(1) - u - v
    t0, t1, t2 = (_corner(mesh.fixed_uvs, prim, k, 2, 2) for k in range(3))
    return v[..., None] * t2 + u[..., None] * t1 + w[..., None] * t0


def _pixels(textures, index):
    return np.asarray(textures[index], np.uint32).reshape(-1)


def material(mesh, textures, prim, u, v):
    """Scene::GetMaterialBRDF (Scene.cpp:140-218) for a textured game object: dict of base (n,3), metalness (n),
    roughness (n), emissive (n,3).  A map the mesh lacks (index -1) leaves its values 0."""
    uv = hit_uv(mesh, prim, u, v)
    alb = np.asarray(textures[mesh.albedo])
    px = texel_index(uv, alb.shape[1], alb.shape[0])                                          # :160-165
    n = px.shape[0]
    base = srgb_to_linear(color_from_texel(_pixels(textures, mesh.albedo)[px]))              # :168-172
    metal, rough, emis = np.zeros(n, F), np.zeros(n, F), np.zeros((n, 3), F)
    if mesh.metalness >= 0:                                                                   # :175-181
        c = _pixels(textures, mesh.metalness)[px]
        rough, metal = extract_channel(GREEN, c), extract_channel(BLUE, c)
    if mesh.emission >= 0:                                                                    # :184-188
        emis = color_from_texel(_pixels(textures, mesh.emission)[px])
    return dict(base=base, metalness=metal, roughness=rough, emissive=emis, texel=px)


def _interp_normal(mesh, prim, u, v):
    u, v = np.asarray(u, F), np.asarray(v, F)
    w = F(1) - u - v
    n0, n1, n2 = (_corner(mesh.fixed_normals, prim, k, 4, 3) for k in range(3))
    return n0 * w[..., None] + n1 * u[..., None] + n2 * v[..., None]                         # :105-107,126-128


def shading_normal(mesh, textures, normal_matrix, prim, u, v, normalmapped):
    """Scene::GetShadingNormal (Scene.cpp:60-138).  normal_matrix: inverse-transpose of the instance transform; a
    float32 matrix keeps the whole computation in float32 (exact tier), a float64 one (normal_matrix()) carries the
    rest in float64 (closed-form tier).  The smooth branch returns the transformed interpolated normal as it is, NOT
    normalised (:126-136); the mapped branch uses object-space T and B against the world-space N (:88-121)."""
    prim = np.asarray(prim, np.int64)
    interp = transform_vector(_interp_normal(mesh, prim, u, v), normal_matrix)               # :113,134
    if not (mesh.normal >= 0 and normalmapped):                                               # :73
        return interp
    uv = hit_uv(mesh, prim, u, v)
    alb = np.asarray(textures[mesh.albedo])
    px = texel_index(uv, alb.shape[1], alb.shape[0])                                          # :79-85
    nc = normal_from_texel(_pixels(textures, mesh.normal)[px])
    idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)[prim]
    vert = np.asarray(mesh.vertices, F).reshape(-1, 3)
    edge1, edge2 = vert[idx[:, 1]] - vert[idx[:, 0]], vert[idx[:, 2]] - vert[idx[:, 0]]    # :93-94
    t0, t1, t2 = (_corner(mesh.fixed_uvs, prim, k, 2, 2) for k in range(3))
    d1, d2 = t1 - t0, t2 - t0
    det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    inv_det = (F(1) / det)[:, None]
    T = normalize(inv_det * (d2[:, 1:2] * edge1 - d1[:, 1:2] * edge2))                        # :102
    B = normalize(inv_det * (-d2[:, 0:1] * edge1 + d1[:, 0:1] * edge2))                       # :103
    N = normalize(interp)                                                                     # :115
    # glm: colorNorm * transpose(TBN) = (dot((T.x, B.x, N.x), c), ...) (type_mat3x3.inl:477-483), glm::dot sums
    # x + y + z left to right
    r = (T * nc[:, 0:1] + B * nc[:, 1:2]) + N * nc[:, 2:3]                                    # :117-119
    return normalize(r)


def geometry_normal(mesh, normal_matrix, prim):
    """Scene::GetGeometryNormal (Scene.cpp:47-58): the face normal through the normal matrix, not normalised."""
    fn = np.asarray(mesh.face_normals, F).reshape(-1, 3)[np.asarray(prim, np.int64)]
    return transform_vector(fn, normal_matrix)


def normal_matrix(transform):
    """inverse(T) transposed, in float64 (the reference's mat4::Inverted is a long float32 cofactor expansion that
    is not restated).  Exact for the identity and pure translations, where the exact tier applies to it."""
    T = np.asarray(transform, np.float64).reshape(4, 4)
    return np.linalg.inv(T).T


# ------------------------------------------------------------------------------------------------ lights (float64)
def _unit(v):
    d = np.linalg.norm(v, axis=-1)
    return v / d[..., None], d


def _light_list(lights):
    """(name, position, kind) of the six lights; lights: anything with scenes.Lights' attributes."""
    pp = np.asarray(lights.point_pos, np.float64).reshape(4, 3)
    return ([("point%d" % i, pp[i], "point") for i in range(4)]
            + [("dir", np.asarray(lights.dir_pos, np.float64), "dir"),
               ("spot", np.asarray(lights.spot_pos, np.float64), "spot")])


def _tri_hits(O, D, tmax, tris):
    """float64 Moeller-Trumbore of rays (n,3) against triangles (k,3,3): bool (n,k), hit when 0 < t < tmax."""
    O, D = O[:, None, :], D[:, None, :]
    v0, e1, e2 = tris[None, :, 0], (tris[:, 1] - tris[:, 0])[None], (tris[:, 2] - tris[:, 0])[None]
    p = np.cross(D, e2)
    det = np.sum(e1 * p, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = O - v0
        uu = np.sum(s * p, -1) * inv
        q = np.cross(s, e1)
        vv = np.sum(D * q, -1) * inv
        t = np.sum(e2 * q, -1) * inv
        return (np.abs(det) > 1e-300) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > 0) & (t < tmax[:, None])


def shadow_hits(I, lights, tris, physical=False):
    """Which world-space triangles (k,3,3) each light's shadow ray from hit points I (n,3) meets: bool (n, 6, k) in
    the order point 0..3, directional, spot.  The ray is the reference's: origin I + L * EPSILON, direction L, and
    tmax = d^2 - EPSILON for a point light (Renderer.cpp:257: the SQUARED distance), d - EPSILON for the directional
    and the spot light (:277,297,320).  physical=True ends a point light's ray at d - EPSILON instead: what a
    renderer that is not the reference would do, for tests that must tell the two apart."""
    I = np.asarray(I, np.float64)
    tris = np.asarray(tris, np.float64)
    eps = float(EPSILON)
    out = []
    for _, pos, kind in _light_list(lights):
        L, d = _unit(pos - I)
        tmax = (d * d if kind == "point" and not physical else d) - eps
        out.append(_tri_hits(I + L * eps, L, tmax, tris))
    return np.stack(out, 1)


def visibility(I, lights, tris, physical=False):
    """bool (n, 6): light j's shadow ray from I is not occluded (shadow_hits)."""
    return ~shadow_hits(I, lights, tris, physical).any(-1)


def spot_factor(I, lights):
    """dot(L, rotation) of the spot light (Renderer.cpp:295); inside the cone when (double)factor > 0.9 (:301)."""
    L, _ = _unit(np.asarray(lights.spot_pos, np.float64) - np.asarray(I, np.float64))
    return L @ np.asarray(lights.spot_rot, np.float64)


def direct_light(I, N, V, mat, lights, visible):
    """The pixel value of a one-bounce path, Renderer.cpp:196-326, in float64 for each outcome of the random choice.
    I, N, V: (n,3) hit point, shading normal, -ray.D; mat: material()'s dict; visible: (n,6) bool (visibility()).
    Returns dict: "point" (4,n,3) the point class with whichLight = 0..3, "dir", "spot" (n,3) the two other classes,
    "plain" (n,3) the non-stochastic value (:312-326).

    point class: every light adds colour * (1 / d) * max(0, N.L) -- a 1/d falloff -- when unoccluded; the sum is
    divided by 0.3 and multiplied by the BRDF towards light whichLight alone (:251-268).  directional: colour * cos
    / 0.5.  spot: colour * (1 / d^2) * cos inside the cone / 0.2."""
    from test_brdf_vectors import eval_brdf   # the independent float64 closed form of Core/BRDF.cpp
    I, N, V = (np.asarray(a, np.float64) for a in (I, N, V))
    n = I.shape[0]
    base = np.asarray(mat["base"], np.float64)
    metal = np.asarray(mat["metalness"], np.float64)
    rough = np.asarray(mat["roughness"], np.float64)
    emis = np.asarray(mat["emissive"], np.float64)
    visible = np.asarray(visible, bool)

    def brdf(L):
        return np.array([eval_brdf(N[k], L[k], V[k], tuple(base[k]), float(metal[k]), float(rough[k]))
                         for k in range(n)], np.float64).reshape(n, 3)

    pp = np.asarray(lights.point_pos, np.float64).reshape(4, 3)
    pc = np.asarray(lights.point_col, np.float64).reshape(4, 3)
    contrib = np.zeros((n, 3))
    Ls = []
    for i in range(4):
        L, d = _unit(pp[i] - I)
        cosa = np.maximum(0.0, np.sum(N * L, -1))
        contrib += np.where(visible[:, i, None], pc[i][None, :] * ((1.0 / d) * cosa)[:, None], 0.0)
        Ls.append(L)
    contrib /= float(P_POINT)
    point = np.stack([emis + brdf(Ls[i]) * contrib for i in range(4)])

    L, d = _unit(np.asarray(lights.dir_pos, np.float64) - I)
    cosa = np.maximum(0.0, np.sum(N * L, -1))
    dcon = np.where(visible[:, 4, None], np.asarray(lights.dir_col, np.float64)[None, :] * cosa[:, None], 0.0)
    f_dir = brdf(L)
    plain = emis + f_dir * dcon
    dirv = emis + f_dir * (dcon / float(P_DIR))

    L, d = _unit(np.asarray(lights.spot_pos, np.float64) - I)
    cosa = np.maximum(0.0, np.sum(N * L, -1))
    inside = (L @ np.asarray(lights.spot_rot, np.float64)) > 0.9
    scon = np.where((visible[:, 5] & inside)[:, None],
                    np.asarray(lights.spot_col, np.float64)[None, :] * (1.0 / (d * d))[:, None] * cosa[:, None], 0.0)
    spot = emis + brdf(L) * (scon / float(P_SPOT))
    return dict(point=point, dir=dirv, spot=spot, plain=plain)
