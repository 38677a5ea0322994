"""Independent float64 reference of the two estimators that have no reference output: the area light with its
power-heuristic MIS, and the dielectric split.  TEST INFRASTRUCTURE ONLY.

Written from include/prt.h (prt_area_light), the DESIGN.md area-light paragraph and the reference's
Core/Renderer.cpp:331-404,522-550 and Core/BRDF.cpp -- not from csrc/prt_path.h nor oracle/prt_oracle.c, and this
module imports neither `oracle` nor `prt`: a slip that the two restatements share disagrees with it.

The BRDF closed forms below are numpy-vectorised restatements of the scalar float64 closed forms of
tests/test_brdf_vectors.py (EVAL, PROBABILITY, INDIRECT, VNDF, GGX_D); tests/test_estimator_ref.py holds them to those
scalars point by point.

What a path's area-light term is (one path, one shaded point x with normal N and view direction V; the light is the
parallelogram corner + a eu + b ev with radiance Le on the side of n = normalize(cross(eu, ev)), both sides when
two-sided; y a point on it, L = normalize(y - x), d = |y - x|, cos_l = -n.L, or its absolute value when two-sided):

  light sampling     y uniform on the light: solid-angle density pl = d^2 / (area cos_l); the sample carries
                     f(L) Le w / pl with f = evalCombinedBRDF (which holds the cosine N.L)
  BRDF sampling      the lobe pick p_spec = getBrdfProbability, then the cosine hemisphere (density pd = N.L / pi,
                     BRDF.cpp:62-82) or the GGX VNDF reflection (density ps = D G1 / (4 N.V), BRDF.cpp:224-269); the
                     mixture density is pb = p_spec ps + (1 - p_spec) pd.  A ray that reaches the light first carries
                     Le w thr, thr = weight / p_lobe with evalIndirectCombinedBRDF's weight: (1, 1, 1) for the specular
                     lobe, base (1 - metalness) (1 - F) for the diffuse one, F at the VNDF half vector of the same u
  power heuristic    w(a, b) = a^2 / (a^2 + b^2): w(pl, pb) for the light sample, w(pb, pl) for the BRDF ray
  last segment       no BRDF ray follows a path's last segment, so light sampling is the only strategy there and its
                     sample is unweighted

Per solid angle the BRDF strategy therefore integrates g = ps (1, 1, 1) + pd w_diff, NOT f: the reference's indirect
weights are what they are (tests/test_brdf_vectors.py pins them), and expected_direct models them.
"""
import numpy as np

PI = float(np.float32(3.141592653589))   # Core/BRDF.h:27
F0_MIN = 0.4                              # MIN_DIELECTRICS_F0 (BRDF.h:65)
_LUM = np.array([0.2126, 0.7152, 0.0722])


# ------------------------------------------------------------------------------------------------ BRDF closed forms
def _dot(a, b):
    return np.sum(a * b, -1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _mat(mat, n):
    """scene_ref.material()'s dict (or scalars / one colour) -> base (n,3), metalness (n,), roughness (n,)."""
    base = np.broadcast_to(np.asarray(mat["base"], np.float64), (n, 3))
    metal = np.broadcast_to(np.asarray(mat["metalness"], np.float64), (n,))
    rough = np.broadcast_to(np.asarray(mat["roughness"], np.float64), (n,))
    return base, metal, rough


def _f0(base, metal):
    return F0_MIN + (base - F0_MIN) * metal[..., None]                                     # BRDF.cpp:21-30


def _f90(F0):
    return np.minimum(1.0, (F0 @ _LUM) / F0_MIN)                                           # :100-104


def _schlick(F0, f90, x):
    return F0 + (f90[..., None] - F0) * ((1.0 - x) ** 5)[..., None]                        # :84-87


def ggx_d(a2, nh):
    b = (a2 - 1.0) * nh * nh + 1.0                                                         # :218-222
    return a2 / (PI * b * b)


def eval_brdf(N, L, V, base, metal, rough):
    """evalCombinedBRDF (BRDF.cpp:398-452), cosine included.  N, V: (P,3); L: (P,M,3); base (P,3); metal, rough (P,).
    Returns (P,M,3)."""
    N, V = N[:, None, :], V[:, None, :]
    base, metal, rough = base[:, None, :], metal[:, None], rough[:, None]
    H = _unit(L + V)
    nl, nv = _dot(N, L), _dot(N, V)
    lit = (nl > 0) & (nv > 0)
    nl, nv = np.clip(nl, 1e-5, 1.0), np.clip(nv, 1e-5, 1.0)
    lh, nh = np.clip(_dot(L, H), 0.0, 1.0), np.clip(_dot(N, H), 0.0, 1.0)
    F0 = _f0(base, metal)
    F = _schlick(F0, _f90(F0), lh)
    a2 = (rough * rough) ** 2
    D = ggx_d(np.maximum(1e-5, a2), nh)
    G = 0.5 / (nv * np.sqrt(a2 + nl * (nl - a2 * nl)) + nl * np.sqrt(a2 + nv * (nv - a2 * nv)))   # :170-175
    diff = base * ((1.0 - metal) * nl / PI)[..., None]
    out = (1.0 - F) * diff + F * (G * D * nl)[..., None]
    return np.where(lit[..., None], out, 0.0)


def probability(N, V, base, metal):
    """getBrdfProbability (BRDF.cpp:504-526): (P,)."""
    sF0 = _f0(base, metal) @ _LUM
    dR = (base * (1.0 - metal)[:, None]) @ _LUM
    ff = np.maximum(0.0, _dot(V, N))
    f90 = np.minimum(1.0, sF0 / F0_MIN)       # shadowedF90 of the grey (sF0, sF0, sF0): the weights sum to 1
    fr = np.clip(sF0 + (f90 - sF0) * (1.0 - ff) ** 5, 0.0, 1.0)
    spec = 0.5 * fr
    diff = dR * (1.0 - 0.5 * fr) * 1.5
    return np.clip(spec / np.maximum(1e-4, spec + diff), 0.05, 0.7)


def rotation_to_z(N):
    """getRotationToZAxis (BRDF.cpp:43-49): the quaternion (P,4) that takes N to +z."""
    N = np.asarray(N, np.float64)
    q = np.stack([N[:, 1], -N[:, 0], np.zeros(len(N)), 1.0 + N[:, 2]], -1)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True).clip(1e-300)
    q[N[:, 2] < -0.99999] = (1.0, 0.0, 0.0, 0.0)
    return q


def rotate(q, v):
    """rotatePoint (BRDF.cpp:56-60).  q: (P,4); v: (P,3) or (P,M,3)."""
    a, w = q[:, :3], q[:, 3]
    if v.ndim == 3:
        a, w = a[:, None, :], w[:, None]
    aa = _dot(a, a)
    return (2.0 * _dot(a, v))[..., None] * a + (w * w - aa)[..., None] * v + (2.0 * w)[..., None] * np.cross(a, v)


def sample_hemisphere(u):
    """sampleHemisphere (BRDF.cpp:62-82): u (...,2) -> the local direction (..., 3); its density is z / pi."""
    a, b = np.sqrt(u[..., 0]), 2.0 * PI * u[..., 1]
    return np.stack([a * np.cos(b), a * np.sin(b), np.sqrt(1.0 - u[..., 0])], -1)


def invert_hemisphere(l):
    """The u in [0,1)^2 whose sample_hemisphere is the local unit direction l (z >= 0): u.x = x^2 + y^2 = 1 - z^2,
    u.y = the azimuth in [0, 2 pi) over 2 PI -- PI being the reference's float macro, which the forward map multiplies
    by, while the turn added to a negative atan2 is the true one."""
    ux = l[..., 0] ** 2 + l[..., 1] ** 2
    ang = np.arctan2(l[..., 1], l[..., 0])
    uy = np.where(ang < 0, ang + 2.0 * np.pi, ang) / (2.0 * PI)
    return np.stack([ux, uy], -1)


def vndf(Vl, alpha, u):
    """sampleGGXVNDF (BRDF.cpp:224-269, Heitz 2018) with alpha_x = alpha_y.  Vl: (P,3); alpha: (P,); u: (P,M,2)."""
    Vh = _unit(np.stack([alpha * Vl[:, 0], alpha * Vl[:, 1], Vl[:, 2]], -1))
    lensq = Vh[:, 0] ** 2 + Vh[:, 1] ** 2
    T1 = np.where((lensq > 0)[:, None],
                  np.stack([-Vh[:, 1], Vh[:, 0], np.zeros(len(Vh))], -1) / np.sqrt(np.where(lensq > 0, lensq, 1.0))[:, None],
                  np.array([1.0, 0.0, 0.0]))
    T2 = np.cross(Vh, T1)
    r, phi = np.sqrt(u[..., 0]), 2.0 * PI * u[..., 1]
    t1, t2 = r * np.cos(phi), r * np.sin(phi)
    s = 0.5 * (1.0 + Vh[:, 2])[:, None]
    t2 = (1.0 - s) * np.sqrt(np.maximum(0.0, 1.0 - t1 * t1)) + s * t2
    Nh = (t1[..., None] * T1[:, None, :] + t2[..., None] * T2[:, None, :]
          + np.sqrt(np.maximum(0.0, 1.0 - t1 * t1 - t2 * t2))[..., None] * Vh[:, None, :])
    a = alpha[:, None]
    return _unit(np.stack([a * Nh[..., 0], a * Nh[..., 1], np.maximum(0.0, Nh[..., 2])], -1))


def diffuse_weight(u, N, V, base, metal, rough):
    """The weight evalIndirectCombinedBRDF leaves for the diffuse lobe at sample u (BRDF.cpp:454-502):
    base (1 - metalness) (1 - F), F the Schlick term at the VNDF half vector drawn from the SAME u.  (P,M,3)."""
    Vl = rotate(rotation_to_z(N), V)
    Hs = vndf(Vl, rough * rough, u)
    vh = np.clip(_dot(Vl[:, None, :], Hs), 1e-5, 1.0)
    F0 = _f0(base, metal)[:, None, :]
    F = _schlick(F0, _f90(F0), vh)
    return (base * (1.0 - metal)[:, None])[:, None, :] * (1.0 - F)


# ------------------------------------------------------------------------------------------------ densities
def mis_power(a, b):
    """The power heuristic w(a, b) = a^2 / (a^2 + b^2); an infinite a gives 1 and an infinite b gives 0."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        w = a * a / (a * a + b * b)
    return np.where(np.isinf(a), 1.0, np.where(np.isinf(b), 0.0, w))


def lobe_densities(N, L, V, rough):
    """(pd, ps): cosine-hemisphere and VNDF-reflection solid-angle densities of direction L, 0 below the horizon."""
    N, V = N[:, None, :], V[:, None, :]
    nl = _dot(N, L)
    up = nl > 0
    pd = np.where(up, nl / PI, 0.0)
    H = _unit(L + V)
    nv = np.clip(_dot(N, V), 1e-5, 1.0)
    nh = np.clip(_dot(N, H), 0.0, 1.0)
    a2 = np.maximum(1e-5, (rough * rough) ** 2)[:, None]
    G1 = 2.0 * nv / (nv + np.sqrt(a2 + (1.0 - a2) * nv * nv))                              # Smith_G1_GGX, BRDF.cpp:149-154
    ps = np.where(up, ggx_d(a2, nh) * G1 / (4.0 * nv), 0.0)
    return pd, ps


# ------------------------------------------------------------------------------------------------ the area light
def light_geometry(light):
    """corner, eu, ev, n, Le, area, two_sided of a prt_area_light dict (scenes.ceiling_light's keys)."""
    c, eu, ev = (np.asarray(light[k], np.float64) for k in ("corner", "edge_u", "edge_v"))
    nn = np.cross(eu, ev)
    area = float(np.linalg.norm(nn))
    return c, eu, ev, nn / area, np.asarray(light["radiance"], np.float64), area, bool(light.get("two_sided", False))


def quadrature(I, N, V, mat, light, K):
    """Every per-point term on the K x K midpoints of the light, for hit points I (P,3): what expected_direct and
    second_moment integrate (both take it as `q`, so that one evaluation serves several integrals)."""
    I, N, V = (np.asarray(a, np.float64) for a in (I, N, V))
    P = I.shape[0]
    base, metal, rough = _mat(mat, P)
    c, eu, ev, n, Le, area, two = light_geometry(light)
    t = (np.arange(K) + 0.5) / K
    a, b = np.meshgrid(t, t, indexing="ij")
    Y = c + a.reshape(-1, 1) * eu + b.reshape(-1, 1) * ev                                  # (M,3)
    Lv = Y[None, :, :] - I[:, None, :]
    dsq = _dot(Lv, Lv)
    L = Lv / np.sqrt(dsq)[..., None]
    cos_l = -(L @ n)
    if two:
        cos_l = np.abs(cos_l)
    seen = (cos_l > 0) & (_dot(N[:, None, :], L) > 0)
    cos_l = np.where(seen, cos_l, 0.0)
    dw = cos_l / dsq * (area / (K * K))          # solid angle of one cell; 0 where the light faces away
    f = eval_brdf(N, L, V, base, metal, rough)
    pd, ps = lobe_densities(N, L, V, rough)
    p_spec = probability(N, V, base, metal)[:, None]
    pb = p_spec * ps + (1.0 - p_spec) * pd
    with np.errstate(divide="ignore"):
        pl = np.where(seen, dsq / (area * np.where(seen, cos_l, 1.0)), np.inf)
    u = invert_hemisphere(rotate(rotation_to_z(N), L))
    wd = diffuse_weight(u, N, V, base, metal, rough)
    return dict(f=f, pd=pd, ps=ps, p_spec=p_spec, pb=pb, pl=pl, dw=dw, wd=wd, Le=Le, seen=seen, area=area)


def expected_direct(I, N, V, mat, light, bounces_left, K=64, g_is_f=False, q=None):
    """The per-channel expectation (P,3) of one path's area-light term at shaded points I with unit normals N and
    view directions V (= -ray.D), by a midpoint quadrature over K x K cells of the light.
      bounces_left == 0   the path's last segment: the integral of f Le over the light's solid angle
      otherwise           the integral of [w(pl, pb) f + w(pb, pl) g] Le, g = ps (1,1,1) + pd w_diff
    g_is_f replaces g by f (the partition-of-unity self-check)."""
    q = quadrature(I, N, V, mat, light, K) if q is None else q
    if bounces_left == 0:
        integrand = q["f"]
    else:
        g = q["f"] if g_is_f else q["ps"][..., None] + q["pd"][..., None] * q["wd"]
        integrand = mis_power(q["pl"], q["pb"])[..., None] * q["f"] + mis_power(q["pb"], q["pl"])[..., None] * g
    return np.sum(integrand * q["dw"][..., None], 1) * q["Le"]


def second_moment(I, N, V, mat, light, bounces_left, K=64, q=None):
    """Per-sample first and second moments of the two terms, from the same quadrature: dict of (P,3) arrays
    nee_m1, nee_m2, brdf_m1, brdf_m2, and sigma_nee, sigma_brdf = sqrt(m2 - m1^2).
      light sample  y uniform on the light: X = w f Le / pl where the light faces the point, else 0
      BRDF ray      the lobe mixture: with probability p_spec the specular lobe (direction density ps, X = w Le / p_spec),
                    else the diffuse one (density pd, X = w Le w_diff / (1 - p_spec)); 0 when the ray misses the light
    At the last segment (bounces_left == 0) w = 1 for the light sample and there is no BRDF ray."""
    q = quadrature(I, N, V, mat, light, K) if q is None else q
    Le, dw = q["Le"], q["dw"][..., None]
    last = bounces_left == 0
    wl = 1.0 if last else mis_power(q["pl"], q["pb"])[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(q["seen"][..., None], wl * q["f"] / q["pl"][..., None], 0.0) * Le    # the sample's value
    # y has density pl per solid angle: E[X^k] = integral of X^k pl dw
    pl_dw = np.where(q["seen"], q["pl"], 0.0)[..., None] * dw
    out = dict(nee_m1=np.sum(x * pl_dw, 1), nee_m2=np.sum(x * x * pl_dw, 1))
    if last:
        out["brdf_m1"] = out["brdf_m2"] = np.zeros_like(out["nee_m1"])
    else:
        wb = mis_power(q["pb"], q["pl"])[..., None]
        p = q["p_spec"][..., None]
        xs = wb * Le / p
        xd = wb * Le * q["wd"] / (1.0 - p)
        ps, pd = q["ps"][..., None], q["pd"][..., None]
        out["brdf_m1"] = np.sum((p * ps * xs + (1.0 - p) * pd * xd) * dw, 1)
        out["brdf_m2"] = np.sum((p * ps * xs * xs + (1.0 - p) * pd * xd * xd) * dw, 1)
    for k in ("nee", "brdf"):
        out["sigma_" + k] = np.sqrt(np.maximum(0.0, out[k + "_m2"] - out[k + "_m1"] ** 2))
    return out


# ------------------------------------------------------------------------------------------------ glass
N1, N2 = 1.0, 1.46                         # Renderer.cpp:337-338


def refract(D, N, eta):
    """Renderer::refract (Renderer.cpp:522-550), literally: `eta` is taken for the material's index, so the caller's
    eta = n1 / n2 makes a ray that enters (D.N < 0) bend by etai / etat = 1 / eta = 1.46, and k < 0 returns the zero
    direction.  D, N: (P,3)."""
    cosi = np.clip(_dot(D, N), -1.0, 1.0)
    inside = cosi > 0
    ratio = np.where(inside, eta / 1.0, 1.0 / eta)                                         # swap(etai, etat) :529-532
    cos_t = np.abs(cosi)
    k = 1.0 - ratio * ratio * (1.0 - cos_t * cos_t)
    T = ratio[:, None] * (D - N * cos_t[:, None]) - N * np.sqrt(np.maximum(k, 0.0))[:, None]
    return np.where((k < 0)[:, None], 0.0, T), k


def glass(D, N):
    """The dielectric split of Renderer::Trace (Renderer.cpp:331-372) for ray directions D and shading normals N
    (P,3), in float64: dict of
      R         the reflection direction reflect(D, N) = D - 2 (D.N) N
      T         refract(D, N, n1 / n2): possibly the zero direction
      traced    k > 0 (:352,355): the refraction ray is traced at all (else refracted = 0)
      fres      R0 + (1 - R0) (1 - cosTheta)^5 with cosTheta = clamp(-D.N, 0, 1); 1 when k <= 0
      k_refract the k inside refract(), whose sign decides the zero direction
    and combine(reflected, refracted) = fres reflected + (1 - fres) refracted (albedo 1, :371)."""
    D, N = np.asarray(D, np.float64), np.asarray(N, np.float64)
    cos_theta = np.clip(-_dot(D, N), 0.0, 1.0)
    R = D - 2.0 * _dot(D, N)[:, None] * N
    eta = N1 / N2
    k = 1.0 - eta * eta * (1.0 - cos_theta * cos_theta)
    T, k_refract = refract(D, N, eta)
    R0 = ((N1 - N2) / (N1 + N2)) ** 2
    fres = np.where(k <= 0, 1.0, R0 + (1.0 - R0) * (1.0 - cos_theta) ** 5)
    return dict(R=R, T=T, traced=k > 0, fres=fres, k_refract=k_refract, cos_theta=cos_theta)


def glass_combine(g, reflected, refracted):
    refracted = np.where(g["traced"][:, None], refracted, 0.0)
    return g["fres"][:, None] * reflected + (1.0 - g["fres"])[:, None] * refracted
