"""tests/estimator_ref.py proven on the CPU, then the checks of tests/test_gpu_estimator.py run against the oracle
(oracle/prt_oracle.c trace_ext): the statistical cases, the exact cases and the glass cases.

What the reference asserts about itself: its vectorised BRDF closed forms equal the scalar ones of
tests/test_brdf_vectors.py; with g replaced by f the two power-heuristic weights add up to the last-segment
expectation (the partition of unity); the inverse of the cosine-hemisphere map round-trips, and the two lobe densities
are those of the samplers; doubling the quadrature changes every expectation by less than a quarter of the pixel's
standard error; the bound of every statistical case is tight enough to catch a 10 % bias; and `glass` gives the
hand-worked vectors of the reference's lines.

What the checks found in the restatements: at a path's last segment (depth == bounces - 1) the area-light sample was
multiplied by the power-heuristic weight w(pl, pb) although no BRDF ray follows there, so the complement was never
added: with bounces = 1 the 91 tested pixels under the big light summed (red) to 13.65 against an expectation of 21.13
for (roughness, metalness) = (1, 0), 13.71 against 28.78 for (0.5, 0.5) and 3.54 against 31.40 for (0.25, 1).  Both
restatements now leave that sample unweighted, and the sums are 21.14, 28.74 and 31.44.  Nothing else disagreed: the
densities, the heuristic's arguments, the light's two sides, the blocked light and the glass split all match the
reference within the bounds stated in test_gpu_estimator.py.

Each of these changes to the restatement fails the named tests here (tried on copies of prt_oracle.c):
  the weight of a last segment's light sample kept      area_light_expectation, bounces 1, the three big-light cases
  the heuristic's arguments swapped at the light sample  area_light_expectation, bounces 2, all six cases
  ... swapped where a BRDF ray reaches the light         area_light_expectation, bounces 2, all six cases
  the balance heuristic a / (a + b)                      area_light_expectation, bounces 2, five of the six cases
  pb = the diffuse density alone (no lobe mixture)       area_light_expectation, bounces 2, big (0.5, 0.5) and (0.25, 1)
  pl without the light's cosine                          area_light_expectation, all twelve
  the shadow ray's answer ignored                        fully_blocked_light
  the light's back emitting as if two-sided              light_back[False], light_from_behind[up], light_seen_directly
  Schlick without the fifth power                        glass[front]
  refract()'s index swap on the other side               glass[front]

What the reference found about the reference renderer's own lines: refract() (Renderer.cpp:547) subtracts
normal * cosTheta from an entering direction whose normal part is already -cosTheta, so the refracted direction's
normal part is doubled rather than removed (test_glass_by_hand).  Both restatements keep the line as it is.
"""
import dataclasses

import numpy as np
import pytest

import estimator_ref as E
import scene_ref as R
import test_gpu_estimator as Q


# ------------------------------------------------------------------------------------------------ the reference alone
def _points(seed=3, P=5, M=7):
    rng = np.random.default_rng(seed)
    N = E._unit(np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.6, 0.6, (P, 3)))
    V = E._unit(N + rng.uniform(-0.7, 0.7, (P, 3)))
    L = E._unit(N[:, None, :] + rng.uniform(-0.9, 0.9, (P, M, 3)))
    base = rng.uniform(0.05, 0.95, (P, 3))
    metal = np.array([0.0, 1.0, 0.5, 0.2, 0.9])[:P]
    rough = np.array([1.0, 0.25, 0.5, 0.7, 0.1])[:P]
    return N, V, L, base, metal, rough


def test_vectorised_closed_forms_equal_the_scalar_ones():
    import test_brdf_vectors as B
    N, V, L, base, metal, rough = _points()
    f = E.eval_brdf(N, L, V, base, metal, rough)
    p = E.probability(N, V, base, metal)
    q = E.rotation_to_z(N)
    rng = np.random.default_rng(9)
    u = rng.uniform(0.02, 0.98, L.shape[:2] + (2,))
    wd = E.diffuse_weight(u, N, V, base, metal, rough)
    Hs = E.vndf(E.rotate(q, V), rough * rough, u)
    for i in range(N.shape[0]):
        assert np.isclose(p[i], B.probability(N[i], V[i], tuple(base[i]), metal[i]), rtol=1e-12)
        qs, rot = B.to_local(N[i])
        assert np.allclose(q[i], qs, rtol=1e-12, atol=1e-15)
        assert np.allclose(E.rotate(q[i:i + 1], V[i:i + 1])[0], rot(qs, V[i]), rtol=1e-12, atol=1e-15)
        for j in range(L.shape[1]):
            assert np.allclose(f[i, j], B.eval_brdf(N[i], L[i, j], V[i], tuple(base[i]), metal[i], rough[i]),
                               rtol=1e-11, atol=1e-15)
            a = rough[i] * rough[i]
            assert np.allclose(Hs[i, j], B.vndf(rot(qs, V[i]), a, a, u[i, j]), rtol=1e-10, atol=1e-13)
            ok, d, w = B.indirect(u[i, j], N[i], V[i], tuple(base[i]), metal[i], rough[i], 1)
            assert np.allclose(wd[i, j], w, rtol=1e-10, atol=1e-14)
            if ok:      # the direction the diffuse lobe draws from u is sample_hemisphere(u) in N's frame
                qi = q[i:i + 1] * np.array([-1.0, -1.0, -1.0, 1.0])
                assert np.allclose(E.rotate(qi, E.sample_hemisphere(u[i, j])[None])[0], d, rtol=1e-10, atol=1e-13)
    assert np.isclose(E.ggx_d(0.09, 0.7), B.ggx(0.09, 0.7), rtol=1e-15)


def test_inverse_hemisphere_map_round_trips():
    rng = np.random.default_rng(5)
    u = rng.uniform(0.0, 1.0, (4000, 2))
    u[:4] = [[0.0, 0.0], [0.5, 0.0], [0.999999, 0.75], [1e-12, 0.5]]
    l = E.sample_hemisphere(u)
    back = E.invert_hemisphere(l)
    assert np.allclose(back[:, 0], u[:, 0], rtol=0, atol=1e-14)
    d = np.abs(back[:, 1] - u[:, 1])[u[:, 0] > 1e-9]        # the azimuth of the pole itself is arbitrary
    assert d.max() < 1e-12
    assert np.allclose(E.sample_hemisphere(back), l, rtol=0, atol=1e-12)
    # and the map's density is z / pi: the Jacobian of (u.x, u.y) -> direction, numerically
    u0 = np.array([0.3, 0.2])
    h = 1e-5
    a = E.sample_hemisphere(u0 + [h, 0]) - E.sample_hemisphere(u0 - [h, 0])
    b = E.sample_hemisphere(u0 + [0, h]) - E.sample_hemisphere(u0 - [0, h])
    area = np.linalg.norm(np.cross(a, b)) / (4 * h * h)
    assert np.isclose(1.0 / area, E.sample_hemisphere(u0)[2] / E.PI, rtol=1e-6)


def test_densities_integrate_to_one():
    """pd and ps are densities over the upper hemisphere: pd integrates to 1, ps to at most 1 (the VNDF reflection
    sends the rest below the horizon), and the specular strategy's samples do follow ps (a histogram of reflections
    of estimator_ref.vndf half vectors against the integral of ps over a cone)."""
    N = np.array([[0.0, 0.0, 1.0]])
    V = E._unit(np.array([[0.5, 0.1, 0.8]]))
    n = 600
    ct = (np.arange(n) + 0.5) / n
    ph = (np.arange(2 * n) + 0.5) / (2 * n) * 2 * np.pi
    c, p = np.meshgrid(ct, ph, indexing="ij")
    s = np.sqrt(1 - c * c)
    L = np.stack([s * np.cos(p), s * np.sin(p), c], -1).reshape(1, -1, 3)
    dw = 2 * np.pi / (2 * n * n)
    for rough in (1.0, 0.5):
        pd, ps = E.lobe_densities(N, L, V, np.array([rough]))
        assert np.isclose(pd.sum() * dw, np.pi / E.PI, rtol=1e-5)
        total = ps.sum() * dw
        assert 0.4 < total <= 1.0 + 1e-4, total      # at roughness 1 nearly half the reflections point below
        axis = E._unit(2.0 * V[0, 2] * N[0] - V[0])           # the mirror direction
        cone = (L[0] @ axis) > 0.9
        rng = np.random.default_rng(11)
        u = rng.uniform(0, 1, (1, 200000, 2))
        Hh = E.vndf(V, np.array([rough * rough]), u)[0]
        Rr = 2.0 * (Hh @ V[0])[:, None] * Hh - V[0]
        share = ((Rr @ axis > 0.9) & (Rr[:, 2] > 0)).mean()
        expect = ps[0][cone].sum() * dw
        assert abs(share - expect) < 5 * np.sqrt(expect * (1 - expect) / 200000) + 2e-3, (rough, share, expect)


@pytest.mark.parametrize("light,rough,metal", Q.STAT_CASES)
def test_partition_of_unity(light, rough, metal):
    """With g = f the two weights sum to 1 at every point, so the MIS expectation is the last-segment one."""
    sd = Q.stat_scene(light, rough, metal)
    g = Q.Geometry(sd)
    sel = np.flatnonzero(g.floor)[::7]
    mat = {k: g.mat[k][sel] for k in ("base", "metalness", "roughness")}
    args = (g.I[sel], g.N[sel], g.V[sel], mat, sd.area_light)
    last = E.expected_direct(*args, 0, K=16)
    both = E.expected_direct(*args, 1, K=16, g_is_f=True)
    assert np.allclose(both, last, rtol=1e-12)
    assert (last > 0).all()


@pytest.mark.parametrize("light,rough,metal", Q.STAT_CASES)
def test_quadrature_converged_and_bound_is_tight(light, rough, metal):
    """Doubling K changes each expectation by less than a quarter of the pixel's standard error (so the allowance
    never carries the bound), and 6 summed standard errors plus the summed allowance stay below 10 % of the summed
    expectation: a 10 % bias cannot pass."""
    ref = Q.stat_ref(light, rough, metal)
    for left in (0, 1):
        assert (ref.allow[left] <= 0.25 * ref.se[left]).all(), (left, float((ref.allow[left] / ref.se[left]).max()))
        bound = 6.0 * np.sqrt((ref.se[left] ** 2).sum(0)) + ref.allow[left].sum(0)
        assert (bound < 0.1 * ref.exp[left].sum(0)).all(), (left, bound / ref.exp[left].sum(0))


def test_glass_by_hand():
    """D = (0.6, -0.8, 0) onto N = (0, 1, 0): cosTheta = 0.8.  Reflection (0.6, 0.8, 0).  The literal refract() takes
    n1 / n2 for the material's index, so the entering ray bends by etai / etat = 1.46: k = 1 - 1.46^2 * 0.36 = 0.232624.
    Snell's direction would be 1.46 (D + 0.8 N) - sqrt(k) N = (0.876, -0.48231, 0), a unit vector with
    sin_t / sin_i = 1.46 -- and the tangential part of the reference's T is that one: 0.876.  But its line :547 reads
    etaRatio * (D - N * cosTheta): for an entering ray D.N = -cosTheta, so the subtraction doubles the normal part
    instead of removing it, and T = 1.46 (0.6, -1.6, 0) - sqrt(k) N = (0.876, -2.81831, 0), which the ray constructor
    then normalises.  Restated literally, as both restatements do.  R0 = (0.46 / 2.46)^2,
    fres = R0 + (1 - R0) 0.2^5."""
    s = E.glass(np.array([[0.6, -0.8, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    assert np.allclose(s["R"][0], [0.6, 0.8, 0.0], rtol=1e-15)
    assert np.isclose(s["k_refract"][0], 0.232624, rtol=1e-12)
    assert np.isclose(s["T"][0][0] / 0.6, 1.46, rtol=1e-12)                   # Snell's tangential part, swapped indices
    assert np.allclose(s["T"][0], [0.876, -1.46 * 1.6 - np.sqrt(0.232624), 0.0], rtol=1e-12)
    R0 = (0.46 / 2.46) ** 2
    assert np.isclose(s["fres"][0], R0 + (1 - R0) * 0.2 ** 5, rtol=1e-14) and s["traced"][0]
    # past asin(1 / 1.46) = 43.2 degrees refract() returns the zero direction, yet the ray is traced (k of :352 > 0)
    s = E.glass(np.array([[0.8, -0.6, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    assert (s["T"][0] == 0).all() and s["traced"][0] and s["k_refract"][0] < 0 and s["fres"][0] < 1
    # a back-face hit: cosTheta clamps to 0, fres = 1; refract() leaves by 1 / 1.46
    s = E.glass(np.array([[0.6, 0.8, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    assert s["fres"][0] == 1.0 and s["traced"][0] and np.allclose(s["R"][0], [0.6, -0.8, 0.0])
    eta = 1 / 1.46
    assert np.allclose(s["T"][0], [eta * 0.6, -np.sqrt(1 - eta * eta * 0.36), 0.0], rtol=1e-12)
    out = E.glass_combine(s, np.array([[1.0, 2.0, 3.0]]), np.array([[5.0, 5.0, 5.0]]))
    assert np.array_equal(out, [[1.0, 2.0, 3.0]])


# ------------------------------------------------------------------------------------------------ the oracle
class OracleView:
    def __init__(self, oracle_mod, sd):
        self.o, self.sd = oracle_mod, sd
        self.osc = oracle_mod.OracleScene(sd, Q.W, Q.H)

    def without_light(self):
        return OracleView(self.o, dataclasses.replace(self.sd, area_light=None))

    def frames(self, bounces, k, frame_index=0):
        avg, rgb8, _, st = self.osc.render(Q.W, Q.H, spp=k, bounces=bounces, flags=Q.scene_flags(self.sd),
                                           frame_index=frame_index, seed=Q.SEED)
        return avg[:, :3].copy(), rgb8, int(st.segments), int(st.shadow_rays)

    def mean(self, bounces, n):
        total = np.zeros((Q.W * Q.H, 3), np.float64)
        for f0 in range(0, n, Q.CHUNK):
            total += self.frames(bounces, Q.CHUNK, f0)[0].astype(np.float64)
        return total / (n // Q.CHUNK)


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("light,rough,metal", Q.STAT_CASES)
def test_oracle_area_light_expectation(oracle_mod, light, rough, metal, bounces):
    Q.check_statistical(OracleView(oracle_mod, Q.stat_scene(light, rough, metal)), Q.stat_ref(light, rough, metal),
                        bounces)


def test_oracle_mirror_floor_returns_le_exactly(oracle_mod):
    Q.check_mirror(OracleView(oracle_mod, Q.mirror_scene()))


@pytest.mark.parametrize("two_sided", [False, True])
def test_oracle_light_back(oracle_mod, two_sided):
    Q.check_light_back(OracleView(oracle_mod, Q.light_side_scene(two_sided)), two_sided)


@pytest.mark.parametrize("variant", ["below", "up"])
def test_oracle_light_from_behind(oracle_mod, variant):
    Q.check_light_from_behind(OracleView(oracle_mod, Q.behind_scene(variant)), variant)


def test_oracle_fully_blocked_light(oracle_mod):
    Q.check_blocked(OracleView(oracle_mod, Q.blocked_scene()))


def test_oracle_light_seen_directly(oracle_mod):
    Q.check_seen_directly(OracleView(oracle_mod, Q.seen_scene()))


@pytest.mark.parametrize("camera", ["front", "below"])
def test_oracle_glass(oracle_mod, camera):
    print("largest error / tolerance:", Q.check_glass(OracleView(oracle_mod, Q.glass_scene(camera)), camera))
