"""tests/path_ref.py proven on the CPU, then the checks of tests/test_gpu_path.py run against the oracle
(oracle/prt_oracle.c).

What the reference is held to:
  a deterministic reference   on sky-floor at bounces 2 a path's expectation is a 2-D integral over the unit square
      of the indirect sample's u: E_u[sky(L_spec(u))] + E_u[w_diff(u) sky(L_diff(u))] -- the lobe probability cancels
      against the division by it, the specular weight is (1, 1, 1), and every bounced ray leaves the one planar quad,
      also the specular ones that start below it.  A K x K midpoint quadrature of it, built from estimator_ref's
      rotate / vndf / sample_hemisphere / diffuse_weight and scene_ref.sample_sky (no path_ref code), must agree with the
      Monte Carlo mean within 6 of ITS standard errors plus |E_K - E_2K| (K = 48).
  scene_ref.direct_light      at bounces 1 the corner's pixels are emission + one light class: the plain value exactly,
      the stochastic mean within 6 standard errors of 0.3 sum_i P(whichLight = i) point_i + 0.5 dir + 0.2 spot.
  power                       for every case and channel 6 sqrt(sum sigma^2 (1 / n + 1 / M)) is below 10 % of the summed
      expectation, and every tested pixel's sigma is above 1e-3 of its mean, so that the float32 arithmetic of an
      implementation (1e-6 of the mean) is nothing against the pixel's bound.
  the slips                   each planted defect moves the summed expectation of the case named below by more than that
      case's summed bound (plus 6 standard errors of the slipped run itself, which uses SLIP_M paths per pixel):
        no_lobe_division                  sky-floor (0.5, 0.5), bounces 2
        direct_not_scaled_by_throughput   corner-plain, bounces 3
        indirect_miss_is_black            sky-floor (1, 0), bounces 2
        emission_only_at_first_hit        glass-over-floor, bounces 3
        cap_one_early                     sky-floor (0.25, 1), bounces 2
        cap_one_late                      corner-plain, bounces 2
        spec_below_horizon_ends_path      sky-floor (1, 0), bounces 2
        last_segment_weighted_everywhere  corner-area, bounces 1
        glass_children_swapped            glass-over-floor, bounces 3
        bounced_ray_not_transformed       corner-turned-plain, bounces 3 (a hit at depth >= 1 shaded with the
                                          rectangle's object-space normal; moved / needed 7 to 9)
      Smallest margin: direct_not_scaled_by_throughput, 2.8 times what is needed in blue (0.8 in red): the lobe mixture
      hides most of it (the specular lobe's throughput 1 / p is above 1, the diffuse one's below), which is why the
      corner's floor is all metal.  The weighted last segment moves corner-area at bounces 3 by 0.05 of its bound -- the
      third vertex carries little -- so that scene is also run at bounces 1, where its first hit is the last segment.

What the checks found in the restatements: nothing.  The oracle lies inside every bound.  Largest z (the bound is 6)
seen on the oracle, as largest pixel / largest channel sum:
  sky-floor (1, 0)      bounces 2: 2.75 / 0.63   bounces 3: 2.75 / 0.62
  sky-floor (0.5, 0.5)  bounces 2: 2.42 / 1.95   bounces 3: 2.42 / 1.95
  sky-floor (0.25, 1)   bounces 2: 2.81 / 1.10   bounces 3: 2.81 / 1.10
  corner-plain          bounces 2: 2.49 / 0.89   bounces 3: 2.81 / 1.83   bounces 4: 2.71 / 1.71
  corner-stochastic     bounces 3: 2.11 / 0.37
  corner-area           bounces 1: 2.23 / 0.39   bounces 3: 3.05 / 1.50
  glass-over-floor      bounces 3: 2.57 / 1.22   bounces 4: 2.51 / 1.21
  corner-turned         plain, bounces 3: 2.80 / 2.17   stochastic, bounces 3: 2.47 / 0.55
  mirror-corner         largest error / tolerance 0.0019
(the cases share their seeds: the same sign of the summed deviation in most of them is one draw, not fourteen).
With a (0.25, 1) floor in the corner one pixel of corner-stochastic stood at z = 6.08: the narrow lobe's BRDF towards a
point light is a heavy-tailed term, whose sigma 16384 paths underestimate by half (65536 paths of three other seeds
and four other blocks of 4096 oracle frames agree with each other); the corner's floor is (0.5, 1) for that reason.

The reference's CPU time: 3 to 7 s per case, 60 tested pixels x 16384 paths each (the 16 cases together about 70 s);
the oracle's 4096 frames take 3 to 6 s per case, a slipped run of 8192 paths about 2 s.
"""
import numpy as np
import pytest

import estimator_ref as E
import path_ref as P
import scene_ref as R
import test_gpu_estimator as Q
import test_gpu_path as T
import test_gpu_scene_queries as SQ

SLIP_M = 8192
SLIP_CASES = {
    "no_lobe_division": ("sky-floor-0.5-0.5", 2),
    "direct_not_scaled_by_throughput": ("corner-plain", 3),
    "indirect_miss_is_black": ("sky-floor-1.0-0.0", 2),
    "emission_only_at_first_hit": ("glass-over-floor", 3),
    "cap_one_early": ("sky-floor-0.25-1.0", 2),
    "cap_one_late": ("corner-plain", 2),
    "spec_below_horizon_ends_path": ("sky-floor-1.0-0.0", 2),
    "last_segment_weighted_everywhere": ("corner-area", 1),
    "glass_children_swapped": ("glass-over-floor", 3),
    "bounced_ray_not_transformed": ("corner-turned-plain", 3),
}


# ------------------------------------------------------------------------------------------------ the reference alone
def test_path_ref_imports_neither_restatement():
    import sys
    src = open(P.__file__).read()
    assert "import oracle" not in src and "import prt" not in src and "from prt" not in src
    assert set(SLIP_CASES) == set(P.SLIPS)
    assert P.__name__ in sys.modules


def _sky_floor_quadrature(name, sel, K):
    """E_u[sky(L_spec(u))] + E_u[w_diff(u) sky(L_diff(u))] per pixel of `sel`, on the K x K midpoints."""
    sd = T.scene_table()[name][0]
    g = Q.Geometry(sd)
    n = sel.size
    N, V = g.N[sel], g.V[sel]
    base, metal, rough = (np.asarray(g.mat[k][sel], np.float64) for k in ("base", "metalness", "roughness"))
    t = (np.arange(K) + 0.5) / K
    u = np.broadcast_to(np.stack(np.meshgrid(t, t, indexing="ij"), -1).reshape(1, K * K, 2), (n, K * K, 2))
    q = E.rotation_to_z(N)
    back = q * np.array([-1.0, -1.0, -1.0, 1.0])
    Vl = E.rotate(q, V)
    Hs = E.vndf(Vl, rough * rough, u)
    Ls = 2.0 * E._dot(Vl[:, None, :], Hs)[..., None] * Hs - Vl[:, None, :]
    Ld = E.sample_hemisphere(u)
    wd = E.diffuse_weight(u, N, V, base, metal, rough)

    def sky(Ll):
        Dw = E._unit(E.rotate(back, Ll)).reshape(-1, 3)
        return R.sample_sky(sd.sky, R.ray_ctor_dir(Dw.astype(np.float32))).astype(np.float64).reshape(n, K * K, 3)

    dead = (wd @ np.array([0.2126, 0.7152, 0.0722])) == 0.0          # a weight of zero luminance ends the path
    return sky(Ls).mean(1) + np.where(dead[..., None], 0.0, wd * sky(Ld)).mean(1)


@pytest.mark.parametrize("rough,metal", Q.MATERIALS)
def test_monte_carlo_agrees_with_the_quadrature(rough, metal):
    name = f"sky-floor-{rough}-{metal}"
    ref = T.path_ref(name, 2)
    assert np.array_equal(ref.sel, np.intersect1d(ref.sel, np.flatnonzero(Q.Geometry(T.scene_table()[name][0]).floor)))
    coarse, fine = _sky_floor_quadrature(name, ref.sel, 48), _sky_floor_quadrature(name, ref.sel, 96)
    allow = np.abs(fine - coarse)
    se = ref.sigma / np.sqrt(ref.M)
    zp = (np.abs(ref.mean - fine) - allow) / se
    zs = (np.abs(ref.mean.sum(0) - fine.sum(0)) - allow.sum(0)) / np.sqrt((se ** 2).sum(0))
    print(f"{name}: Monte Carlo sum {ref.mean.sum(0).round(3)} quadrature {fine.sum(0).round(3)} allowance "
          f"{allow.sum(0).round(3)}, largest z pixel {zp.max():.2f} sum {zs.max():.2f}")
    assert (allow.sum(0) <= 0.1).all()
    assert (zp <= 6.0).all() and (zs <= 6.0).all(), (float(zp.max()), zs)


@pytest.mark.parametrize("variant", ["plain", "stochastic"])
def test_one_bounce_equals_scene_ref(variant):
    name = "corner-" + variant
    sd = T.scene_table()[name][0]
    ref = T.path_ref(name, 1)
    s = T.ref_scene(name)
    O, D = s.primary(T.W, T.H)
    O, D = O[ref.sel], D[ref.sel]
    t, idx = s.closest(O, D)
    I = O + t[:, None] * D
    N = np.stack([s.rects[k].N for k in idx])
    mat = {k: np.stack([np.asarray(getattr(s.rects[j], a), np.float64) for j in idx])
           for k, a in (("base", "base"), ("metalness", "metal"), ("roughness", "rough"), ("emissive", "emis"))}
    d = R.direct_light(I, N, -D, mat, sd.lights, R.visibility(I, sd.lights, SQ.world_triangles(sd)[0]))
    if variant == "plain":
        assert np.allclose(ref.mean, d["plain"], rtol=1e-6, atol=1e-12)
        assert (ref.sigma <= 1e-9 * (1.0 + np.abs(ref.mean))).all()
        assert ((d["plain"] - mat["emissive"]).sum(1) > 0).sum() >= 40        # lit, and some pixels in the quad's shadow
        dark = (d["plain"] - mat["emissive"]).sum(1) == 0
        assert dark[ref.cls == "floor"].sum() >= 1 and dark[ref.cls == "wall"].sum() >= 1 and dark.sum() >= 3, (dark.sum(), ref.cls[dark])
        return
    which = np.array([0.3, 0.3, 0.2, 0.2])                                    # (int)(u * 10) % 4: {0,4,8} {1,5,9} {2,6} {3,7}
    exp = (float(R.P_POINT) * np.tensordot(which, d["point"], 1) + float(R.P_DIR) * d["dir"]
           + float(R.P_SPOT) * d["spot"])
    for k in ("dir", "spot"):                                                 # every class contributes
        assert ((d[k] - mat["emissive"]).sum(1) > 0).sum() >= 10, k
    assert ((d["point"] - mat["emissive"]).sum(-1) > 0).all(0).sum() >= 10
    se = ref.sigma / np.sqrt(ref.M)
    z = np.abs(ref.mean - exp) / se
    zs = np.abs(ref.mean.sum(0) - exp.sum(0)) / np.sqrt((se ** 2).sum(0))
    print(f"{name}: largest z pixel {z.max():.2f} sum {zs.max():.2f}")
    assert (z <= 6.0).all() and (zs <= 6.0).all(), (float(z.max()), zs)


@pytest.mark.parametrize("name,bounces", T.STAT_CASES)
def test_bound_is_tight(name, bounces):
    ref = T.path_ref(name, bounces)
    print(f"{name} bounces {bounces}: reference {ref.seconds:.1f} s, bound / expectation "
          f"{(ref.sum_bound / ref.mean.sum(0)).round(4)}")
    assert ref.M >= 4 * ref.n and ref.n >= 4096
    assert ref.sel.size >= 60 and all((ref.cls == c).sum() >= 20 for c in set(ref.cls))
    assert (ref.sum_bound < 0.1 * ref.mean.sum(0)).all(), ref.sum_bound / ref.mean.sum(0)
    assert (ref.sigma >= 1e-3 * ref.mean).all() and (ref.mean >= 0).all()


@pytest.mark.parametrize("slip", P.SLIPS)
def test_slip_is_caught(slip):
    name, bounces = SLIP_CASES[slip]
    ref = T.path_ref(name, bounces)
    mean, sigma = T.ref_scene(name).estimate(ref.sel, T.W, T.H, bounces, SLIP_M, T.REF_SEED + 1, slip=slip)
    moved = np.abs(mean.sum(0) - ref.mean.sum(0))
    need = ref.sum_bound + 6.0 * np.sqrt((sigma ** 2).sum(0) / SLIP_M)
    print(f"{slip} on {name} bounces {bounces}: sum {mean.sum(0).round(3)} against {ref.mean.sum(0).round(3)}, "
          f"moved / needed {(moved / need).round(2)}")
    assert (moved > need).any(), (slip, moved, need)


# ------------------------------------------------------------------------------------------------ the oracle
class OracleView:
    def __init__(self, oracle_mod, sd, flags):
        self.sd, self.flags = sd, flags
        self.osc = oracle_mod.OracleScene(sd, T.W, T.H)

    def frames(self, bounces, k, frame_index=0):
        avg, rgb8, _, st = self.osc.render(T.W, T.H, spp=k, bounces=bounces, flags=self.flags,
                                           frame_index=frame_index, seed=Q.SEED)
        return avg[:, :3].copy(), rgb8, int(st.segments), int(st.shadow_rays)

    def mean(self, bounces, n):
        total = np.zeros((T.W * T.H, 3), np.float64)
        for f0 in range(0, n, Q.CHUNK):
            total += self.frames(bounces, Q.CHUNK, f0)[0].astype(np.float64)
        return total / (n // Q.CHUNK)


@pytest.mark.parametrize("name,bounces", T.STAT_CASES)
def test_oracle_path_expectation(oracle_mod, name, bounces):
    T.check_path(OracleView(oracle_mod, T.scene_table()[name][0], T.scene_flags(name)), T.path_ref(name, bounces))


def test_oracle_mirror_corner(oracle_mod):
    print("largest error / tolerance:",
          T.check_mirror_corner(OracleView(oracle_mod, T.corner_scene("mirror"), T.scene_flags("mirror-corner"))))
