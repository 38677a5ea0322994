"""tests/bounce_ref.py proven on the CPU, every condition on the scenes of tests/test_gpu_bounce.py asserted from the
reference alone, then that file's checks run against the oracle (oracle/prt_oracle.c).

What the reference is held to:
  geometry     the brute force's first hits are the mirror / the pane where a closed form says so (t = (y - O.y) / D.y
               inside the quad's outline), and the counts of second hits per instance are the ones a separate float64
               simulation gave when the scenes were designed (mirror 144 / 118 / 155, glass 189 / 140 / 181 of 1,708)
  conditions   per second-hit instance at least half of the pixels that reach it, and at least 60, are tested; the
               tested second hits cover the mapped and the smooth branch, a wrapped UV, a map whose own dimensions
               would place the texel elsewhere and the non-uniformly scaled instance; in every lit case at least 30 are
               lit and 30 shadowed; NORMALMAP moves at least 60 tested pixels by more than 100 tol; the hall gives at
               least 20 tested pixels with k = bounces - 1 and 20 with k = bounces at bounces 5, 9 and 16
  the slips    every planted defect of bounce_ref.SLIPS moves at least 20 tested pixels of some case by more than
               100 tol (the emission-only case: in its bits), and cap_one_early / cap_one_late fail at every bounce count

What the checks found in the restatements: see tests/test_gpu_bounce.py.
"""
import numpy as np
import pytest

import bounce_ref as B
import scene_ref as R
import test_gpu_bounce as T
import test_gpu_estimator as Q
import test_gpu_scene_queries as SQ

REACH = {"mirror-over-attr": (144, 118, 155), "glass-over-attr": (189, 140, 181)}


# ------------------------------------------------------------------------------------------------ the reference alone
def test_bounce_ref_imports_neither_restatement():
    import sys
    src = open(B.__file__).read()
    assert "import oracle" not in src and "import prt" not in src and "from prt" not in src
    assert B.__name__ in sys.modules
    tris, first = B.world_triangles(SQ.attr_scene())
    want = SQ.world_triangles(SQ.attr_scene())
    assert np.array_equal(tris, want[0]) and np.array_equal(first, want[1])


@pytest.mark.parametrize("name", ["mirror-over-attr", "glass-over-attr"])
def test_first_and_second_hits(name):
    sd = T.over_attr_scene(name, "dark")
    ref = T.bounce_ref(name, "dark", True)
    O, D = SQ.camera_rays(sd, T.W, T.H)
    O, D = O.astype(np.float64), R.ray_ctor_dir(D).astype(np.float64)
    v = np.asarray(sd.meshes[-1].vertices, np.float64).reshape(-1, 3)
    y = v[0, 1]
    t = (y - O[:, 1]) / D[:, 1]
    I = O + t[:, None] * D
    inside = (t > 0) & (I[:, 0] > v[:, 0].min()) & (I[:, 0] < v[:, 0].max()) & (I[:, 2] > v[:, 2].min()) & (I[:, 2] < v[:, 2].max())
    # nothing lies between the camera and the quad: the quad is the first hit exactly where the plane point is inside
    assert np.array_equal(ref.first, inside)
    assert int(ref.first.sum()) == (1728 if name.startswith("mirror") else 1708)
    assert tuple(int((ref.reach == i).sum()) for i in range(3)) == REACH[name]
    if name.startswith("glass"):
        assert not ref.excluded["k_refract"].any()                 # every camera ray refracts


@pytest.mark.parametrize("name,lights,normalmap", T.CASES)
def test_conditions(name, lights, normalmap):
    ref = T.bounce_ref(name, lights, normalmap)
    lost = {k: int((v & ref.first).sum()) for k, v in ref.excluded.items()}
    print(f"{name} {lights} normalmap={normalmap}: first {int(ref.first.sum())}, tested {int(ref.tested.sum())}, "
          f"excluded by {lost}, cover {ref.cover}, lit {int((ref.lit & ref.tested).sum())}, "
          f"shadowed {int((ref.shadowed & ref.tested).sum())}")
    for i in range(3):
        reach, tested = ref.reach == i, (ref.reach == i) & ref.tested
        assert tested.sum() >= 60 and tested.sum() >= 0.5 * reach.sum(), (i, int(tested.sum()), int(reach.sum()))
    c = ref.cover
    assert c["smooth"] > 0 and c["uv_ge_1"] > 0 and c["own_dims_differ"] > 0 and c["scaled"] > 0, c
    assert (c["mapped"] > 0) == normalmap, c
    if lights == "dir":
        assert (ref.lit & ref.tested).sum() >= 30 and (ref.shadowed & ref.tested).sum() >= 30
    if ref.exact:       # many different texels are met
        assert len(np.unique(ref.expected[ref.tested & (ref.reach >= 0)], axis=0)) >= 20


def test_normalmap_flag_is_observable():
    on, off = (T.bounce_ref("mirror-over-attr", "dir", nm) for nm in (True, False))
    both = on.tested & off.tested
    far = (np.abs(on.expected - off.expected) > 100 * np.maximum(on.tol, off.tol)).any(-1) & both
    print("NORMALMAP moves", int(far.sum()), "of", int(both.sum()), "pixels tested under both flags")
    assert far.sum() >= 60, int(far.sum())


def test_dark_mirror_is_the_emission_texel():
    """The exact case's expectation is scene_ref.material()'s emission at the brute force's hit, float32 as decoded."""
    ref = T.bounce_ref("mirror-over-attr", "dark", True)
    t = ref.tested & (ref.reach >= 0)
    assert np.array_equal(ref.expected[t], ref.expected[t].astype(np.float32).astype(np.float64))
    emis = np.concatenate([R.color_from_texel(np.asarray(x).reshape(-1)) for x in (SQ.attr_scene().textures[3],)])
    rows = {tuple(r) for r in emis.astype(np.float64)} | {(0.0, 0.0, 0.0)}
    assert all(tuple(r) in rows for r in ref.expected[t])
    assert (ref.expected[t & (ref.reach == 1)] == 0).all()        # mesh 1 has no emission map


@pytest.mark.parametrize("slip", B.SLIPS)
def test_slip_is_caught(slip):
    best = (-1, ())
    for name, lights, normalmap in T.CASES:
        true = T.bounce_ref(name, lights, normalmap)
        n = true.differs(T.bounce_ref(name, lights, normalmap, slip), true.tested)
        best = max(best, (n, (name, lights, normalmap)))
    print(f"{slip}: {best[0]} tested pixels of {best[1]} differ")
    assert best[0] >= 20, best


@pytest.mark.parametrize("camera", ["short", "long"])
def test_hall_histogram(camera):
    ref = T.hall_ref(camera)
    hist = np.bincount(ref.k[ref.ok], minlength=25)
    print(camera, "k histogram of the tested pixels", hist.tolist(), "excluded", int((~ref.ok).sum()))
    want = range(10, 20) if camera == "long" else range(0, 10)
    assert all(hist[k] >= 32 for k in want), hist
    assert not ref.capped[ref.k < 20].any()
    assert float(ref.emis.min()) > 0


@pytest.mark.parametrize("bounces", sorted(T.HALL_CASES))
def test_hall_conditions_and_slips(bounces):
    ref = T.hall_ref(T.HALL_CASES[bounces])
    exp, sky, tol = ref.expected(bounces)
    t = ref.ok & (~sky | ref.seam_free)
    assert (t & (ref.k == bounces - 1)).sum() >= 20 and (t & (ref.k == bounces)).sum() >= 20
    floor_hits = (ref.floor[:, :bounces]).sum(1)
    assert floor_hits[t & (ref.k == bounces)].min() >= bounces // 2          # emission is gathered at every other hit
    for slip in B.HALL_SLIPS:
        got = ref.expected(bounces, slip)[0]
        far = (np.abs(got.astype(np.float64) - exp.astype(np.float64)) > 100 * np.maximum(tol, 1e-7)).any(-1) & t
        print(f"bounces {bounces} {slip}: {int(far.sum())} tested pixels differ")
        assert far.sum() >= 20, (slip, int(far.sum()))


# ------------------------------------------------------------------------------------------------ the oracle
class OracleView:
    pipeline = None

    def __init__(self, oracle_mod, sd):
        self.o, self.sd = oracle_mod, sd

    def calls(self, w, h, bounces, flags, n=3, spp=1, seed=Q.SEED):
        out = []
        for _ in range(n):       # a fresh scene per call: the oracle keeps no records
            avg, rgb8, _, st = self.o.OracleScene(self.sd, w, h).render(w, h, spp=spp, bounces=bounces, flags=flags,
                                                                      seed=seed)
            out.append((avg[:, :3].copy(), rgb8, int(st.segments), int(st.shadow_rays)))
        return out


@pytest.mark.parametrize("name,lights,normalmap", T.CASES)
def test_oracle_second_hit(oracle_mod, name, lights, normalmap):
    T.check_second_hit(OracleView(oracle_mod, T.over_attr_scene(name, lights)), T.bounce_ref(name, lights, normalmap))


@pytest.mark.parametrize("bounces", sorted(T.HALL_CASES))
def test_oracle_depth_cap(oracle_mod, bounces):
    T.check_hall(OracleView(oracle_mod, T.hall_scene(T.HALL_CASES[bounces])), T.hall_ref(T.HALL_CASES[bounces]), bounces)
