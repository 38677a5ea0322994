"""tests/test_gpu_texel.py's checks on the CPU: the oracle's texel_index (oracle/prt_oracle.c, through
orc_brdf_probe's PRT_PROBE_TEXEL) and the oracle's images of `uv_scene` against scene_ref.texel_index, bit for bit,
every record and every hit pixel.

The records are only as good as the wrong rules they tell apart: for each planted defect of scene_ref.TEXEL_SLIPS
the oracle disagrees with the slipped reference on at least one record (test_slip_is_caught prints which).  The
scenes of prt/scenes.py that the goldens and the benchmark use keep every UV >= 0, where the rule is the reference's
own (int)x % n, so defining the rest moves none of their results (test_shipped_scenes_have_no_negative_uv).
"""
import os

import numpy as np
import pytest

import scene_ref as R
import test_gpu_scene_queries as Q
import test_gpu_texel as T
from prt import _lib, scenes
from test_scene_ref import OracleView

F = np.float32


def test_texel_index_by_hand():
    """8 x 4 albedo.  Truncation toward zero, then a wrap into [0, n); 0 where uv * n has no int."""
    cases = [((-0.05, 0.0), 0),              # x = -0.4 truncates to 0: texel 0 is two texels wide around uv = 0
             ((-0.125, 0.0), 7),             # x = -1 -> 7
             ((-0.3, 0.0), 6),               # x = -2.4 -> -2 -> 6 (floor would say 5)
             ((-1.0, -1.0), 0),              # x = -8, -4 -> 0, 0
             ((0.0, -0.3), 3 * 8),           # y: -1.2 -> -1 -> 3
             ((-2.25, 2.6), 6 + 2 * 8),      # -18 -> -2 -> 6; 10.4 -> 10 % 4 = 2
             ((268435456.0, 0.3), 8),        # x = 2^31 exactly: out of range -> 0; row 1
             ((-268435456.0, 0.3), 8),       # x = -2^31 is an int, and still counts as out of range
             ((268435440.0, 0.0), 0),        # the float below 2^28: x = 2^31 - 128, a multiple of 8
             ((16777217.0 / 8, 0.0), 0),     # 2097152.125 * 8 = 16777217 is no float32: the product rounds to 2^24
             ((np.nan, 0.3), 8), ((0.3, np.nan), 2), ((np.inf, -np.inf), 0), ((3.4e38, -3.4e38), 0)]
    for uv, want in cases:
        assert R.texel_index(np.array(uv, F), 8, 4) == want, (uv, want)
    # int64 throughout: nothing wraps at 2^31 inside the reference itself
    assert R.texel_index(np.array([0.999, 0.999], F), 16384, 16384) == 16367 + 16367 * 16384


def test_vector_counts():
    rec, shape = T.texel_vectors()
    counts = [int((shape == i).sum()) for i in range(len(T.SHAPES))]
    print("records per shape:", dict(zip(T.SHAPES, counts)), "total", rec.shape[0])
    assert 1500 <= rec.shape[0] <= 6000   # a probe of a few thousand records stays a matter of milliseconds
    assert np.isnan(rec[:, :2]).any() and np.isinf(rec[:, :2]).any() and (rec[:, :2] < 0).any()
    for n in (1, 3, 5, 7, 8, 1000, 16384):   # the floats either side of 2^31 / n: the product decides, in float32
        below, at = T._range_edge(n)
        assert float(below) * n < 2.0 ** 31 <= float(at) * n and np.nextafter(below, F(np.inf)) == at


def test_oracle_probe_texel(oracle_mod):
    bad, rec, got, exp = T.check_texel_probe(oracle_mod.brdf_probe)
    assert bad.size == 0, (bad.size, [T.describe(rec, i) for i in bad[:5]], got[bad[:5], :2], exp[bad[:5], :2])


def test_oracle_probe_refuses_bad_sizes(oracle_mod):
    for w, h in ((0, 4), (4, 0), (-8, 4), (16385, 1), (2.5, 4), (np.nan, 4)):
        rec = np.zeros((1, 24), F)
        rec[0, 2:4] = (w, h)
        with pytest.raises(ValueError):
            oracle_mod.brdf_probe(_lib.PROBE_TEXEL, rec)


@pytest.mark.parametrize("slip", R.TEXEL_SLIPS)
def test_slip_is_caught(oracle_mod, slip):
    """The oracle disagrees with the slipped reference on some record: the records can see this wrong rule."""
    bad, rec, got, exp = T.check_texel_probe(oracle_mod.brdf_probe, slip)
    assert bad.size > 0, slip
    i = bad[0]
    print("%s: %d records differ, first %s: oracle (%g, %g), slipped reference (%g, %g)"
          % (slip, bad.size, T.describe(rec, i), got[i, 0], got[i, 1], exp[i, 0], exp[i, 1]))


@pytest.fixture(scope="module")
def uv_view(oracle_mod):
    return OracleView(oracle_mod, Q.uv_scene(), T.UV_W, T.UV_H)


def test_oracle_uv_scene_every_hit_pixel(uv_view):
    cov = T.check_uv_scene(uv_view, uv_view.sd)
    print("coverage:", cov)
    assert cov["pixels"] > 1000


def test_oracle_uv_scene_shifted(oracle_mod):
    """The scene the update tests move to: the same checks and the same coverage."""
    sd = Q.uv_scene(7)
    T.check_uv_scene(OracleView(oracle_mod, sd, T.UV_W, T.UV_H), sd, 7)


def test_uv_scene_layout():
    """The triangles stay inside the image, each class is present in both components, and the 12 varying triangles
    straddle 0 or -1 in each component."""
    sd = Q.uv_scene()
    classes, const = Q.uv_triangle_classes()
    assert len(classes) == 60 and sd.meshes[0].tri_count == 60
    uv = sd.meshes[0].fixed_uvs.reshape(60, 3, 2)
    assert (uv[:48] == uv[:48, :1]).all() and np.array_equal(uv[:48, 0], const)
    assert np.isfinite(uv).all() and (uv == -1).any() and (np.abs(uv) > 1e30).any()
    for axis in (0, 1):
        assert {c[axis] for c in classes} == {name for name, _ in Q.UV_CLASSES} | {"straddle"}
    lo, hi = uv[48:].min(1), uv[48:].max(1)
    assert (((lo < 0) & (hi > 0)) | ((lo < -1) & (hi > -1))).all()
    for t in sd.textures:   # distinct texels: a wrong texel shows
        assert np.unique(t).size == t.size
    m = sd.textures[2]
    assert np.unique(m & 0xFF).size == m.size and np.unique((m >> 8) & 0xFF).size == m.size


# ------------------------------------------------------------------------------------------------ defined results stay
SHIPPED = {"config_small": scenes.config_small, "multi_instance": lambda: scenes.multi_instance(scenes.config_small()),
           "config_c2": scenes.config_c2, "config_c3": scenes.config_c3, "config_c4": scenes.config_c4,
           "config_c5": scenes.config_c5, "instance_field": scenes.instance_field, "deep_bvh": scenes.deep_bvh,
           "torus": lambda: scenes.torus(), "config_c1": scenes.config_c1, "config_spaceship": scenes.config_spaceship}


@pytest.mark.parametrize("name", sorted(SHIPPED))
def test_shipped_scenes_have_no_negative_uv(name):
    """Every scene of prt/scenes.py behind tests/golden and bench.py keeps its UVs finite and >= 0: texel addressing
    there is the reference's own (int)x % n, which this rule leaves as it was, so no golden moves.  The two scenes
    read from the reference's asset tree are checked where that tree is."""
    if name in ("config_c1", "config_spaceship") and not os.path.isdir(os.path.join(scenes.REFERENCE_ROOT, "Core", "assets")):
        return
    sd = SHIPPED[name]()
    for m in (sd.meshes if hasattr(sd, "meshes") else [sd]):
        uv = np.asarray(m.fixed_uvs)
        assert np.isfinite(uv).all() and uv.min() >= 0, (name, float(uv.min()))
