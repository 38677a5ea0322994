"""Hit attributes and light at a path's SECOND hit, and the depth cap up to 16 bounces, on the device against the
independent reference tests/bounce_ref.py.  tests/test_bounce_ref.py runs the same checks (the check_* functions
below) against the oracle on the CPU, proves the reference and asserts every condition on the scenes from it alone.

tests/test_gpu_scene_queries.py pins hit_attributes (prt_shade.h) to scene_ref through the debug, AOV and query
kernels at FIRST hits; since the plain pipelines shade iteration 0 from the primary-surface record, the production
call sites (shade2_body in prt_shade2.h, k_shade2m in prt_wave2.hip) met varying UVs, maps of differing dimensions,
non-unit normals, a normal map or a non-identity instance only in device-against-oracle comparisons.  Here a mirror
or a glass pane sends every camera ray on to `attr`'s three instances, so those sites decode instance and primitive
from the queue word, take u, v from the hit record and build I and V = -D from a bounced ray -- and the expected
values are bounce_ref's.

Part 1 (48 x 36, bounces 2, one frame per call, test_gpu_estimator.FLAGS without the stochastic bit):
  mirror-over-attr  test_gpu_scene_queries.attr_scene()'s meshes, textures and instances under a MIRROR quad at
                    y = 2.5 facing down, camera (0.1, 0.8, -3) -> (-0.3, 5, 0.2); settings: every light dark (the
                    pixel is the second hit's emission texel, bit for bit), the directional light with NORMALMAP on,
                    and with it off
  glass-over-attr   the same instances under a DIELECTRIC pane at y = 1, camera (0, 5, -2) -> (-0.3, 0, 0.2);
                    settings: dark, and the directional light with NORMALMAP on; the extension kernels
The tolerance is bounce_ref's (derived in its docstring, no free factor); check_second_hit prints the worst
error / tolerance.  Every case renders three times on one context (dense, learning the records, answered from them)
and the three images are equal in every bit.  mirror-over-attr runs deferred (prt_stats.pipeline 3) and per-iteration
(2), and at 4 spp with AA in the three pipelines of test_gpu_pipeline_parity for equal bits.

Part 2 (32 x 24, every light dark, sky_ramp()): `hall`, a floor at y = 0 and a ceiling at y = 2 facing each other
over z in [0, length], |x| <= 100.  The ceiling is a MIRROR instance.  The floor is a TEXTURED instance whose
metalness texel reads metalness 1 / roughness 0 -- the same delta lobe (Core/Renderer.cpp:376) -- because a MIRROR
instance's emission is never set (Core/Scene.cpp:199-204, both restatements) and the floor's emission texel is what
shows the unwinding.  bounces 5 and 9 from camera (0, 0.7, -0.5) -> (0, 1.3, 10) in a hall 80 long, bounces 16 from
(0, 0.7, -0.5) -> (0, 1.6, 10) in a hall 100 long: at least 20 tested pixels with k = bounces - 1 mirror hits (the
sky arrives) and 20 with k = bounces (capped one short, exact).

Worst error / tolerance seen (the bound is 1); the oracle and an MI355X printed the same digits, the device
reproducing the oracle bit for bit (test_device_equals_oracle), in both pipelines:
  mirror-over-attr  dark 0 (exact)   directional, NORMALMAP on 0.0049   NORMALMAP off 0.0156
  glass-over-attr   dark 0.0039      directional, NORMALMAP on 0.0040
  hall              bounces 5, 9 and 16: 0.0044 (the sky's pixels; the capped ones exact)
Tested 1,497 to 1,550 of the 1,708 / 1,728 pixels that meet the pane / the mirror first.

What the checks found in the restatements: nothing.  What they found on the way: on the flat top of a narrow GGX lobe
(a2 clamped to 1e-5, nh clamped to 1 under a non-unit smooth normal) both restatements stand 0.27 % below the float64
closed form, which is the float32 cancellation in (a2 - 1) nh^2 + 1 that the reference's own arithmetic has;
bounce_ref.B_MIN leaves those hits out, from the reference alone (28 pixels at most in a case).
"""
import functools

import numpy as np
import pytest

import bounce_ref as B
import test_gpu_estimator as Q
import test_gpu_scene_queries as SQ
from prt import _lib, scenes
from test_gpu_pipeline_parity import PIPELINES
from wave_env import contexts, env_or_unset

F = np.float32
W, H = 48, 36
HALL_W, HALL_H = 32, 24
FLAGS = Q.FLAGS & ~_lib.FLAG_STOCHASTIC
MIRROR_CAM = ((0.1, 0.8, -3.0), (-0.3, 5.0, 0.2))
GLASS_CAM = ((0.0, 5.0, -2.0), (-0.3, 0.0, 0.2))
# the directional light (a position: Core/Renderer.cpp:272 aims at it from the hit point).  Mirror: below the mirror's
# plane y = 2.5 and off to one side, so no shadow ray that starts on a patch (y < 1) crosses the mirror.  Glass: below
# the pane's plane y = 1, for the same reason.
DIR_LIGHT = {"mirror-over-attr": ((-7.0, 2.0, -4.0), (24.0, 20.0, 16.0)),
             "glass-over-attr": ((-9.0, 0.9, -3.0), (24.0, 20.0, 16.0))}
# (scene, lights, NORMALMAP)
CASES = [("mirror-over-attr", "dark", True), ("mirror-over-attr", "dir", True), ("mirror-over-attr", "dir", False),
         ("glass-over-attr", "dark", True), ("glass-over-attr", "dir", True)]
HALL_CASES = {5: "short", 9: "short", 16: "long"}      # bounces -> camera
HALL_CAMS = {"short": ((0.0, 0.7, -0.5), (0.0, 1.3, 10.0), 80.0), "long": ((0.0, 0.7, -0.5), (0.0, 1.6, 10.0), 100.0)}


# ------------------------------------------------------------------------------------------------ scenes
def _level_quad(x0, x1, z0, z1, y, up, **tex):
    """A quad at height y whose face and vertex normals are (0, up, 0), as (v00, v01, v10), (v10, v01, v11)."""
    a, b = ((x0, z1), (x1, z0)) if up > 0 else ((x1, z0), (x0, z1))     # v01, v10: cross(v01 - v00, v10 - v00) = up
    c = np.array([[x0, y, z0], [a[0], y, a[1]], [b[0], y, b[1]], [x1, y, z1]])
    Pp = np.array([[c[0], c[1], c[2]], [c[2], c[1], c[3]]])
    return SQ._mesh(Pp, np.tile(np.array([0.0, float(up), 0.0]), (2, 3, 1)), np.full((2, 3, 2), 0.5), **tex)


@functools.lru_cache(None)
def over_attr_scene(name, lights):
    """`attr`'s meshes, textures and three instances under one more instance (identity): the mirror or the pane, with a
    1 x 1 albedo of its own."""
    a = SQ.attr_scene()
    tex = list(a.textures) + [np.array([[0x00D0C0B0]], np.uint32)]
    if name == "mirror-over-attr":
        top, kind, cam = _level_quad(-6.0, 6.0, -5.0, 4.0, 2.5, -1, albedo=len(tex) - 1), _lib.MAT_MIRROR, MIRROR_CAM
    else:
        top, kind, cam = _level_quad(-5.0, 4.5, -3.0, 3.0, 1.0, +1, albedo=len(tex) - 1), _lib.MAT_DIELECTRIC, GLASS_CAM
    lg = Q._dark_lights()
    if lights == "dir":
        lg.dir_pos[:], lg.dir_col[:] = DIR_LIGHT[name]
    inst = list(a.instances) + [(len(a.meshes), np.eye(4, dtype=F))]
    return scenes.SceneData(list(a.meshes) + [top], tex, inst, lg, None, np.array(cam[0], F), np.array(cam[1], F),
                            f"{name}-{lights}", materials=[_lib.MAT_TEXTURED] * 3 + [kind])


def case_flags(normalmap):
    return (FLAGS | _lib.FLAG_NORMALMAP) if normalmap else (FLAGS & ~_lib.FLAG_NORMALMAP)


@functools.lru_cache(None)
def bounce_ref(name, lights, normalmap, slip=None):
    return B.Bounce(over_attr_scene(name, lights), W, H, normalmap, lights != "dark", slip=slip)


@functools.lru_cache(None)
def hall_scene(camera):
    pos, target, length = HALL_CAMS[camera]
    tex = [np.array([[0x00C0B0A0]], np.uint32), np.array([[(0 << 8) | 255]], np.uint32),      # roughness 0, metalness 1
           np.array([[0x00302010]], np.uint32)]
    meshes = [_level_quad(-100.0, 100.0, 0.0, length, 0.0, +1, albedo=0, metalness=1, emission=2),
              _level_quad(-100.0, 100.0, 0.0, length, 2.0, -1, albedo=0)]
    inst = [(k, np.eye(4, dtype=F)) for k in range(2)]
    return scenes.SceneData(meshes, tex, inst, Q._dark_lights(), Q.sky_ramp(), np.array(pos, F), np.array(target, F),
                            "hall-" + camera, materials=[_lib.MAT_TEXTURED, _lib.MAT_MIRROR])


@functools.lru_cache(None)
def hall_ref(camera):
    return B.Hall(hall_scene(camera), HALL_W, HALL_H, Q.MARGIN)


HALL_FLAGS = FLAGS | _lib.FLAG_SKYBOX


# ------------------------------------------------------------------------------------------------ shared checks
# A `view` is one implementation under test loaded with one scene: view.calls(w, h, bounces, flags, n=3, spp=1) ->
# n consecutive calls with a static camera, each (avg [pixels, 3] float32, rgb8, segments, shadow_rays); the device's
# view also leaves prt_stats.pipeline of the last call in view.pipeline.
def same_calls(calls, what):
    """The dense pass, the pass that learns the records and the pass answered from them: equal in every bit."""
    for k in (1, 2):
        assert np.array_equal(SQ.bits(calls[k][0]), SQ.bits(calls[0][0])), (what, k, "avg")
        assert np.array_equal(calls[k][1], calls[0][1]), (what, k, "rgb8")
        assert calls[k][2:] == calls[0][2:], (what, k, "rays")
    return calls[0]


def check_second_hit(view, ref):
    """Every tested pixel of one case against bounce_ref.Bounce; returns the worst error / tolerance."""
    what = (view.sd.name, ref.normalmap)
    got = same_calls(view.calls(W, H, 2, case_flags(ref.normalmap)), what)[0]
    t = ref.tested
    assert t.sum() >= 180, (what, int(t.sum()))
    if ref.exact:
        SQ.assert_bits(got[t], ref.expected[t].astype(F), what)
    err = np.abs(got.astype(np.float64) - ref.expected)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / ref.tol, 0.0)[t]
    worst = float(ratio.max())
    print(f"{what}: tested {int(t.sum())} of {int(ref.first.sum())}, worst error / tolerance {worst:.4f}")
    bad = np.flatnonzero(t)[(ratio > 1.0).any(-1)]
    assert bad.size == 0, (what, bad.size, worst, bad[:5], got[bad[:3]], ref.expected[bad[:3]], ref.reach[bad[:5]])
    return worst


def check_hall(view, ref, bounces):
    """The depth cap at `bounces`: emission-only pixels (k >= bounces) exactly, the others within the tolerance."""
    exp, sky, tol = ref.expected(bounces)
    got = same_calls(view.calls(HALL_W, HALL_H, bounces, HALL_FLAGS), (view.sd.name, bounces))[0]
    t = ref.ok & (~sky | ref.seam_free)
    arrives, capped = t & (ref.k == bounces - 1), t & (ref.k == bounces)
    assert arrives.sum() >= 20 and capped.sum() >= 20, (bounces, int(arrives.sum()), int(capped.sum()))
    assert sky[arrives].all() and not sky[capped].any()
    SQ.assert_bits(got[t & ~sky], exp[t & ~sky], (view.sd.name, bounces, "emission only"))
    err = np.abs(got.astype(np.float64) - exp.astype(np.float64))[t & sky]
    worst = float((err / tol[t & sky]).max())
    print(f"{view.sd.name} bounces {bounces}: tested {int(t.sum())}, worst error / tolerance {worst:.4f}")
    assert (err <= tol[t & sky]).all(), (bounces, worst)
    return worst


def exact_runs():
    """(scene, w, h, bounces, flags) of every setting of this file, for the device = oracle comparison."""
    out = [(over_attr_scene(name, lights), W, H, 2, case_flags(nm)) for name, lights, nm in CASES]
    out += [(hall_scene(cam), HALL_W, HALL_H, b, HALL_FLAGS) for b, cam in HALL_CASES.items()]
    return out


def aa_runs():
    """(scene, w, h, bounces, flags) rendered at 4 spp with AA in the three pipelines."""
    return [(over_attr_scene("mirror-over-attr", "dir"), W, H, 2, case_flags(True) | _lib.FLAG_AA),
            (hall_scene("long"), HALL_W, HALL_H, 16, HALL_FLAGS | _lib.FLAG_AA)]


# ------------------------------------------------------------------------------------------------ the device
pytestmark = pytest.mark.gpu


class GpuView:
    """One scene on one context; the first call after loading is the dense one."""

    def __init__(self, ctx, sd):
        self.ctx, self.sd, self.pipeline, self.reused = ctx, sd, None, []

    def calls(self, w, h, bounces, flags, n=3, spp=1, seed=Q.SEED):
        from helpers import gpu_scene
        self.ctx.set_postfx(None)
        gpu_scene(self.ctx, self.sd, w, h)
        Q.GpuView._loaded = SQ.GpuView._loaded = None       # the other modules' views share this context
        out = []
        self.ctx.surface_reuse(reset=True)
        self.reused = []        # per call, the work items shaded from the primary-surface record
        for _ in range(n):
            self.ctx.reset_accumulation(full=True)
            avg, rgb8, st = self.ctx.render(w, h, spp, bounces, flags, 0, 0, seed)
            self.pipeline = int(st.pipeline)
            self.reused.append(int(self.ctx.surface_reuse(reset=True)))
            out.append((avg[:, :3].copy(), rgb8.copy(), int(st.segments), int(st.shadow_rays)))
        return out


PER_ITERATION = dict(PRT_MERGE="0", PRT_DEFER_RESOLVE="0")
DEFERRED = dict(PRT_MERGE=None, PRT_DEFER_RESOLVE=None)


@pytest.mark.parametrize("switches,pipeline", [(DEFERRED, 3), (PER_ITERATION, 2)], ids=["deferred", "per-iteration"])
@pytest.mark.parametrize("lights,normalmap", [c[1:] for c in CASES if c[0] == "mirror-over-attr"])
def test_second_hit_under_a_mirror(gpu_ctx, monkeypatch, lights, normalmap, switches, pipeline):
    view = GpuView(gpu_ctx, over_attr_scene("mirror-over-attr", lights))
    with env_or_unset(monkeypatch, **switches):
        check_second_hit(view, bounce_ref("mirror-over-attr", lights, normalmap))
    assert view.pipeline == pipeline
    assert view.reused == [0, 0, W * H], view.reused      # dense, learning, answered from the record


@pytest.mark.parametrize("lights,normalmap", [c[1:] for c in CASES if c[0] == "glass-over-attr"])
def test_second_hit_under_glass(gpu_ctx, lights, normalmap):
    view = GpuView(gpu_ctx, over_attr_scene("glass-over-attr", lights))
    check_second_hit(view, bounce_ref("glass-over-attr", lights, normalmap))
    assert view.pipeline == 2 and view.reused == [0, 0, 0], (view.pipeline, view.reused)    # the extension kernels


@pytest.mark.parametrize("switches,pipeline", [(DEFERRED, 3), (PER_ITERATION, 2)], ids=["deferred", "per-iteration"])
@pytest.mark.parametrize("bounces", sorted(HALL_CASES))
def test_depth_cap(gpu_ctx, monkeypatch, bounces, switches, pipeline):
    view = GpuView(gpu_ctx, hall_scene(HALL_CASES[bounces]))
    with env_or_unset(monkeypatch, **switches):
        check_hall(view, hall_ref(HALL_CASES[bounces]), bounces)
    assert view.pipeline == pipeline
    assert view.reused == [0, 0, HALL_W * HALL_H], view.reused


def test_three_pipelines_same_bits_with_aa(monkeypatch, oracle_mod):
    """mirror-over-attr (bounces 2) and the long hall (bounces 16) at 4 spp with AA: the per-iteration, the deferred and
    the merged pipeline, and the oracle, give the same average image, RGB8 image and ray counts."""
    for sd, w, h, bounces, flags in aa_runs():
        a_o, r_o, _, s_o = oracle_mod.OracleScene(sd, w, h).render(w, h, spp=4, bounces=bounces, flags=flags, seed=Q.SEED)
        want = (SQ.bits(a_o[:, :3]), r_o, (int(s_o.segments), int(s_o.shadow_rays)))
        with contexts(len(PIPELINES)) as cs:
            for c, (name, (switches, pipeline, launches)) in zip(cs, PIPELINES.items()):
                view = GpuView(c, sd)
                with env_or_unset(monkeypatch, **switches):
                    avg, rgb8, seg, sh = view.calls(w, h, bounces, flags, n=1, spp=4)[0]
                assert view.pipeline == pipeline, (sd.name, name, view.pipeline)
                assert np.array_equal(SQ.bits(avg), want[0]), (sd.name, name, "avg")
                assert np.array_equal(rgb8, want[1]), (sd.name, name, "rgb8")
                assert (seg, sh) == want[2], (sd.name, name, "rays")


def test_device_equals_oracle(gpu_ctx, oracle_mod):
    """Both scenes of part 1 under every setting, and the hall at every tested bounce count: image, RGB8, segments and
    shadow rays bit for bit."""
    for sd, w, h, bounces, flags in exact_runs():
        a_o, r_o, _, s_o = oracle_mod.OracleScene(sd, w, h).render(w, h, spp=1, bounces=bounces, flags=flags, seed=Q.SEED)
        a_g, r_g, seg, sh = GpuView(gpu_ctx, sd).calls(w, h, bounces, flags, n=1)[0]
        assert np.array_equal(SQ.bits(a_o[:, :3]), SQ.bits(a_g)), (sd.name, bounces, flags)
        assert np.array_equal(r_o, r_g), (sd.name, bounces, flags)
        assert (int(s_o.segments), int(s_o.shadow_rays)) == (seg, sh), (sd.name, bounces, flags)
