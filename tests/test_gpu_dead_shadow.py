"""Dead shadow rays (include/prt.h prt_shadow_dead, prt_wave2.hip): a next-event shadow ray whose unoccluded
contribution is exactly zero in every channel (the light behind the shading normal, the hit point outside the spot's
cone, a black light), or any shadow ray of a render without PRT_FLAG_LIGHTED, cannot change a bit of the image.  The
shading kernels count such rays instead of queueing them (the extensions form too, for its light-class rays); the rays
under the light-visibility record (iteration 0 of a static view) are asked, learned and counted as before.

Everything here is exact: each call's avg and rgb8 (np.array_equal), its (segments, shadow_rays) and the running
ray_totals() equal those of a fresh context rendering the same calls with PRT_DEAD_SHADOW=0, where every shadow ray
is traced.  The dead count is asserted throughout: without it the comparisons would pass with nothing skipped, and
without its upper bound they would pass with live rays skipped wherever those happen to be occluded
(test_gpu_shadow_reuse.py test_scene_has_both_answers: the instance field has unoccluded rays).

Shapes as test_gpu_shadow_reuse.py: 96x64 and 70x45, bounces 3; spp 4 is two reference frames per call, spp 6
three."""
import dataclasses

import numpy as np
import pytest

import prt
from helpers import gpu_scene
from prt import _lib, scenes, tiles
from wave_env import contexts, env as _env

pytestmark = pytest.mark.gpu

B = 3
SIZES = [(96, 64), (70, 45)]
DEFAULT = _lib.FLAGS_DEFAULT


def _contexts(n=2):
    return contexts(n)


def _call(c, W, H, spp, fi, **kw):
    a, r, st = c.render(W, H, spp, kw.pop("bounces", B), frame_index=fi, **kw)
    return a, r, (st.segments, st.shadow_rays)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


def _pair(monkeypatch, c, ref, W, H, spp, fi, what="", **kw):
    """One call on c and the same call with every shadow ray traced on ref: equal, and ref counted no dead ray.
    Returns (dead rays of c's call, shadow rays of the call)."""
    got = _call(c, W, H, spp, fi, **kw)
    with _env(monkeypatch, PRT_DEAD_SHADOW="0"):
        want = _call(ref, W, H, spp, fi, **kw)
    _same(got, want, what)
    assert ref.shadow_dead() == 0, what
    return c.shadow_dead(reset=True), got[2][1]


def _camera(sd, W, H, k):
    return prt.Camera(np.asarray(sd.cam_pos, np.float32) + np.float32(0.125 * k), sd.cam_target,
                      np.float32(W) / np.float32(H))


def _scene(name):
    return scenes.instance_field(40, seed=9) if name == "field" else scenes.config_small()


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("spp", [4, 6])
@pytest.mark.parametrize("W,H", SIZES)
def test_engages_and_is_exact(monkeypatch, W, H, spp, moving, merge):
    """Six calls with rising frame_index.  moving: a new camera before every call, so every call traces its primary
    hits anew and iteration 0 runs the plain shading form, dead rays skipped there too; static: from call 2 on
    iteration 0 runs under the light-visibility record.  Some but not all shadow rays of every call are dead, the
    switched-off context counts none, and every call and the running totals are equal."""
    sd = _scene("field")
    F = spp // 2
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        assert c.shadow_dead() == 0
        for k in range(6):
            if moving:
                for x in (c, ref):
                    x.set_camera(_camera(sd, W, H, k + 1))
            dead, shadow = _pair(monkeypatch, c, ref, W, H, spp, F * k, k)
            assert 0 < dead < shadow, (k, dead, shadow)
        assert c.ray_totals() == ref.ray_totals()
        assert c.shadow_dead() == 0  # (every read above reset it)
        assert (c.shadow_reuse() == 0) == moving


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("what,scene", [("unlit", "field"), ("unlit", "small"), ("black", "field"),
                                        ("black", "small"), ("below", "small")])
def test_exact_counts(monkeypatch, what, scene, merge):
    """With PRT_PRIMARY_REUSE=0 no ray is under the record, and every shadow ray of a call is dead by construction:
    unlit: PRT_FLAG_LIGHTED off; black: every light colour zero; below: without PRT_FLAG_STOCHASTIC every hit asks
    for the directional light alone, which stands far below the scene, so every up-facing hit has a clearly negative
    cosine.  `below` runs on config_small with the normal map off only (a heightfield's normals all face up; the
    instance field's tori have faces that look down and keep some rays live)."""
    sd = _scene(scene)
    lt = sd.lights
    flags = DEFAULT
    if what == "unlit":
        flags = DEFAULT & ~_lib.FLAG_LIGHTED
    elif what == "black":
        z3 = np.zeros(3, np.float32)
        lt = dataclasses.replace(lt, point_col=np.zeros((4, 3), np.float32), dir_col=z3, spot_col=z3)
    else:
        flags = DEFAULT & ~_lib.FLAG_STOCHASTIC & ~_lib.FLAG_NORMALMAP
        lt = dataclasses.replace(lt, dir_pos=np.array([0.0, -1000.0, 0.0], np.float32))
    sd = dataclasses.replace(sd, lights=lt)
    W, H = 70, 45
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge, PRT_PRIMARY_REUSE="0"):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(3):
            dead, shadow = _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k, flags=flags)
            assert shadow > 0 and dead == shadow, (k, dead, shadow)
        assert c.ray_totals() == ref.ray_totals()


@pytest.mark.parametrize("merge", ["0", "1"])
def test_nothing_is_cached(monkeypatch, merge):
    """Deadness depends on the spot direction, the colours and the flags, none of which clear the primary hits or the
    light-visibility record: between the calls of a static view the spot's cone leaves the frame and comes back, a
    light turns black and back, and the normal map goes off and on.  Every call equals the switched-off render, and
    the dead count follows the colours."""
    sd = _scene("field")
    W, H = 96, 64
    away = dataclasses.replace(sd.lights, spot_rot=np.array([1.0, 0.0, 0.0], np.float32))
    black = dataclasses.replace(sd.lights, point_col=np.array(sd.lights.point_col, np.float32) * np.float32(0),
                                dir_col=np.zeros(3, np.float32))
    nomap = DEFAULT & ~_lib.FLAG_NORMALMAP
    steps = [(sd.lights, DEFAULT), (sd.lights, DEFAULT), (sd.lights, DEFAULT), (away, DEFAULT), (sd.lights, DEFAULT),
             (black, DEFAULT), (sd.lights, DEFAULT), (sd.lights, nomap), (sd.lights, DEFAULT), (away, nomap),
             (sd.lights, DEFAULT)]
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        share = []
        for k, (lt, flags) in enumerate(steps):
            for x in (c, ref):
                x.set_lights(lt)
            dead, shadow = _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k, flags=flags)
            assert 0 < dead < shadow, (k, dead, shadow)
            share.append(dead / shadow)
        # (with the point lights and the directional light black every ray towards them is dead, not about a third)
        assert share[5] > share[4] and share[5] > share[6], share
        assert c.ray_totals() == ref.ray_totals()
        assert c.primary_rays() == (W * H, W * H * (2 * len(steps) - 1))  # one dense pass in all


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("W,H", SIZES)
def test_with_the_record(monkeypatch, W, H, merge):
    """Static camera, six calls: the light-visibility record answers nothing in calls 1 (dense) and 2 (learning)
    and something in every later call, as test_gpu_shadow_reuse.py asserts; a ray is counted at most once, so what the
    record answered plus the dead rays never exceeds the call's shadow rays."""
    sd = _scene("field")
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(6):
            dead, shadow = _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k)
            reused = c.shadow_reuse(reset=True)
            assert (reused == 0) if k < 2 else (reused > 0), (k, reused)
            assert 0 < dead and reused + dead <= shadow, (k, reused, dead, shadow)
            assert ref.shadow_reuse(reset=True) == reused, k  # (the switch leaves the record alone)
        assert c.ray_totals() == ref.ray_totals()


def _flight_frames(c, sd, W, H, n, moving, stream):
    """n frames with device outputs and a closing stats call (host outputs); moving: a new camera before every call."""
    import torch
    outs = []
    for f in range(n):
        if moving:
            c.set_camera(_camera(sd, W, H, f + 1))
        with torch.cuda.stream(stream):
            avg = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        c.render(W, H, 4, B, frame_index=2 * f, avg=avg.data_ptr(), rgb8=rgb.data_ptr(), device_out=True, stats=False)
        outs.append((avg, rgb))
    host = _call(c, W, H, 4, 100)
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), r.cpu().numpy()) for a, r in outs], host, c.ray_totals()


@pytest.mark.parametrize("moving", [True, False])
def test_frames_in_flight(monkeypatch, moving):
    """Two frames in flight (two wavefront states, one running total): every frame equals the one-at-a-time,
    switched-off render."""
    import torch
    sd = scenes.instance_field(120, seed=9)
    W, H, n = 70, 45, 8
    stream = torch.cuda.Stream()
    with _contexts() as (c, ref):
        for x, fl in ((c, 2), (ref, 1)):
            x.set_stream(stream.cuda_stream)
            gpu_scene(x, sd, W, H)
            x.set_frames_in_flight(fl)
        got = _flight_frames(c, sd, W, H, n, moving, stream)
        with _env(monkeypatch, PRT_DEAD_SHADOW="0"):
            want = _flight_frames(ref, sd, W, H, n, moving, stream)
        for k, (g, w) in enumerate(zip(got[0], want[0])):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), k
        _same(got[1], want[1], "stats call")
        assert got[2] == want[2]
        assert 0 < c.shadow_dead() < got[2][1]
        assert ref.shadow_dead() == 0


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("W,H", SIZES)
def test_multi_pass(monkeypatch, W, H, merge):
    """A 3-frame call in 3 passes (PRT_MAX_ITEMS: one frame per pass): the dead rays of every pass are carried into
    the call's shadow-ray count; equal to the one-pass switched-off render."""
    sd = _scene("field")
    items = ((W + 7) // 8) * ((H + 7) // 8) * 64  # entries of the 8x8-block tile map of one frame
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(3):
            with _env(monkeypatch, PRT_MAX_ITEMS=str(items + 7)):
                got = _call(c, W, H, 6, 3 * k)
            with _env(monkeypatch, PRT_DEAD_SHADOW="0"):
                want = _call(ref, W, H, 6, 3 * k)
            _same(got, want, k)
            assert 0 < c.shadow_dead(reset=True) < got[2][1], k
            assert ref.shadow_dead() == 0
        assert c.ray_totals() == ref.ray_totals()


def test_tile_maps(monkeypatch):
    """prt_render_tiles of both ranks of a two-rank tile map on one GPU (70x45 in 32-pixel tiles, most of them with
    padding entries), three calls each: exact tile buffers and counts."""
    import torch
    sd = _scene("field")
    W, H, ts = 70, 45, 32
    maps = [(0, 2)] * 3 + [(1, 2)] * 3
    with _contexts() as (c, ref):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k, (rank, world) in enumerate(maps):
            per = c.tile_buffer_pixels(W, H, ts, world)
            px = int((tiles.tile_pixel_map(W, H, ts, rank, world) >= 0).sum())
            assert 0 < px < per
            bufs = [torch.zeros((per, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
            for x in (c, ref):
                x.reset_accumulation(full=True)
            st = c.render_tiles(W, H, 4, B, ts, rank, world, bufs[0].data_ptr(), frame_index=2 * k, stats=True)
            with _env(monkeypatch, PRT_DEAD_SHADOW="0"):
                so = ref.render_tiles(W, H, 4, B, ts, rank, world, bufs[1].data_ptr(), frame_index=2 * k, stats=True)
            torch.cuda.synchronize()
            assert np.array_equal(bufs[0].cpu().numpy(), bufs[1].cpu().numpy()), k
            assert (st.segments, st.shadow_rays) == (so.segments, so.shadow_rays), k
            assert 0 < c.shadow_dead(reset=True) < st.shadow_rays, k
            assert ref.shadow_dead() == 0
        assert c.ray_totals() == ref.ray_totals()


@pytest.mark.parametrize("what", ["area_light", "dielectric", "both"])
def test_extensions(monkeypatch, what):
    """The extensions pipeline skips the dead rays of its light classes (the area light's own ray is queued as ever):
    equal to the switched-off render, some but not all shadow rays dead."""
    base = scenes.multi_instance(scenes.config_small(50, 40))
    sd = scenes.with_extensions(base, area_light=None if what == "dielectric" else scenes.ceiling_light(),
                                materials=None if what == "area_light" else [1, 2, 0])
    W, H = 70, 45
    with _contexts() as (c, ref):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(3):
            dead, shadow = _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k)
            assert 0 < dead < shadow, (k, dead, shadow)
        assert c.ray_totals() == ref.ray_totals()


@pytest.mark.parametrize("mode", [1, 3, 6])
def test_debug_modes_untouched(monkeypatch, mode):
    """The debug render modes cast no shadow rays: no dead ray counted, and they render what they render with the
    switch off."""
    sd = scenes.multi_instance(scenes.config_small(50, 40))
    W, H = 70, 45
    with _contexts() as (c, ref):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(2):
            dead, shadow = _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k, mode=mode)
            assert dead == 0 and shadow == 0, (k, dead, shadow)
