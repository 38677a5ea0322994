"""Shadow-ray reuse (include/prt.h prt_shadow_reuse, prt_wave2.hip): the next-event shadow rays of a pixel's fixed
path-1 primary hit run from that hit to a light, so their any-hit answers repeat while the primary hits and the light
positions stay put.  Calls that reuse the primary hits record each answer the first time a frame traces it and skip
the ray afterwards.  Everything here is exact: each call's avg and rgb8 (np.array_equal) and its ray counts equal
those of a fresh context rendering the same calls with PRT_PRIMARY_REUSE=0, where every ray is traced in every frame.
The skipped count is asserted throughout: without it the comparisons would pass with the record never hitting.

A static view needs two calls before it skips: call 1 traces the primary hits (it neither reads nor fills the
record), call 2 learns (all its frames shade before any answer is known), call 3 skips.

Shapes as test_gpu_primary_reuse.py: 96x64 and 70x45, bounces 3; spp 4 is two reference frames per call, spp 6
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
EPS = np.float32(0.01)  # kEpsilon (prt_math.h)
NONSTOCH = _lib.FLAGS_DEFAULT & ~_lib.FLAG_STOCHASTIC


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
    """One call on c and the same call, everything traced, on ref: equal; returns what c skipped in it."""
    got = _call(c, W, H, spp, fi, **kw)
    with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
        want = _call(ref, W, H, spp, fi, **kw)
    _same(got, want, what)
    assert ref.shadow_reuse() == 0, what
    return c.shadow_reuse(reset=True)


def _moved(sd, k=1):
    """sd's instances with the tori (mesh 1) shifted, the heightfield in place."""
    out = []
    for m, T in sd.instances:
        T = np.array(T, np.float32)
        if m == 1:
            T[0, 3] += np.float32(0.07 * k)
            T[2, 3] -= np.float32(0.05 * k)
        out.append((m, T))
    return out


def _camera(sd, W, H, k):
    return prt.Camera(np.asarray(sd.cam_pos, np.float32) + np.float32(0.125 * k), sd.cam_target,
                      np.float32(W) / np.float32(H))


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("spp", [4, 6])
@pytest.mark.parametrize("W,H", SIZES)
def test_engages_and_is_exact(monkeypatch, W, H, spp, merge):
    """Six calls, static camera, rising frame_index: nothing skipped in calls 1 (dense) and 2 (learning), something
    in every later call; every call equals the everything-traced render and the primary-ray counters are what they
    were."""
    sd = scenes.instance_field(40, seed=9)
    F = spp // 2
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        assert c.shadow_reuse() == 0
        for k in range(6):
            skipped = _pair(monkeypatch, c, ref, W, H, spp, F * k, k)
            assert (skipped == 0) if k < 2 else (skipped > 0), (k, skipped)
            assert c.primary_rays() == (W * H, W * H * (F * (k + 1) - 1)), k
        assert c.ray_totals() == ref.ray_totals()
        assert c.shadow_reuse() == 0  # (every read above reset it)


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("W,H", SIZES)
def test_exact_count(monkeypatch, W, H, merge):
    """Without PRT_FLAG_STOCHASTIC every hit asks for the directional light only, so from call 3 on a call skips
    exactly frames x (pixels whose primary ray hits)."""
    sd = scenes.instance_field(40, seed=9)
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        hits, _ = c.trace_primary(W, H)
        nhit = int((hits["t"] < np.float32(1e30)).sum())
        assert 0 < nhit <= W * H
        for k in range(5):
            skipped = _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k, flags=NONSTOCH)
            assert skipped == (0 if k < 2 else 2 * nhit), (k, skipped, nhit)


def test_scene_has_both_answers():
    """The test scene's primary hit points see the directional light and point light 0 from some pixels and not from
    others (the library's occlusion query on the shadow rays light_ray builds), so a wrong or stale record would
    change pixels."""
    sd = scenes.instance_field(40, seed=9)
    W, H = 96, 64
    with _contexts(1) as (c,):
        _, cam = gpu_scene(c, sd, W, H)
        hits, _ = c.trace_primary(W, H)
        d = cam.desc
        pos, tl, tr, bl = (np.array(v[:], np.float32) for v in (d.pos, d.top_left, d.top_right, d.bottom_left))
        ys, xs = np.mgrid[0:H, 0:W]
        u = (xs.reshape(-1, 1) / np.float32(W)).astype(np.float32)
        v = (ys.reshape(-1, 1) / np.float32(H)).astype(np.float32)
        P = tl + u * (tr - tl) + v * (bl - tl)
        D = P - pos
        D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
        hit = hits["t"] < np.float32(1e30)
        I = (pos + hits["t"].reshape(-1, 1) * D)[hit].astype(np.float32)
        for name, lp, squared in (("directional", sd.lights.dir_pos, False), ("point 0", sd.lights.point_pos[0], True)):
            L = np.asarray(lp, np.float32) - I
            dist = np.linalg.norm(L, axis=1).astype(np.float32)
            L = (L / dist.reshape(-1, 1)).astype(np.float32)
            tmax = (dist * dist if squared else dist) - EPS  # (the point lights' limit is the squared distance)
            occ = c.occluded(I + L * EPS, L, tmax)
            n_occ = int((occ != 0).sum())
            assert 0 < n_occ < len(I), (name, n_occ, len(I))


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("what", ["camera", "instances40", "instances120", "builder", "resolution"])
def test_every_invalidation(monkeypatch, what, merge):
    """After three warm calls (the third skips), one change of what the primary hits depend on: the next two calls
    skip nothing and equal a fresh context's, the third skips again."""
    n_inst = 120 if what == "instances120" else 40  # 120: the instance BVH; 40: the linear list
    sd = scenes.instance_field(n_inst, seed=9)
    W, H = 96, 64
    W2, H2 = (70, 45) if what == "resolution" else (W, H)

    def change(c):
        if what == "camera":
            c.set_camera(_camera(sd, W, H, 1))
        elif what.startswith("instances"):
            c.set_instances(_moved(sd))
        elif what == "builder":
            c.set_bvh_builder(_lib.BUILDER_HOST_SBVH)
            gpu_scene(c, sd, W, H)  # the meshes again: their BLASes are rebuilt by the new builder

    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        for k in range(3):
            _call(c, W, H, 4, 2 * k)
        assert c.shadow_reuse(reset=True) > 0
        change(c)
        c.reset_accumulation(full=True)
        gpu_scene(ref, sd, W, H)
        change(ref)
        ref.reset_accumulation(full=True)
        for k in range(3):
            skipped = _pair(monkeypatch, c, ref, W2, H2, 4, 2 * (k + 3), k)
            assert (skipped == 0) if k < 2 else (skipped > 0), (k, skipped)
        assert c.primary_rays()[0] == W * H + W2 * H2


def test_tile_map_invalidation(monkeypatch):
    """prt_render_tiles with another (rank, world) is another tile map: its dense pass, then a learning call, then
    skipping; exact tile buffers throughout.  70x45 in 32-pixel tiles, most of them with padding entries."""
    import torch
    sd = scenes.instance_field(40, seed=9)
    W, H, ts = 70, 45, 32
    maps = [(0, 2)] * 3 + [(1, 2)] * 3 + [(0, 3)] * 3
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
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                so = ref.render_tiles(W, H, 4, B, ts, rank, world, bufs[1].data_ptr(), frame_index=2 * k, stats=True)
            torch.cuda.synchronize()
            assert np.array_equal(bufs[0].cpu().numpy(), bufs[1].cpu().numpy()), k
            assert (st.segments, st.shadow_rays) == (so.segments, so.shadow_rays), k
            skipped = c.shadow_reuse(reset=True)
            assert (skipped == 0) if k % 3 < 2 else (skipped > 0), (k, skipped)


@pytest.mark.parametrize("merge", ["0", "1"])
def test_lights(monkeypatch, merge):
    """Point light 1 moved from above the scene to below the ground (the tori and the ground now lie between it and
    what it lit): the record is cleared, the next call skips nothing, the one after skips again, and no new dense
    pass runs.  New colours and a new spot direction alone clear nothing."""
    sd = scenes.instance_field(40, seed=9)
    W, H = 96, 64
    pp = np.array(sd.lights.point_pos, np.float32)
    pp[1] = (2.0, -5.0, 2.0)
    below = dataclasses.replace(sd.lights, point_pos=pp)
    tinted = dataclasses.replace(below, point_col=np.array(sd.lights.point_col, np.float32)[::-1].copy(),
                                 dir_col=np.array([1.0, 3.0, 2.0], np.float32),
                                 spot_col=np.array([3.0, 1.0, 0.5], np.float32),
                                 spot_rot=np.array([0.0, 0.8, 0.6], np.float32))
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        got = [_pair(monkeypatch, c, ref, W, H, 4, 2 * k, k) for k in range(3)]
        assert got[0] == 0 and got[1] == 0 and got[2] > 0, got
        for x in (c, ref):
            x.set_lights(below)
        got = [_pair(monkeypatch, c, ref, W, H, 4, 2 * k + 6, ("below", k)) for k in range(2)]
        assert got[0] == 0 and got[1] > 0, got
        for x in (c, ref):
            x.set_lights(tinted)
        got = [_pair(monkeypatch, c, ref, W, H, 4, 2 * k + 10, ("tinted", k)) for k in range(2)]
        assert got[0] > 0 and got[1] > 0, got
        assert c.primary_rays() == (W * H, 2 * 7 * W * H - W * H)  # one dense pass in all


def _flight_frames(c, sd, W, H, n, moving, stream):
    """n frames with device outputs, a stats call (host outputs: it runs on the context's own wavefront state, in
    the context stream's order) after frame 2, and a closing one; moving: a new camera before every call."""
    import torch
    outs, host = [], []
    cam = 0
    for f in range(n):
        if moving:
            cam += 1
            c.set_camera(_camera(sd, W, H, cam))
        with torch.cuda.stream(stream):
            avg = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        c.render(W, H, 4, B, frame_index=2 * f, avg=avg.data_ptr(), rgb8=rgb.data_ptr(), device_out=True, stats=False)
        outs.append((avg, rgb))
        if f == 2:
            if moving:
                cam += 1
                c.set_camera(_camera(sd, W, H, cam))
            host.append(_call(c, W, H, 4, 100))
    host.append(_call(c, W, H, 4, 102))
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), r.cpu().numpy()) for a, r in outs], host, c.ray_totals()


@pytest.mark.parametrize("flights,moving", [(2, True), (4, True), (2, False), (4, False)])
def test_frames_in_flight(monkeypatch, flights, moving):
    """Every chain owns its record: with a static camera each wavefront state traces, learns and then skips on its
    own; with the camera changed before every call nothing is ever skipped.  Every frame equals the one-at-a-time,
    everything-traced render."""
    import torch
    sd = scenes.instance_field(120, seed=9)
    W, H, n = 70, 45, 14
    stream = torch.cuda.Stream()
    with _contexts() as (c, ref):
        for x, fl in ((c, flights), (ref, 1)):
            x.set_stream(stream.cuda_stream)
            gpu_scene(x, sd, W, H)
            x.set_frames_in_flight(fl)
        got = _flight_frames(c, sd, W, H, n, moving, stream)
        with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
            want = _flight_frames(ref, sd, W, H, n, moving, stream)
        for k, (g, w) in enumerate(zip(got[0], want[0])):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), k
        for k, (g, w) in enumerate(zip(got[1], want[1])):
            _same(g, w, ("stats call", k))
        assert got[2] == want[2]
        skipped = c.shadow_reuse()
        assert (skipped == 0) if moving else (skipped > 0), skipped
        assert ref.shadow_reuse() == 0


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("W,H", SIZES)
def test_multi_pass(monkeypatch, W, H, merge):
    """A 3-frame call in 3 passes (PRT_MAX_ITEMS: one frame per pass): the first pass traces the primary hits, the
    second learns, the third skips; equal to the one-pass everything-traced render."""
    sd = scenes.instance_field(40, seed=9)
    items = ((W + 7) // 8) * ((H + 7) // 8) * 64  # entries of the 8x8-block tile map of one frame
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(3):
            with _env(monkeypatch, PRT_MAX_ITEMS=str(items + 7)):
                got = _call(c, W, H, 6, 3 * k)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, W, H, 6, 3 * k)
            _same(got, want, k)
            assert c.shadow_reuse(reset=True) > 0, k
        assert c.ray_totals() == ref.ray_totals()


@pytest.mark.parametrize("what", ["area_light", "dielectric", "debug_mode", "switched_off"])
def test_untouched_paths(monkeypatch, what):
    """The extension pipelines, the debug render modes and PRT_SHADOW_REUSE=0 skip nothing and render what the
    everything-traced context renders; the switch leaves primary-hit reuse on."""
    base = scenes.multi_instance(scenes.config_small(50, 40))
    sd = {"area_light": scenes.with_extensions(base, area_light=scenes.ceiling_light()),
          "dielectric": scenes.with_extensions(base, materials=[1, 2, 0]),
          "debug_mode": base, "switched_off": base}[what]
    mode = 3 if what == "debug_mode" else 0
    W, H = 70, 45
    env = {"PRT_SHADOW_REUSE": "0"} if what == "switched_off" else {}
    with _contexts() as (c, ref), _env(monkeypatch, **env):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(4):
            assert _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k, mode=mode) == 0, k
        assert c.primary_rays() == ((W * H, 7 * W * H) if what == "switched_off" else (0, 0))
