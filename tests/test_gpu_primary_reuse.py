"""Primary-hit reuse (include/prt.h prt_primary_rays, prt_wave2.hip): path 1 of a pixel starts at the pixel centre,
so its primary ray repeats in every reference frame while camera, tile map, scene and instances stay put.  Renders
without extensions in render mode 0 trace it once per such state (a dense pass over the tile map's entries) and take
its hit from the kept records afterwards.  Everything here is exact: each frame's avg and rgb8 (np.array_equal) and
its ray counts equal those of a fresh context rendering the same calls with PRT_PRIMARY_REUSE=0, where every item's
primary ray is traced in every frame; the first test also holds the frames against the oracle.  The counters are
asserted throughout: without them the comparisons would pass vacuously if the stamp never matched.

Sizes: 96x64 and 70x45.  prt_render cuts the image into 8x8 blocks (70x45: 72x48 entries, 306 of them padding,
and partly filled waves at the right and bottom edges), prt_render_tiles into 32-pixel tiles (70x45: 96x64
entries).  bounces 3; spp 4 is two reference frames per call, spp 6 three."""

import numpy as np
import pytest

import oracle
import prt
from helpers import RMSE_TOL, gpu_scene, rmse
from prt import _lib, scenes, tiles
from wave_env import contexts, env as _env

pytestmark = pytest.mark.gpu

B = 3
SIZES = [(96, 64), (70, 45)]


def _contexts(n=2):
    return contexts(n)


def _call(c, W, H, spp, fi, **kw):
    a, r, st = c.render(W, H, spp, kw.pop("bounces", B), frame_index=fi, **kw)
    return a, r, (st.segments, st.shadow_rays)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


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
def test_reuse_engages_and_is_exact(monkeypatch, W, H, spp, merge):
    """Three calls, static camera, rising frame_index: call 1 traces one primary ray per pixel and reuses it for its
    other frames, calls 2 and 3 trace none; every frame equals the switch-off render and the oracle's."""
    sd = scenes.instance_field(40, seed=9)
    F = spp // 2
    osc = oracle.OracleScene(sd, W, H)
    ost = oracle.new_state(W, H)
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        assert c.primary_rays() == (0, 0)
        for k in range(3):
            got = _call(c, W, H, spp, F * k)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, W, H, spp, F * k)
            _same(got, want, k)
            assert c.primary_rays() == (W * H, W * H * (F * (k + 1) - 1)), k
            a_o, r_o, ost, s_o = osc.render(W, H, spp=spp, bounces=B, frame_index=F * k, state=ost)
            # (the bar and the segment rule of test_gpu_parity._compare_render)
            assert rmse(a_o, got[0]) <= RMSE_TOL, k
            assert abs(int(got[2][0]) - int(s_o.segments)) <= 0.001 * s_o.segments, k
        assert c.ray_totals() == ref.ray_totals()
        assert ref.primary_rays() == (0, 0)  # switched off: nothing handed to a dense pass, nothing reused
        assert c.primary_rays(reset=True)[0] == W * H and c.primary_rays() == (0, 0)


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("what", ["camera", "instances40", "instances120", "builder", "resolution"])
def test_every_invalidation(monkeypatch, what, merge):
    """After a warm call, one change of what the kept hits depend on: the next frame equals a fresh context's, a new
    dense pass ran, and the call after that reuses the new records."""
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
        _call(c, W, H, 4, 0)
        assert c.primary_rays() == (W * H, W * H)
        change(c)
        c.reset_accumulation(full=True)
        gpu_scene(ref, sd, W, H)
        change(ref)
        ref.reset_accumulation(full=True)
        for k in (1, 2):
            got = _call(c, W2, H2, 4, 2 * k)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, W2, H2, 4, 2 * k)
            _same(got, want, k)
            assert c.primary_rays() == (W * H + W2 * H2, W * H + W2 * H2 * (2 * k - 1)), k


def test_tile_map_invalidation(monkeypatch):
    """prt_render_tiles with another (rank, world) is another tile map: its own dense pass, exact tile buffers; the
    same map again reuses.  70x45 in 32-pixel tiles: 6 tiles of 1024 entries, most of them with padding."""
    import torch
    sd = scenes.instance_field(40, seed=9)
    W, H, ts = 70, 45, 32
    maps = [(0, 2), (1, 2), (1, 2), (0, 3), (0, 2)]
    with _contexts() as (c, ref):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        traced = reused = 0
        last = None
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
            fresh = (rank, world) != last
            traced += px if fresh else 0
            reused += px if fresh else 2 * px
            last = (rank, world)
            assert c.primary_rays() == (traced, reused), k


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


@pytest.mark.parametrize("flights,moving", [(2, True), (4, True), (2, False)])
def test_frames_in_flight(monkeypatch, flights, moving):
    """Every chain owns its records and stamp: with the camera changed before every call the chains never wait for
    one another and every call runs its own dense pass; with a static camera each wavefront state (the context's
    own, shared by slot 0 and the stats calls, and one per further slot) fills its copy once.  Every frame equals
    the one-at-a-time, switch-off render."""
    import torch
    sd = scenes.instance_field(120, seed=9)
    W, H, n = 70, 45, 6
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
        traced, reused = c.primary_rays()
        calls = n + 2
        assert traced + reused == 2 * calls * W * H
        assert traced == (calls if moving else flights) * W * H
        assert ref.primary_rays() == (0, 0)


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("W,H", SIZES)
def test_multi_pass(monkeypatch, W, H, merge):
    """A 3-frame call in 3 passes (PRT_MAX_ITEMS: one frame per pass): the first pass fills the records, the later
    passes of the call and the next call reuse them; equal to the one-pass switch-off render."""
    sd = scenes.instance_field(40, seed=9)
    items = ((W + 7) // 8) * ((H + 7) // 8) * 64  # entries of the 8x8-block tile map of one frame
    with _contexts() as (c, ref), _env(monkeypatch, PRT_MERGE=merge):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(2):
            with _env(monkeypatch, PRT_MAX_ITEMS=str(items + 7)):
                got = _call(c, W, H, 6, 3 * k)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, W, H, 6, 3 * k)
            _same(got, want, k)
            assert c.primary_rays() == (W * H, W * H * (3 * (k + 1) - 1)), k


@pytest.mark.parametrize("what", ["area_light", "dielectric", "debug_mode"])
def test_untouched_paths(monkeypatch, what):
    """The extension pipelines and the debug render modes keep tracing every primary ray: same images with the
    switch on and off, nothing handed to a dense pass, nothing reused."""
    base = scenes.multi_instance(scenes.config_small(50, 40))
    sd = {"area_light": scenes.with_extensions(base, area_light=scenes.ceiling_light()),
          "dielectric": scenes.with_extensions(base, materials=[1, 2, 0]),
          "debug_mode": base}[what]
    mode = 3 if what == "debug_mode" else 0
    W, H = 70, 45
    with _contexts() as (c, ref):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(2):
            got = _call(c, W, H, 4, 2 * k, mode=mode)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, W, H, 4, 2 * k, mode=mode)
            _same(got, want, k)
            assert c.primary_rays() == (0, 0)
        if what != "debug_mode":  # the materials / light taken away again: the plain pipeline, reuse from here on
            for x in (c, ref):
                x.set_materials(None)
                x.set_area_light(None)
                x.reset_accumulation(full=True)
            for k in range(2):
                got = _call(c, W, H, 4, 2 * k)
                with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                    want = _call(ref, W, H, 4, 2 * k)
                _same(got, want, ("plain", k))
            assert c.primary_rays() == (W * H, 3 * W * H)


def test_bounces_zero_and_one_pixel(monkeypatch):
    """bounces = 0 (Trace returns 0: no ray at all) and a 1x1 image return what they return with the switch off."""
    sd = scenes.instance_field(40, seed=9)
    with _contexts() as (c, ref):
        gpu_scene(c, sd, 96, 64)
        gpu_scene(ref, sd, 96, 64)
        for k in range(2):
            got = _call(c, 96, 64, 4, 2 * k, bounces=0)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, 96, 64, 4, 2 * k, bounces=0)
            _same(got, want, k)
            assert got[2] == (0, 0) and c.primary_rays() == (0, 0)
        for k in range(2):
            got = _call(c, 1, 1, 4, 2 * k)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, 1, 1, 4, 2 * k)
            _same(got, want, k)
            assert c.primary_rays() == (1, 1 + 2 * k)
