"""Deferred resolve (prt_defer.hip): the plain wavefront pipeline (no extensions, render mode 0, not merged)
lets the shading of every iteration write its NEE record into a plane of its own and resolves a pass's paths in one
launch behind the last traversal, instead of one resolve launch per iteration.  The arithmetic and its order are the
per-iteration resolve's, so everything here is exact: images (uint32 views: NaN payloads included), (segments,
shadow_rays), ray_totals(), shadow_reuse() and shadow_dead() against a fresh context that renders the same calls with
PRT_DEFER_RESOLVE=0.  prt_stats.pipeline tells which chain a call ran (3 deferred, 2 per iteration), so no comparison
is of a chain with itself.

PRT_MERGE=0 throughout the deferred cases: calls this small take the merged pipeline by default, which keeps its
per-iteration resolve.  Shapes 96x64 and 70x45, spp 4."""
import dataclasses

import numpy as np
import pytest

import prt
from helpers import gpu_scene
from prt import _lib, scenes, tiles
from wave_env import contexts, env_or_unset as _env

pytestmark = pytest.mark.gpu

DEFAULT = _lib.FLAGS_DEFAULT
MODES = (None, "0")  # PRT_DEFER_RESOLVE of the two contexts of a test: default, per-iteration resolves
DEFERRED, PER_ITERATION = 3, 2


def _contexts(n=2):
    return contexts(n)


def _call(c, W, H, spp, fi, bounces=3, **kw):
    a, r, st = c.render(W, H, spp, bounces, frame_index=fi, **kw)
    return a, r, (st.segments, st.shadow_rays), st.pipeline


def _same(got, want, what=""):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


def _pair(monkeypatch, cs, W, H, spp, fi, what="", pipeline=DEFERRED, env0=None, **kw):
    """One call on each context: the default one runs `pipeline`, the other the per-iteration chain; equal results.
    env0: further switches for the first context's call alone."""
    res = []
    for c, mode in zip(cs, MODES):
        with _env(monkeypatch, PRT_DEFER_RESOLVE=mode, **((env0 or {}) if mode is None else {})):
            res.append(_call(c, W, H, spp, fi, **kw))
    assert res[0][3] == pipeline and res[1][3] == PER_ITERATION, (what, res[0][3], res[1][3])
    _same(res[0], res[1], what)
    return res[0]


def _counters_equal(cs):
    assert cs[0].ray_totals() == cs[1].ray_totals()
    assert cs[0].shadow_reuse() == cs[1].shadow_reuse()
    assert cs[0].shadow_dead() == cs[1].shadow_dead()


def _camera(sd, W, H, k):
    return prt.Camera(np.asarray(sd.cam_pos, np.float32) + np.float32(0.125 * k), sd.cam_target,
                      np.float32(W) / np.float32(H))


def _field():
    return scenes.instance_field(40, seed=9)


SCENES = {"field": _field, "small": scenes.config_small}


@pytest.mark.parametrize("bounces", [1, 2, 3, 4])
@pytest.mark.parametrize("W,H,scene", [(96, 64, "field"), (70, 45, "small")])
def test_bounces_and_flags(monkeypatch, W, H, scene, bounces):
    """AA on / off x gamma on / off, two calls each (a dense call, then calls on kept primary hits), for every path
    length from 1 (no continuing segment; with AA path 2 starts in the iteration after the one path 1 started and
    ended in) to 4.  Both scenes carry the emission map (kRiEmissive loads) and show sky above the ground (misses at
    iteration 0, the kStMiss loads); checked here so that a changed scene cannot hollow the test out."""
    sd = SCENES[scene]()
    emis = sd.meshes[0].emission
    assert emis >= 0 and np.any(np.asarray(sd.textures[emis]) != 0)
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE="0"):
        for c in cs:
            gpu_scene(c, sd, W, H)
        for c in cs:
            t = c.trace_primary(W, H)[0]["t"]
            assert 0 < int(np.sum(t >= np.float32(1e30))) < W * H
        fi = 0
        for aa in (_lib.FLAG_AA, 0):
            for gamma in (_lib.FLAG_GAMMA, 0):
                flags = (DEFAULT & ~(_lib.FLAG_AA | _lib.FLAG_GAMMA)) | aa | gamma
                for k in range(2):
                    _pair(monkeypatch, cs, W, H, 4, fi, (aa, gamma, k), flags=flags, bounces=bounces)
                    fi += 4
        _counters_equal(cs)


@pytest.mark.parametrize("W,H,scene", [(96, 64, "field"), (70, 45, "small")])
def test_static_camera_learns_uses_and_relearns(monkeypatch, W, H, scene):
    """Static camera: call 0 is the dense pass, call 1 learns the light-visibility record (the end pass's LEARN form,
    from plane 0), calls 2 and 3 use it (k_shade2d<true>).  A moved point light clears it: the next call skips nothing
    and learns again, the one after skips again."""
    sd = SCENES[scene]()
    pp = np.array(sd.lights.point_pos, np.float32)
    pp[1] = (2.0, -5.0, 2.0)
    below = dataclasses.replace(sd.lights, point_pos=pp)
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE="0"):
        for c in cs:
            gpu_scene(c, sd, W, H)
        reuse = []
        for k in range(7):
            if k == 4:
                for c in cs:
                    c.set_lights(below)
            _pair(monkeypatch, cs, W, H, 4, 2 * k, k, bounces=4)
            got = [c.shadow_reuse(reset=True) for c in cs]
            assert got[0] == got[1], (k, got)
            reuse.append(got[0])
        print("shadow rays answered from the record per call:", reuse)
        assert reuse[0] == 0 and reuse[1] == 0 and reuse[2] > 0 and reuse[3] > 0, reuse
        assert reuse[4] == 0 and reuse[5] > 0 and reuse[6] > 0, reuse
        _counters_equal(cs)


def _flight_frames(c, sd, W, H, n, stream):
    """n frames with device outputs, a new camera before every call, and a closing stats call (host outputs)."""
    import torch
    outs = []
    for f in range(n):
        c.set_camera(_camera(sd, W, H, f + 1))
        with torch.cuda.stream(stream):
            avg = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        c.render(W, H, 4, 3, frame_index=2 * f, avg=avg.data_ptr(), rgb8=rgb.data_ptr(), device_out=True, stats=False)
        outs.append((avg, rgb))
    host = _call(c, W, H, 4, 100)
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), r.cpu().numpy()) for a, r in outs], host, c.ray_totals()


def test_moving_camera_two_frames_in_flight(monkeypatch):
    """Two frames in flight (two wavefront states, each with its own planes), a new camera before every call, on both
    contexts (which state a call runs on decides whether it finds its primary hits kept, and with that how its zero
    rays are counted): every frame equals the per-iteration render."""
    import torch
    sd = _field()
    W, H, n = 70, 45, 6
    stream = torch.cuda.Stream()
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE="0"):
        for x, fl in zip(cs, (2, 2)):
            x.set_stream(stream.cuda_stream)
            gpu_scene(x, sd, W, H)
            x.set_frames_in_flight(fl)
        res = []
        for c, mode in zip(cs, MODES):
            with _env(monkeypatch, PRT_DEFER_RESOLVE=mode):
                res.append(_flight_frames(c, sd, W, H, n, stream))
        for k, (g, w) in enumerate(zip(res[0][0], res[1][0])):
            assert np.array_equal(g[0].view(np.uint32), w[0].view(np.uint32)) and np.array_equal(g[1], w[1]), k
        assert res[0][1][3] == DEFERRED and res[1][1][3] == PER_ITERATION
        _same(res[0][1], res[1][1], "stats call")
        assert res[0][2] == res[1][2]
        _counters_equal(cs)


def test_multi_pass(monkeypatch):
    """A 3-frame call (spp 6) in 3 passes (PRT_MAX_ITEMS: one frame per pass) on both contexts (the later passes of
    a call find their primary hits kept, which moves rays between the reuse and the dead counts): every pass resolves
    at its own end."""
    sd = _field()
    W, H = 70, 45
    items = ((W + 7) // 8) * ((H + 7) // 8) * 64  # entries of the 8x8-block tile map of one frame
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE="0", PRT_MAX_ITEMS=str(items + 7)):
        for c in cs:
            gpu_scene(c, sd, W, H)
        for k in range(3):
            _pair(monkeypatch, cs, W, H, 6, 3 * k, k)
        _counters_equal(cs)


def test_tile_maps(monkeypatch):
    """prt_render_tiles of both ranks of a two-rank tile map on one GPU (70x45 in 32-pixel tiles, most of them with
    padding entries, which the end pass skips), two calls each: exact tile buffers and counts."""
    import torch
    sd = _field()
    W, H, ts = 70, 45, 32
    maps = [(0, 2)] * 2 + [(1, 2)] * 2
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE="0"):
        for c in cs:
            gpu_scene(c, sd, W, H)
        for k, (rank, world) in enumerate(maps):
            per = cs[0].tile_buffer_pixels(W, H, ts, world)
            px = int((tiles.tile_pixel_map(W, H, ts, rank, world) >= 0).sum())
            assert 0 < px < per
            bufs = [torch.zeros((per, 4), dtype=torch.float32, device="cuda") for _ in cs]
            sts = []
            for c, mode, buf in zip(cs, MODES, bufs):
                c.reset_accumulation(full=True)
                with _env(monkeypatch, PRT_DEFER_RESOLVE=mode):
                    sts.append(c.render_tiles(W, H, 4, 3, ts, rank, world, buf.data_ptr(), frame_index=2 * k,
                                              stats=True))
            torch.cuda.synchronize()
            assert (sts[0].pipeline, sts[1].pipeline) == (DEFERRED, PER_ITERATION), k
            assert np.array_equal(bufs[0].cpu().numpy().view(np.uint32), bufs[1].cpu().numpy().view(np.uint32)), k
            assert (sts[0].segments, sts[0].shadow_rays) == (sts[1].segments, sts[1].shadow_rays), k
        _counters_equal(cs)


def test_budget_too_small_runs_the_per_iteration_chain(monkeypatch):
    """PRT_DEFER_BUDGET_MB=1: the planes of the call (96x64 x 2 frames x 8 iterations x 72 B = 6.75 MiB) do not fit, the
    per-iteration chain runs and the image is the same; without the override the same context defers again."""
    sd = _field()
    W, H = 96, 64
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE="0"):
        for c in cs:
            gpu_scene(c, sd, W, H)
        _pair(monkeypatch, cs, W, H, 4, 0, "fits", bounces=4)
        _pair(monkeypatch, cs, W, H, 4, 2, "over budget", pipeline=PER_ITERATION, env0={"PRT_DEFER_BUDGET_MB": "1"},
              bounces=4)
        _pair(monkeypatch, cs, W, H, 4, 4, "fits again", bounces=4)
        _counters_equal(cs)


@pytest.mark.parametrize("what", ["area light", "merged"])
def test_out_of_scope_pipelines_are_unaffected(monkeypatch, what):
    """An area-light scene (the extensions pipeline) and PRT_MERGE=1 (the merged pipeline) keep their per-iteration
    resolves whatever PRT_DEFER_RESOLVE says."""
    W, H = 70, 45
    if what == "area light":
        base = scenes.multi_instance(scenes.config_small(50, 40))
        sd = scenes.with_extensions(base, area_light=scenes.ceiling_light(), materials=None)
        merge = "0"
    else:
        sd, merge = _field(), "1"
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE=merge):
        for c in cs:
            gpu_scene(c, sd, W, H)
        for k in range(3):
            _pair(monkeypatch, cs, W, H, 4, 2 * k, k, pipeline=PER_ITERATION)
        _counters_equal(cs)
