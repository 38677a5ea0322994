"""Shadow rays that a zero BRDF value multiplies (prt_path.h nee_live, PRT_DEAD_SHADOW levels): nee_resolve adds
brdf * c to the emissive term, c the summed contributions of the item's unoccluded shadow rays and brdf the item's
one BRDF value, which is exactly (0,0,0) whenever the shading normal faces away from the viewer or from the light
the BRDF was evaluated for.  With a zero BRDF value and bounded contributions no ray of the item can change a bit, so
level 2 (the default) counts all of them instead of queueing them; level 1 is the contribution rule alone
(test_gpu_dead_shadow.py), level 0 traces every ray.

Everything here is exact: images (np.array_equal, or the uint32 views where NaNs are expected), (segments,
shadow_rays) and ray_totals() against a fresh context that renders the same calls at level 0.  The dead counts are
asserted throughout: default > level 1 > 0 == level 0 shows that the new rule engages on top of the old one.

Shapes as test_gpu_dead_shadow.py: 96x64 and 70x45, bounces 3, spp 4 = two reference frames per call."""
import dataclasses

import numpy as np
import pytest

import prt
from helpers import gpu_scene
from prt import _lib, scenes, tiles
from wave_env import contexts, env_or_unset as _env

pytestmark = pytest.mark.gpu

B = 3
SIZES = [(96, 64), (70, 45)]
DEFAULT = _lib.FLAGS_DEFAULT
LEVELS = (None, "1", "0")  # the contexts of a test, in this order: default (both rules), contribution rule, off


def _contexts(n=3):
    return contexts(n)


def _call(c, W, H, spp, fi, **kw):
    a, r, st = c.render(W, H, spp, kw.pop("bounces", B), frame_index=fi, **kw)
    return a, r, (st.segments, st.shadow_rays)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


def _same_bits(got, want, what=""):
    """As _same with the float image compared bit for bit (NaN payloads included)."""
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


def _triple(monkeypatch, cs, W, H, spp, fi, what="", same=_same, **kw):
    """One call on each of the three contexts at its level: all equal to the level-0 render, which counts no dead
    ray.  Returns (dead at the default level, dead at level 1, shadow rays of the call)."""
    res = []
    for c, lv in zip(cs, LEVELS):
        with _env(monkeypatch, PRT_DEAD_SHADOW=lv):
            res.append(_call(c, W, H, spp, fi, **kw))
    same(res[0], res[2], what)
    same(res[1], res[2], what)
    assert cs[2].shadow_dead() == 0, what
    return cs[0].shadow_dead(reset=True), cs[1].shadow_dead(reset=True), res[2][2][1]


def _camera(sd, W, H, k):
    return prt.Camera(np.asarray(sd.cam_pos, np.float32) + np.float32(0.125 * k), sd.cam_target,
                      np.float32(W) / np.float32(H))


def _field():
    return scenes.instance_field(40, seed=9)


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("moving", [True, False])
@pytest.mark.parametrize("W,H", SIZES)
def test_engages_and_is_exact(monkeypatch, W, H, moving, merge):
    """Six calls with rising frame_index, three contexts.  moving: a new camera before every call, iteration 0 runs
    the plain shading form; static: from call 2 on iteration 0 runs under the light-visibility record, which the
    levels leave alone.  In every call the BRDF rule finds dead rays beyond the contribution rule's."""
    sd = _field()
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE=merge):
        for c in cs:
            gpu_scene(c, sd, W, H)
        for k in range(6):
            if moving:
                for c in cs:
                    c.set_camera(_camera(sd, W, H, k + 1))
            d2, d1, shadow = _triple(monkeypatch, cs, W, H, 4, 2 * k, k)
            print(f"call {k}: shadow {shadow} dead default {d2} level 1 {d1}")
            assert shadow > d2 > d1 > 0, (k, d2, d1, shadow)
        assert cs[0].ray_totals() == cs[2].ray_totals() == cs[1].ray_totals()
        reuse = [c.shadow_reuse() for c in cs]
        assert reuse[0] == reuse[1] == reuse[2] and (reuse[0] == 0) == moving, reuse


def _below(W, H):
    """config_small seen from below: every primary hit has N.V < 0 with the normal map off, so with bounces 1 every
    shaded hit's BRDF value is exactly zero (a camera at (0.3, -3, -7) would not do: some faces look at it)."""
    sd = scenes.config_small()
    cam = prt.Camera(np.array([0.0, -12.0, -1.0], np.float32), np.zeros(3, np.float32), np.float32(W) / np.float32(H))
    return sd, cam


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("W,H", SIZES)
def test_exact_count_from_below(monkeypatch, W, H, merge):
    """Every shadow ray is dead by the BRDF rule's construction (default level: dead == shadow_rays), while the
    contribution rule alone finds only the rays whose light is behind the normal (level 1: some, not all).
    PRT_PRIMARY_REUSE=0: no ray is under the record."""
    sd, cam = _below(W, H)
    flags = DEFAULT & ~_lib.FLAG_NORMALMAP
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE=merge, PRT_PRIMARY_REUSE="0"):
        for c in cs:
            gpu_scene(c, sd, W, H)
            c.set_camera(cam)
        for k in range(3):
            d2, d1, shadow = _triple(monkeypatch, cs, W, H, 4, 2 * k, k, flags=flags, bounces=1)
            print(f"call {k}: shadow {shadow} dead default {d2} level 1 {d1}")
            assert shadow > 0 and d2 == shadow, (k, d2, shadow)
            assert 0 < d1 < shadow, (k, d1, shadow)
        assert cs[0].ray_totals() == cs[2].ray_totals() == cs[1].ray_totals()


@pytest.mark.parametrize("merge", ["0", "1"])
def test_non_finite_stays_on_the_old_path(monkeypatch, merge):
    """The same view with one point light's colour infinite: a point-light item's contributions are inf or NaN
    (inf x a zero cosine), 0 x inf would make the rays' answers matter, so such items keep the contribution rule
    alone (their ray towards that light stays live) and the image, NaN payloads included, is the level-0 render's."""
    W, H = 70, 45
    sd, cam = _below(W, H)
    col = np.array(sd.lights.point_col, np.float32)
    col[1] = np.float32(np.inf)
    sd = dataclasses.replace(sd, lights=dataclasses.replace(sd.lights, point_col=col))
    flags = DEFAULT & ~_lib.FLAG_NORMALMAP
    with _contexts() as cs, _env(monkeypatch, PRT_MERGE=merge, PRT_PRIMARY_REUSE="0"):
        for c in cs:
            gpu_scene(c, sd, W, H)
            c.set_camera(cam)
        for k in range(3):
            d2, d1, shadow = _triple(monkeypatch, cs, W, H, 4, 2 * k, k, same=_same_bits, flags=flags, bounces=1)
            print(f"call {k}: shadow {shadow} dead default {d2} level 1 {d1}")
            # the directional and spot classes are all dead as before; the point-light class keeps live rays
            assert 0 < d1 < d2 < shadow, (k, d1, d2, shadow)
        assert cs[0].ray_totals() == cs[2].ray_totals()


def _flight_frames(c, sd, W, H, n, stream):
    """n frames with device outputs, a new camera before every call, and a closing stats call (host outputs)."""
    import torch
    outs = []
    for f in range(n):
        c.set_camera(_camera(sd, W, H, f + 1))
        with torch.cuda.stream(stream):
            avg = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
            rgb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        c.render(W, H, 4, B, frame_index=2 * f, avg=avg.data_ptr(), rgb8=rgb.data_ptr(), device_out=True, stats=False)
        outs.append((avg, rgb))
    host = _call(c, W, H, 4, 100)
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), r.cpu().numpy()) for a, r in outs], host, c.ray_totals()


def test_frames_in_flight(monkeypatch):
    """Two frames in flight (two wavefront states, one running total), moving camera: every frame equals the
    one-at-a-time level-0 render; the level-1 context in flight counts fewer dead rays."""
    import torch
    sd = scenes.instance_field(120, seed=9)
    W, H, n = 70, 45, 6
    stream = torch.cuda.Stream()
    with _contexts() as cs:
        for x, fl in zip(cs, (2, 2, 1)):
            x.set_stream(stream.cuda_stream)
            gpu_scene(x, sd, W, H)
            x.set_frames_in_flight(fl)
        res = []
        for c, lv in zip(cs, LEVELS):
            with _env(monkeypatch, PRT_DEAD_SHADOW=lv):
                res.append(_flight_frames(c, sd, W, H, n, stream))
        for got in res[:2]:
            for k, (g, w) in enumerate(zip(got[0], res[2][0])):
                assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), k
            _same(got[1], res[2][1], "stats call")
            assert got[2] == res[2][2]
        assert res[2][2][1] > cs[0].shadow_dead() > cs[1].shadow_dead() > 0 == cs[2].shadow_dead()


def test_multi_pass(monkeypatch):
    """A 3-frame call (spp 6) in 3 passes (PRT_MAX_ITEMS: one frame per pass): the dead rays of every pass are
    carried into the call's shadow-ray count; equal to the one-pass level-0 render."""
    sd = _field()
    W, H = 70, 45
    items = ((W + 7) // 8) * ((H + 7) // 8) * 64  # entries of the 8x8-block tile map of one frame
    with _contexts() as cs:
        for c in cs:
            gpu_scene(c, sd, W, H)
        for k in range(3):
            res = []
            for c, lv in zip(cs, LEVELS):
                with _env(monkeypatch, PRT_DEAD_SHADOW=lv, PRT_MAX_ITEMS=None if lv == "0" else str(items + 7)):
                    res.append(_call(c, W, H, 6, 3 * k))
            _same(res[0], res[2], k)
            _same(res[1], res[2], k)
            d2, d1 = cs[0].shadow_dead(reset=True), cs[1].shadow_dead(reset=True)
            assert res[2][2][1] > d2 > d1 > 0 == cs[2].shadow_dead(), (k, d2, d1)
        assert cs[0].ray_totals() == cs[2].ray_totals() == cs[1].ray_totals()


def test_tile_maps(monkeypatch):
    """prt_render_tiles of both ranks of a two-rank tile map on one GPU (70x45 in 32-pixel tiles, most of them with
    padding entries), two calls each: exact tile buffers and counts."""
    import torch
    sd = _field()
    W, H, ts = 70, 45, 32
    maps = [(0, 2)] * 2 + [(1, 2)] * 2
    with _contexts() as cs:
        for c in cs:
            gpu_scene(c, sd, W, H)
        for k, (rank, world) in enumerate(maps):
            per = cs[0].tile_buffer_pixels(W, H, ts, world)
            px = int((tiles.tile_pixel_map(W, H, ts, rank, world) >= 0).sum())
            assert 0 < px < per
            bufs = [torch.zeros((per, 4), dtype=torch.float32, device="cuda") for _ in cs]
            sts = []
            for c, lv, buf in zip(cs, LEVELS, bufs):
                c.reset_accumulation(full=True)
                with _env(monkeypatch, PRT_DEAD_SHADOW=lv):
                    sts.append(c.render_tiles(W, H, 4, B, ts, rank, world, buf.data_ptr(), frame_index=2 * k,
                                              stats=True))
            torch.cuda.synchronize()
            want = bufs[2].cpu().numpy()
            for buf, st in zip(bufs[:2], sts[:2]):
                assert np.array_equal(buf.cpu().numpy(), want), k
                assert (st.segments, st.shadow_rays) == (sts[2].segments, sts[2].shadow_rays), k
            d2, d1 = cs[0].shadow_dead(reset=True), cs[1].shadow_dead(reset=True)
            assert sts[2].shadow_rays > d2 > d1 > 0 == cs[2].shadow_dead(), (k, d2, d1)
        assert cs[0].ray_totals() == cs[2].ray_totals() == cs[1].ray_totals()


def test_extensions_area_light(monkeypatch):
    """The extensions pipeline applies the rule to its light-class rays (the area light's own ray is queued as ever,
    and its NEE record is kept): equal to the level-0 render, more dead rays than the contribution rule finds."""
    base = scenes.multi_instance(scenes.config_small(50, 40))
    sd = scenes.with_extensions(base, area_light=scenes.ceiling_light(), materials=None)
    W, H = 70, 45
    with _contexts() as cs:
        for c in cs:
            gpu_scene(c, sd, W, H)
        for k in range(3):
            d2, d1, shadow = _triple(monkeypatch, cs, W, H, 4, 2 * k, k)
            print(f"call {k}: shadow {shadow} dead default {d2} level 1 {d1}")
            assert shadow > d2 > d1 > 0, (k, d2, d1, shadow)
        assert cs[0].ray_totals() == cs[2].ray_totals() == cs[1].ray_totals()
