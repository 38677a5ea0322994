"""Primary-surface reuse (include/prt.h prt_surface_reuse, csrc/prt_surface.hip): what the shading of a pixel's fixed
path-1 primary hit reads before its first random draw -- shading normal, material, hit point, or a miss's sky radiance
-- repeats while the primary hits, the textures, the sky, the instance materials and the normal-map and skybox flags
stay put.  In the plain wavefront pipeline the first call that reuses the primary hits keeps those values per pixel
and later calls shade iteration 0 from them.

Everything here is exact: each call's avg and rgb8 (np.array_equal) and its (segments, shadow_rays) equal those of a
second context rendering the same calls with PRT_PRIMARY_REUSE=0, where every frame gathers everything anew.  The
counter is asserted in every case: without it the comparisons would pass with the record never read.  It counts work
items (pixels x reference frames) on the host: a call whose passes all shade from the record adds frames x pixels.

A static view needs two calls before it reads: call 1 traces the primary hits (dense), call 2 fills the record, call
3 reads it.  A change of what the record was shaded from (textures, sky, materials, the two flags) makes the next call
fill again; a change of the primary hits themselves (instances, a mesh, the camera, the resolution) makes the next call
dense and the one after fill.

The record belongs to the plain pipeline (deferred resolve or not).  The merged small-call pipeline is out of its scope,
so the cases run with PRT_MERGE=0 unless they say otherwise; merged, extension and debug calls must stay at 0.  A
deferred pass that reads the record also does the wave init's work in iteration 0 and launches no k_wave_init
(PRT_INIT_FOLD=0 keeps it): the cases below run the fold wherever they defer, which is the default, and the static and
multi-pass cases run it both ways.

The scene: scenes.instance_field with all four texture slots (albedo, normal, roughness-metal, emission) on both meshes,
every fifth torus a mirror, and the procedural sky.  Shapes 96x64 and 70x45 (tile-map padding entries), bounces 3; spp 4
is two reference frames per call, spp 6 three."""
import dataclasses

import numpy as np
import pytest

import deform
import prt
from helpers import gpu_scene
from prt import _lib, scenes, tiles
from wave_env import contexts, env as _env

pytestmark = pytest.mark.gpu

B = 3
SIZES = [(96, 64), (70, 45)]


def _field(n=40):
    sd = scenes.instance_field(n, seed=9)
    meshes = [dataclasses.replace(m, albedo=0, normal=1, metalness=2, emission=3) for m in sd.meshes]
    kinds = [_lib.MAT_TEXTURED] + [_lib.MAT_MIRROR if k % 5 == 0 else _lib.MAT_TEXTURED for k in range(n)]
    return dataclasses.replace(sd, meshes=meshes, materials=kinds)


def _call(c, W, H, spp, fi, **kw):
    a, r, st = c.render(W, H, spp, kw.pop("bounces", B), frame_index=fi, **kw)
    return a, r, (st.segments, st.shadow_rays)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


def _same_bits(got, want, what=""):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what


def _pair(monkeypatch, c, ref, W, H, spp, fi, what="", same=_same, **kw):
    """One call on c and the same call, nothing reused, on ref: equal; returns the items c shaded from the record."""
    got = _call(c, W, H, spp, fi, **kw)
    with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
        want = _call(ref, W, H, spp, fi, **kw)
    same(got, want, what)
    assert ref.surface_reuse() == 0, what
    return c.surface_reuse(reset=True)


def _camera(sd, W, H, k):
    return prt.Camera(np.asarray(sd.cam_pos, np.float32) + np.float32(0.125 * k), sd.cam_target,
                      np.float32(W) / np.float32(H))


def _set_textures(c, textures):
    keep = [np.ascontiguousarray(t, np.uint32) for t in textures]
    texs = (_lib.Texture * len(keep))()
    for i, t in enumerate(keep):
        texs[i] = _lib.Texture(t.shape[1], t.shape[0], t.ctypes.data)
    prt.renderer.check(c.L.prt_set_textures(c.h, texs, len(keep)))


def _set_sky(c, sky):
    sky = np.ascontiguousarray(sky, np.float32)
    prt.renderer.check(c.L.prt_set_sky(c.h, sky.ctypes.data, sky.shape[1], sky.shape[0]))


@pytest.mark.parametrize("defer,fold", [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")])
@pytest.mark.parametrize("spp", [4, 6])
@pytest.mark.parametrize("W,H", SIZES)
def test_static_view(monkeypatch, W, H, spp, defer, fold):
    """Six calls: 0 in call 1 (dense) and call 2 (the fill), frames x pixels in every later call; every call exact."""
    sd = _field()
    F = spp // 2
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0", PRT_DEFER_RESOLVE=defer, PRT_INIT_FOLD=fold):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(6):
            n = _pair(monkeypatch, c, ref, W, H, spp, F * k, k)
            assert n == (0 if k < 2 else F * W * H), (k, n)
            assert c.primary_rays() == (W * H, W * H * (F * (k + 1) - 1)), k
        assert c.ray_totals() == ref.ray_totals()
        assert c.shadow_reuse() > 0


def test_scene_covers_both_branches():
    """The view has sky pixels and hit pixels, emissive texels under some of them and mirror instances under others."""
    sd = _field()
    W, H = 96, 64
    with contexts(1) as (c,):
        gpu_scene(c, sd, W, H)
        hits, _ = c.trace_primary(W, H)
        hit = hits["t"] < np.float32(1e30)
        assert 0 < int(hit.sum()) < W * H
        kinds = np.asarray(sd.materials)
        assert (kinds[hits["inst"][hit]] == _lib.MAT_MIRROR).any() and (kinds[hits["inst"][hit]] == 0).any()
        emis = c.render(W, H, 1, 1, flags=_lib.FLAGS_DEFAULT & ~_lib.FLAG_AA, mode=_lib.MODE_EMISSIVE)[0]
        assert (emis[:, :3] > 0).any()


@pytest.mark.parametrize("what", ["switch", "shadow_switch", "merged"])
def test_switched_off_or_out_of_scope(monkeypatch, what):
    """PRT_SURFACE_REUSE=0, PRT_SHADOW_REUSE=0 (the record rides on the light-visibility record) and the merged
    pipeline: 0 throughout, exact, primary-hit reuse untouched."""
    sd = _field()
    W, H = 70, 45
    env = {"switch": dict(PRT_MERGE="0", PRT_SURFACE_REUSE="0"), "shadow_switch": dict(PRT_MERGE="0", PRT_SHADOW_REUSE="0"),
           "merged": dict(PRT_MERGE="1")}[what]
    with contexts(2) as (c, ref), _env(monkeypatch, **env):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(4):
            assert _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k) == 0, k
        assert c.primary_rays() == (W * H, 7 * W * H)


RECORD_ONLY = ["textures", "sky", "materials", "normalmap", "skybox"]
PRIMARY_HITS = ["instances", "update_mesh", "camera", "resolution"]


@pytest.mark.parametrize("what", RECORD_ONLY + PRIMARY_HITS)
def test_every_invalidation(monkeypatch, what):
    """Three warm calls (the third reads), then one change.  What only the record depends on: the next call fills (0),
    the one after reads.  What the primary hits depend on: dense (0), fill (0), read.  Exact throughout."""
    sd = _field()
    W, H = 96, 64
    W2, H2 = (70, 45) if what == "resolution" else (W, H)
    flags = _lib.FLAGS_DEFAULT
    flags2 = {"normalmap": flags & ~_lib.FLAG_NORMALMAP, "skybox": flags & ~_lib.FLAG_SKYBOX}.get(what, flags)

    def change(c):
        if what == "textures":  # one albedo texel
            tex = [np.array(t, np.uint32) for t in sd.textures]
            tex[0][128, 128] ^= np.uint32(0x00FF00)
            _set_textures(c, tex)
        elif what == "sky":
            _set_sky(c, np.asarray(sd.sky, np.float32)[:, ::-1] * np.float32(0.5))
        elif what == "materials":
            kinds = list(sd.materials)
            kinds[0] = _lib.MAT_MIRROR  # the ground
            c.set_materials(kinds)
        elif what == "instances":
            out = []
            for m, T in sd.instances:
                T = np.array(T, np.float32)
                if m == 1:
                    T[0, 3] += np.float32(0.07)
                out.append((m, T))
            c.set_instances(out)
        elif what == "update_mesh":
            c.update_mesh(1, deform.scaled(sd.meshes[1], 1.25))
        elif what == "camera":
            c.set_camera(_camera(sd, W, H, 1))

    want = [0, F_ * W2 * H2] if what in RECORD_ONLY else [0, 0, F_ * W2 * H2]
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0"):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        got = [_pair(monkeypatch, c, ref, W, H, 4, 2 * k, k) for k in range(3)]
        assert got == [0, 0, F_ * W * H], got
        change(c)
        change(ref)
        for x in (c, ref):
            x.reset_accumulation(full=True)
        got = [_pair(monkeypatch, c, ref, W2, H2, 4, 2 * (k + 3), (what, k), flags=flags2) for k in range(len(want))]
        assert got == want, (what, got)
        if what in ("normalmap", "skybox"):  # ... and back: another fill
            got = [_pair(monkeypatch, c, ref, W, H, 4, 2 * (k + 6), ("back", k)) for k in range(2)]
            assert got == want, (what, got)
        assert c.primary_rays()[0] == (W * H if what in RECORD_ONLY else W * H + W2 * H2)


F_ = 2  # reference frames of an spp-4 call


def test_lights_and_dead_shadow_levels_keep_the_record(monkeypatch):
    """The record holds no light term: new colours, new positions (which clear the light-visibility record) and a new
    spot direction leave it valid and the image follows them; so do the PRT_DEAD_SHADOW levels."""
    sd = _field()
    W, H = 96, 64
    pp = np.array(sd.lights.point_pos, np.float32)
    pp[1] = (2.0, -5.0, 2.0)
    steps = [
        dataclasses.replace(sd.lights, point_col=np.array(sd.lights.point_col, np.float32)[::-1].copy(),
                            dir_col=np.array([1.0, 3.0, 2.0], np.float32), spot_col=np.array([3.0, 1.0, 0.5], np.float32)),
        dataclasses.replace(sd.lights, point_pos=pp, spot_pos=np.array([0.5, 3.5, 0.25], np.float32),
                            dir_pos=np.array([-80.0, 40.0, 20.0], np.float32)),
        dataclasses.replace(sd.lights, spot_rot=np.array([0.0, 0.8, 0.6], np.float32)),
    ]
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0"):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        got = [_pair(monkeypatch, c, ref, W, H, 4, 2 * k, k) for k in range(3)]
        assert got == [0, 0, F_ * W * H], got
        fi = 6
        for s, lt in enumerate(steps):
            for x in (c, ref):
                x.set_lights(lt)
            assert _pair(monkeypatch, c, ref, W, H, 4, fi, ("lights", s)) == F_ * W * H
            fi += 2
        for lv in ("0", "1", "2"):
            with _env(monkeypatch, PRT_DEAD_SHADOW=lv):
                assert _pair(monkeypatch, c, ref, W, H, 4, fi, ("dead", lv)) == F_ * W * H
            fi += 2
        assert c.primary_rays()[0] == W * H


def _flight_frames(c, sd, W, H, n, moving, stream):
    """n frames with device outputs, a stats call on the context's own state after frame 2, and a closing one."""
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
    """Every chain owns its record.  Static camera, 14 frames and 2 stats calls: each of the `flights` states goes
    dense, fill, read on its own calls, so all but 2 x flights calls read; a camera that moves every call: 0."""
    import torch
    sd = _field()
    W, H, n = 70, 45, 14
    stream = torch.cuda.Stream()
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0"):
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
        reused = c.surface_reuse()
        assert reused == (0 if moving else (n + 2 - 2 * flights) * F_ * W * H), reused
        assert ref.surface_reuse() == 0


@pytest.mark.parametrize("defer,fold", [("1", "1"), ("1", "0"), ("0", "1")])
@pytest.mark.parametrize("W,H", SIZES)
def test_multi_pass(monkeypatch, W, H, defer, fold):
    """A 3-frame call in 3 passes (PRT_MAX_ITEMS: one frame per pass).  Call 1: dense, fill, read; later calls read in
    every pass.  Equal to the one-pass render that reuses nothing."""
    sd = _field()
    items = ((W + 7) // 8) * ((H + 7) // 8) * 64  # entries of the 8x8-block tile map of one frame
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0", PRT_DEFER_RESOLVE=defer, PRT_INIT_FOLD=fold):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(3):
            with _env(monkeypatch, PRT_MAX_ITEMS=str(items + 7)):
                got = _call(c, W, H, 6, 3 * k)
            with _env(monkeypatch, PRT_PRIMARY_REUSE="0"):
                want = _call(ref, W, H, 6, 3 * k)
            _same(got, want, k)
            assert c.surface_reuse(reset=True) == (1 if k == 0 else 3) * W * H, k
        assert c.ray_totals() == ref.ray_totals()


def test_tile_maps(monkeypatch):
    """prt_render_tiles with the two ranks' tile maps of a 2-rank frame on one GPU (70x45 in 32-pixel tiles, most with
    padding entries): each map goes dense, fill, read; exact tile buffers throughout."""
    import torch
    sd = _field()
    W, H, ts = 70, 45, 32
    maps = [(0, 2)] * 3 + [(1, 2)] * 3
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0"):
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
            assert c.surface_reuse(reset=True) == (0 if k % 3 < 2 else F_ * px), k
            assert ref.surface_reuse() == 0


@pytest.mark.parametrize("what", ["area_light", "dielectric", "debug_mode"])
def test_untouched_pipelines(monkeypatch, what):
    """The extension pipeline and the debug render modes: 0 throughout, exact."""
    base = scenes.multi_instance(scenes.config_small(50, 40))
    sd = {"area_light": scenes.with_extensions(base, area_light=scenes.ceiling_light()),
          "dielectric": scenes.with_extensions(base, materials=[1, 2, 0]), "debug_mode": base}[what]
    mode = 3 if what == "debug_mode" else 0
    W, H = 70, 45
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0"):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        for k in range(4):
            assert _pair(monkeypatch, c, ref, W, H, 4, 2 * k, k, mode=mode) == 0, k


def test_an_infinite_light_colour(monkeypatch):
    """One point light's colour infinite: inf and NaN radiances (payloads included) match bit for bit while the record
    is dense, filled and read."""
    sd = _field()
    W, H = 96, 64
    col = np.array(sd.lights.point_col, np.float32)
    col[1] = np.float32(np.inf)
    sd = dataclasses.replace(sd, lights=dataclasses.replace(sd.lights, point_col=col))
    with contexts(2) as (c, ref), _env(monkeypatch, PRT_MERGE="0"):
        gpu_scene(c, sd, W, H)
        gpu_scene(ref, sd, W, H)
        got = [_pair(monkeypatch, c, ref, W, H, 4, 2 * k, k, same=_same_bits) for k in range(4)]
        assert got == [0, 0, F_ * W * H, F_ * W * H], got
        a = _call(c, W, H, 4, 8)[0]
        assert not np.isfinite(a[:, :3]).all()
