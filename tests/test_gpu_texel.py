"""Texel addressing for every UV, on the device, against tests/scene_ref.py's texel_index.

include/prt.h (prt_mesh.fixed_uvs) defines the texel a map is read at for any float UV: per component x = uv * n is
truncated toward zero and wrapped into [0, n), and NaN, +-inf and |x| >= 2^31 give 0.  Two kinds of test, each bit
for bit and with nothing left out:

  the probe   prt_brdf_probe's PRT_PROBE_TEXEL runs the texel_index the shading kernels inline (prt_shade.h) on the
              records of texel_vectors(): every k / n around the wraps with its two neighbouring floats, +-0, the
              denormals, +-2^24 / n, the floats either side of +-2^31 / n, +-3.4e38, +-inf and NaN, on six texture
              shapes (a 1x1, non-powers of two, a 1-high, the largest the probe takes), with the other component
              fixed once inside the texture and once negative.
  the scene   `uv_scene` (tests/test_gpu_scene_queries.py): triangles whose corners share one UV of each class --
              negative, exactly -1, >= 2, on a texel boundary, huge -- and triangles whose UVs vary across 0 and -1.
              At EVERY hit pixel the expected UV is scene_ref.hit_uv of the device's own (prim, u, v), then
              texel_index, then the exact-tier decoders: the AOV albedo and the modes 1, 3 (smooth and normal-mapped),
              4, 5 and 6; a mode-0 frame equals the oracle's; and UVs re-pointed with prt_update_mesh (host arrays and
              device tensors) render what a fresh context renders.

tests/test_texel_ref.py runs the same records and the same scene checks against the oracle on the CPU, and shows for
each planted slip of scene_ref.TEXEL_SLIPS that the records catch it.

A triangle whose three UVs coincide has no tangent frame: the reference divides by the UV triangle's area
(Scene.cpp:99-100), 1 / 0 * 0, and its normal-mapped shading normal is NaN in every channel.  The arithmetic defines
neither the sign nor the payload of that NaN (x86 and the device differ), so where the expected value is NaN the
image must be NaN, and everywhere else the bits must agree (assert_bits_nan).  The map's texel is still read there.
"""
from fractions import Fraction

import numpy as np
import pytest

import scene_ref as R
import test_gpu_scene_queries as Q
from prt import _lib

F = np.float32
NORMALMAP, LIGHTED, STOCHASTIC = Q.NORMALMAP, Q.LIGHTED, Q.STOCHASTIC
SHAPES = ((1, 1), (5, 3), (8, 4), (3, 7), (1000, 1), (16384, 2))
OTHER = (F(0.40625), F(-0.65625))   # the other component: 13/32 inside the texture, -21/32 below it
UV_W, UV_H = 96, 72


# ------------------------------------------------------------------------------------------------ probe records
def _range_edge(n):
    """(the largest float32 below 2^31 / n, the first at or above it), decided in exact arithmetic."""
    c = F(2.0 ** 31 / n)
    while Fraction(float(c)) * n >= 2 ** 31:
        c = np.nextafter(c, F(0))
    while Fraction(float(np.nextafter(c, F(np.inf)))) * n < 2 ** 31:
        c = np.nextafter(c, F(np.inf))
    return c, np.nextafter(c, F(np.inf))


def axis_values(n):
    """The float32 values one component takes against a texture of size n along it."""
    if n >= 1000:   # only k within 2 of each multiple of n
        ks = sorted({m * n + d for m in range(-2, 3) for d in range(-2, 3) if abs(m * n + d) <= 2 * n + 1})
    else:
        ks = range(-2 * n - 1, 2 * n + 2)
    out = []
    for k in ks:
        c = F(k) / F(n)
        out += [c, np.nextafter(c, F(-np.inf)), np.nextafter(c, F(np.inf))]
    tiny, below_one = np.nextafter(F(0), F(1)), F(1.0 - 2.0 ** -24)
    below, at = _range_edge(n)
    big = F(2.0 ** 24) / F(n)
    out += [F(0.0), F(-0.0), tiny, -tiny, F(1e-8), F(-1e-8), below_one, -below_one, F(1), F(-1), big, -big,
            below, at, -below, -at, F(3.4e38), F(-3.4e38), F(np.inf), F(-np.inf), F(np.nan)]
    return np.array(out, F)


def texel_vectors():
    """(records float32 [n, 24] of PRT_PROBE_TEXEL, shape index [n]): per shape and axis every axis_values() against
    both OTHER values of the other component."""
    rec, shape = [], []
    for si, (w, h) in enumerate(SHAPES):
        for axis, n in ((0, w), (1, h)):
            for c in axis_values(n):
                for o in OTHER:
                    r = np.zeros(24, F)
                    r[axis], r[1 - axis], r[2], r[3] = c, o, w, h
                    rec.append(r)
                    shape.append(si)
    return np.array(rec, F), np.array(shape)


def check_texel_probe(probe, slip=None):
    """Runs `probe(op, records)` on texel_vectors() and compares both outputs of every record with
    scene_ref.texel_index (slip: one of its planted defects).  Returns the indices of the records that differ and the
    records; asserts nothing."""
    rec, shape = texel_vectors()
    got = probe(_lib.PROBE_TEXEL, rec)
    assert got.shape == (rec.shape[0], 8)
    exp = np.zeros((rec.shape[0], 8), F)
    for si, (w, h) in enumerate(SHAPES):
        k = shape == si
        px = R.texel_index(rec[k, :2], w, h, slip)
        exp[k, 0], exp[k, 1] = px % w, px // w
    return np.flatnonzero((Q.bits(got) != Q.bits(exp)).any(-1)), rec, got, exp


def describe(rec, i):
    return "record %d: uv (%r, %r) on %d x %d" % (i, float(rec[i, 0]), float(rec[i, 1]), rec[i, 2], rec[i, 3])


# ------------------------------------------------------------------------------------------------ the uv scene
def assert_bits_nan(got, exp, what):
    """assert_bits where the expected value is a number; NaN where it is NaN (module docstring)."""
    got, exp = np.ascontiguousarray(got, F), np.ascontiguousarray(exp, F)
    same = np.where(np.isnan(exp), np.isnan(got), Q.bits(got) == Q.bits(exp))
    bad = np.flatnonzero(~same.reshape(got.shape[0], -1).all(-1))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:3]], exp[bad[:3]])


def check_uv_scene(view, sd, shift=0, aov=None):
    """Every hit pixel of `view` (a view of test_gpu_scene_queries on uv_scene(shift)) against scene_ref at the
    view's own primary hit records: modes 1, 3 (with and without NORMALMAP), 4, 5, 6 and, with aov = {flags: (albedo,
    normal_depth)}, the AOV albedo and normal.  Asserts that every UV class is seen in each component and returns
    the coverage."""
    h = view.hits()
    sel = np.flatnonzero(h["t"] < R.BVH_FAR)
    assert (h["inst"][sel] == 0).all()
    mesh, prim, u, v = sd.meshes[0], h["prim"][sel], h["u"][sel], h["v"][sel]
    alb = sd.textures[mesh.albedo]
    eye = np.eye(4, dtype=F)
    with np.errstate(all="ignore"):   # 3.4e38 * 8 overflows and 1 / 0 * 0 is NaN on purpose
        uv = R.hit_uv(mesh, prim, u, v)
        m = R.material(mesh, sd.textures, prim, u, v)
        x = uv * np.array([alb.shape[1], alb.shape[0]], F)
        normals = {fl: R.shading_normal(mesh, sd.textures, eye, prim, u, v, bool(fl)) for fl in (0, NORMALMAP)}
    assert ((m["texel"] >= 0) & (m["texel"] < alb.size)).all()
    for fl in (0, NORMALMAP):
        what = (sd.name, fl)
        assert_bits_nan(view.render(fl, 1)[sel], m["base"], what + ("mode 1",))
        with np.errstate(invalid="ignore"):
            assert_bits_nan(view.render(fl, 3)[sel], (normals[fl] + F(1)) * F(0.5), what + ("mode 3",))
        for mode, key in ((4, "metalness"), (5, "roughness")):
            assert_bits_nan(view.render(fl, mode)[sel], np.repeat(m[key][:, None], 3, 1), what + (mode,))
        assert_bits_nan(view.render(fl, 6)[sel], m["emissive"], what + ("mode 6",))
        if aov is not None:
            albedo, nd = aov[fl]
            assert_bits_nan(albedo[sel, :3], m["base"], what + ("aov albedo",))
            assert_bits_nan(nd[sel, :3], normals[fl], what + ("aov normal",))
    # the normal-mapped normal is a number wherever the UVs vary, and there alone it is not
    classes, _ = Q.uv_triangle_classes()
    classes = np.roll(np.array(classes), -shift, 0)
    varying = classes[prim, 0] == "straddle"
    assert np.array_equal(np.isfinite(normals[NORMALMAP]).all(-1), varying)
    cov = {}
    for axis in (0, 1):
        for name in [c for c, _ in Q.UV_CLASSES] + ["straddle"]:
            cov[name, axis] = int((classes[prim, axis] == name).sum())
        with np.errstate(invalid="ignore"):
            inside = np.abs(x[:, axis]) < F(2147483648.0)
        cov["guard", axis] = int((~inside).sum())                               # the out-of-range branch
        cov["x <= -1", axis] = int((inside & (x[:, axis] <= -1)).sum())         # what used to index outside
        cov["-1 < x < 0", axis] = int(((x[:, axis] > -1) & (x[:, axis] < 0)).sum())    # truncates to texel 0
        for centre in (0.0, -1.0):   # both sides of 0 and of -1 inside the varying triangles
            cov["below %g" % centre, axis] = int((varying & (uv[:, axis] < centre)).sum())
            cov["above %g" % centre, axis] = int((varying & (uv[:, axis] > centre) & (uv[:, axis] < centre + 1)).sum())
    missing = [k for k, n in cov.items() if n == 0]
    assert not missing, missing
    own = R.texel_index(uv, sd.textures[mesh.normal].shape[1], sd.textures[mesh.normal].shape[0])
    assert (own != m["texel"]).any()     # the normal map's own 16x4 would place some texel elsewhere
    cov["pixels"] = int(sel.size)
    cov["texels read"] = int(np.unique(m["texel"]).size)
    w = alb.shape[1]                                                            # every column and every row is read
    assert np.unique(m["texel"] % w).size == w and np.unique(m["texel"] // w).size == alb.shape[0]
    return cov


# ------------------------------------------------------------------------------------------------ the device
pytestmark = pytest.mark.gpu


def test_probe_texel(gpu_ctx, oracle_mod):
    """Every record: the device's texel_index equals scene_ref's, in both outputs, and the oracle's."""
    bad, rec, got, exp = check_texel_probe(gpu_ctx.brdf_probe)
    assert bad.size == 0, (bad.size, [describe(rec, i) for i in bad[:5]], got[bad[:5], :2], exp[bad[:5], :2])
    assert np.array_equal(Q.bits(got), Q.bits(oracle_mod.brdf_probe(_lib.PROBE_TEXEL, rec)))


def test_probe_texel_refuses_bad_sizes(gpu_ctx):
    """w or h outside 1..16384, or not an integer, is PRT_ERR_INVALID_ARGUMENT: the kernel divides by them."""
    import prt
    for w, h in ((0, 4), (4, 0), (-8, 4), (16385, 1), (2.5, 4), (np.nan, 4), (4, np.inf)):
        rec = np.zeros((2, 24), F)
        rec[:, 2:4] = (8, 4)
        rec[1, 2:4] = (w, h)
        with pytest.raises(prt.PrtError):
            gpu_ctx.brdf_probe(_lib.PROBE_TEXEL, rec)


def _aov(ctx, W, H):
    return {fl: ctx.render_aov(W, H, fl)[:2] for fl in (0, NORMALMAP)}


@pytest.fixture(scope="module")
def uv_view(gpu_ctx):
    sd = Q.uv_scene()
    view = Q.GpuView(gpu_ctx, sd, UV_W, UV_H)
    view.load()
    return view, _aov(gpu_ctx, UV_W, UV_H)


def test_uv_scene_every_hit_pixel(uv_view):
    view, aov = uv_view
    print("coverage:", check_uv_scene(view, view.sd, 0, aov))


@pytest.mark.parametrize("flags", [LIGHTED | STOCHASTIC, LIGHTED | STOCHASTIC | _lib.FLAG_AA | _lib.FLAG_ACCUMULATE | _lib.FLAG_GAMMA])
def test_uv_scene_mode0_equals_oracle(uv_view, oracle_mod, flags):
    """A mode-0 frame of two bounces, smooth normals: every pixel and the packed screen equal the oracle's."""
    view, _ = uv_view
    ctx = view.load()
    ctx.reset_accumulation(full=True)
    avg, rgb8, _ = ctx.render(UV_W, UV_H, 2, 2, flags, 0)
    a_o, r_o, _, _ = oracle_mod.OracleScene(view.sd, UV_W, UV_H).render(UV_W, UV_H, spp=2, bounces=2, flags=flags)
    hit = view.hits()["t"] < R.BVH_FAR
    assert np.isfinite(a_o).all() and (a_o[hit, :3].max(-1) > 0).mean() > 0.9
    Q.assert_bits(avg[:, :3], a_o[:, :3], "mode 0")
    assert np.array_equal(rgb8, r_o)


class _DeviceMesh:
    def __init__(self, m):
        import torch
        for n in ("triangles", "fixed_normals", "fixed_uvs", "vertices", "face_normals"):
            setattr(self, n, torch.from_numpy(np.ascontiguousarray(getattr(m, n), F)).cuda())
        self.indices = torch.from_numpy(np.ascontiguousarray(m.indices, np.int32)).cuda()
        self.albedo, self.normal, self.metalness, self.emission = m.albedo, m.normal, m.metalness, m.emission
        torch.cuda.synchronize()


def _images(ctx):
    out = {}
    for fl in (0, NORMALMAP):
        albedo, nd = ctx.render_aov(UV_W, UV_H, fl)[:2]
        out[fl, "albedo"], out[fl, "nd"] = albedo.copy(), nd.copy()
        for mode in (1, 3, 4, 5, 6):
            ctx.reset_accumulation(full=True)
            out[fl, mode] = ctx.render(UV_W, UV_H, 1, 1, fl, mode)[0].copy()
    return out


@pytest.mark.parametrize("device", [False, True])
def test_repointed_uvs_equal_a_fresh_context(device):
    """uv_scene's UVs moved 7 triangles on by prt_update_mesh, from host arrays and from device tensors: the AOVs and
    the mode images are a fresh context's of the moved scene (NaN where that is NaN), and scene_ref's."""
    import prt
    from helpers import gpu_scene
    sd0, sd1 = Q.uv_scene(), Q.uv_scene(7)
    fresh, moved = prt.Context(0), prt.Context(0)
    try:
        gpu_scene(fresh, sd1, UV_W, UV_H)
        want = _images(fresh)
        gpu_scene(moved, sd0, UV_W, UV_H)
        before = _images(moved)
        assert not np.array_equal(Q.bits(before[0, 1]), Q.bits(want[0, 1]))      # the move changes the picture
        moved.update_mesh(0, _DeviceMesh(sd1.meshes[0]) if device else sd1.meshes[0], device=device)
        got = _images(moved)
        for k in want:
            assert_bits_nan(got[k], want[k], k)
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        view = Q.GpuView(moved, sd1, UV_W, UV_H)
        Q.GpuView._loaded = view                                                 # its scene is what `moved` holds now
        try:
            check_uv_scene(view, sd1, 7, {fl: (got[fl, "albedo"], got[fl, "nd"]) for fl in (0, NORMALMAP)})
        finally:
            Q.GpuView._loaded = None
    finally:
        fresh.close()
        moved.close()
