"""prt_query_rays / prt_query_surface (k_query around the persistent traversal engine, k_query_surface) against the
references the lock-step query kernels are pinned to: the numpy brute force on the far-scale placements, the oracle on
the instance fields, prt_intersect / prt_occluded elsewhere, scene_ref for the surface attributes.  Every comparison
is np.array_equal on every field of every ray unless it says otherwise; the host path and the device path (torch
tensors on a non-default stream handed to set_stream) must return the same bytes.

The brute-force and oracle references are tests/test_gpu_traverse_scales.py's (_ref, _field_ref): computed once per
session, shared with that file's tests, never written to."""
import contextlib

import numpy as np
import pytest

import degenerate as dg
import far_scenes as fs
import scene_ref as R
import test_gpu_scene_queries as sq
from helpers import gpu_scene
from prt import _lib, scenes
from test_gpu_traverse_scales import NAMES, _assert_hits, _field_ref, _ref

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 32, 24
HIT = np.dtype([("t", F), ("u", F), ("v", F), ("prim", np.uint32), ("inst", np.uint32)])


# ------------------------------------------------------------------------------------------------ the two paths
@contextlib.contextmanager
def device_stream(ctx):
    """The context on a torch stream of its own; everything before and after is complete on the host."""
    import torch
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            yield s
        s.synchronize()
    finally:
        torch.cuda.synchronize()
        ctx.set_stream(None)


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to("cuda")


def _records(t):
    """query_rays' [n, 5] float32 tensor as intersect()'s records (the same 20 bytes per ray)."""
    return np.ascontiguousarray(t.cpu().numpy()).view(HIT).reshape(-1)


def host_query(ctx, O, D, tm=None, closest=True, any_hit=True):
    return ctx.query_rays(O, D, tm, closest=closest, any_hit=any_hit)


def dev_query(ctx, O, D, tm=None, closest=True, any_hit=True):
    """The device path; returns numpy after one synchronisation (the copies back)."""
    h, o = ctx.query_rays(_t(O), _t(D), _t(tm), closest=closest, any_hit=any_hit)
    return (None if h is None else _records(h)), (None if o is None else o.cpu().numpy())


def _same(a, b):
    return (a is None and b is None) or a.tobytes() == b.tobytes()


def _check_batch(query, O, D, tm, want_hits, want_occ, what):
    """One batch: both answers in one call, then each alone; returns the bytes of the joint call."""
    hits, occ = query(O, D, tm)
    assert hits.dtype == HIT and occ.dtype == np.int32 and hits.shape == occ.shape == (O.shape[0],)
    _assert_hits(hits, want_hits, what)
    assert np.array_equal(occ, want_occ), (what, int((occ != want_occ).sum()))
    h1, none = query(O, D, tm, any_hit=False)
    assert none is None and _same(h1, hits), what
    none, o1 = query(O, D, tm, closest=False)
    assert none is None and _same(o1, occ), what
    return hits.tobytes() + occ.tobytes()


def _check_against_ref(ctx, ref, min_hits):
    """ref: a reference of tests/test_gpu_traverse_scales.py (hit records without a tmax and with tmax at and one ulp
    past the hit, the any-hit answers of both)."""
    O, D, hit = ref["O"], ref["D"], ref["hit"]
    assert O.shape[0] % 64 != 0 and hit.sum() >= min_hits
    got = {}
    for path, query in (("host", host_query), ("device", dev_query)):
        with device_stream(ctx) if path == "device" else contextlib.nullcontext():
            q = lambda *a, **k: query(ctx, *a, **k)  # noqa: E731
            b = [_check_batch(q, O, D, None, ref["hits"], hit.astype(np.int32), path + " all")]
            for k in ("at", "past"):
                tm = ref["tmax"][k]
                b.append(_check_batch(q, O, D, tm, ref["hits_tmax"][k], (ref["occ"][k] != 0).astype(np.int32),
                                      path + " tmax " + k))
            tm = ref["tmax"]["past"]
            for name, s in fs.SLICES.items():  # n = 1, 63, 65
                b.append(_check_batch(q, O[s], D[s], tm[s], [a[s] for a in ref["hits_tmax"]["past"]],
                                      (ref["occ"]["past"][s] != 0).astype(np.int32), path + " " + name))
            h0, o0 = q(O[:0], D[:0], tm[:0])  # n = 0
            assert h0.shape == o0.shape == (0,)
            got[path] = b"".join(b)
    assert got["host"] == got["device"]
    _, st = ctx.trace_primary(16, 8)  # the context's overflow count is cumulative
    assert st.stack_overflows == 0


# ------------------------------------------------------------------------------------------------ 1: brute force
@pytest.mark.parametrize("name,tail", [(n, None) for n in NAMES] + [("C", "0")])
def test_queries_equal_the_brute_force(gpu_ctx, monkeypatch, name, tail):
    """Every far-scale placement and the point P on the host SAH builder; C once more without the cooperative tail."""
    if tail is not None:
        monkeypatch.setenv("PRT_TAIL", tail)
    ref = _ref(name)
    gpu_ctx.set_bvh_builder(_lib.BUILDER_HOST_SAH)
    gpu_scene(gpu_ctx, ref["sd"], W, H)
    _check_against_ref(gpu_ctx, ref, 0 if name == "P" else 3000)


# ------------------------------------------------------------------------------------------------ 2: instances
@pytest.mark.parametrize("dist", fs.FIELD_DISTS)
@pytest.mark.parametrize("n", [65, 300])
def test_instance_bvh_queries_equal_the_oracle(gpu_ctx, n, dist):
    ref = _field_ref(n, dist)
    gpu_scene(gpu_ctx, ref["sd"], W, H)
    assert gpu_ctx.scene_info().tlas_depth > 0
    _check_against_ref(gpu_ctx, ref, 100)


def _lockstep(ctx, O, D, scale=F(0.999)):
    """prt_intersect without a tmax, a tmax that ends some rays before their hit, and prt_intersect / prt_occluded
    under it."""
    h0 = ctx.intersect(O, D)
    hit = h0["t"] < dg.FAR
    k = np.arange(O.shape[0])
    tm = np.where(hit & (k % 3 == 0), h0["t"] * scale, np.where(hit, np.nextafter(h0["t"], F(np.inf)), dg.FAR)).astype(F)
    return h0, hit, tm, ctx.intersect(O, D, tm), ctx.occluded(O, D, tm)


def _check_against_lockstep(ctx, O, D, min_hits):
    h0, hit, tm, htm, otm = _lockstep(ctx, O, D)
    assert hit.sum() >= min_hits and 0 < otm.sum() < hit.sum()
    got = {}
    for path, query in (("host", host_query), ("device", dev_query)):
        with device_stream(ctx) if path == "device" else contextlib.nullcontext():
            hits, occ = query(ctx, O, D)
            assert _same(hits, h0) and np.array_equal(occ, hit.astype(np.int32)), path
            hits, occ = query(ctx, O, D, tm)
            assert _same(hits, htm) and np.array_equal(occ, otm), path
            got[path] = hits.tobytes() + occ.tobytes()
    assert got["host"] == got["device"]
    _, st = ctx.trace_primary(16, 8)
    assert st.stack_overflows == 0


def test_linear_instance_list_equals_the_lockstep_kernels(gpu_ctx):
    """At most 64 instances: no instance BVH, the engine's linear instance loop (and its reload per instance)."""
    sd = fs.field(40)
    gpu_scene(gpu_ctx, sd, W, H)
    assert gpu_ctx.scene_info().tlas_depth == 0
    O, D = fs.field_rays(40, 30.0)
    _check_against_lockstep(gpu_ctx, O, D, 100)


# ------------------------------------------------------------------------------------------------ 3: spill
def test_deep_bvh_spills_to_hbm(gpu_ctx):
    """scenes.deep_bvh (deeper than the 18 LDS groups of the 4-wave form): the HBM spill columns."""
    sd = scenes.deep_bvh()
    gpu_scene(gpu_ctx, sd, 64, 48)
    assert gpu_ctx.scene_info().max_depth > 19
    rng = np.random.default_rng(3)
    O = np.tile(np.array([0.0, 0.0, -2.0], F), (20000, 1))
    O[:, :2] = rng.uniform(-0.5, 0.5, (20000, 2)).astype(F)
    D = np.zeros_like(O)
    D[:, :2] = rng.uniform(-0.3, 0.3, (20000, 2)).astype(F)
    D[:, 2] = 1.0
    _check_against_lockstep(gpu_ctx, O, D, 10000)


# ------------------------------------------------------------------------------------------------ 4: refill
def test_a_batch_larger_than_the_resident_lanes(gpu_ctx):
    """600,001 rays, both answers (1,200,002 entries against at most 458,752 resident lanes): every wave refills from
    the fetch counters and steals from the other parts.  Placement A's rays tiled with a seeded jitter, built in
    device memory."""
    import torch
    ref = _ref("A")
    gpu_scene(gpu_ctx, ref["sd"], W, H)
    n = 600001
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    rep = -(-n // ref["O"].shape[0])
    O = _t(ref["O"]).repeat(rep, 1)[:n].contiguous()
    D = (_t(ref["D"]).repeat(rep, 1)[:n] + 0.05 * torch.randn((n, 3), generator=g, device="cuda")).contiguous()
    On, Dn = O.cpu().numpy(), D.cpu().numpy()
    h0, hit, tm, htm, otm = _lockstep(gpu_ctx, On, Dn, F(0.5))
    assert hit.sum() > n // 4 and (~hit).sum() > 1000 and 0 < otm.sum() < hit.sum()
    tmd = _t(tm)
    with device_stream(gpu_ctx):
        hits, occ = gpu_ctx.query_rays(O, D, tmd, closest=True, any_hit=True)
        hits, occ = _records(hits), occ.cpu().numpy()
    assert _same(hits, htm), int((hits["t"] != htm["t"]).sum())
    assert np.array_equal(occ, otm), int((occ != otm).sum())
    _, st = gpu_ctx.trace_primary(16, 8)
    assert st.stack_overflows == 0


# ------------------------------------------------------------------------------------------------ 5: bad rays
def test_never_traversed_rays(gpu_ctx):
    """Rays that must not be traversed among valid ones: the defined miss record (t = the tmax as given, bit for bit),
    occluded = 0, and the valid neighbours' answers as without them."""
    ref = _ref("A")
    gpu_scene(gpu_ctx, ref["sd"], W, H)
    n = 321
    O, D = ref["O"][:n].copy(), ref["D"][:n].copy()
    h0 = gpu_ctx.intersect(O, D)  # the lock-step reference sees the valid rays only
    hit = h0["t"] < dg.FAR
    assert hit.sum() > 200
    tm = np.where(hit, np.nextafter(h0["t"], F(np.inf)), dg.FAR).astype(F)
    # eight rays that would be hits if they were traversed, spread over the batch's waves
    at = np.flatnonzero(hit)[np.linspace(0, hit.sum() - 1, 8).astype(int)]
    bad = dict(zip(at.tolist(), ("o_nan", "d_inf", "d_zero", "t_zero", "t_neg", "t_nan", "d_nan", "o_inf")))
    assert len(bad) == 8
    i = {k: j for j, k in bad.items()}
    O[i["o_nan"], 1] = np.nan
    O[i["o_inf"], 0] = -np.inf
    D[i["d_inf"], 2] = np.inf
    D[i["d_zero"]] = 0.0
    D[i["d_nan"], 0] = np.nan
    tm_bad = tm.copy()
    tm_bad[i["t_zero"]], tm_bad[i["t_neg"]], tm_bad[i["t_nan"]] = 0.0, -2.5, np.nan
    for tmax, t_miss in ((tm_bad, tm_bad), (None, np.full(n, dg.FAR, F))):
        rays_bad = [j for j, k in bad.items() if tmax is not None or not k.startswith("t_")]
        sel = np.ones(n, bool)
        sel[rays_bad] = False
        want = gpu_ctx.intersect(O[sel], D[sel], None if tmax is None else tmax[sel])
        got = {}
        for path, query in (("host", host_query), ("device", dev_query)):
            with device_stream(gpu_ctx) if path == "device" else contextlib.nullcontext():
                hits, occ = query(gpu_ctx, O, D, tmax)
            assert _same(hits[sel], want), path
            assert np.array_equal(occ[sel], (want["t"] < t_miss[sel]).astype(np.int32)), path
            b = hits[rays_bad]
            assert np.array_equal(b["t"].view(np.uint32), t_miss[rays_bad].view(np.uint32)), (path, b["t"])
            for f in ("u", "v", "prim", "inst"):
                assert not b[f].view(np.uint32).any(), (path, f)
            assert not occ[rays_bad].any(), path
            got[path] = hits.tobytes() + occ.tobytes()
        assert got["host"] == got["device"]


# ------------------------------------------------------------------------------------------------ 6: stream order
def test_queries_and_instance_updates_keep_stream_order(gpu_ctx):
    """query, update_instances(B), query on one stream with no synchronisation between them: the first answers for
    the transforms A, the second for B (the update waits for the first query's read of the instance state, the second
    query follows the update)."""
    sd = fs.field(65)
    gpu_scene(gpu_ctx, sd, W, H)
    assert gpu_ctx.scene_info().tlas_depth > 0
    O, D = fs.field_rays(65, 30.0)
    A = np.ascontiguousarray(np.stack([T for _, T in sd.instances]), F)
    B = A.copy()
    B[:, :3, 3] += np.array([0.21, 0.13, -0.17], F)
    want_a = gpu_ctx.intersect(O, D)
    gpu_ctx.update_instances(B)
    want_b = gpu_ctx.intersect(O, D)
    gpu_ctx.update_instances(A)
    assert (want_a["t"] < dg.FAR).sum() > 100 and (want_a["t"] != want_b["t"]).sum() > 100
    with device_stream(gpu_ctx):
        Od, Dd, Bd = _t(O), _t(D), _t(B.reshape(-1))
        first, _ = gpu_ctx.query_rays(Od, Dd)
        gpu_ctx.update_instances(Bd, device=True)
        second, _ = gpu_ctx.query_rays(Od, Dd)
    assert _same(_records(first), want_a)
    assert _same(_records(second), want_b)


# ------------------------------------------------------------------------------------------------ 7: surface
SW, SH = 96, 72


def _surface_both_paths(ctx, hits, tm, normalmap, **which):
    """query_surface on the host path and on the device path: the same bytes; returns the host path's."""
    host = ctx.query_surface(hits, tm, normalmap, **which)
    with device_stream(ctx):
        ht = _t(np.ascontiguousarray(hits).view(F).reshape(-1, 5))
        dev = {k: v.cpu().numpy() for k, v in ctx.query_surface(ht, _t(tm), normalmap, **which).items()}
    assert host.keys() == dev.keys()
    for k in host:
        assert host[k].tobytes() == dev[k].tobytes(), k
    return host


def test_surface_at_camera_rays_equals_the_aov_pass(gpu_ctx):
    """(a) scene_ref's camera rays on the attribute scene: query_rays' hits are trace_primary's, query_surface's albedo
    and normal_depth are render_aov's, with and without the normal map."""
    sd = sq.attr_scene()
    gpu_scene(gpu_ctx, sd, SW, SH)
    O, D = sq.camera_rays(sd, SW, SH)
    traced, _ = gpu_ctx.trace_primary(SW, SH)
    hits, _ = gpu_ctx.query_rays(O, D)
    sq.check_primary(traced, hits)
    with device_stream(gpu_ctx):
        dh, _ = gpu_ctx.query_rays(_t(O), _t(D))
        dh = _records(dh)
    assert _same(dh, hits)
    for fl in (0, _lib.FLAG_NORMALMAP):
        albedo, nd = gpu_ctx.render_aov(SW, SH, flags=fl)
        s = _surface_both_paths(gpu_ctx, hits, None, bool(fl))
        assert np.array_equal(sq.bits(s["albedo"]), sq.bits(albedo)), fl
        assert np.array_equal(sq.bits(s["normal_depth"]), sq.bits(nd)), fl


def test_surface_off_camera_equals_scene_ref(gpu_ctx):
    """(b) rays from above the attribute scene, a third of the hits ended by their tmax: material, shading normal and
    geometry normal against scene_ref under check_attributes' rules (bit for bit where the float32 order is restated:
    the texel-derived values everywhere, the normals under an exact normal matrix; within scene_ref.CLOSED_TOL of the
    normal's length under the rotated, non-uniformly scaled instance); misses give the defined zeros; outputs not
    asked for are not written and change nothing of the others."""
    sd = sq.attr_scene()
    gpu_scene(gpu_ctx, sd, SW, SH)
    rng = np.random.default_rng(5)
    n = 6001
    O = np.stack([rng.uniform(-4.5, 4.0, n), rng.uniform(2.0, 4.0, n), rng.uniform(-2.0, 2.0, n)], 1).astype(F)
    tgt = np.stack([rng.uniform(-4.5, 4.0, n), np.zeros(n), rng.uniform(-1.5, 1.5, n)], 1)
    D = (tgt - O).astype(F)
    h0, _ = gpu_ctx.query_rays(O, D)
    was_hit = h0["t"] < dg.FAR
    tm = np.where(was_hit & (np.arange(n) % 3 == 0), h0["t"] * F(0.5), dg.FAR).astype(F)
    h, _ = gpu_ctx.query_rays(O, D, tm)
    hit = h["t"] < tm
    assert np.array_equal(hit, was_hit & (np.arange(n) % 3 != 0)) and hit.sum() > 1500 and (was_hit & ~hit).sum() > 500
    assert _same(h[hit], h0[hit])
    out = {fl: _surface_both_paths(gpu_ctx, h, tm, bool(fl)) for fl in (0, _lib.FLAG_NORMALMAP)}
    worst = 0.0
    for fl, s in out.items():
        assert s["albedo"].shape == (n, 4) and s["material"].shape == (n, 8)
        miss = ~hit  # the defined zeros
        assert not s["albedo"][miss].any() and not s["geometry_normal"][miss].any() and not s["material"][miss].any()
        assert not s["normal_depth"][miss, :3].any() and (s["normal_depth"][miss, 3] == dg.FAR).all()
        assert (s["albedo"][hit, 3] == 1).all() and (s["geometry_normal"][hit, 3] == 1).all()
        sq.assert_bits(s["normal_depth"][hit, 3], h["t"][hit], "depth")
        for inst, (mi, T) in enumerate(sd.instances):
            sel = np.flatnonzero(hit & (h["inst"] == inst))
            assert sel.size > 200, (inst, sel.size)
            mesh, prim, u, v = sd.meshes[mi], h["prim"][sel], h["u"][sel], h["v"][sel]
            exact = inst in (0, 1)
            nm = R.normal_matrix(T)
            if exact:
                nm = nm.astype(F)
                assert np.array_equal(nm[:3, :3], np.eye(3, dtype=F))
            m = R.material(mesh, sd.textures, prim, u, v)
            what = (inst, fl)
            sq.assert_bits(s["albedo"][sel, :3], m["base"], what + ("albedo",))
            sq.assert_bits(s["material"][sel, 0:3], m["base"], what + ("base",))
            sq.assert_bits(s["material"][sel, 3], m["metalness"], what + ("metalness",))
            sq.assert_bits(s["material"][sel, 4:7], m["emissive"], what + ("emissive",))
            sq.assert_bits(s["material"][sel, 7], m["roughness"], what + ("roughness",))
            g = R.geometry_normal(mesh, nm, prim)
            nrm = R.shading_normal(mesh, sd.textures, nm, prim, u, v, bool(fl))
            if exact:
                sq.assert_bits(s["geometry_normal"][sel, :3], g, what + ("geometry normal",))
                sq.assert_bits(s["normal_depth"][sel, :3], nrm, what + ("shading normal",))
            else:
                worst = max(worst, sq._normal_close(s["geometry_normal"][sel, :3], g, what + ("geometry normal",)),
                            sq._normal_close(s["normal_depth"][sel, :3], nrm, what + ("shading normal",)))
    print("largest normal deviation under the general transform, / length:", worst)
    assert not np.array_equal(out[0]["normal_depth"], out[_lib.FLAG_NORMALMAP]["normal_depth"])  # the flag is read
    # outputs not asked for: NULL pointers, the others as before
    full = out[_lib.FLAG_NORMALMAP]
    for k in full:
        only = _surface_both_paths(gpu_ctx, h, tm, True, **{j: j == k for j in full})
        assert list(only) == [k] and only[k].tobytes() == full[k].tobytes(), k
