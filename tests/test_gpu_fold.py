"""The last stage of a frame on the device -- pixel_value / finish_path (prt_shade2.h), k_accumulate, k_postfx, k_untile
(prt_render.hip), the host's choice of acc_new / acc_prev (prt_api_render.cpp) and prt_reset_accumulation -- against
the literal reference tests/fold_ref.py.  tests/test_fold_ref.py runs the same checks (the check_* functions below)
against the oracle on the CPU, and shows that each planted slip of fold_ref.SLIPS fails one of them.

What is pinned is everything between a frame value and the outputs: the frame values are the implementation's own
(captured one frame at a time with ACCUMULATE off, where avg is the frame; the existing references own those), and the
reference folds them.  Every comparison of the fold is exact, as uint32 views.

The fold scene: test_gpu_estimator.floor_scene's floor (roughness 1, metalness 0, every light black) with one quad as
a second instance, stood upright by its instance transform, under sky_ramp(); camera (1.5, 2.5, -4) -> (-0.5, 0, 0.5),
image 23 x 15, bounces 2, default flags (AA, GAMMA, ACCUMULATE ...).  The quad's instance transform takes four states:
A, B (moved sideways: pixels restart), C and D (B moved 0.006 and 0.012 along the view: |dt| < EPSILON per move on the
quad's pixels, which go on accumulating over moved geometry as the reference does; D is further than EPSILON from B,
so an implementation that keeps the key of the last restart restarts there).

The script (SCRIPT): calls of 1 and of 3 frames (three calls per geometry state, so that the device's kept primary
hits, light visibility and surface records are all in play when the quad moves), the moves, prt_reset_accumulation(0)
(the averages darken: the counts stay), a checkpoint taken, a !ACCUMULATE frame and 3 accumulating ones, the
checkpoint loaded and the same two calls again, prt_reset_accumulation(1), two more frames.  It runs without a screen
pass, with aberration +2 under a non-unit grading and vignette (Panini rays: fov 1.2, distortion 0.5), with
aberration -1, with aberration W + 3 (both taps clamp), in passes of one frame (PRT_MAX_ITEMS = W * H) and on a local
group of 3 with tile 8 (neither side of 23 x 15 is a multiple of it; without aberration and without the checkpoint,
which a group refuses).  Its first call accumulates: see test_fold_ref.py on the literal initial state.

The jitter (checks (a) and (d)): the floor alone (its image is one convex polygon, which fold_ref.coverage needs), render
mode BASECOLOR, bounces 1, SKYBOX and GAMMA off: a path returns the floor's base colour c or 0, so a frame is
0.5 * (s1 + s2) with s2 in {0, c}, and P(s2 = c) is the covered share of the pixel's jitter footprint.
  exact        every AA capture is one of the two values bit for bit; coverage 1 gives c and coverage 0 gives 0 always
  frequency    N = 4096 frames in accumulating calls of 256 (the float32 accumulator of a call sums 256 values), the
               averages summed in float64, against 0.5 * (s1 + c p): |mean - expectation| <= 6 sigma + allowance,
               sigma = 0.5 c sqrt(p (1 - p) / N) from fold_ref.coverage's p, pixels with p in (0.02, 0.98).
               allowance: a call's accumulator adds 256 terms of at most c; each addition rounds by at most
               2^-24 of a partial sum of at most 256 c, so the sum is off by at most 256 * 2^-24 * 256 c and the
               average (the division by 256 is exact) by at most 256 * 2^-24 c = 1.6e-5 c -- derived, not measured.
  pairs        K = 1024 single-frame captures give the indicator of path 2's hit per frame; for every two pixels with
               p in (0.2, 0.8) the joint frequency is within 6 standard errors sqrt(q (1 - q) / K), q = p_a p_b
  lag 1        per such pixel the frequency of a hit in two consecutive frames is within 6 standard errors of p^2;
               the products of consecutive pairs overlap, so the variance of their mean over K - 1 pairs is
               (p^2 (1 - p^2) + 2 (p^3 - p^4)) / (K - 1)
The seeds are fixed, so the outcome is deterministic.

Largest z seen (`pytest -s` prints them), on the oracle and on the device alike -- the device's frames are the
oracle's bit for bit, so the two see the same jitter:
  frequency  29 pixels tested (18 with p in (0.2, 0.8)), largest z 2.35
  pairs      153 pairs, largest z 2.29        lag 1  largest z 1.42
Measured wall time of (d) on the MI355X: the 16 calls of 256 frames under 0.02 s, the 1024 single-frame captures 0.24 s
(not halved); a scripted run with its reference fold 0.1 s.
"""
import contextlib
import dataclasses
import functools
import os

import numpy as np
import pytest

import fold_ref as FR
import scene_ref as R
import test_gpu_estimator as Q
import test_gpu_scene_queries as SQ
from prt import _lib

F = np.float32
W, H = 23, 15                            # neither side a multiple of the group's tile (8)
N_PX = W * H
BOUNCES = 2
SEED = 20250921
CAM = ((1.5, 2.5, -4.0), (-0.5, 0.0, 0.5))
QUAD_HALF = 1.2
QUAD_AT = (-0.4, -0.6)                    # x, z of the upright quad's foot in state A
ACC = _lib.FLAGS_DEFAULT
NOACC = _lib.FLAGS_DEFAULT & ~_lib.FLAG_ACCUMULATE

POSTS = {
    "none": None,
    "ab+2": FR.Post(2, 1.2, 0.5, 15.0, 0.4, (0.9, 1.1, 0.8, 1.0)),
    "ab-1": FR.Post(-1, 1.2, 0.5, 15.0, 0.4, (0.9, 1.1, 0.8, 1.0)),
    "ab-clamped": FR.Post(W + 3, 1.2, 0.5, 15.0, 0.4, (0.9, 1.1, 0.8, 1.0)),
    "no-ab": FR.Post(0, 1.2, 0.5, 15.0, 0.4, (0.9, 1.1, 0.8, 1.0)),
}

# three calls before every move but the last: the device's first call on a view traces its primary hits, the second
# learns the light-visibility and surface records, the third uses them -- so each move finds every record in play
_HEAD = [("render", 1, ACC), ("render", 3, ACC), ("render", 1, ACC), ("move", "B"), ("render", 1, ACC),
         ("render", 3, ACC), ("render", 1, ACC), ("move", "C"), ("render", 2, ACC), ("render", 1, ACC),
         ("render", 1, ACC), ("move", "D"), ("render", 3, ACC), ("reset", 0), ("render", 1, ACC)]
N_VIEWS = 4          # geometry states the script renders: the dense primary passes a context runs over it
_TWO = [("render", 1, NOACC), ("render", 3, ACC)]
_TAIL = [("reset", 1), ("render", 2, ACC)]
SCRIPT = tuple(_HEAD + [("save",)] + _TWO + [("load",)] + _TWO + _TAIL)
SCRIPT_NO_CHECKPOINT = tuple(_HEAD + _TWO + _TAIL)      # a local group keeps no checkpoints (see test_script_on_a_group)


# ------------------------------------------------------------------------------------------------ scenes
def _ahead():
    return R.camera(CAM[0], CAM[1], F(W) / F(H))["ahead"].astype(np.float64)


def quad_transform(state):
    """The flat quad (normal +y, centred at the origin) stood upright facing -z with its foot on the floor, then
    carried to its place in `state`."""
    off = {"A": np.zeros(3), "B": np.array([1.1, 0.0, 0.0]), "C": np.array([1.1, 0.0, 0.0]) + 0.006 * _ahead(),
           "D": np.array([1.1, 0.0, 0.0]) + 0.012 * _ahead()}[state]
    T = np.eye(4)
    T[:3, :3] = [[1, 0, 0], [0, 0, 1], [0, -1, 0]]
    T[:3, 3] = np.array([QUAD_AT[0], QUAD_HALF, QUAD_AT[1]]) + off
    return T.astype(F)


@functools.lru_cache(None)
def fold_scene(state="A"):
    sd = Q.floor_scene(rough=1.0, metal=0.0, blocker=(0.0, 0.0, 0.0, QUAD_HALF), sky=Q.sky_ramp(), cam=CAM,
                       name="fold-" + state)
    return dataclasses.replace(sd, instances=[(0, np.eye(4, dtype=F)), (1, quad_transform(state))])


@functools.lru_cache(None)
def jitter_scene():
    return Q.floor_scene(rough=1.0, metal=0.0, sky=None, cam=CAM, name="fold-jitter")


JIT_FLAGS = _lib.FLAGS_DEFAULT & ~(_lib.FLAG_GAMMA | _lib.FLAG_SKYBOX)
JIT_MODE = 1                              # RENDER_STATES::BASECOLOR
FLOOR = [(-Q.HALF, 0.0, -Q.HALF), (-Q.HALF, 0.0, Q.HALF), (Q.HALF, 0.0, Q.HALF), (Q.HALF, 0.0, -Q.HALF)]
N_FREQ, CHUNK, K_FRAMES = 4096, Q.CHUNK, 1024


@functools.lru_cache(None)
def jitter_ref():
    """(coverage [n], c [3] float32): fold_ref.coverage of the floor and the floor's base colour from scene_ref."""
    sd = jitter_scene()
    cam = R.camera(sd.cam_pos, sd.cam_target, F(W) / F(H))
    one = np.zeros(1, np.int64)
    c = R.material(sd.meshes[0], sd.textures, one, np.full(1, 0.25, F), np.full(1, 0.25, F))["base"][0].astype(F)
    return FR.coverage(cam, W, H, FLOOR), c


# ------------------------------------------------------------------------------------------------ shared checks
# A fold `view` is one implementation under test at 23 x 15 with the fold scene's four states:
#   view.capture(state, frame_index, flags, post) -> [n, 3] float32: that one reference frame, rendered alone with
#                                                    ACCUMULATE off on a fresh accumulation state
#   view.t1(state, post)                          -> [n] float32: the primary hit distances (Panini rays under `post`)
#   view.run(script, post)                        -> (per render step (avg [n, 4], rgb8 [n], (segments, shadow_rays)),
#                                                     the state (acc [n, 4], samples [n], distances [n]) at "save")
# A jitter `view` is one over the jitter scene:
#   view.centre() -> [n, 3] the non-AA frame;  view.aa_frames(k) -> [k, n, 3] single AA frames 0 .. k - 1
#   view.aa_mean(n) -> [n, 3] float64: the mean of n AA frames (averages of accumulating calls of CHUNK frames)
def check_gamma(view):
    """(a) For the same frame_index and seed a capture with GAMMA on is np.sqrt of the capture with GAMMA off."""
    for post in (None, POSTS["ab+2"]):
        for fi in (0, 5):
            for flags in (NOACC, NOACC & ~_lib.FLAG_AA):
                on = view.capture("A", fi, flags, post)
                off = view.capture("A", fi, flags & ~_lib.FLAG_GAMMA, post)
                assert (off > 1).any() and ((off > 0) & (off < 1)).any()
                assert flags & _lib.FLAG_AA or (off == 0).any()      # (one path: some end black)
                assert np.array_equal(SQ.bits(on), SQ.bits(FR.gamma(off))), (fi, flags)
                assert not np.array_equal(SQ.bits(on), SQ.bits(off))


def reference_run(view, script, post, slip=None):
    """fold_ref.Fold over `script`, fed with the view's captures and primary distances; the conditions the script has
    to meet are asserted here, on the reference's state alone."""
    fold = FR.Fold(W, H, slip)
    state, fi, saved, outs = "A", 0, None, []
    moved_from = None
    seen = dict(rows=0, restarted=0, kept=0, miss=0, above=False, zero=False, between=False, darkened=False)
    cleared = False
    for step in script:
        if step[0] == "render":
            _, k, flags = step
            for j in range(k):
                raw = view.capture(state, fi + j, flags & ~_lib.FLAG_GAMMA, post)
                frame = FR.gamma(raw, slip) if flags & _lib.FLAG_GAMMA else raw
                t = view.t1(state, post)
                before = fold.samplesPerPixel.copy()
                avg, rgb8 = fold.tick(frame, t, bool(flags & _lib.FLAG_ACCUMULATE), post)
                n = fold.samplesPerPixel
                if flags & _lib.FLAG_ACCUMULATE:
                    seen["miss"] += int(((t >= R.BVH_FAR) & (n > 1)).sum())
                    if moved_from is not None:
                        told = view.t1(moved_from, post)
                        seen["restarted"] += int(((before > 1) & (n == 1)).sum())
                        seen["kept"] += int(((told != t) & (t < R.BVH_FAR) & (n == before + 1) & (before > 0)).sum())
                moved_from = None
                if post is not None and post.aberration:
                    g = n.reshape(H, W)
                    xs = np.arange(W)
                    differ = np.zeros(H, bool)
                    for s in (post.aberration, -post.aberration):
                        differ |= (g[:, np.clip(xs + s, 0, W - 1)] != g).any(1)
                    seen["rows"] = max(seen["rows"], int(differ.sum()))
            fi += k
            if cleared:      # the memset of :147 left the counts: the next average is this frame over the old count
                seen["darkened"] |= bool(avg[:, :3].sum() < 0.5 * outs[-1][0][:, :3].sum())
                cleared = False
            seen["above"] |= bool((avg[:, :3] > 1).any())
            seen["zero"] |= bool((avg[:, :3] == 0).any())
            seen["between"] |= bool(((avg[:, :3] > 0) & (avg[:, :3] < 1)).any())
            outs.append((avg, rgb8))
        elif step[0] == "move":
            moved_from, state = state, step[1]
        elif step[0] == "reset":
            fold.fresh() if step[1] else fold.camera_moved()
            cleared = not step[1]
        elif step[0] == "save":
            saved = (fold.copy_state(), fi)
        elif step[0] == "load":
            fold.set_state(saved[0])
            fi = saved[1]
    if slip is None:
        print(f"fold conditions: {seen}")
        assert seen["restarted"] >= 1 and seen["kept"] >= 1 and seen["miss"] >= 1, seen
        assert seen["above"] and seen["zero"] and seen["between"] and seen["darkened"], seen
        if post is not None and post.aberration:
            assert seen["rows"] >= 3, seen
    return outs, (saved[0] if saved else None)


def check_script(view, post, script=SCRIPT, slip=None):
    """(b) After every call of the script avg and rgb8 equal fold_ref.Fold's, as uint32 views; so does the state
    (accumulator, samplesPerPixel, distances) at the script's checkpoint, where the view can read it."""
    want, want_state = reference_run(view, script, post, slip)
    got, got_state = view.run(script, post)
    assert len(got) == len(want)
    bad = []
    for i, ((a_w, r_w), (a_g, r_g, _)) in enumerate(zip(want, got)):
        pa = np.flatnonzero((SQ.bits(a_w) != SQ.bits(a_g)).any(1))
        pr = np.flatnonzero(r_w != r_g)
        if pa.size:
            bad.append(("avg", i, pa.size, pa[:4].tolist(), a_w[pa[:2]].tolist(), a_g[pa[:2]].tolist()))
        if pr.size:
            bad.append(("rgb8", i, pr.size, pr[:4].tolist(), [hex(v) for v in r_w[pr[:2]]],
                        [hex(v) for v in r_g[pr[:2]]]))
    assert not bad, (sorted({(b[0], b[1]) for b in bad}), bad[:2])
    if got_state is not None:
        assert np.array_equal(SQ.bits(want_state[0]), SQ.bits(got_state[0])), "accumulator"
        assert np.array_equal(want_state[1], got_state[1]), "samplesPerPixel"
        assert np.array_equal(SQ.bits(want_state[2]), SQ.bits(got_state[2])), "distances"


def check_aa_exact(view, frames=32):
    """(a) Every AA capture equals 0.5 * (s1 + s2) with s2 in {0, c} and s1 the non-AA capture; a pixel of coverage 1
    equals c in every frame and a pixel of coverage 0 equals 0 in every frame."""
    cov, c = jitter_ref()
    s1 = view.centre()
    assert (SQ.bits(s1) == SQ.bits(np.where((s1 != 0).any(1)[:, None], c, F(0)))).all()
    lo, hi = FR.aa_mean(s1, np.zeros(3, F)), FR.aa_mean(s1, c)
    caps = view.aa_frames(frames)
    is_lo = (SQ.bits(caps) == SQ.bits(lo)[None]).all(2)
    is_hi = (SQ.bits(caps) == SQ.bits(hi)[None]).all(2)
    assert (is_lo | is_hi).all(), int((~(is_lo | is_hi)).sum())
    full, empty = cov >= 1 - 1e-12, cov <= 1e-12
    part = (cov > 0.2) & (cov < 0.8)
    assert full.sum() >= 20 and empty.sum() >= 20 and part.sum() >= 5, (full.sum(), empty.sum(), part.sum())
    assert (SQ.bits(caps[:, full]) == SQ.bits(c)).all()
    assert (SQ.bits(caps[:, empty]) == 0).all()
    assert is_lo[:, part].any(0).all() and is_hi[:, part].any(0).all()     # both values occur at every such pixel


def check_jitter_frequency(view):
    """(d) The per-pixel mean of N_FREQ frames against 0.5 * (s1 + c p); returns the largest z."""
    cov, c = jitter_ref()
    c64 = c.astype(np.float64)
    s1 = view.centre().astype(np.float64)
    mean = view.aa_mean(N_FREQ)
    sel = np.flatnonzero((cov > 0.02) & (cov < 0.98))
    assert sel.size >= 12, sel.size
    p = cov[sel][:, None]
    exp = 0.5 * (s1[sel] + c64[None] * p)
    sigma = c64[None] * 0.5 * np.sqrt(p * (1 - p) / N_FREQ)
    allow = CHUNK * 2.0 ** -24 * c64[None]
    z = (np.abs(mean[sel] - exp) - allow) / sigma
    print(f"jitter frequency: {sel.size} pixels, largest z {z.max():.2f}")
    assert (z <= 6.0).all(), (float(z.max()), sel[(z > 6.0).any(1)], cov[sel[(z > 6.0).any(1)]])
    return float(z.max())


def indicators(view, k=K_FRAMES):
    """[k, n] bool: path 2 of frame f met the floor (the frame is the larger of its two possible values)."""
    cov, c = jitter_ref()
    s1 = view.centre()
    caps = view.aa_frames(k)
    hi = FR.aa_mean(s1, c)
    return (SQ.bits(caps) == SQ.bits(hi)[None]).all(2)


def check_jitter_pairs(view):
    """(d) Joint frequencies of two pixels, and of one pixel in consecutive frames; returns the two largest z."""
    cov, _ = jitter_ref()
    ind = indicators(view).astype(np.float64)
    k = ind.shape[0]
    sel = np.flatnonzero((cov > 0.2) & (cov < 0.8))
    assert sel.size >= 8, sel.size
    p = cov[sel]
    I = ind[:, sel]
    joint = (I.T @ I) / k
    q = np.outer(p, p)
    zp = np.abs(joint - q) / np.sqrt(q * (1 - q) / k)
    iu = np.triu_indices(sel.size, 1)
    lag = (I[:-1] * I[1:]).mean(0)
    var = (p ** 2 * (1 - p ** 2) + 2 * (p ** 3 - p ** 4)) / (k - 1)
    zl = np.abs(lag - p ** 2) / np.sqrt(var)
    print(f"jitter pairs: {sel.size} pixels, {iu[0].size} pairs, largest z {zp[iu].max():.2f}; lag 1 largest z "
          f"{zl.max():.2f}")
    assert (zp[iu] <= 6.0).all(), float(zp[iu].max())
    assert (zl <= 6.0).all(), float(zl.max())
    return float(zp[iu].max()), float(zl.max())


# ------------------------------------------------------------------------------------------------ the device
pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _postfx(post):
    pf = _lib.PostFx()
    if post is not None:
        pf.enabled, pf.aberration, pf.fov, pf.distortion = 1, int(post.aberration), post.fov, post.distortion
        pf.vignette_intensity, pf.vignette_radius = post.vignette_intensity, post.vignette_radius
        for i in range(4):
            pf.color_grading[i] = post.color_grading[i]
    return pf


def _rays(post):
    return None if post is None else (post.fov, post.distortion)


class Captures:
    """The device's frame values and primary distances, from a context of its own that keeps no primary-hit, light
    or surface records (PRT_PRIMARY_REUSE=0): the inputs of the fold do not pass through what the script exercises."""

    def __init__(self):
        import prt
        self.ctx = prt.Context(0)
        self.loaded = None
        self.frames, self.dists = {}, {}

    def _load(self, sd, post):
        from helpers import gpu_scene
        if self.loaded is not sd:
            gpu_scene(self.ctx, sd, W, H)
            self.loaded = sd
        self.ctx.set_postfx(_postfx(post))

    def frame(self, sd, fi, flags, post, mode=0, bounces=BOUNCES):
        key = (sd.name, fi, flags, _rays(post), mode, bounces)
        if key not in self.frames:
            self._load(sd, post)
            with _env(PRT_PRIMARY_REUSE="0"):
                self.ctx.reset_accumulation(full=True)
                spp = 2 if flags & _lib.FLAG_AA else 1
                avg = self.ctx.render(W, H, spp, bounces, flags & ~_lib.FLAG_ACCUMULATE, mode, fi, SEED)[0]
            self.frames[key] = avg[:, :3].copy()
        return self.frames[key]

    def t1(self, sd, post):
        key = (sd.name, _rays(post))
        if key not in self.dists:
            self._load(sd, post)
            self.dists[key] = self.ctx.trace_primary(W, H)[0]["t"].copy()
        return self.dists[key]

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def captures():
    c = Captures()
    yield c
    c.close()


@pytest.fixture(scope="module")
def script_ctx():
    import prt
    c = prt.Context(0)
    yield c
    c.close()


class GpuFoldView:
    def __init__(self, ctx, captures, env=None):
        self.ctx, self.cap, self.env = ctx, captures, env or {}

    def capture(self, state, fi, flags, post):
        return self.cap.frame(fold_scene(state), fi, flags, post)

    def t1(self, state, post):
        return self.cap.t1(fold_scene(state), post)

    def run(self, script, post):
        from helpers import gpu_scene
        ctx, fi, blob, out, state = self.ctx, 0, None, [], None
        scene, _ = gpu_scene(ctx, fold_scene("A"), W, H)
        ctx.set_postfx(_postfx(post))
        ctx.primary_rays(reset=True)
        ctx.surface_reuse(reset=True)
        with _env(**self.env):
            for step in script:
                if step[0] == "render":
                    _, k, flags = step
                    avg, rgb8, st = ctx.render(W, H, 2 * k, BOUNCES, flags, 0, fi, SEED)
                    out.append((avg.copy(), rgb8.copy(), (int(st.segments), int(st.shadow_rays))))
                    fi += k
                elif step[0] == "move":
                    T = [scene.blases[0][1], quad_transform(step[1])]
                    if step[1] == "B":         # a fresh instance BVH; the later moves refit it on the device
                        ctx.set_instances([(0, T[0]), (1, T[1])])
                    else:
                        ctx.update_instances(np.stack(T))
                elif step[0] == "reset":
                    ctx.reset_accumulation(full=bool(step[1]))
                elif step[0] == "save":
                    blob, saved_fi = ctx.save_accumulation(), fi
                    raw = np.frombuffer(blob, np.uint8)[len(blob) - 24 * N_PX:]      # (after the header)
                    state = (raw[:16 * N_PX].view(F).reshape(N_PX, 4), raw[16 * N_PX:20 * N_PX].view(np.int32),
                             raw[20 * N_PX:].view(F))
                elif step[0] == "load":
                    ctx.load_accumulation(blob)
                    fi = saved_fi
        self.reuse = (ctx.primary_rays(), ctx.surface_reuse())
        ctx.set_postfx(None)
        return out, state


class GpuJitterView:
    def __init__(self, captures):
        self.cap, self.sd = captures, jitter_scene()

    def centre(self):
        return self.cap.frame(self.sd, 0, JIT_FLAGS & ~_lib.FLAG_AA, None, JIT_MODE, 1)

    def aa_frames(self, k):
        return np.stack([self.cap.frame(self.sd, f, JIT_FLAGS, None, JIT_MODE, 1) for f in range(k)])

    def aa_mean(self, n):
        self.cap._load(self.sd, None)
        total = np.zeros((N_PX, 3), np.float64)
        for f0 in range(0, n, CHUNK):
            self.cap.ctx.reset_accumulation(full=True)
            avg = self.cap.ctx.render(W, H, 2 * CHUNK, 1, JIT_FLAGS, JIT_MODE, f0, SEED)[0]
            total += avg[:, :3].astype(np.float64)
        return total / (n // CHUNK)


def test_gamma_is_the_square_root_of_the_frame(script_ctx, captures):
    check_gamma(GpuFoldView(script_ctx, captures))


def test_aa_frame_is_one_of_two_values(captures):
    check_aa_exact(GpuJitterView(captures))


@pytest.mark.parametrize("post", ["none", "ab+2", "ab-1", "ab-clamped"])
def test_script_matches_the_literal_fold(script_ctx, captures, post):
    """The script's context keeps its records (no switch set; at this size the two AA paths run merged): its primary
    hits were traced once per geometry state and taken from the kept record in every other frame."""
    view = GpuFoldView(script_ctx, captures)
    check_script(view, POSTS[post])
    (traced, reused), surface = view.reuse
    frames = sum(s[1] for s in SCRIPT if s[0] == "render")
    print(f"primary rays traced {traced} reused {reused}, surface items reused {surface}")
    assert traced == N_VIEWS * N_PX and reused == (frames - N_VIEWS) * N_PX


@pytest.mark.parametrize("post", ["none", "ab+2"])
def test_script_unmerged_with_the_surface_record(script_ctx, captures, post):
    """PRT_MERGE=0: the plain pipeline with the deferred resolve, which frames above 2^21 items take and which alone
    keeps the primary-surface record; the third call on every geometry state shades from it."""
    view = GpuFoldView(script_ctx, captures, env={"PRT_MERGE": "0"})
    check_script(view, POSTS[post])
    (traced, reused), surface = view.reuse
    frames = sum(s[1] for s in SCRIPT if s[0] == "render")
    print(f"primary rays traced {traced} reused {reused}, surface items reused {surface}")
    assert traced == N_VIEWS * N_PX and reused == (frames - N_VIEWS) * N_PX and surface >= N_VIEWS * N_PX


def test_script_in_passes_of_one_frame(script_ctx, captures):
    """PRT_MAX_ITEMS = W * H: a call of 3 frames runs as three passes, each folded into the state in order."""
    check_script(GpuFoldView(script_ctx, captures, env={"PRT_MAX_ITEMS": str(N_PX)}), POSTS["ab+2"])


def test_script_on_a_group(captures):
    """(c) A local group of 3 with tile 8 over 23 x 15 (neither side a multiple of the tile): member 0's outputs equal
    the fold's, through k_untile's vignette and grading and the tile map's overhang; no aberration (a group refuses
    it: the taps would need the neighbouring tiles' accumulators).  The group refuses one step of the script, the
    checkpoint (prt_save_accumulation: "accumulation checkpoints of a local group"), so the script runs without it:
    the two calls that follow it run once."""
    import prt
    assert W % 8 and H % 8
    g = prt.Context(group=[0] * 3, tile=8)
    try:
        with pytest.raises(prt.PrtError, match="checkpoints of a local group"):
            g.save_accumulation()
        check_script(GpuFoldView(g, captures), POSTS["no-ab"], SCRIPT_NO_CHECKPOINT)
    finally:
        g.close()


def test_jitter_frequency(captures):
    check_jitter_frequency(GpuJitterView(captures))


def test_jitter_pairs_and_lag(captures):
    check_jitter_pairs(GpuJitterView(captures))


def test_device_equals_oracle(script_ctx, captures, oracle_mod):
    """(e) Every call of the script, per screen pass: avg, rgb8 and (segments, shadow_rays) bit for bit."""
    import test_fold_ref as T
    for name in ("none", "ab+2", "ab-1", "ab-clamped"):
        got, state_g = GpuFoldView(script_ctx, captures).run(SCRIPT, POSTS[name])
        want, state_w = T.OracleFoldView(oracle_mod).run(SCRIPT, POSTS[name])
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(state_w, state_g)), name
        for i, ((a_w, r_w, s_w), (a_g, r_g, s_g)) in enumerate(zip(want, got)):
            assert np.array_equal(SQ.bits(a_w), SQ.bits(a_g)), (name, i)
            assert np.array_equal(r_w, r_g), (name, i)
            assert s_w == s_g, (name, i, s_w, s_g)
