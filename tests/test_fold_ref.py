"""tests/fold_ref.py proven on the CPU, then the checks of tests/test_gpu_fold.py run against the oracle
(oracle/prt_oracle.c orc_render / pixel_frame), and every planted slip of fold_ref.SLIPS shown to fail one of them.

What the reference asserts about itself: `coverage` agrees with a 64 x 64 supersample of every pixel and its sum with
the area of the projected polygon inside the image; frames drawn from the jitter's definition (simulate_aa) pass the
jitter checks.

The conditions of the script (asserted in test_gpu_fold.reference_run on Fold's state alone): a pixel restarted by the
move, one kept across the sub-EPSILON moves, an accumulating miss, averages above 1, equal to 0 and in between, and
under an aberration at least 3 rows with a pixel whose tap has another sample count.

Each slip fails a check on the data the unslipped reference passes (test_slip_is_caught).  The fold's slips are run
through check_script on the oracle under the screen pass "ab+2"; the calls of the script (numbered from 0: 0-2 on
state A, 3-5 on B, 6-8 on C, 9 on D, 10 after the partial reset, 11-12 and 13-14 the two calls around the checkpoint,
15 after the full reset) whose outputs then differ:
  aberration_neighbour_count, aberration_new_both_sides, aberration_sign_swapped,
  vignette_at_centre, pack_rounds                  rgb8 of every call (pack_rounds also without a screen pass)
  gamma_after_mean, restart_keeps_count            avg of every call of more than one accumulated frame, rgb8 of all
  distance_only_on_restart                         avg and rgb8 from call 9 on: state D lies further than EPSILON from B
  moved_resets_counts                              avg and rgb8 from call 10 on (the partial reset)
  no_accumulate_leaves_accumulator                 avg and rgb8 of calls 12 and 14 (the frames after the !ACCUMULATE one)
The jitter's slips are run on simulated frames (fold_ref.simulate_aa); each of the four fails check_aa_exact,
check_jitter_frequency (largest z 37 to 406 against 1.8 for the unslipped simulation) and check_jitter_pairs (largest
z 25 to 37 against 2.7).  On the oracle: frequency 2.35, pairs 2.29, lag 1 1.42.
"""
import functools

import numpy as np
import pytest

import fold_ref as FR
import scene_ref as R
import test_gpu_fold as T
from prt import _lib

F = np.float32
W, H = T.W, T.H


# ------------------------------------------------------------------------------------------------ the reference alone
def _cam():
    sd = T.jitter_scene()
    return R.camera(sd.cam_pos, sd.cam_target, F(W) / F(H))


def test_coverage_against_a_supersample():
    """64 x 64 cell centres per pixel.  A pixel's cells that the polygon's outline crosses number at most 2 * 64 per
    edge through the pixel, at most two edges cross a pixel here, and a crossed cell is off by at most half a cell:
    |coverage - supersample| <= 2 * 2 * 64 * 0.5 / 64^2 = 1 / 32.  The summed coverage is the area of the projected
    polygon clipped to the image, exactly."""
    cam = _cam()
    cov, _ = T.jitter_ref()
    poly = FR.project(cam, W, H, T.FLOOR)
    s = (np.arange(64) + 0.5) / 64
    for y in range(H):
        for x in range(W):
            px, py = np.meshgrid(x + s, y + s)
            ss = FR.inside(poly, px, py).mean()
            assert abs(ss - cov[y * W + x]) <= 1 / 32, (x, y, ss, cov[y * W + x])
    c = [np.array(p) for p in poly]
    for axis, bound, below in ((0, 0, False), (0, W, True), (1, 0, False), (1, H, True)):
        c = FR._clip(c, axis, bound, below)
    assert abs(cov.sum() - FR._area(c)) < 1e-9
    part = (cov > 0.02) & (cov < 0.98)
    assert part.sum() >= 12 and (cov == 1).sum() >= 20 and (cov == 0).sum() >= 20
    # by hand: the unit square's corners seen from the plane's own parametrisation project onto themselves
    pos, tl, ex, ey = FR._plane(cam, W, H)
    q = tl + 3.25 * ex + 7.5 * ey
    assert np.allclose(FR.project(cam, W, H, [pos + 2.7 * (q - pos)])[0], [3.25, 7.5], atol=1e-9)


def test_literal_initial_state_is_spent_by_an_accumulating_frame():
    """Renderer.h:61-62 initialise element 0 alone (count 1, distance -1; every other count and distance 0), where the
    restatements start every pixel at count 0 and distance -1.  One accumulating frame makes the two the same state
    and gives the same outputs: every pixel restarts (no primary distance lies within EPSILON of 0 or of -1) or, from
    distance 0, adds to a zero accumulator under the count 0 + 1.  Only a first frame with accumulates off could tell
    them apart, through the aberration's division by the count: that divides by zero at every pixel but the first in
    the reference, so the scripts of these tests begin with an accumulating call."""
    rng = np.random.default_rng(1)
    frame = rng.uniform(0, 2, (6, 3)).astype(F)
    t = np.array([1.5, 0.005, 1e30, 0.02, 3.0, 1e30], F)
    post = FR.Post(1, 1.0, 0.0, 4.0, 0.5, (1.0, 0.5, 2.0, 1.0))
    a, b = FR.Fold(3, 2), FR.Fold(3, 2)
    b.set_state((np.zeros((6, 4), F), np.zeros(6, np.int32), np.full(6, -1.0, F)))
    (avg_a, rgb_a), (avg_b, rgb_b) = a.tick(frame, t, True, post), b.tick(frame, t, True, post)
    assert np.array_equal(avg_a, avg_b) and np.array_equal(rgb_a, rgb_b)
    for x, y in zip(a.copy_state(), b.copy_state()):
        assert np.array_equal(x, y)
    assert a.samplesPerPixel.tolist() == [1] * 6


def test_fold_by_hand():
    """Two pixels, three frames, worked by hand: the literal initial state (element 0 alone initialised), a restart, an
    accumulation, the aberration's row walk and the pack."""
    f = FR.Fold(2, 1)
    assert f.samplesPerPixel.tolist() == [1, 0] and f.distances.tolist() == [-1.0, 0.0]
    post = FR.Post(1, 1.0, 0.0, 4.0, 0.0, (1.0, 1.0, 1.0, 1.0))      # pow(v, 0) = 1: no vignette
    t = np.array([2.0, 1e30], F)
    a, r = f.tick(np.array([[0.5, 0.25, 1.0], [2.0, 0.0, 0.5]], F), t, True, post)
    assert f.samplesPerPixel.tolist() == [1, 1] and np.array_equal(a[:, :3], [[0.5, 0.25, 1.0], [2.0, 0.0, 0.5]])
    # pixel 0: red taps x + 1 (not yet walked: the zero accumulator), blue taps x - 1 -> clamped to itself (new)
    assert r[0] == (int(255 * (0.75 * 0.5)) << 16) + (int(255 * 0.25) << 8) + 255
    # pixel 1: red taps x + 1 -> clamped to itself, blue taps pixel 0's new accumulator
    assert r[1] == (255 << 16) + 0 + int(255 * (0.75 * 0.5 + 0.25 * 1.0))
    a, r = f.tick(np.array([[1.5, 0.75, 0.0], [0.0, 1.0, 0.5]], F), t, True, post)
    assert f.samplesPerPixel.tolist() == [2, 2] and np.array_equal(a[:, :3], [[1.0, 0.5, 0.5], [1.0, 0.5, 0.5]])
    # pixel 0: red = 0.75 * 1 + 0.25 * (2.0 / 2) (pixel 1's accumulator of the frame before, over pixel 0's count)
    assert r[0] == (255 << 16) + (127 << 8) + int(255 * (0.75 * 0.5 + 0.25 * 0.5))
    f.camera_moved()
    a, _ = f.tick(np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], F), np.array([2.005, 3.0], F), True, None)
    assert f.samplesPerPixel.tolist() == [3, 1]                      # |dt| < EPSILON goes on, the count stayed
    assert np.array_equal(a[:, :3], np.array([[1 / 3] * 3, [1.0] * 3], F) * F(1))
    a, _ = f.tick(np.array([[4.0, 4.0, 4.0], [4.0, 4.0, 4.0]], F), np.array([2.005, 3.0], F), False, None)
    assert (f.accumulator == 0).all() and f.samplesPerPixel.tolist() == [3, 1] and (a[:, :3] == 4).all()


# ------------------------------------------------------------------------------------------------ the oracle
class OracleFoldView:
    """One OracleScene per geometry state, sharing one accumulation state."""

    def __init__(self, oracle_mod):
        self.o = oracle_mod
        self.scenes = {}

    def _scene(self, state, post):
        if state not in self.scenes:
            self.scenes[state] = self.o.OracleScene(T.fold_scene(state), W, H)
        osc = self.scenes[state]
        if post is None:
            osc.set_postfx(False)
        else:
            osc.set_postfx(True, post.aberration, post.fov, post.distortion, post.vignette_intensity,
                           post.vignette_radius, post.color_grading)
        return osc

    @functools.lru_cache(None)
    def capture(self, state, fi, flags, post):
        out, _, _ = self._scene(state, post).render_frames(W, H, spp=2 if flags & _lib.FLAG_AA else 1, bounces=T.BOUNCES,
                                                           flags=flags & ~_lib.FLAG_ACCUMULATE, frame_index=fi,
                                                           seed=T.SEED)
        return out[0, :, :3].copy()

    @functools.lru_cache(None)
    def t1(self, state, post):
        return self._scene(state, post).primary_hits(W, H)[0].copy()

    @functools.lru_cache(None)
    def run(self, script, post):
        state, fi, saved, out, at_save = "A", 0, None, [], None
        acc = self.o.new_state(W, H)
        for step in script:
            if step[0] == "render":
                _, k, flags = step
                avg, rgb8, _, st = self._scene(state, post).render(W, H, spp=2 * k, bounces=T.BOUNCES, flags=flags,
                                                                   frame_index=fi, seed=T.SEED, state=acc)
                out.append((avg.copy(), rgb8.copy(), (int(st.segments), int(st.shadow_rays))))
                fi += k
            elif step[0] == "move":
                state = step[1]
            elif step[0] == "reset":
                if step[1]:
                    acc = self.o.new_state(W, H)
                else:
                    acc[0][:] = 0
            elif step[0] == "save":
                saved = (tuple(a.copy() for a in acc), fi)
                at_save = saved[0]
            elif step[0] == "load":
                acc, fi = tuple(a.copy() for a in saved[0]), saved[1]
        return out, at_save


class OracleJitterView:
    def __init__(self, oracle_mod):
        self.osc = oracle_mod.OracleScene(T.jitter_scene(), W, H)

    def centre(self):
        return self.osc.render_frames(W, H, spp=1, bounces=1, flags=T.JIT_FLAGS & ~_lib.FLAG_AA, mode=T.JIT_MODE,
                                      seed=T.SEED)[0][0, :, :3].copy()

    @functools.lru_cache(None)
    def aa_frames(self, k):
        return self.osc.render_frames(W, H, spp=2 * k, bounces=1, flags=T.JIT_FLAGS, mode=T.JIT_MODE,
                                      seed=T.SEED)[0][:, :, :3].copy()

    def aa_mean(self, n):
        total = np.zeros((T.N_PX, 3), np.float64)
        for f0 in range(0, n, T.CHUNK):
            avg = self.osc.render(W, H, spp=2 * T.CHUNK, bounces=1, flags=T.JIT_FLAGS, mode=T.JIT_MODE,
                                  frame_index=f0, seed=T.SEED)[0]
            total += avg[:, :3].astype(np.float64)
        return total / (n // T.CHUNK)


@pytest.fixture(scope="module")
def fold_view(oracle_mod):
    return OracleFoldView(oracle_mod)


@pytest.fixture(scope="module")
def jitter_view(oracle_mod):
    return OracleJitterView(oracle_mod)


def test_oracle_gamma_is_the_square_root_of_the_frame(fold_view):
    T.check_gamma(fold_view)


def test_oracle_aa_frame_is_one_of_two_values(jitter_view):
    T.check_aa_exact(jitter_view)


@pytest.mark.parametrize("post", ["none", "ab+2", "ab-1", "ab-clamped", "no-ab"])
def test_oracle_script_matches_the_literal_fold(fold_view, post):
    T.check_script(fold_view, T.POSTS[post], T.SCRIPT)


def test_oracle_script_without_checkpoint(fold_view):
    T.check_script(fold_view, T.POSTS["no-ab"], T.SCRIPT_NO_CHECKPOINT)


def test_oracle_jitter_frequency(jitter_view):
    T.check_jitter_frequency(jitter_view)


def test_oracle_jitter_pairs_and_lag(jitter_view):
    T.check_jitter_pairs(jitter_view)


# ------------------------------------------------------------------------------------------------ the slips
class SimView:
    """Frames drawn from the jitter's definition (fold_ref.simulate_aa), scaled by the floor's colour."""

    def __init__(self, slip=None, seed=7):
        cov, self.c = T.jitter_ref()
        cam = _cam()
        self.sim = FR.simulate_aa(cam, W, H, T.FLOOR, T.N_FREQ, seed, slip)
        poly = FR.project(cam, W, H, T.FLOOR)
        ys, xs = np.mgrid[0:H, 0:W]
        self.s1 = FR.inside(poly, xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64))

    def _colour(self, v):
        # v = 0.5 * (s1 + s2) in {0, 0.5, 1}: the same float32 operations as aa_mean on the coloured samples
        lo, hi = FR.aa_mean(np.zeros(3, F), self.c), FR.aa_mean(self.c, self.c)
        return np.where((v == 0.5)[..., None], lo, np.where((v == 1.0)[..., None], hi, F(0))).astype(F)

    def centre(self):
        return np.where(self.s1[:, None], self.c, F(0)).astype(F)

    def aa_frames(self, k):
        return self._colour(self.sim[:k])

    def aa_mean(self, n):
        return self._colour(self.sim[:n]).astype(np.float64).mean(0)


def test_simulated_jitter_passes():
    v = SimView()
    T.check_aa_exact(v)
    T.check_jitter_frequency(v)
    T.check_jitter_pairs(v)


JITTER_CHECKS = (T.check_aa_exact, T.check_jitter_frequency, T.check_jitter_pairs)


@pytest.mark.parametrize("slip", FR.SLIPS)
def test_slip_is_caught(fold_view, slip):
    if slip in FR.FOLD_SLIPS:
        with pytest.raises(AssertionError):
            T.check_script(fold_view, T.POSTS["ab+2"], T.SCRIPT, slip=slip)
        return
    failed = []
    v = SimView(slip)
    for check in JITTER_CHECKS:
        try:
            check(v)
        except AssertionError:
            failed.append(check.__name__)
    print(f"{slip}: fails {failed}")
    assert failed, slip
