"""Literal numpy reference for the last stage of a frame: what Renderer::Tick does once Trace has returned
(Core/Renderer.cpp:58-147) -- the AA mean, the square root, the distance-keyed progressive mean with its restart, its
!accumulates branch and the end-of-frame memset, the chromatic aberration that reads its neighbours' accumulators in
row-walk order, vignette, grading and RGBF32_to_RGB8 (template/precomp.h:311-314).  TEST INFRASTRUCTURE ONLY.

Written from those source lines, Core/Renderer.h:61-63 (the state and its initialisers), Core/Camera.cpp:113-122 (the
screen plane the jitter walks on) and include/prt.h (which call is which reference event), not from the C restatement
(oracle/prt_oracle.c) nor from the device code: this module imports neither `oracle` nor `prt`, and `scene_ref` only
for the camera's screen plane, so a slip that the two restatements share disagrees with it.

Fold          the state and one Tick, pixel by pixel in the reference's loop order, every intermediate np.float32 (each
              + - * / sqrt one rounding, as C built with -ffp-contract=off); pow in float64 rounded once, the
              convention of prt_math.h.  The aberration reads the live accumulator, so that a tap left of x sees this
              frame and a tap right of x the frame before -- or the memset -- without that being restated.
gamma, aa_mean  the two lines :73-79 and :65.
coverage      the exact probability that a pixel's jittered path 2 meets a convex world-space polygon.
simulate_aa   frames of a two-valued scene drawn from the jitter's definition (for the planted jitter slips).

`slip=` plants one named defect (SLIPS) to show that a comparison against this reference has the power to notice it;
tests/test_fold_ref.py runs every one of them.
"""
import collections

import numpy as np

import scene_ref as R

F = np.float32
EPSILON = R.EPSILON      # template/common.h:26

# the six screen-pass members of the camera (Core/Camera.h:12,23,27); aberration is an int
Post = collections.namedtuple("Post", "aberration fov distortion vignette_intensity vignette_radius color_grading")

SLIPS = (
    # Fold.tick / Fold.camera_moved
    "aberration_neighbour_count",     # :115-116 divide by the tapped pixel's sample count
    "aberration_new_both_sides",      # the taps right of x read this frame's accumulator too
    "aberration_sign_swapped",        # red taps x - a, blue taps x + a
    "gamma_after_mean",               # :73-79 applied to the average instead of the frame
    "restart_keeps_count",            # :93 missing
    "distance_only_on_restart",       # :98 moved into the else branch
    "moved_resets_counts",            # :147 also clears samplesPerPixel and distances
    "no_accumulate_leaves_accumulator",   # :147 without `|| !accumulates`
    "vignette_at_centre",             # :124 (x + 0.5) / SCRWIDTH
    "pack_rounds",                    # precomp.h:311 rounds to nearest
    # simulate_aa
    "jitter_centred",                 # :61 RandomFloat() - 0.5
    "jitter_one_draw",                # :61 one RandomFloat() for both axes
    "jitter_x_only",                  # :61 y not jittered
    "jitter_path1_too",               # :58 r1 jittered as well (by its own two draws)
)
FOLD_SLIPS, JITTER_SLIPS = SLIPS[:10], SLIPS[10:]


def gamma(frame, slip=None):
    """Core/Renderer.cpp:73-79 on an [n, 3] float32 frame (the caller holds GAMMACORRECTED)."""
    frame = np.asarray(frame, F)
    if slip == "gamma_after_mean":
        return frame
    return np.sqrt(frame)                                                                   # :76-78


def aa_mean(s1, s2):
    """Core/Renderer.cpp:65."""
    return F(0.5) * (np.asarray(s1, F) + np.asarray(s2, F))                                 # :65


def _min(a, b):
    return a if a < b else b                                                                # tmpl8math.h min(float, float)


def pack_rgb8(v, slip=None):
    """RGBF32_to_RGB8, template/precomp.h:311-314 (the scalar path) of one float4.  The conversion of a negative or
    NaN channel is undefined there; neither occurs in the unslipped reference (a planted slip may divide by a zero
    count: such a channel packs as 0 here, whatever the implementation under test makes of it)."""
    out = []
    for k in range(3):
        q = F(255.0) * _min(F(1.0), v[k])                                                   # :311-313
        if not q >= 0:
            q = F(0)
        out.append(int(q + F(0.5)) if slip == "pack_rounds" else int(q))
    return (out[0] << 16) + (out[1] << 8) + out[2]                                          # :314


class Fold:
    """accumulator, samplesPerPixel, distances (Core/Renderer.h:61-63, Renderer.cpp:11-12) and Tick's fold."""

    def __init__(self, W, H, slip=None):
        assert slip is None or slip in FOLD_SLIPS
        self.W, self.H, self.slip = W, H, slip
        self.fresh()

    def fresh(self):
        """A new Renderer."""
        n = self.W * self.H
        self.accumulator = np.zeros((n, 4), F)                                              # Renderer.cpp:11-12
        self.samplesPerPixel = np.zeros(n, np.int32)                                        # Renderer.h:61: { 1 } sets
        self.samplesPerPixel[0] = 1                                                         #   element 0 alone
        self.distances = np.zeros(n, F)                                                     # Renderer.h:62: { -1.f }
        self.distances[0] = F(-1.0)                                                         #   likewise

    def camera_moved(self):
        """camera.HandleInput() returned true: the memset of :147."""
        self.accumulator[:] = F(0)                                                          # :147
        if self.slip == "moved_resets_counts":
            n = self.W * self.H
            self.samplesPerPixel = np.zeros(n, np.int32)
            self.distances = np.full(n, F(-1.0))

    def copy_state(self):
        return self.accumulator.copy(), self.samplesPerPixel.copy(), self.distances.copy()

    def set_state(self, state):
        self.accumulator, self.samplesPerPixel, self.distances = (a.copy() for a in state)

    def tick(self, frame_rgb, t1, accumulates, post):
        """One reference frame: frame_rgb [n, 3] float32 is traceResult after :79, t1 [n] float32 is r1.hit.t.
        Returns (avg_rgba [n, 4] float32, rgb8 [n] uint32)."""
        W, H, slip = self.W, self.H, self.slip
        frame_rgb, t1 = np.asarray(frame_rgb, F), np.asarray(t1, F)
        acc, spp, dist = self.accumulator, self.samplesPerPixel, self.distances
        avg = np.zeros((W * H, 4), F)
        rgb8 = np.zeros(W * H, np.uint32)
        if slip == "aberration_new_both_sides":      # fold the whole frame first, then walk the screen pass
            passes = ((True, False), (False, True))
        else:
            passes = ((True, True),)
        with np.errstate(divide="ignore", invalid="ignore"):
            for fold, screen in passes:
                for y in range(H):                                                          # :44
                    pixelHeight = y * W                                                     # :46
                    for x in range(W):                                                      # :47
                        p = x + pixelHeight
                        if fold:
                            avg[p] = self._fold(p, frame_rgb[p], t1[p], accumulates)
                        if not screen:
                            continue
                        average = avg[p]
                        if post is None:                                                    # :136
                            rgb8[p] = pack_rgb8(average, slip)                              # :137
                            continue
                        ab = average.copy()                                                 # :110
                        a = int(post.aberration)
                        if a != 0:                                                          # :111
                            sR = min(max(x + a, 0), W - 1)                                  # :113
                            sB = min(max(x - a, 0), W - 1)                                  # :114
                            if slip == "aberration_sign_swapped":
                                sR, sB = sB, sR
                            nR = nB = spp[p]
                            if slip == "aberration_neighbour_count":
                                nR, nB = spp[sR + pixelHeight], spp[sB + pixelHeight]
                            color_R = acc[sR + pixelHeight] * (F(1.0) / F(nR))              # :115
                            color_B = acc[sB + pixelHeight] * (F(1.0) / F(nB))              # :116
                            red = F(0.75) * average[0] + F(0.25) * color_R[0]               # :117
                            g = average[1]                                                  # :118
                            b = F(0.75) * average[2] + F(0.25) * color_B[2]                 # :119
                            ab = np.array([red, g, b, average[3]], F)                       # :120
                        xs = F(x) + F(0.5) if slip == "vignette_at_centre" else F(x)
                        ys = F(y) + F(0.5) if slip == "vignette_at_centre" else F(y)
                        ux, uy = xs / F(W), ys / F(H)                                       # :124
                        ux, uy = ux * (F(1.0) - ux), uy * (F(1.0) - uy)                     # :125
                        vig = ux * uy * F(post.vignette_intensity)                          # :126
                        vig = F(np.power(np.float64(vig), np.float64(F(post.vignette_radius))))   # :127
                        ab = ab * np.asarray(post.color_grading, F)                         # :130
                        rgb8[p] = pack_rgb8(ab * vig, slip)                                 # :133
        if not accumulates and slip != "no_accumulate_leaves_accumulator":                  # :147
            acc[:] = F(0)
        return avg, rgb8

    def _fold(self, p, traceResult, t, accumulates):
        acc, spp, dist, slip = self.accumulator, self.samplesPerPixel, self.distances, self.slip
        if accumulates:                                                                     # :82
            if abs(dist[p] - t) < EPSILON:                                                  # :84
                spp[p] += 1                                                                 # :86
                acc[p, :3] += traceResult                                                   # :88
                average = acc[p] * (F(1.0) / F(spp[p]))                                     # :89
            else:
                if slip != "restart_keeps_count":
                    spp[p] = 1                                                              # :93
                acc[p, :3] = traceResult                                                    # :94
                acc[p, 3] = F(0)
                average = acc[p].copy()                                                     # :95
                if slip == "distance_only_on_restart":
                    dist[p] = t
            if slip != "distance_only_on_restart":
                dist[p] = t                                                                 # :98
        else:
            acc[p, :3] = traceResult                                                        # :102
            acc[p, 3] = F(0)
            average = acc[p].copy()                                                         # :103
        if slip == "gamma_after_mean":
            average = np.sqrt(average)
        return average


# ------------------------------------------------------------------------------------------------ the jitter
def _plane(cam, W, H):
    """The screen plane in pixel units, float64: P(px, py) = tl + px ex + py ey (Core/Camera.cpp:116-120)."""
    tl, tr, bl, pos = (np.asarray(cam[k], F).astype(np.float64) for k in ("tl", "tr", "bl", "pos"))
    return pos, tl, (tr - tl) / W, (bl - tl) / H


def project(cam, W, H, points):
    """World points -> (px, py) such that the ray through P(px, py) passes through the point: pos + s d = tl + px ex +
    py ey solved per point (every point must lie in front of the camera: s > 0)."""
    pos, tl, ex, ey = _plane(cam, W, H)
    out = []
    for q in np.asarray(points, np.float64):
        d = q - pos
        px, py, s = np.linalg.solve(np.stack([ex, ey, -d], 1), pos - tl)
        assert s > 0, "a polygon corner behind the camera"
        out.append((px, py))
    return np.array(out)


def _clip(poly, axis, bound, keep_below):
    """Sutherland-Hodgman against one axis-aligned half plane."""
    out = []
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        ina = a[axis] <= bound if keep_below else a[axis] >= bound
        inb = b[axis] <= bound if keep_below else b[axis] >= bound
        if ina:
            out.append(a)
        if ina != inb:
            s = (bound - a[axis]) / (b[axis] - a[axis])
            out.append(a + s * (b - a))
    return out


def _area(poly):
    if len(poly) < 3:
        return 0.0
    q = np.array(poly)
    x, y = q[:, 0], q[:, 1]
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


def coverage(cam, W, H, polygon):
    """[H * W] float64: the area fraction of each pixel's jitter footprint [x, x + 1) x [y, y + 1) (Renderer.cpp:61:
    x + RandomFloat(), y + RandomFloat(), RandomFloat() uniform over [0, 1)) that the convex world-space `polygon`
    covers.  The plane projection is affine in pixel coordinates, so the polygon's corners are projected, the projected
    polygon is clipped to the unit square, and the area is the shoelace sum."""
    poly = [np.array(p) for p in project(cam, W, H, polygon)]
    out = np.zeros(W * H)
    for y in range(H):
        for x in range(W):
            c = poly
            for axis, bound, below in ((0, x, False), (0, x + 1, True), (1, y, False), (1, y + 1, True)):
                c = _clip(c, axis, bound, below)
                if not c:
                    break
            out[y * W + x] = _area(c)
    return np.clip(out, 0.0, 1.0)


def inside(poly, px, py):
    """Points (px, py) inside the convex polygon `poly` (its corners in order, either orientation)."""
    q = np.asarray(poly)
    sign = None
    ok = np.ones(np.shape(px), bool)
    for i in range(len(q)):
        a, b = q[i], q[(i + 1) % len(q)]
        cr = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
        if sign is None:
            ctr = q.mean(0)
            sign = np.sign((b[0] - a[0]) * (ctr[1] - a[1]) - (b[1] - a[1]) * (ctr[0] - a[0]))
        ok &= cr * sign >= 0
    return ok


def simulate_aa(cam, W, H, polygon, frames, seed, slip=None):
    """[frames, H * W] float64: 0.5 * (s1 + s2) of a scene that returns 1 inside `polygon` and 0 outside, with the
    jitter of :58-65 drawn from numpy's generator (two independent draws per pixel and frame)."""
    assert slip is None or slip in JITTER_SLIPS
    rng = np.random.default_rng(seed)
    poly = project(cam, W, H, polygon)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
    jx, jy = rng.random((frames, W * H)), rng.random((frames, W * H))                       # :61
    if slip == "jitter_centred":
        jx, jy = jx - 0.5, jy - 0.5
    elif slip == "jitter_one_draw":
        jy = jx
    elif slip == "jitter_x_only":
        jy = np.zeros_like(jx)
    x1, y1 = np.broadcast_to(xs, jx.shape), np.broadcast_to(ys, jx.shape)                   # :58
    if slip == "jitter_path1_too":
        x1, y1 = xs + rng.random((frames, W * H)), ys + rng.random((frames, W * H))
    s1 = inside(poly, x1, y1).astype(np.float64)                                            # :63
    s2 = inside(poly, xs + jx, ys + jy).astype(np.float64)                                  # :64
    return 0.5 * (s1 + s2)                                                                  # :65
