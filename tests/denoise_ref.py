"""numpy float32 reference of the edge-avoiding a-trous filter (include/prt.h prt_denoise, DESIGN.md "Denoiser").

Every operation is one correctly rounded f32 + - * / or sqrt in the order the definition writes it, vectorised over
the pixels with a loop over the 25 taps in their stated order, so csrc/prt_denoise.hip (built without FMA contraction,
with IEEE division) must reproduce it bit for bit."""
import numpy as np

F = np.float32
DEFAULTS = dict(iterations=5, normal_power=3, sigma_color=4.0, sigma_depth=0.1, sigma_albedo=0.25)
H5 = [F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0)]
FAR = F(1e30)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _shift(a, oy, ox, fill):
    """out[y, x] = a[y + oy, x + ox], `fill` where that lies outside the image."""
    Hh, Ww = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -oy), min(Hh, Hh - oy)
    xs0, xs1 = max(0, -ox), min(Ww, Ww - ox)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return out


def denoise(color, albedo, normal_depth, W, H, iterations=5, normal_power=3, sigma_color=4.0, sigma_depth=0.1,
            sigma_albedo=0.25):
    """color / albedo / normal_depth: float32 [W*H, 4] (albedo may be None when sigma_albedo == 0).  Returns the
    filtered [W*H, 4] image: rgb filtered, w copied from color."""
    color = np.asarray(color, F).reshape(H, W, 4)
    nd = np.asarray(normal_depth, F).reshape(H, W, 4)
    sigma_color, sigma_depth, sigma_albedo = F(sigma_color), F(sigma_depth), F(sigma_albedo)
    use_albedo = sigma_albedo > 0
    A = np.asarray(albedo, F).reshape(H, W, 4)[..., :3] if use_albedo else None
    Z = nd[..., 3]
    hit = Z < FAR
    N = nd[..., :3]
    with np.errstate(all="ignore"):
        inv = F(1) / np.sqrt(_dot(N, N))
        n = N * inv[..., None]
        I = color[..., :3].copy()
        for i in range(iterations):
            s = 1 << i
            sc = sigma_color * F(2.0 ** -i)
            sc2 = sc * sc
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ok = _shift(hit, s * dy, s * dx, False)  # inside the image and a hit
                    Iq = _shift(I, s * dy, s * dx, F(0))
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), H5[2] * H5[2], F)
                    else:
                        nq = _shift(n, s * dy, s * dx, F(0))
                        Zq = _shift(Z, s * dy, s * dx, F(1))
                        dn = _dot(n, nq)
                        wn = np.where(dn > 0, dn, F(0))
                        for _ in range(normal_power):
                            wn = wn * wn
                        dist = F(s * max(abs(dx), abs(dy)))
                        rz = (Zq - Z) / ((sigma_depth * Z) * dist)
                        wz = F(1) / (F(1) + rz * rz)
                        dc = Iq - I
                        c2 = _dot(dc, dc)
                        wc = F(1) / (F(1) + c2 / sc2)
                        w = ((H5[dy + 2] * H5[dx + 2]) * wn) * wz
                        w = w * wc
                        if use_albedo:
                            da = _shift(A, s * dy, s * dx, F(0)) - A
                            w = w * (F(1) / (F(1) + _dot(da, da) / (sigma_albedo * sigma_albedo)))
                    assert w.dtype == F
                    acc = np.where(ok[..., None], acc + w[..., None] * Iq, acc)
                    wsum = np.where(ok, wsum + w, wsum)
            I = np.where(hit[..., None], acc / wsum[..., None], I)  # miss pixels pass through
            assert I.dtype == F
    out = color.copy()
    out[..., :3] = I
    return out.reshape(-1, 4)


def pack_rgb8(rgba):
    """RGBF32_to_RGB8 (template/precomp.h:310-315, scalar path) of a float32 [n, >= 3] image -> uint32 0x00RRGGBB."""
    x = np.asarray(rgba, F)[:, :3]
    mm = np.minimum(F(1), x)
    with np.errstate(all="ignore"):
        c = np.where(mm > 0, (F(255) * mm).astype(np.uint32), np.uint32(0)).astype(np.uint32)
    return (c[:, 0] << np.uint32(16)) + (c[:, 1] << np.uint32(8)) + c[:, 2]


def rmse(a, b):
    d = np.asarray(a, np.float64)[:, :3] - np.asarray(b, np.float64)[:, :3]
    return float(np.sqrt(np.mean(d * d)))


# ---- the two small scenes the denoiser tests share (oracle renders, made once per process)
CASES = {"multi_96x72": (True, 96, 72), "small_70x45": (False, 70, 45)}
_cache = {}


def scene_of(name):
    from prt import scenes
    multi, W, H = CASES[name]
    sd = scenes.config_small(40, 30)
    return (scenes.multi_instance(sd) if multi else sd), W, H


def oracle_guides(osc, W, H, flags):
    """(albedo[n,4], normal_depth[n,4], mode1, mode3) from the oracle's debug renders: base colour, the shading normal
    restored from the SHADINGNORMAL view (2 * view - 1: good to an ulp or so, enough to guide) and the primary t."""
    m1, tp, _ = osc.render_frames(W, H, spp=1, bounces=1, flags=flags, mode=1)
    m3, _, _ = osc.render_frames(W, H, spp=1, bounces=1, flags=flags, mode=3)
    hit = tp[0] < FAR
    alb = np.zeros((W * H, 4), F)
    alb[hit, :3] = m1[0][hit, :3]
    alb[hit, 3] = 1
    nd = np.zeros((W * H, 4), F)
    nd[hit, :3] = m3[0][hit, :3] * F(2) - F(1)
    nd[:, 3] = np.where(hit, tp[0], FAR)
    return alb, nd, m1[0], m3[0]


def case(name):
    """dict(sd, W, H, osc, noisy, converged, albedo, nd): the oracle's 2-spp frame, its 1024-spp frame
    (frame_index 1000) and the guides, default flags, depth 4."""
    if name not in _cache:
        import oracle
        sd, W, H = scene_of(name)
        osc = oracle.OracleScene(sd, W, H)
        noisy = osc.render(W, H, spp=2, bounces=4)[0]
        conv = osc.render(W, H, spp=1024, bounces=4, frame_index=1000)[0]
        alb, nd, _, _ = oracle_guides(osc, W, H, oracle.NORMALMAP)
        _cache[name] = dict(sd=sd, W=W, H=H, osc=osc, noisy=noisy, converged=conv, albedo=alb, nd=nd)
    return _cache[name]
