"""numpy float32 restatement of the edge-aware a-trous denoiser (include/rayfinder_amd.h, "Edge-aware a-trous denoiser"): the GPU tests compare
rf_denoise_images / rf_renderer_denoise against it bit for bit.  Vectorised over pixels, one elementwise step per tap in tap order; every
constant is an np.float32 and every operation is one IEEE f32 operation, in the order the header writes it."""
import numpy as np

F = np.float32
EPS_A = F(2.0 ** -8)                 # εa: albedo floor of the demodulation
EPS_L = F(2.0 ** -8)                 # εℓ: floor of the colour term's scale
K = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
DEFAULTS = dict(iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1)


def _tukey(x):
    """T(x) = x < 1 ? (1 - x)(1 - x) : 0 (NaN: 0)."""
    one_m = F(1) - x
    return np.where(x < F(1), one_m * one_m, F(0)).astype(np.float32)


def prep(color_sum, albedo_coverage, normal_depth, samples):
    """-> c (H,W,3), e (H,W,3), lum (H,W), n (H,W,3), z (H,W), a_eps (H,W,3) = a + εa, bg (H,W) bool."""
    S = np.asarray(color_sum, np.float32)
    AC = np.asarray(albedo_coverage, np.float32)
    ND = np.asarray(normal_depth, np.float32)
    nf = F(samples)
    c = S[..., :3] / nf
    with np.errstate(all="ignore"):
        a = AC[..., :3] / nf
        m = ND[..., :3] / nf
        d = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
        ok = (d != F(0)) & np.isfinite(d)
        inv = F(1) / np.sqrt(np.where(ok, d, F(1)))
        n = np.where(ok[..., None], m * inv[..., None], F(0)).astype(np.float32)
        z = ND[..., 3] / AC[..., 3]
        a_eps = a + EPS_A
        e = c / a_eps
    bg = (AC[..., 3] == F(0)) | ~(z > F(0))
    e = np.where(bg[..., None], c, e).astype(np.float32)
    lum = (e[..., 0] + e[..., 1]) + e[..., 2]
    return c, e, lum, n, z, a_eps, bg


def _shift(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx] where that lies in the frame, `fill` elsewhere."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = a[ys, xs]
    return out


def iterate(e, lum, n, z, bg, i, sigma_color, sigma_normal, sigma_depth):
    """One a-trous pass, step 2^i: -> e' (H,W,3), ℓ' (H,W).  Background pixels keep e."""
    s = 1 << i
    sc2 = (F(sigma_color) * F(sigma_color)) * F(2.0 ** -i)
    sn = F(sigma_normal)
    szs = F(sigma_depth) * F(s)
    with np.errstate(all="ignore"):
        den_c = sc2 * (lum * lum + EPS_L)
        den_z = szs * z
        sum_w = np.zeros(lum.shape, np.float32)
        sum_e = np.zeros(e.shape, np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                h = K[dx + 2] * K[dy + 2]
                if dx == 0 and dy == 0:
                    w = np.full(lum.shape, h, np.float32)
                    eq = e
                    valid = np.ones(lum.shape, bool)
                else:
                    eq = _shift(e, s * dx, s * dy, F(0))
                    nq = _shift(n, s * dx, s * dy, F(0))
                    zq = _shift(z, s * dx, s * dy, F(0))
                    valid = ~_shift(bg, s * dx, s * dy, True)
                    d = eq - e
                    dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    xc = dc / den_c
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    xn = (F(1) - dot) / sn
                    xz = np.abs(zq - z) / den_z
                    w = ((h * _tukey(xc)) * _tukey(xn)) * _tukey(xz)
                sum_w = np.where(valid, sum_w + w, sum_w).astype(np.float32)
                sum_e = np.where(valid[..., None], sum_e + w[..., None] * eq, sum_e).astype(np.float32)
        out = sum_e / sum_w[..., None]
    out = np.where(bg[..., None], e, out).astype(np.float32)
    return out, (out[..., 0] + out[..., 1]) + out[..., 2]


def denoise(color_sum, albedo_coverage, normal_depth, samples, iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1):
    """-> (H,W,3) f32 denoised mean (the .rgb of what the library returns; its .w is 1)."""
    c, e, lum, n, z, a_eps, bg = prep(color_sum, albedo_coverage, normal_depth, samples)
    if iterations == 0:
        return c
    for i in range(iterations):
        e, lum = iterate(e, lum, n, z, bg, i, sigma_color, sigma_normal, sigma_depth)
    with np.errstate(all="ignore"):
        out = e * a_eps
    return np.where(bg[..., None], c, out).astype(np.float32)


def radius(iterations):
    """How far (in pixels) the output of a pixel reaches: 2 * (2^L - 1)."""
    return 2 * ((1 << iterations) - 1)


def denoise_window(color_sum, albedo_coverage, normal_depth, samples, x0, y0, x1, y1, **params):
    """The denoised mean of the window [y0, y1) x [x0, x1) of a larger frame, computed on that window plus a margin of radius(L) (clipped to the
    frame): bit-identical to the same window of denoise() on the whole frame."""
    H, W = color_sum.shape[:2]
    r = radius(params.get("iterations", DEFAULTS["iterations"]))
    X0, Y0, X1, Y1 = max(0, x0 - r), max(0, y0 - r), min(W, x1 + r), min(H, y1 + r)
    out = denoise(color_sum[Y0:Y1, X0:X1], albedo_coverage[Y0:Y1, X0:X1], normal_depth[Y0:Y1, X0:X1], samples, **params)
    return out[y0 - Y0:y1 - Y0, x0 - X0:x1 - X0]
