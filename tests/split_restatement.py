"""numpy float32 restatement of the split-component denoiser (include/rayfinder_amd.h, "Split-component denoiser"): the direct light D and the indirect light
S - D, demodulated by the same a + εa, each filtered by a chain of the one filter's passes (tests/denoise_restatement.py) with its own parameters, added and
remodulated.  The GPU tests compare rf_denoise_split_images / rf_renderer_denoise_split against it bit for bit."""
import numpy as np

from denoise_restatement import DEFAULTS, F, iterate, prep, radius

KEYS = ("iterations", "sigma_color", "sigma_normal", "sigma_depth")
# the two components' defaults (include/rayfinder_amd.h: rf_denoise_split_default_parameters); a parameter a caller leaves out is its own component's default
DIRECT_DEFAULTS = dict(DEFAULTS, iterations=1, sigma_color=0.25)
INDIRECT_DEFAULTS = dict(DEFAULTS, iterations=2, sigma_color=256.0)


def _params(p, base):
    p = dict(base, **(p or {}))
    assert set(p) == set(KEYS), sorted(p)
    return p


def split_prep(color_sum, direct_sum, albedo_coverage, normal_depth, samples):
    """-> c (H,W,3), eD (H,W,3), eI (H,W,3), n, z, a_eps, bg.  Background: eD = c, eI = 0."""
    S = np.asarray(color_sum, np.float32)
    D = np.asarray(direct_sum, np.float32)
    c, _, _, n, z, a_eps, bg = prep(S, albedo_coverage, normal_depth, samples)
    nf = F(samples)
    with np.errstate(all="ignore"):
        cD = D[..., :3] / nf
        cI = (S[..., :3] - D[..., :3]) / nf
        eD = cD / a_eps
        eI = cI / a_eps
    eD = np.where(bg[..., None], c, eD).astype(np.float32)
    eI = np.where(bg[..., None], F(0), eI).astype(np.float32)
    return c, eD, eI, n, z, a_eps, bg


def _chain(e, n, z, bg, p):
    lum = (e[..., 0] + e[..., 1]) + e[..., 2]
    for i in range(p["iterations"]):
        e, lum = iterate(e, lum, n, z, bg, i, p["sigma_color"], p["sigma_normal"], p["sigma_depth"])
    return e


def denoise_split(color_sum, direct_sum, albedo_coverage, normal_depth, samples, direct=None, indirect=None):
    """-> (H,W,3) f32 denoised mean.  direct / indirect: dicts of iterations, sigma_color, sigma_normal, sigma_depth (missing keys: that component's defaults)."""
    pd, pi = _params(direct, DIRECT_DEFAULTS), _params(indirect, INDIRECT_DEFAULTS)
    c, eD, eI, n, z, a_eps, bg = split_prep(color_sum, direct_sum, albedo_coverage, normal_depth, samples)
    if pd["iterations"] == 0 and pi["iterations"] == 0:
        return c
    eD = _chain(eD, n, z, bg, pd)
    eI = _chain(eI, n, z, bg, pi)
    with np.errstate(all="ignore"):
        out = (eD + eI) * a_eps
    return np.where(bg[..., None], c, out).astype(np.float32)


def denoise_split_window(color_sum, direct_sum, albedo_coverage, normal_depth, samples, x0, y0, x1, y1, direct=None, indirect=None):
    """The window [y0, y1) x [x0, x1) of denoise_split on a larger frame, computed on the window plus a margin of the longer chain's radius (clipped to the frame):
    bit-identical to the same window of the whole frame's result."""
    H, W = color_sum.shape[:2]
    r = radius(max(_params(direct, DIRECT_DEFAULTS)["iterations"], _params(indirect, INDIRECT_DEFAULTS)["iterations"]))
    X0, Y0, X1, Y1 = max(0, x0 - r), max(0, y0 - r), min(W, x1 + r), min(H, y1 + r)
    out = denoise_split(color_sum[Y0:Y1, X0:X1], direct_sum[Y0:Y1, X0:X1], albedo_coverage[Y0:Y1, X0:X1], normal_depth[Y0:Y1, X0:X1], samples, direct, indirect)
    return out[y0 - Y0:y1 - Y0, x0 - X0:x1 - X0]
