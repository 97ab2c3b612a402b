"""numpy float32 restatement of the edge-aware a-trous denoiser with one sample count per 32x32 tile (include/rayfinder_amd.h, "Edge-aware a-trous denoiser": the
per-tile paragraph): rf_denoise_tiles and rf_renderer_denoise in the non-uniform state are compared against it bit for bit.  The definition differs from the
one-count filter in prep alone -- Nf of pixel p is float(tile_samples[tile of p]) for c, a and m -- so prep is restated here with a per-pixel Nf and the passes are
denoise_restatement.iterate's, untouched.  With equal counts the result is denoise_restatement.denoise's, bit for bit."""
import numpy as np

from denoise_restatement import EPS_A, F, iterate

TILE = 32


def pixel_counts(tile_samples, height, width):
    """(H, W) f32: Nf of every pixel = float(the count of its tile), tile t = tile_y * ceil(W / 32) + tile_x"""
    tiles_x, tiles_y = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    counts = np.asarray(tile_samples).reshape(-1)
    assert counts.size == tiles_x * tiles_y and (counts > 0).all(), counts
    grid = counts.reshape(tiles_y, tiles_x).astype(np.float32)               # float(uint32): exact below 2^24, rounded to nearest above, as the device's conversion
    return np.repeat(np.repeat(grid, TILE, 0), TILE, 1)[:height, :width]


def prep_tiles(color_sum, albedo_coverage, normal_depth, tile_samples):
    """denoise_restatement.prep with the per-pixel Nf -> c (H,W,3), e (H,W,3), lum (H,W), n (H,W,3), z (H,W), a_eps (H,W,3) = a + εa, bg (H,W) bool."""
    S = np.asarray(color_sum, np.float32)
    AC = np.asarray(albedo_coverage, np.float32)
    ND = np.asarray(normal_depth, np.float32)
    nf = pixel_counts(tile_samples, S.shape[0], S.shape[1])[..., None]
    c = S[..., :3] / nf
    with np.errstate(all="ignore"):
        a = AC[..., :3] / nf
        m = ND[..., :3] / nf
        d = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
        ok = (d != F(0)) & np.isfinite(d)
        inv = F(1) / np.sqrt(np.where(ok, d, F(1)))
        n = np.where(ok[..., None], m * inv[..., None], F(0)).astype(np.float32)
        z = ND[..., 3] / AC[..., 3]                                          # (no N in it)
        a_eps = a + EPS_A
        e = c / a_eps
    bg = (AC[..., 3] == F(0)) | ~(z > F(0))
    e = np.where(bg[..., None], c, e).astype(np.float32)
    lum = (e[..., 0] + e[..., 1]) + e[..., 2]
    return c, e, lum, n, z, a_eps, bg


def denoise_tiles(color_sum, albedo_coverage, normal_depth, tile_samples, iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1):
    """-> (H,W,3) f32 denoised mean (the .rgb of what the library returns; its .w is 1)."""
    c, e, lum, n, z, a_eps, bg = prep_tiles(color_sum, albedo_coverage, normal_depth, tile_samples)
    if iterations == 0:
        return c
    for i in range(iterations):
        e, lum = iterate(e, lum, n, z, bg, i, sigma_color, sigma_normal, sigma_depth)
    with np.errstate(all="ignore"):
        out = e * a_eps
    return np.where(bg[..., None], c, out).astype(np.float32)
