"""numpy float32 restatement of the split-component denoiser with one sample count per 32x32 tile (include/rayfinder_amd.h, "Split-component denoiser": ONE COUNT
PER TILE): rf_denoise_split_tiles and rf_renderer_denoise_split in the non-uniform state are compared against it bit for bit.  The definition differs from the
one-count split filter in prep alone -- Nf of pixel p is float(tile_samples[tile of p]) for c, a, m, cD and cI -- so prep is split_restatement.split_prep handed the
per-pixel Nf of denoise_tiles_restatement.pixel_counts (an (H, W, 1) f32 array broadcasts through every division by it, and F(array) is the array), and the chains
and the finish are split_restatement's own, imported and untouched."""
import numpy as np

from denoise_tiles_restatement import pixel_counts
from split_restatement import denoise_split, split_prep


def _nf(color_sum, tile_samples):
    H, W = np.asarray(color_sum).shape[:2]
    return pixel_counts(tile_samples, H, W)[..., None]


def split_prep_tiles(color_sum, direct_sum, albedo_coverage, normal_depth, tile_samples):
    """split_prep with the per-pixel Nf -> c, eD, eI, n, z, a_eps, bg"""
    return split_prep(color_sum, direct_sum, albedo_coverage, normal_depth, _nf(color_sum, tile_samples))


def denoise_split_tiles(color_sum, direct_sum, albedo_coverage, normal_depth, tile_samples, direct=None, indirect=None):
    """-> (H,W,3) f32 denoised mean.  direct / indirect: dicts of iterations, sigma_color, sigma_normal, sigma_depth (missing keys: that component's defaults)."""
    return denoise_split(color_sum, direct_sum, albedo_coverage, normal_depth, _nf(color_sum, tile_samples), direct, indirect)
