"""numpy float32 restatement of the firefly-robust mean with one sample count per 32x32 tile (include/rayfinder_amd.h, "Bucket sums and the robust mean": the tiles
combine, and rf_renderer_denoise_robust in the non-uniform state): rf_renderer_robust_mean / rf_robust_mean_tiles / rf_renderer_denoise_robust on a frame of
rf_renderer_render_adaptive with RF_BUCKETS_TILE_COUNTS are compared against it bit for bit.  Nothing is restated twice: the combine is robust_restatement.robust_mean
once per distinct count, and the denoise is robust_restatement.denoise_robust with a per-pixel Nf."""
import numpy as np

from adaptive_restatement import tile_slices
from denoise_tiles_restatement import pixel_counts
from robust_restatement import denoise_robust, robust_mean


def robust_mean_tiles(buckets, counts, width, height):
    """-> (M (H, W, 3) f32, trim (H, W) u8): every tile's pixels from robust_mean(buckets, counts[t]), tile t = tile_y * ceil(W / 32) + tile_x; every count >= K."""
    B = np.asarray(buckets, np.float32)
    counts = np.asarray(counts).reshape(-1)
    assert B.shape[1:3] == (height, width) and counts.size == len(tile_slices(width, height))
    per_n = {int(n): robust_mean(B, int(n)) for n in np.unique(counts)}
    M = np.zeros((height, width, 3), np.float32)
    trim = np.zeros((height, width), np.uint8)
    for t, (rows, cols) in enumerate(tile_slices(width, height)):
        m, c = per_n[int(counts[t])]
        M[rows, cols] = m[rows, cols]
        trim[rows, cols] = c[rows, cols]
    return M, trim


def denoise_robust_tiles(mean, albedo_coverage, normal_depth, counts, **params):
    """robust_restatement.denoise_robust with Nf the per-pixel count image: c = M.rgb as it is, a = AC.rgb / Nf and m = ND.xyz / Nf with Nf = float(the count of the
    pixel's tile); the passes and the finish untouched.  -> (H, W, 3) f32."""
    h, w = np.asarray(mean).shape[:2]
    return denoise_robust(mean, albedo_coverage, normal_depth, pixel_counts(counts, h, w)[..., None], **params)
