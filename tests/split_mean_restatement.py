"""NumPy restatement of rf_comm_read_split (include/rayfinder_amd.h, "DIRECT SUMS ACROSS RANKS"): the direct and the indirect light of a frame as means, from its
radiance sums S and its direct sums D.  f32 throughout, one IEEE operation at a time: direct = D.rgb / float(n); indirect = (S.rgb - D.rgb) / float(n), the
subtraction first; alpha = 1.  n is one count for the frame, or one per 32 x 32 tile (tile_y * ceil(W / 32) + tile_x); a pixel whose count is 0 reads {0, 0, 0, 1}
in both images.  No GPU."""
import numpy as np

TILE = 32


def pixel_counts(counts, width, height):
    """One count per pixel, (H, W) u32, from one count for the frame or one per tile"""
    counts = np.asarray(counts, np.uint32)
    if counts.ndim == 0:
        return np.full((height, width), counts, np.uint32)
    tiles_x, tiles_y = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    grid = counts.reshape(tiles_y, tiles_x)
    return np.ascontiguousarray(np.repeat(np.repeat(grid, TILE, 0), TILE, 1)[:height, :width])


def read_split(S, D, counts):
    """S, D: (H, W, 4) f32 sums; counts: an int, or the per-tile counts.  -> (direct, indirect), (H, W, 4) f32 each"""
    S, D = np.asarray(S, np.float32), np.asarray(D, np.float32)
    h, w = S.shape[:2]
    assert S.shape == D.shape == (h, w, 4)
    n = pixel_counts(counts, w, h)
    nf = n.astype(np.float32)[..., None]
    direct, indirect = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    with np.errstate(all="ignore"):
        d = (D[..., :3] / nf).astype(np.float32)
        i = ((S[..., :3] - D[..., :3]).astype(np.float32) / nf).astype(np.float32)
    some = (n > 0)[..., None]
    direct[..., :3] = np.where(some, d, np.float32(0.0))
    indirect[..., :3] = np.where(some, i, np.float32(0.0))
    direct[..., 3] = indirect[..., 3] = 1.0
    return direct, indirect
