"""The feature export (include/rayfinder_amd.h, "Feature export") restated in numpy float32, one IEEE operation at a time in the header's order.  Where the formulas
coincide with the denoiser's prep and the noise estimate, their restatements are reused (denoise_restatement.prep, noise_restatement.pixel_variance / pixel_errors):
the normal, the depth and the background test are prep's, mu, v and e the estimate's."""
import numpy as np

import denoise_restatement as dr
import noise_restatement as nr

F = np.float32
TILE = 32
GROUPS = (("color", 0x001, 3), ("albedo", 0x002, 3), ("normal", 0x004, 3), ("depth", 0x008, 1), ("coverage", 0x010, 1), ("direct", 0x020, 3), ("indirect", 0x040, 3),
          ("variance", 0x080, 3), ("error", 0x100, 1), ("samples", 0x200, 1))
ALL = 0x3FF


def mask_of(names):
    bit = {n: b for n, b, _ in GROUPS}
    m = 0
    for n in names:
        m |= bit[n]
    return m


def channel_count(mask):
    return sum(c for _, b, c in GROUPS if mask & b)


def pixel_counts(width, height, samples, tile_samples=None):
    """-> (H, W) uint32: every pixel's sample count (its tile's, or `samples`)"""
    if tile_samples is None:
        return np.full((height, width), samples, np.uint32)
    tx, ty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    t = np.asarray(tile_samples, np.uint32).reshape(ty, tx)
    return np.repeat(np.repeat(t, TILE, 0), TILE, 1)[:height, :width]


def _groups_for_count(mask, k, S, Q, AC, ND, D):
    """The selected groups' (H, W, c) f32 values with ONE count k > 0 for every pixel"""
    nf = F(k)
    out = {}
    with np.errstate(all="ignore"):
        if mask & 0x001:
            out["color"] = S[..., :3] / nf
        if mask & 0x002:
            out["albedo"] = AC[..., :3] / nf
        if mask & (0x004 | 0x008):
            _, _, _, n, z, _, bg = dr.prep(np.zeros_like(AC), AC, ND, k)
            out["normal"] = np.where(bg[..., None], F(0), n).astype(np.float32)
            out["depth"] = np.where(bg, F(0), z).astype(np.float32)[..., None]
        if mask & 0x010:
            out["coverage"] = (AC[..., 3] / nf)[..., None]
        if mask & 0x020:
            out["direct"] = D[..., :3] / nf
        if mask & 0x040:
            out["indirect"] = (S[..., :3] - D[..., :3]) / nf
        if mask & 0x080:
            _, v = nr.pixel_variance(S, Q, k)
            out["variance"] = v / nf
        if mask & 0x100:
            out["error"] = nr.pixel_errors(S, Q, k)[0][..., None]
        if mask & 0x200:
            out["samples"] = np.full(AC.shape[:2] + (1,), nf, np.float32)
    return out


def features(mask, width, height, S=None, Q=None, AC=None, ND=None, D=None, samples=0, tile_samples=None, layout="chw", dtype="f32"):
    """-> (C, H, W) or (H, W, C) float32 / float16.  The sums are (H, W, 4) f32 (None where no selected channel reads them)."""
    counts = pixel_counts(width, height, samples, tile_samples)
    C = channel_count(mask)
    hwc = np.zeros((height, width, C), np.float32)
    planes = [None if a is None else np.asarray(a, np.float32) for a in (S, Q, AC, ND, D)]
    blank = np.zeros((height, width, 4), np.float32)
    S_, Q_, AC_, ND_, D_ = (blank if a is None else a for a in planes)
    for k in np.unique(counts):
        if k == 0:
            continue  # +0 in every channel
        g = _groups_for_count(mask, int(k), S_, Q_, AC_, ND_, D_)
        one = np.concatenate([np.asarray(g[name], np.float32).reshape(height, width, c) for name, bit, c in GROUPS if mask & bit], -1)
        hwc = np.where((counts == k)[..., None], one, hwc).astype(np.float32)
    out = hwc if layout == "hwc" else np.ascontiguousarray(hwc.transpose(2, 0, 1))
    with np.errstate(all="ignore"):
        return out.astype(np.float16) if dtype == "f16" else out


def same(got, want):
    """Bit for bit, but for the payload of a NaN: the shapes and dtypes agree, NaNs sit at the same places and every other element has the same bits"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = np.uint16 if got.dtype == np.float16 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(np.ascontiguousarray(got).view(u)[~gn], np.ascontiguousarray(want).view(u)[~wn]))


def first_difference(got, want):
    u = np.uint16 if got.dtype == np.float16 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)))
    idx = np.argwhere(bad)
    return None if not len(idx) else (tuple(idx[0]), got[tuple(idx[0])], want[tuple(idx[0])], int(bad.sum()))
