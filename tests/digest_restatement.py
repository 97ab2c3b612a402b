"""The state digest of include/rayfinder_amd.h ("State digest and checkpoints"), restated: once in plain Python integers (term, plane_digest_ints), once over numpy
uint64 arrays for whole frames (tile_digests, plane_digest).  All arithmetic is mod 2^64.  Inputs are what the handle's reads return: row-major (H, W, 4) float32 sums,
the per-tile sample counts of the frame's 32 x 32 grid and the handle's tile ids (shard_tiles())."""
import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
PLANE_S, PLANE_AC, PLANE_ND, PLANE_Q, PLANE_D, PLANE_BUCKET0, COUNTS_ID = 0, 1, 2, 3, 5, 16, 0xC0
TILE = 32


def mix64(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def term(plane, i, w):
    """One in-frame pixel: plane id, frame index i = y * width + x, w = the bit patterns of the texel's four floats."""
    k = mix64((plane << 32) | i)
    return (mix64(k ^ ((w[1] << 32) | w[0])) + mix64(((k + GOLDEN) & MASK) ^ ((w[3] << 32) | w[2]))) & MASK


def tiles_x(width):
    return (width + TILE - 1) // TILE


def tile_of(x, y, width):
    return (y // TILE) * tiles_x(width) + x // TILE


def plane_digest_ints(plane, image, tiles=None):
    """The plane digest over `tiles` (None: every tile) in Python integers, pixel by pixel: for small planes."""
    bits = np.ascontiguousarray(image, np.float32).view(np.uint32)
    h, w = bits.shape[:2]
    total = 0
    for y in range(h):
        for x in range(w):
            if tiles is not None and tile_of(x, y, w) not in tiles:
                continue
            total = (total + term(plane, y * w + x, [int(v) for v in bits[y, x]])) & MASK
    return total


def _mix64_np(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def tile_digests(plane, image):
    """-> {tile id: digest} for every tile of the frame (numpy uint64: multiplication and addition wrap mod 2^64)."""
    bits = np.ascontiguousarray(image, np.float32).view(np.uint32).astype(np.uint64)
    h, w = bits.shape[:2]
    with np.errstate(over="ignore"):
        ys, xs = np.mgrid[0:h, 0:w]
        i = (ys * w + xs).astype(np.uint64)
        k = _mix64_np((np.uint64(plane) << np.uint64(32)) | i)
        terms = _mix64_np(k ^ ((bits[..., 1] << np.uint64(32)) | bits[..., 0])) + _mix64_np((k + np.uint64(GOLDEN)) ^ ((bits[..., 3] << np.uint64(32)) | bits[..., 2]))
        tile = (ys // TILE) * tiles_x(w) + xs // TILE
        return {int(t): int(terms[tile == t].sum(dtype=np.uint64)) for t in np.unique(tile)}


def plane_digest(plane, image, tiles=None):
    d = tile_digests(plane, image)
    return sum(v for t, v in d.items() if tiles is None or t in set(int(x) for x in tiles)) & MASK


def counts_digest(tile_samples, tiles):
    """tile_samples: one count per tile of the frame's grid; tiles: the handle's own tile ids."""
    return sum(mix64(mix64((COUNTS_ID << 32) | int(t)) ^ int(tile_samples[int(t)])) for t in tiles) & MASK


def handle_digest(reads, tile_samples, tiles):
    """The digest dict of a handle from its reads: reads = {"accumulation": img, "albedo_coverage": img or None, "normal_depth": ..., "moments": ..., "direct": ...,
    "buckets": (K, H, W, 4) or None}; a family that is off (None) digests 0."""
    tiles = [int(t) for t in tiles]
    out = {}
    for name, plane in (("accumulation", PLANE_S), ("albedo_coverage", PLANE_AC), ("normal_depth", PLANE_ND), ("moments", PLANE_Q), ("direct", PLANE_D)):
        out[name] = 0 if reads.get(name) is None or not tiles else plane_digest(plane, reads[name], tiles)
    buckets = reads.get("buckets")
    out["bucket"] = [0] * 15
    if buckets is not None and tiles:
        for b in range(len(buckets)):
            out["bucket"][b] = plane_digest(PLANE_BUCKET0 + b, buckets[b], tiles)
    out["counts"] = counts_digest(tile_samples, tiles)
    return out
