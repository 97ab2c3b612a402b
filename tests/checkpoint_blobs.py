"""Checkpoint blobs crafted in numpy from the byte layout INTEGRATION.md 3 documents (no library call): for the parser's tests."""
import numpy as np

HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("header_bytes", "<u4"), ("total_bytes", "<u8"),
                   ("width", "<u4"), ("height", "<u4"), ("num_tiles", "<u4"), ("frame_count", "<u4"), ("accumulated", "<u4"),
                   ("frame_leading_samples", "<u4"), ("frame_min_tile_samples", "<u4"),
                   ("aov_flags", "<u4"), ("moments", "<u4"), ("direct_word", "<u4"), ("buckets_word", "<u4"),
                   ("family", "<u4", (5, 2)), ("camera", "<u4", 19), ("sky", "<u4", 6), ("num_bounces", "<u4"), ("pad0", "<u4"),
                   ("scene_counts", "<u8", 4), ("root_bounds", "<u4", 6), ("reserved", "<u4", 4)])
assert HEADER.itemsize == 288
TILE_BYTES = 1024 * 16


def stored_planes(aov_flags, moments, direct_word, buckets_word, family):
    """Digest plane ids of the stored planes, in blob order; family: (5, 2) {samples, restarted}."""
    ids = []
    if not family[0][1]:
        ids.append(0)
    if aov_flags & 1 and not family[1][1]:
        ids += [1, 2]
    if moments and not family[2][1]:
        ids.append(3)
    if direct_word & 1 and not family[3][1]:
        ids.append(5)
    if buckets_word & 0xFF and not family[4][1]:
        ids += [16 + b for b in range(buckets_word & 0xFF)]
    return ids


def make_blob(width=70, height=45, tiles=(0, 1, 2, 3, 4, 5), accumulated=4, frame_count=7, aov_flags=1, moments=1, direct_word=0, buckets_word=3, tile_samples=None, seed=1):
    """A well-formed blob: every family that is on holds `accumulated` samples; the planes and tile digests are seeded noise (the parser does not look at them)."""
    rng = np.random.default_rng(seed)
    n = len(tiles)
    h = np.zeros((), HEADER)
    h["magic"], h["version"], h["header_bytes"] = b"RFCKPT1", 1, 288
    h["width"], h["height"], h["num_tiles"], h["frame_count"], h["accumulated"] = width, height, n, frame_count, accumulated
    h["aov_flags"], h["moments"], h["direct_word"], h["buckets_word"] = aov_flags, moments, direct_word, buckets_word
    on = [True, bool(aov_flags & 1), bool(moments), bool(direct_word & 1), bool(buckets_word & 0xFF)]
    family = [[accumulated, 0] if (o and accumulated) else [0, 1] for o in on]
    h["family"] = family
    h["camera"] = rng.integers(0, 2**32, 19, dtype=np.uint64)
    h["sky"] = rng.integers(0, 2**32, 6, dtype=np.uint64)
    h["num_bounces"] = 3
    h["scene_counts"] = [11, 22, 1, 64]
    planes = stored_planes(aov_flags, moments, direct_word, buckets_word, family)
    body = [np.asarray(tiles, "<u4").tobytes(), np.asarray(tile_samples if tile_samples is not None else [accumulated] * n, "<u4").tobytes(),
            rng.integers(0, 2**63, len(planes) * n, dtype=np.uint64).astype("<u8").tobytes(),
            rng.standard_normal(len(planes) * n * 1024 * 4).astype("<f4").tobytes()]
    body = b"".join(body)
    h["total_bytes"] = 288 + len(body)
    return h.tobytes() + body


def patched(blob, field, value):
    """The blob with one header field overwritten (total_bytes is NOT adjusted)."""
    h = np.frombuffer(blob[:288], HEADER).copy()
    h[field] = value
    return h.tobytes() + blob[288:]


def field_boundaries():
    return sorted({off for _, off in (v[:2] for v in HEADER.fields.values())} | {288})
