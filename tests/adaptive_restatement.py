"""numpy float32 restatement of tile-adaptive sampling as include/rayfinder_amd.h defines it ("Tile-adaptive sampling"): the loop of rf_renderer_render_adaptive
played over per-sample radiance images (the oracle's, through noise_restatement.oracle_samples), with the sums and the estimate of noise_restatement.py.  Every
output is meant to be compared with the GPU's bit for bit."""
import numpy as np

from noise_restatement import F, TILE, estimate

U32_MAX = 0xFFFFFFFF


def tile_grid(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def tile_slices(width, height):
    """-> per tile t = ty * tiles_x + tx: (rows, columns) of its in-frame pixels"""
    tx_n, ty_n = tile_grid(width, height)
    return [(slice(ty * TILE, min((ty + 1) * TILE, height)), slice(tx * TILE, min((tx + 1) * TILE, width))) for ty in range(ty_n) for tx in range(tx_n)]


def prefix_sums(samples):
    """S_n and Q_n for n = 0 .. len(samples): the sums of the first n samples IN THE ORDER GIVEN, each addition (and each square) one f32 operation, from +0.
    samples: sequence of (H, W, >= 3) f32 per-sample radiance.  -> (S, Q): lists of (H, W, 4) f32, entry n = after n samples; channel 3 stays 0."""
    first = np.asarray(samples[0], np.float32)
    s = np.zeros(first.shape[:2] + (4,), np.float32)
    q = np.zeros_like(s)
    S, Q = [s.copy()], [q.copy()]
    for r in samples:
        r = np.asarray(r, np.float32)[..., :3]
        s[..., :3] = s[..., :3] + r
        q[..., :3] = q[..., :3] + r * r
        S.append(s.copy())
        Q.append(q.copy())
    return S, Q


def sums_for_counts(S, Q, counts, width, height):
    """The defining property: tile t holds the sums of its first counts[t] samples.  -> (S, Q) (H, W, 4) f32"""
    s, q = np.zeros_like(S[0]), np.zeros_like(Q[0])
    for t, (rows, cols) in enumerate(tile_slices(width, height)):
        s[rows, cols] = S[int(counts[t])][rows, cols]
        q[rows, cols] = Q[int(counts[t])][rows, cols]
    return s, q


def tile_errors(est):
    """tile_sum / float(tile_pixels): one f32 division per tile"""
    with np.errstate(all="ignore"):
        return (est["tile_sum"] / est["tile_pixels"].astype(np.float32)).astype(np.float32)


def estimate_over(est, tiles, samples):
    """The frame reduction of an estimate restricted to a list of tiles (ascending): what rf_adaptive_result.last reports for the tiles active in a pass"""
    tiles = sorted(int(t) for t in tiles)
    total = 0.0
    for t in tiles:
        total += float(est["tile_sum"][t])                                  # f64, ascending t
    pixels = int(sum(int(est["tile_pixels"][t]) for t in tiles))
    maxima = est["tile_max"][tiles]
    return dict(mean_error=total / float(pixels), max_error=maxima.max(), worst_tile=tiles[int(np.argmax(maxima))], samples=int(samples), pixels=pixels,
                nonfinite_pixels=int(sum(int(est["tile_nonfinite"][t]) for t in tiles)))


def estimate_tiles(s, q, counts, width, height):
    """The estimate with Nf = float(counts[t]) for the pixels of tile t; samples = the largest count.  -> noise_restatement.estimate's dict"""
    counts = np.asarray(counts).reshape(-1)
    per_n = {int(n): estimate(s, q, int(n)) for n in np.unique(counts)}
    out = None
    for t, (rows, cols) in enumerate(tile_slices(width, height)):
        src = per_n[int(counts[t])]
        if out is None:
            out = {k: np.array(src[k]) for k in ("error_map", "tile_sum", "tile_max", "tile_pixels", "tile_nonfinite")}
        out["error_map"][rows, cols] = src["error_map"][rows, cols]
        for k in ("tile_sum", "tile_max", "tile_pixels", "tile_nonfinite"):
            out[k][t] = src[k][t]
    out.update(estimate_over(out, range(counts.size), int(counts.max())))
    return out


def mean_image(s, counts, width, height):
    """{S.rgb / float(counts[t]), 1}: one f32 division per channel; rgb 0 in a tile without a sample"""
    mean = np.zeros_like(s)
    mean[..., 3] = 1
    for t, (rows, cols) in enumerate(tile_slices(width, height)):
        if counts[t]:
            mean[rows, cols, :3] = s[rows, cols, :3] / F(int(counts[t]))
    return mean


def play(S, Q, width, height, target, check_every, min_samples=0, max_samples=0, spp=None, counts=None):
    """The loop of rf_renderer_render_adaptive over prefix sums (prefix_sums: S[n], Q[n] after n samples; len(S) - 1 >= the cap).  counts: the tile counts before the
    call (None: a fresh accumulation).  -> dict(counts (tiles,) int, S, Q, mean, passes: [dict(L, active, errors)], last, estimate_passes, stopped_tiles, min_tile_samples,
    max_tile_samples, pixel_samples, leading)"""
    spp = len(S) - 1 if spp is None else spp
    cap = spp if max_samples == 0 else min(max_samples, spp)
    tx_n, ty_n = tile_grid(width, height)
    tiles = tx_n * ty_n
    counts = np.zeros(tiles, np.int64) if counts is None else np.array(counts, np.int64).reshape(-1)
    L = int(counts.max())
    active = [t for t in range(tiles) if counts[t] == L]
    target = F(target)
    passes, last = [], None
    while active and L < cap:
        L += min(check_every, cap - L)
        counts[active] = L
        if L < max(2, min_samples):
            continue
        est = estimate(S[L], Q[L], L)                                       # (the active tiles all hold their first L samples: the frame's estimate at L serves them)
        errors = tile_errors(est)
        passes.append(dict(L=L, active=list(active), errors=errors))
        last = estimate_over(est, active, L)
        with np.errstate(invalid="ignore"):
            active = [t for t in active if not (errors[t] <= target)]      # (a NaN never compares true: the tile goes on)
    s, q = sums_for_counts(S, Q, counts, width, height)
    pixels = [(rows.stop - rows.start) * (cols.stop - cols.start) for rows, cols in tile_slices(width, height)]
    return dict(counts=counts, S=s, Q=q, mean=mean_image(s, counts, width, height), passes=passes, last=last, estimate_passes=len(passes),
                stopped_tiles=int((counts != L).sum()), min_tile_samples=int(counts.min()), max_tile_samples=int(counts.max()),
                pixel_samples=int(sum(p * int(c) for p, c in zip(pixels, counts))), leading=L)
