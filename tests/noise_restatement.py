"""numpy float32 restatement of the radiance second moments and the noise estimate as include/rayfinder_amd.h defines them ("Radiance second moments and the
noise estimate"): one IEEE f32 operation at a time in the order written there, so that the GPU's outputs can be compared bit for bit."""
import numpy as np

F = np.float32
TILE = 32
EPS = F(2.0 ** -8)
FLT_MAX = np.finfo(np.float32).max


def moment_sums(samples, start=None):
    """Q = sum over the samples, IN THE ORDER GIVEN, of {r.x r.x, r.y r.y, r.z r.z, 0}: each square one f32 multiply, added in f32 from +0 (or from `start`).
    samples: iterable of (H, W, >= 3) f32 per-sample radiance images.  -> (H, W, 4) f32."""
    q = None if start is None else np.array(start, np.float32)
    for r in samples:
        r = np.asarray(r, np.float32)[..., :3]
        if q is None:
            q = np.zeros(r.shape[:2] + (4,), np.float32)
        q[..., :3] = q[..., :3] + r * r
    return q


def pixel_variance(S, Q, N):
    """Per pixel and channel: mu = S / Nf, v = (Q - S mu) / (Nf - 1) clamped at 0 (NaN -> 0).  -> (mu, v), (H, W, 3) f32 each"""
    S = np.asarray(S, np.float32)[..., :3]
    Q = np.asarray(Q, np.float32)[..., :3]
    nf = F(N)
    nf1 = nf - F(1)
    with np.errstate(all="ignore"):
        mu = S / nf
        v = (Q - S * mu) / nf1
        v = np.where(v > 0, v, F(0)).astype(np.float32)
    return mu, v


def pixel_errors(S, Q, N):
    """-> (e (H, W) f32 with the non-finite entries set to 0, mask of the non-finite pixels)"""
    mu, v = pixel_variance(S, Q, N)
    nf = F(N)
    with np.errstate(all="ignore"):
        s2 = ((v[..., 0] + v[..., 1]) + v[..., 2]) / nf
        lum = (mu[..., 0] + mu[..., 1]) + mu[..., 2]
        e = np.sqrt(s2) / (lum + EPS)
        bad = ~(e <= FLT_MAX)
    e = np.where(bad, F(0), e).astype(np.float32)
    return e, bad


def tile_tree(a):
    """The halving tree over 1024 f32 entries: for h = 512 .. 1, a[i] = a[i] + a[i + h] for i < h.  -> a[0]"""
    a = np.array(a, np.float32).reshape(1024)
    h = 512
    with np.errstate(all="ignore"):
        while h >= 1:
            a[:h] = a[:h] + a[h:2 * h]
            h //= 2
    return a[0]


def estimate(S, Q, N):
    """-> dict(error_map, tile_sum, tile_max, tile_pixels, tile_nonfinite, mean_error (python float = f64), max_error (f32), worst_tile, samples, pixels,
    nonfinite_pixels)"""
    e, bad = pixel_errors(S, Q, N)
    H, W = e.shape
    tx_n, ty_n = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles = tx_n * ty_n
    tile_sum = np.zeros(tiles, np.float32)
    tile_max = np.zeros(tiles, np.float32)
    tile_pixels = np.zeros(tiles, np.uint32)
    tile_bad = np.zeros(tiles, np.uint32)
    for t in range(tiles):
        y0, x0 = (t // tx_n) * TILE, (t % tx_n) * TILE
        part = e[y0:y0 + TILE, x0:x0 + TILE]                       # the in-frame entries
        a = np.zeros((TILE, TILE), np.float32)                      # a[ty * 32 + tx]; 0 outside the frame
        a[:part.shape[0], :part.shape[1]] = part
        tile_sum[t] = tile_tree(a)
        tile_max[t] = part.max() + F(0)                             # (-0 -> +0)
        tile_pixels[t] = part.size
        tile_bad[t] = int(bad[y0:y0 + TILE, x0:x0 + TILE].sum())
    total = 0.0
    for t in range(tiles):
        total += float(tile_sum[t])                                 # f64, ascending t
    pixels = int(tile_pixels.sum())
    return dict(error_map=e, tile_sum=tile_sum, tile_max=tile_max, tile_pixels=tile_pixels, tile_nonfinite=tile_bad, mean_error=total / float(pixels),
                max_error=tile_max.max(), worst_tile=int(np.argmax(tile_max)), samples=int(N), pixels=pixels, nonfinite_pixels=int(tile_bad.sum()))


def oracle_samples(orc, scene, rp, frames, x0=0, y0=0, x1=None, y1=None):
    """Per-sample radiance of the frames, in order: orc.render(scene, rp, k, 1) into a zero image adds sample k alone (0 + r = r).  Yields (y1-y0, x1-x0, 4) f32."""
    x1 = rp.width if x1 is None else x1
    y1 = rp.height if y1 is None else y1
    image = np.zeros((rp.height, rp.width, 4), np.float32)
    for k in frames:
        image[y0:y1, x0:x1] = 0
        orc.render(scene, rp, k, 1, x0, y0, x1, y1, image=image)
        yield image[y0:y1, x0:x1].copy()


def same_estimate(got, want):
    """Every output of an estimate, bit for bit (floats compared as bit patterns).  -> list of the names that differ"""
    b = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    diff = [k for k in ("error_map", "tile_sum", "tile_max") if not np.array_equal(b(got[k]), b(want[k]))]
    if np.float64(got["mean_error"]).view(np.uint64) != np.float64(want["mean_error"]).view(np.uint64):
        diff.append("mean_error")
    if b(np.float32(got["max_error"])) != b(np.float32(want["max_error"])):
        diff.append("max_error")
    diff += [k for k in ("worst_tile", "samples", "pixels", "nonfinite_pixels") if int(got[k]) != int(want[k])]
    return diff
