"""numpy float32 restatement of the bucket sums and the firefly-robust mean as include/rayfinder_amd.h defines them ("Bucket sums and the robust mean"): one IEEE
f32 operation at a time in the order written there, so that the GPU's outputs can be compared bit for bit."""
import numpy as np

import denoise_restatement as dr

F = np.float32
FLT_MAX = np.finfo(np.float32).max
INF = F(np.inf)


def bucket_sums(samples, K, first_ordinal=0, start=None):
    """B[b] = sum over the samples, IN THE ORDER GIVEN, whose ordinal j (first_ordinal, first_ordinal + 1, ...) has j mod K == b, of {r.x, r.y, r.z, 0}, added in f32
    from +0 (or from `start`, a (K, H, W, 4) array).  samples: iterable of (H, W, >= 3) f32 per-sample radiance images.  -> (K, H, W, 4) f32."""
    B = None if start is None else np.array(start, np.float32)
    j = int(first_ordinal)
    for r in samples:
        r = np.asarray(r, np.float32)[..., :3]
        if B is None:
            B = np.zeros((K,) + r.shape[:2] + (4,), np.float32)
        B[j % K, ..., :3] = B[j % K, ..., :3] + r
        j += 1
    return B


def bucket_sizes(K, N):
    """n_b = N / K + (b < N mod K ? 1 : 0)"""
    return [N // K + (1 if b < N % K else 0) for b in range(K)]


def robust_mean(buckets, N):
    """-> (M (H, W, 3) f32, trim (H, W) u8) of (K, H, W, >= 3) bucket sums of N >= K samples."""
    B = np.asarray(buckets, np.float32)
    K = B.shape[0]
    assert K % 2 == 1 and 3 <= K <= 15 and N >= K
    half = (K - 1) // 2
    with np.errstate(all="ignore"):
        m = np.stack([B[b, ..., :3] / F(n) for b, n in enumerate(bucket_sizes(K, N))])             # (K, H, W, 3)
        lum = (m[..., 0] + m[..., 1]) + m[..., 2]
        key = np.where(lum <= FLT_MAX, lum, INF).astype(np.float32)                                  # (K, H, W); NaN -> +inf
        order = np.argsort(key, axis=0, kind="stable")                                               # ascending, ties by bucket index
        key = np.take_along_axis(key, order, 0)
        m = np.take_along_axis(m, order[..., None], 0)
        num = np.zeros(key.shape[1:], np.float32)
        tot = np.zeros(key.shape[1:], np.float32)
        for i in range(K):
            num = num + F(2 * i - (K - 1)) * key[i]
            tot = tot + key[i]
        den = F(K) * tot
        G = np.where(den > F(0), num / den, F(0)).astype(np.float32)
        t = G * (F(K) * F(0.5))
        # min(uint(floor(t)), half), the minimum taken before the conversion; NaN: every comparison false -> half
        floor_t = np.where((t >= F(0)) & (t < F(half)), np.floor(t), F(0)).astype(np.int64)
        c = np.where(t >= F(0), np.where(t >= F(half), half, floor_t), half).astype(np.int64)       # (H, W)
        s = np.zeros(m.shape[1:], np.float32)
        for i in range(K):
            kept = (i >= c) & (i + c <= K - 1)
            s = np.where(kept[..., None], s + m[i], s).astype(np.float32)
        M = s / (K - 2 * c).astype(np.float32)[..., None]
    return M.astype(np.float32), c.astype(np.uint8)


def denoise_robust(mean, albedo_coverage, normal_depth, samples, iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1):
    """The a-trous filter of denoise_restatement with prep's colour c = M.rgb (`mean`, (H, W, 3)) instead of S.rgb / Nf: prep is restated here with that one change,
    the passes and the finish are denoise_restatement's own.  -> (H, W, 3) f32."""
    c = np.asarray(mean, np.float32)[..., :3]
    if iterations == 0:
        return c
    AC = np.asarray(albedo_coverage, np.float32)
    ND = np.asarray(normal_depth, np.float32)
    nf = F(samples)
    with np.errstate(all="ignore"):
        a = AC[..., :3] / nf
        m = ND[..., :3] / nf
        d = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
        ok = (d != F(0)) & np.isfinite(d)
        inv = F(1) / np.sqrt(np.where(ok, d, F(1)))
        n = np.where(ok[..., None], m * inv[..., None], F(0)).astype(np.float32)
        z = ND[..., 3] / AC[..., 3]
        a_eps = a + dr.EPS_A
        e = c / a_eps
    bg = (AC[..., 3] == F(0)) | ~(z > F(0))
    e = np.where(bg[..., None], c, e).astype(np.float32)
    lum = (e[..., 0] + e[..., 1]) + e[..., 2]
    for i in range(iterations):
        e, lum = dr.iterate(e, lum, n, z, bg, i, sigma_color, sigma_normal, sigma_depth)
    with np.errstate(all="ignore"):
        out = e * a_eps
    return np.where(bg[..., None], c, out).astype(np.float32)
