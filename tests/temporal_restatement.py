"""numpy float32 restatement of the temporal history as include/rayfinder_amd.h defines it ("Temporal history"): the GPU tests compare rf_temporal_images and
rf_renderer_temporal_accumulate against it bit for bit.  Vectorised over pixels, one elementwise step per operation, the four taps in tap order; every constant is an
np.float32 and every operation is one IEEE f32 operation, in the order the header writes it.  Prep is tests/denoise_restatement.py's, the mean-input filter
tests/robust_restatement.py's (prep with a given colour, then denoise_restatement's passes)."""
import numpy as np

import denoise_restatement as dr
from robust_restatement import denoise_robust as denoise_mean

F = np.float32
DEFAULTS = dict(max_history=64.0, depth_tolerance=0.05, min_normal_dot=0.9)


def camera_members(cam19):
    """-> origin, lower_left_corner, horizontal, vertical: (3,) f32 each (up, right and lens_radius are not read: the pinhole centre)"""
    c = np.asarray(cam19, np.float32).reshape(19)
    return c[0:3], c[3:6], c[6:9], c[9:12]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0], a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def world_points(width, height, cam19, z):
    """Step 2 for every pixel of the frame: -> P (H, W, 3) f32 from the depths z (H, W)"""
    origin, llc, hor, ver = camera_members(cam19)
    wf, hf = F(width), F(height)
    xs = np.arange(width, dtype=np.uint32).astype(np.float32)[None, :]
    ys = np.arange(height, dtype=np.uint32).astype(np.float32)[:, None]
    with np.errstate(all="ignore"):
        u = (xs + F(0.5)) / wf
        v = (ys + F(0.5)) / hf
        s = np.broadcast_to(u + F(0.5) / wf, (height, width))
        t = np.broadcast_to((F(1) - v) + F(0.5) / hf, (height, width))
        e = ((llc + s[..., None] * hor) + t[..., None] * ver) - origin
        direction = e * (F(1) / np.sqrt(_dot(e, e)))[..., None]
        return origin + z[..., None] * direction


def into_old_view(P, width, height, old19):
    """Step 3 -> dict(den, fx, fy, inside (the guard: k > 0 and the four comparisons), x0, y0 (int64, 0 where not inside), tx, ty, z_old)"""
    origin, llc, hor, ver = camera_members(old19)
    wf, hf = F(width), F(height)
    with np.errstate(all="ignore"):
        w = P - origin
        L = llc - origin
        Nn = _cross(hor, ver)
        den = _dot(Nn, w)
        k = _dot(Nn, L) / den
        q = k[..., None] * w - L
        nn = _dot(Nn, Nn)
        a = _dot(_cross(q, ver), Nn) / nn
        b = _dot(_cross(hor, q), Nn) / nn
        fx = a * wf - F(1)
        fy = (F(1) - b) * hf
        inside = (k > F(0)) & (fx >= F(-1)) & (fx < wf) & (fy >= F(-1)) & (fy < hf)
        xf, yf = np.floor(fx), np.floor(fy)
        tx, ty = fx - xf, fy - yf
        z_old = np.sqrt(_dot(w, w))
    x0 = np.where(inside, xf, F(0)).astype(np.int64)            # (the conversion happens behind the guard)
    y0 = np.where(inside, yf, F(0)).astype(np.int64)
    return dict(den=den, k=k, fx=fx, fy=fy, inside=inside, x0=x0, y0=y0, tx=tx, ty=ty, z_old=z_old)


def reproject(color_sum, albedo_coverage, normal_depth, samples, camera, history=None, max_history=64.0, depth_tolerance=0.05, min_normal_dot=0.9, details=False):
    """-> T (H, W, 4) f32 {rgb, effective sample count}, G (H, W, 4) f32 {n, z} (zeros: background)[, details].  history: None or dict(color, geometry, camera).
    details: dict(bg, inside, took, depth_rejected, normal_rejected, fx, fy, taps) -- which decision every pixel took (depth_rejected / normal_rejected: the pixel lost
    at least one in-frame tap with T'.w > 0 and G'.w > 0 to that test -- the normal test being reached only behind the depth test; it may still have taken history
    from its other taps, and it may count as both), and how many taps of the frame went which way."""
    S = np.asarray(color_sum, np.float32)
    H, W = S.shape[:2]
    nf = F(samples)
    c, _, _, n, z, _, bg = dr.prep(S, albedo_coverage, normal_depth, samples)
    G = np.where(bg[..., None], F(0), np.concatenate([n, z[..., None]], -1)).astype(np.float32)
    T = np.concatenate([c, np.full((H, W, 1), nf, np.float32)], -1).astype(np.float32)
    info = dict(bg=bg, in_front=np.zeros((H, W), bool), inside=np.zeros((H, W), bool), took=np.zeros((H, W), bool), depth_rejected=np.zeros((H, W), bool), normal_rejected=np.zeros((H, W), bool),
                fx=np.full((H, W), np.nan, np.float32), fy=np.full((H, W), np.nan, np.float32))
    if history is None:
        return (T, G, info) if details else (T, G)
    Tp, Gp = np.asarray(history["color"], np.float32), np.asarray(history["geometry"], np.float32)
    mh, dt, mn = F(max_history), F(depth_tolerance), F(min_normal_dot)
    with np.errstate(all="ignore"):
        o = into_old_view(world_points(W, H, camera, z), W, H, history["camera"])
        inside = o["inside"] & ~bg
        z_tol = dt * o["z_old"]
        sum_b = np.zeros((H, W), np.float32)
        sum_c = np.zeros((H, W, 3), np.float32)
        sum_h = np.zeros((H, W), np.float32)
        failed_depth = np.zeros((H, W), bool)
        failed_normal = np.zeros((H, W), bool)
        taps = dict(valid=0, outside=0, dead=0, failed_depth=0, failed_normal=0)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = o["x0"] + i, o["y0"] + j
                in_frame = inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                Tq, Gq = Tp[cy, cx], Gp[cy, cx]
                live = in_frame & (Tq[..., 3] > F(0)) & (Gq[..., 3] > F(0))
                depth_ok = np.abs(Gq[..., 3] - o["z_old"]) <= z_tol
                normal_ok = _dot(n, Gq[..., :3]) >= mn
                valid = live & depth_ok & normal_ok
                failed_depth |= live & ~depth_ok
                failed_normal |= live & depth_ok & ~normal_ok
                for key, mask in (("valid", valid), ("outside", inside & ~in_frame), ("dead", in_frame & ~live), ("failed_depth", live & ~depth_ok),
                                  ("failed_normal", live & depth_ok & ~normal_ok)):
                    taps[key] += int(mask.sum())
                beta = (o["tx"] if i else F(1) - o["tx"]) * (o["ty"] if j else F(1) - o["ty"])
                sum_b = np.where(valid, sum_b + beta, sum_b).astype(np.float32)
                sum_c = np.where(valid[..., None], sum_c + beta[..., None] * Tq[..., :3], sum_c).astype(np.float32)
                sum_h = np.where(valid, sum_h + beta * Tq[..., 3], sum_h).astype(np.float32)
        took = inside & (sum_b > F(0))
        hist = sum_c / sum_b[..., None]
        h = sum_h / sum_b
        he = np.where(h < mh, h, mh).astype(np.float32)
        w_sum = nf + he
        blended = (nf * c + he[..., None] * hist) / w_sum[..., None]
    T = np.where(took[..., None], np.concatenate([blended, w_sum[..., None]], -1), T).astype(np.float32)
    info.update(inside=inside, took=took, depth_rejected=inside & failed_depth, normal_rejected=inside & failed_normal,
                fx=o["fx"], fy=o["fy"], taps=taps, in_front=(o["k"] > F(0)) & ~bg)
    return (T, G, info) if details else (T, G)


def denoise_temporal(T, albedo_coverage, normal_depth, samples, **params):
    """The a-trous filter with prep's colour c = T.rgb: rf_renderer_denoise_temporal's second half -> (H, W, 3) f32"""
    return denoise_mean(np.asarray(T, np.float32)[..., :3], albedo_coverage, normal_depth, samples, **params)
