"""The temporal history on the CPU: tests/temporal_restatement.py (numpy f32, what the GPU tests hold the device to) against an f64 evaluation written from the
header's definition alone, pixel by pixel; against an analytic plane whose history colour is an affine function of the world point; against itself for identical
cameras; and, with the oracle's renders of the Duck, the one claim the feature makes: the reprojected frame is closer to the truth than the new view's own samples.

What "rejected by depth / by normal" counts, here and in the GPU twin: pixels that lost at least one live in-frame tap to that test (temporal_restatement.reproject)."""
import math

import numpy as np
import pytest

import temporal_charts as tc
import temporal_restatement as tr
from conftest import bits

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------------------------- the header's definition in f64, one pixel at a time
def _v(a):
    return [float(x) for x in a]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def _mul(s, a):
    return [s * a[0], s * a[1], s * a[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def pixel_f64(chart, x, y, params, margins):
    """-> (T (4), G (4)) of pixel (x, y) by the header's steps 1 .. 5 in Python floats.  margins: a list that receives how far every decision of the pixel stood from
    its threshold, as (what, distance in the units the chart's construction speaks of)."""
    Wd, Hd, Nf = chart.width, chart.height, float(chart.samples)
    S, AC, ND = _v(chart.S[y, x]), _v(chart.AC[y, x]), _v(chart.ND[y, x])
    c = [S[0] / Nf, S[1] / Nf, S[2] / Nf]
    z = ND[3] / AC[3] if AC[3] != 0 else math.nan
    if AC[3] == 0 or not z > 0:
        return c + [Nf], [0.0, 0.0, 0.0, 0.0]
    m = [ND[0] / Nf, ND[1] / Nf, ND[2] / Nf]
    d = _dot(m, m)
    n = _mul(1 / math.sqrt(d), m) if d != 0 and abs(d) <= FLT_MAX else [0.0, 0.0, 0.0]
    G = n + [z]
    if chart.history is None:
        return c + [Nf], G
    cam = _v(chart.camera)
    origin, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    u, v = (x + 0.5) / Wd, (y + 0.5) / Hd
    s, t = u + 0.5 / Wd, (1 - v) + 0.5 / Hd
    e = _sub(_add(_add(llc, _mul(s, hor)), _mul(t, ver)), origin)
    P = _add(origin, _mul(z / math.sqrt(_dot(e, e)), e))
    old = _v(chart.history["camera"])
    o2, llc2, hor2, ver2 = old[0:3], old[3:6], old[6:9], old[9:12]
    w, L, Nn = _sub(P, o2), _sub(llc2, o2), _cross(hor2, ver2)
    den = _dot(Nn, w)
    k = _dot(Nn, L) / den if den != 0 else math.nan
    margins.append(("in front", abs(k)))
    if not k > 0:
        return c + [Nf], G
    q = _sub(_mul(k, w), L)
    nn = _dot(Nn, Nn)
    fx = _dot(_cross(q, ver2), Nn) / nn * Wd - 1
    fy = (1 - _dot(_cross(hor2, q), Nn) / nn) * Hd
    margins.append(("frame", min(abs(fx + 1), abs(fx - Wd), abs(fy + 1), abs(fy - Hd))))
    if not (fx >= -1 and fx < Wd and fy >= -1 and fy < Hd):
        return c + [Nf], G
    x0, y0 = math.floor(fx), math.floor(fy)
    tx, ty = fx - x0, fy - y0
    z_old = math.sqrt(_dot(w, w))
    sum_b, sum_c, sum_h = 0.0, [0.0, 0.0, 0.0], 0.0
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            if not (0 <= qx < Wd and 0 <= qy < Hd):
                continue
            Tq, Gq = _v(chart.history["color"][qy, qx]), _v(chart.history["geometry"][qy, qx])
            if not (Tq[3] > 0 and Gq[3] > 0):
                continue
            margins.append(("depth", abs(abs(Gq[3] - z_old) - params["depth_tolerance"] * z_old) / z_old))
            if not abs(Gq[3] - z_old) <= params["depth_tolerance"] * z_old:
                continue
            margins.append(("normal", abs(_dot(n, Gq[:3]) - params["min_normal_dot"])))
            if not _dot(n, Gq[:3]) >= params["min_normal_dot"]:
                continue
            beta = (tx if i else 1 - tx) * (ty if j else 1 - ty)
            sum_b += beta
            sum_c = _add(sum_c, _mul(beta, Tq[:3]))
            sum_h += beta * Tq[3]
    margins.append(("weight", sum_b if sum_b > 0 else 1.0))
    if not sum_b > 0:
        return c + [Nf], G
    h = sum_h / sum_b
    he = h if h < params["max_history"] else params["max_history"]
    return [(Nf * c[ch] + he * sum_c[ch] / sum_b) / (Nf + he) for ch in range(3)] + [Nf + he], G


@pytest.fixture(scope="module")
def evaluated():
    """name -> (T64 (H, W, 4), G64 (H, W, 4), the smallest margin of each kind) over every finite chart"""
    out = {}
    for name, chart in tc.finite_charts().items():
        params = dict(tr.DEFAULTS, **chart.params)
        T, G, margins = np.zeros((chart.height, chart.width, 4)), np.zeros((chart.height, chart.width, 4)), []
        for y in range(chart.height):
            for x in range(chart.width):
                T[y, x], G[y, x] = pixel_f64(chart, x, y, params, margins)
        least = {}
        for what, dist in margins:
            least[what] = min(least.get(what, math.inf), dist)
        out[name] = (T, G, least)
    return out


def test_the_finite_charts_stand_clear_of_every_threshold(evaluated):
    """By construction: no decision of any pixel of a finite chart is close enough to its threshold for f32 and f64 to take it differently.  The margins: the in-front
    ratio k and the frame test in pixels (1e-3 and more: positions are good to 1e-5 pixels in f32), the depth test as a fraction of the depth and the normal test as a
    difference of dot products (1e-4 and more: both are good to 1e-6), and the summed tap weight of a pixel that takes history (1e-3 and more)."""
    for name, (_, _, least) in evaluated.items():
        assert least.get("in front", 1) > 1e-3 and least.get("frame", 1) > 1e-3 and least.get("weight", 1) > 1e-3, (name, least)
        assert least.get("depth", 1) > 1e-4 and least.get("normal", 1) > 1e-4, (name, least)


def test_the_restatement_against_the_f64_evaluation(evaluated):
    """Tolerance, relative to |ref| + 2^-8 as tests/test_denoise_charts.py states its own: the largest error measured over every finite chart is 1.9e-7 for T (every
    channel and the count) and 1.2e-7 for G; the bound is 1e-6, a factor of five above.  The taken decisions must agree exactly: which pixels blend is compared through
    T.w, whose values N and N + he are far apart."""
    worst_t = worst_g = 0.0
    for name, (T64, G64, _) in evaluated.items():
        T, G, info = tc.reference(tc.finite_charts()[name])
        assert np.isfinite(T).all() and np.isfinite(G).all(), name
        assert np.array_equal(T64[..., 3] != tc.finite_charts()[name].samples, info["took"]), name
        err_t = np.abs(T - T64) / (np.abs(T64) + 2.0 ** -8)
        err_g = np.abs(G - G64) / (np.abs(G64) + 2.0 ** -8)
        worst_t, worst_g = max(worst_t, float(err_t.max())), max(worst_g, float(err_g.max()))
    print(f"largest error of the restatement against f64: T {worst_t:.3e}, G {worst_g:.3e}")
    assert worst_t <= 1e-6 and worst_g <= 1e-6, (worst_t, worst_g)


def test_the_charts_take_the_decisions_they_are_built_for():
    """So that the GPU twin cannot pass by taking no decision"""
    info = {name: tc.reference(c)[2] for name, c in tc.all_charts().items()}
    n = tc.H * tc.W
    assert not info["no history"]["took"].any()
    assert info["identical cameras"]["took"].all()
    pan = info["a pan that leaves a band without history"]
    assert pan["took"].sum() >= n // 2 and (~pan["inside"]).sum() >= 5 * tc.H                        # the band
    step = info["two planes, a step that disoccludes"]
    assert step["taps"]["failed_depth"] >= 64 and (step["depth_rejected"] & ~step["took"]).sum() >= 16 and step["took"].sum() >= n // 2
    assert info["a fold"]["taps"]["failed_normal"] >= 32 and info["a fold"]["took"].sum() >= n // 2
    stripes = info["stripes of two normals"]
    assert (stripes["normal_rejected"] & ~stripes["took"]).sum() >= 64 and stripes["took"].sum() >= 64
    away = info["the old camera looks the other way"]
    assert not away["in_front"].any() and not away["took"].any()
    sky = info["a panel in front of the sky"]
    assert sky["bg"].sum() >= 64 and sky["taps"]["dead"] >= 16 and sky["took"].sum() >= 64          # (dead taps: the sky of the old view under a panel pixel)
    mirrored = info["a mirrored old camera (horizontal' x vertical' points at the scene)"]
    assert mirrored["took"].all()
    for mh, cap in ((3.0, 3.0), (tc.HISTORY, tc.HISTORY), (20.0, tc.HISTORY)):
        T, _, i = tc.reference(tc.all_charts()[f"max_history {mh:g} against h = {tc.HISTORY:g}"])
        assert i["took"].sum() >= n // 2 and np.allclose(T[i["took"], 3], tc.N + cap, rtol=1e-6), mh
    loose, tight = info["loose tests: depth 0.6, normal -1 (the panel's taps pass for the wall behind it)"], step
    assert loose["taps"]["failed_depth"] == 0 and loose["taps"]["valid"] > tight["taps"]["valid"]
    for name in ("frame 1 x 1", "frame 40 x 1", "frame 1 x 33", "frame 15 x 15", "frame 16 x 16", "frame 17 x 17"):
        assert info[name]["took"].all() and info[name]["taps"]["outside"] >= 1, name                # a footprint that overhangs the frame: taps skipped, history taken
    # the special values: every class sits where its taps are read, and NaN and infinity reach the output only through valid taps
    chart = tc.special_chart()
    T, G, i = tc.reference(chart)
    assert min((chart.cls == k).sum() for k in range(len(chart.names))) >= 5
    bad = ~np.isfinite(T).all(-1)
    assert 16 <= bad.sum() <= n // 4
    ys, xs = np.nonzero(bad)
    reachable = np.zeros((tc.H, tc.W), bool)                                                         # a step of 2.11 pixels to the side: a special pixel is a tap of at most 4 x 2 pixels
    valid_poison = [k for k, name in enumerate(chart.names) if name.endswith("at a valid tap")]
    for y, x in np.argwhere(np.isin(chart.cls, valid_poison)):
        reachable[max(0, y - 1):y + 2, max(0, x - 4):x + 5] = True
    assert not (bad & ~reachable).any(), list(zip(ys, xs))[:5]                                       # (so no invalid tap's NaN or infinity, and no h, reached the output)
    assert 1 <= i["taps"]["dead"] and i["taps"]["failed_depth"] >= 4 and i["taps"]["failed_normal"] >= 4
    # a degenerate old camera: the pixels pass the in-front test and fail the frame test on a NaN or an infinity -- the guard in front of the conversion
    for label, c in tc.degenerate_camera_chart().items():
        T, G, i = tc.reference(c)
        assert not i["took"].any() and np.isfinite(T).all(), label
        if label == "zero horizontal":                                                               # (Nn = 0: k = 0 / 0 fails the first test)
            assert not i["in_front"].any()
            continue
        assert i["in_front"].all() and not i["inside"].any(), label                                  # every pixel reached the frame test, and it refused
        if label == "denormal horizontal":                                                           # dot(Nn, Nn) underflows to 0: a and b are infinities or NaN
            assert not (np.isfinite(i["fx"]) & np.isfinite(i["fy"])).any()


# ---------------------------------------------------------------------------------- the analytic plane
def test_an_affine_history_over_a_plane_is_reproduced_at_the_pixels_own_world_point():
    """A wall z = 5 facing the old camera, which looks straight at it: the old view's pixel grid maps to the wall affinely, so the bilinear interpolation of an affine
    function of the world point at (fx, fy) IS that function at the new pixel's own world point, in real arithmetic.  The new camera differs by a translation and a yaw.
    The expected value is formed from the world point the ORACLE's camera ray gives (orc.generate_camera_ray at the pixel's s, t), not from the restatement's.
    The bound: world points lie within |x|, |y| < 8 and z = 5, so a coordinate carries at most 2^-24 x 8 = 4.8e-7 of rounding per operation; P, w, q, a, b, fx come
    from chains of about 20 operations -> 1e-5 in the world, and through the colour's gradient (at most 0.07 per unit) 7e-7 in the colour; the interpolation and the
    blend add about 10 roundings of values below 1, 6e-7.  Together 1.3e-6; the bound is 2^-19 = 1.9e-6.  Measured: 1.2e-7."""
    from oracle import orc
    chart = tc.finite_charts()["a translation and a small yaw"]
    T, G, info = tc.reference(chart)
    depth, _, P = tc.cast(tc.WALL, chart.camera, tc.W, tc.H)
    # the oracle's own ray through the pixel at the blue-noise pair's mean: s = (x + 1) / W, t = 1 - y / H
    for (y, x) in ((0, 0), (5, 31), (32, 39), (17, 3)):
        ray = orc.generate_camera_ray(chart.camera, F32((x + 1) / tc.W), F32(1 - y / tc.H))
        point = ray[:3].astype(np.float64) + depth[y, x] * ray[3:6].astype(np.float64)
        assert np.abs(point - P[y, x]).max() < 1e-5, ((y, x), point, P[y, x])
    # footprint wholly inside the old frame: all four taps
    with np.errstate(invalid="ignore"):
        whole = info["inside"] & (info["fx"] >= 0) & (info["fx"] < tc.W - 1) & (info["fy"] >= 0) & (info["fy"] < tc.H - 1)
    assert whole.sum() >= tc.H * tc.W // 2 and info["took"][whole].all()
    c = chart.S[..., :3].astype(np.float64) / tc.N
    want = (tc.N * c + tc.HISTORY * tc.affine_colour(P)) / (tc.N + tc.HISTORY)
    err = np.abs(T[..., :3] - want)[whole]
    print(f"largest error against the affine function: {err.max():.3e}")
    assert err.max() <= 2.0 ** -19, err.max()
    assert np.allclose(T[whole, 3], tc.N + tc.HISTORY, rtol=1e-6, atol=0)
    # footprint outside the old frame: the pixel's own mean, exactly
    left = ~info["inside"]
    assert left.sum() >= 3 * tc.H
    assert np.array_equal(bits(T[left][:, :3]), bits((chart.S[..., :3] / F32(tc.N))[left])) and (T[left, 3] == tc.N).all()


def test_the_rays_of_the_charts_are_the_renderers_at_the_blue_noise_mean():
    """kRaygen's ray with the blue-noise pair at its mean is what step 2 writes: the oracle's per-frame camera rays of a pixel, averaged over 64 frames, agree with
    the charts' ray to the spread of the average (the pair is uniform on the unit square: a direction's standard error over 64 frames is about a sixteenth of a pixel)."""
    from oracle import orc
    cam = tc.yawed([0.37, 0.11, -0.2], 2.9)
    rp = orc.make_render_params(tc.W, tc.H, cam, 64, 1, 1.0, np.zeros(40, F32))
    _, d = tc.rays(cam, tc.W, tc.H)
    pixel = np.linalg.norm(np.asarray(cam[6:9], np.float64)) / tc.W
    for (y, x) in ((0, 0), (32, 39), (10, 20)):
        mean = np.mean([orc.wgsl_camera_ray(rp, x, y, f)[3:6] for f in range(64)], 0)
        assert np.linalg.norm(mean / np.linalg.norm(mean) - d[y, x]) < 0.25 * pixel, ((y, x), mean, d[y, x])


# ---------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("scene", ["WALL", "FOLD", "TWO_PLANES"])
def test_identical_cameras_put_every_pixel_on_itself(scene):
    """Same camera, history = the frame's own {c, N} and G: every foreground pixel's (fx, fy) lies within 16 ulps of the frame's extent -- 16 x 2^-23 x 64 = 1.2e-4
    pixels; measured 1.1e-5 -- of (x, y), and T.w = Nf + min(Nf, max_history): exactly where max_history caps it, and within 4 ulps where h itself (a ratio of two sums
    of rounded weights) stands."""
    cam = tc.yawed([0.1, 0.05, 0.0], 4.0)
    S, AC, ND, _ = tc.view_sums(getattr(tc, scene), cam, tc.W, tc.H, 5)
    own_T, own_G = tr.reproject(S, AC, ND, tc.N, cam)
    assert (own_T[..., 3] == tc.N).all()
    hist = dict(color=own_T, geometry=own_G, camera=cam)
    ys, xs = np.mgrid[0:tc.H, 0:tc.W]
    for mh in (4.0, 64.0):
        T, G, info = tr.reproject(S, AC, ND, tc.N, cam, hist, max_history=mh, details=True)
        fg = ~info["bg"]
        assert fg.all() and info["took"].all()
        off = max(float(np.abs(info["fx"] - xs).max()), float(np.abs(info["fy"] - ys).max()))
        print(f"{scene}, max_history {mh:g}: (fx, fy) within {off:.2e} pixels of (x, y)")
        assert off <= 16 * 2.0 ** -23 * 64, off
        want = F32(tc.N) + F32(min(tc.N, mh))
        if mh < tc.N:
            assert (T[..., 3] == want).all()
        else:
            assert np.abs(T[..., 3] - want).max() <= 4 * np.spacing(want)
        # the blend of a pixel with (all but) itself
        assert np.abs(T[..., :3] - own_T[..., :3]).max() <= 1e-4
        assert np.array_equal(bits(G), bits(own_G))


# ---------------------------------------------------------------------------------- with the oracle: the Duck
VIEW_A = dict(position=(0.75, 1.0, -0.75), yaw_degrees=129.64, pitch_degrees=-13.73)
VIEW_B = dict(position=(0.62, 1.02, -0.86), yaw_degrees=123.0, pitch_degrees=-13.0)                  # a small fly-camera step: a stride to the side and 6.6 degrees of yaw
DUCK_W, DUCK_H, DUCK_SPP, DUCK_BOUNCES = 96, 64, 4, 2


def test_the_reprojected_frame_is_closer_to_the_truth_than_the_views_own_samples(duck_oracle):
    """View A at 4 spp becomes the history, view B at 4 spp is reprojected over it, a 256-spp render of B is the truth: the RMSE of T.rgb must be below that of c.
    Only the sign is asserted (measured: 0.79; profiles/temporal/README.md).  And every decision is taken by at least 16 pixels, by the oracle's data alone."""
    import aov_restatement as ar
    import rayfinder_amd as rf
    from oracle import orc
    sky = rf.aligned_sky_state(rf.make_sky())

    def view(pose, spp):
        cam = rf.camera_to_array(rf.fly_camera(DUCK_W, DUCK_H, **pose))
        rp = orc.make_render_params(DUCK_W, DUCK_H, cam, spp, DUCK_BOUNCES, 0.25, sky)
        image, _, _ = orc.render_threads(duck_oracle.scene, rp, 0, spp, 0, 0, DUCK_W, DUCK_H, 8)
        return cam, rp, image

    cam_a, rp_a, s_a = view(VIEW_A, DUCK_SPP)
    cam_b, rp_b, s_b = view(VIEW_B, DUCK_SPP)
    ac_a, nd_a = ar.aov_sums(duck_oracle.scene, rp_a, range(DUCK_SPP))
    ac_b, nd_b = ar.aov_sums(duck_oracle.scene, rp_b, range(DUCK_SPP))
    truth = view(VIEW_B, 256)[2][..., :3].astype(np.float64) / 256
    t_a, g_a = tr.reproject(s_a, ac_a, nd_a, DUCK_SPP, cam_a)
    T, G, info = tr.reproject(s_b, ac_b, nd_b, DUCK_SPP, cam_b, dict(color=t_a, geometry=g_a, camera=cam_a), details=True)
    c = s_b[..., :3] / F32(DUCK_SPP)

    def rmse(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - truth) ** 2)))

    counts = dict(took=int(info["took"].sum()), depth=int(info["depth_rejected"].sum()), normal=int(info["normal_rejected"].sum()),
                  left=int((~info["bg"] & ~info["inside"]).sum()), background=int(info["bg"].sum()))
    print(f"rmse of c {rmse(c):.4f}, of T {rmse(T[..., :3]):.4f}, ratio {rmse(T[..., :3]) / rmse(c):.3f}; {counts}")
    assert min(counts.values()) >= 16, counts
    assert rmse(T[..., :3]) < rmse(c)
