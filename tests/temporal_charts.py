"""Crafted inputs for the temporal history (rf_temporal_images, rf_renderer_temporal_accumulate): small analytic scenes of planes seen by two pinhole cameras, cast in
f64 with the header's own ray (step 2), so that the current view's sums and the old view's planes describe one static world; and a special-value chart that writes
NaN, infinities, zeros and denormals over them.  Shared by tests/test_temporal_restatement.py (CPU: the restatement against an independent f64 evaluation, and the
checks that the charts take the decisions they are built for) and tests/test_gpu_temporal.py (the device against the restatement on the same inputs).  Deterministic.

The frame is 33 rows x 40 columns: 3 x 3 workgroups of 16 x 16 with a ragged last row and column, and 2 x 2 tiles of 32 x 32.  Every chart holds N = 6 samples; the
history holds h = 8 effective samples unless the chart says otherwise.

A FINITE chart keeps every validity decision away from its threshold (check_margins): depth differences are either rounding (one surface) or a good part of the depth
(another surface), normals agree or differ by a fold, and no pixel's footprint touches the frame's edge closer than a thousandth of a pixel -- so that the f32
restatement and an f64 evaluation take the same decisions by construction."""
import functools

import numpy as np

F32 = np.float32
H, W, N = 33, 40, 6
HISTORY = 8.0
INF, NAN = F32(np.inf), F32(np.nan)
A_DENORMAL = F32(1e-40)


# ---------------------------------------------------------------------------------- cameras
def camera(origin, look_at, vfov_degrees=70.0, aspect=W / H, focus=1.0, mirrored=False):
    """A pinhole camera as 19 f32: origin, lower_left_corner, horizontal, vertical, up, right, lens_radius = 0.  As rf_create_camera builds it: right = forward x
    world up, up = right x forward, so horizontal x vertical points AWAY from the scene; mirrored: right negated (the image flipped left to right), and it points at it."""
    origin, look_at = np.asarray(origin, np.float64), np.asarray(look_at, np.float64)
    forward = look_at - origin
    forward /= np.linalg.norm(forward)
    right = np.cross(forward, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, forward)
    if mirrored:
        right = -right
    half_h = np.tan(np.radians(vfov_degrees) / 2) * focus
    half_w = aspect * half_h
    llc = origin - half_w * right - half_h * up + focus * forward
    return np.concatenate([origin, llc, 2 * half_w * right, 2 * half_h * up, up, right, [0.0]]).astype(F32)


def yawed(origin, yaw_degrees, **kw):
    """looking along +z turned by yaw about the y axis"""
    a = np.radians(yaw_degrees)
    return camera(origin, np.asarray(origin, np.float64) + [np.sin(a), 0.0, np.cos(a)], **kw)


def rays(cam19, width, height):
    """The header's step 2 in f64 over the camera's f32 members -> origin (3,), unit directions (H, W, 3)"""
    c = np.asarray(cam19, np.float64)
    origin, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    s = (np.arange(width) + 0.5) / width + 0.5 / width
    t = (1.0 - (np.arange(height) + 0.5) / height) + 0.5 / height
    e = llc + s[None, :, None] * hor + t[:, None, None] * ver - origin
    return origin, e / np.linalg.norm(e, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------- scenes: planes, each bounded by a predicate on the world point
class Plane:
    """where: which world points of the plane exist; shading: the recorded unit normal of a world point where it is not the plane's own (a painted-on relief)"""

    def __init__(self, point, normal, where=None, shading=None):
        self.point, self.normal = np.asarray(point, np.float64), np.asarray(normal, np.float64) / np.linalg.norm(normal)
        self.where = where or (lambda p: np.ones(p.shape[:-1], bool))
        self.shading = shading


def cast(scene, cam19, width, height):
    """-> depth (H, W) f64 (0: a miss), unit normal (H, W, 3) facing the camera, world point (H, W, 3)"""
    origin, d = rays(cam19, width, height)
    depth = np.full((height, width), np.inf)
    normal = np.zeros((height, width, 3))
    for pl in scene:
        with np.errstate(all="ignore"):
            t = ((pl.point - origin) @ pl.normal) / (d @ pl.normal)
        p = origin + t[..., None] * d
        hit = np.isfinite(t) & (t > 1e-6) & (t < depth) & pl.where(p)
        depth = np.where(hit, t, depth)
        facing = np.where((d @ pl.normal)[..., None] < 0, pl.normal, -pl.normal) if pl.shading is None else pl.shading(p)
        normal = np.where(hit[..., None], facing, normal)
    miss = ~np.isfinite(depth)
    depth = np.where(miss, 0.0, depth)
    return depth, normal, origin + depth[..., None] * d


WALL = [Plane([0, 0, 5], [0, 0, -1])]
# a near panel over the left half in front of a far wall: a sideways step uncovers wall that the old view saw the panel in front of
TWO_PLANES = [Plane([0, 0, 3], [0, 0, -1], lambda p: p[..., 0] < -0.2), Plane([0, 0, 6], [0, 0, -1])]
# a gentle roof ridge along the y axis: two faces that meet at x = 0, z = 4, their normals' dot product 0.82 -- below the default 0.9 -- and their slope small enough
# that neighbouring pixels of one face pass the depth test with room to spare
FOLD = [Plane([0, 0, 4], [0.3, 0, -0.9539392], lambda p: p[..., 0] >= 0), Plane([0, 0, 4], [-0.3, 0, -0.9539392], lambda p: p[..., 0] < 0)]
# a wall with vertical stripes of two painted-on normals, narrower than a pixel (0.13 against a pixel's 0.175 at the wall): some pixels see one normal where all
# four of their taps in the old view saw the other
def _stripes(p):
    a, b = np.array([0.6, 0.0, -0.8]), np.array([-0.6, 0.0, -0.8])
    return np.where((np.floor(p[..., 0] / 0.13).astype(np.int64) % 2 == 0)[..., None], a, b)


STRIPES = [Plane([0, 0, 5], [0, 0, -1], shading=_stripes)]
# a panel in front of the sky
PANEL_AND_SKY = [Plane([0, 0, 5], [0, 0, -1], lambda p: np.abs(p[..., 0]) < 2.0)]


def affine_colour(p):
    """A colour that is an affine function of the world point (bilinear interpolation over a plane reproduces it exactly)"""
    return np.stack([0.5 + 0.05 * p[..., 0] + 0.02 * p[..., 2], 0.4 - 0.03 * p[..., 1] + 0.01 * p[..., 0], 0.3 + 0.04 * p[..., 1] + 0.02 * p[..., 2]], -1)


# ---------------------------------------------------------------------------------- the charts
class Chart:
    """S, AC, ND: the current view's sums (H, W, 4) f32 of `samples` samples; camera; history: None or dict(color, geometry, camera); params: the call's parameters"""

    def __init__(self, name, S, AC, ND, cam, history, params, finite=True, samples=N):
        self.name, self.S, self.AC, self.ND, self.camera, self.history, self.params, self.finite, self.samples = name, S, AC, ND, cam, history, dict(params), finite, samples
        self.height, self.width = S.shape[:2]
        for a in (S, AC, ND) + ((history["color"], history["geometry"]) if history else ()):
            a.setflags(write=False)


def view_sums(scene, cam19, width, height, seed):
    """The sums of N samples of a view: every sample hits what the pixel's central ray hits (no sub-pixel spread), radiance = noise around 0.5 -> S, AC, ND, world points"""
    rng = np.random.default_rng(seed)
    depth, normal, p = cast(scene, cam19, width, height)
    hit = depth > 0
    S = np.zeros((height, width, 4), F32)
    S[..., :3] = (0.5 + 0.4 * (rng.random((height, width, 3)) - 0.5)) * N
    AC = np.zeros((height, width, 4), F32)
    AC[hit] = np.array([0.5, 0.35, 0.25, 1.0]) * N
    ND = np.concatenate([normal * N, (depth * N)[..., None]], -1).astype(F32)
    ND[~hit] = 0
    return S, AC, ND, p


def view_history(scene, cam19, width, height, colour=affine_colour, h=HISTORY):
    """The planes a commit of that view would keep: T' = {colour of the world point, h}, G' = {n, z} (zeros on the sky)"""
    depth, normal, p = cast(scene, cam19, width, height)
    hit = depth > 0
    T = np.concatenate([colour(p), np.full((height, width, 1), h)], -1).astype(F32)
    T[~hit, :3] = 0.7                                      # (the sky's colour: never taken)
    G = np.concatenate([normal, depth[..., None]], -1).astype(F32)
    G[~hit] = 0
    return dict(color=T, geometry=G, camera=np.asarray(cam19, F32))


def _chart(name, scene, new, old, width=W, height=H, params=None, seed=7, **hist):
    S, AC, ND, _ = view_sums(scene, new, width, height, seed)
    return Chart(name, S, AC, ND, new, None if old is None else view_history(scene, old, width, height, **hist), params or {})


HERE = yawed([0, 0, 0], 0.0)
STEP = yawed([0.37, 0.0, 0.0], 0.0)                                 # a sideways step of a little more than two pixels at the wall


@functools.lru_cache(maxsize=None)
def finite_charts():
    """name -> Chart: the cases whose reference is finite everywhere and whose decisions stand clear of their thresholds"""
    out = [
        _chart("no history", WALL, HERE, None),
        _chart("identical cameras", WALL, HERE, HERE),
        _chart("a pan that leaves a band without history", WALL, yawed([0, 0, 0], 16.9), HERE),
        _chart("two planes, a step that disoccludes", TWO_PLANES, STEP, HERE),
        _chart("a fold", FOLD, yawed([0.21, 0.0, 0.0], 1.1), HERE),
        _chart("stripes of two normals", STRIPES, yawed([0.31, 0.0, 0.0], 0.7), HERE),
        _chart("the old camera looks the other way", WALL, HERE, yawed([0, 0, 0], 180.0)),
        _chart("a panel in front of the sky", PANEL_AND_SKY, STEP, HERE),
        _chart("a translation and a small yaw", WALL, yawed([0.37, 0.11, -0.2], 2.9), HERE),
        _chart("a mirrored old camera (horizontal' x vertical' points at the scene)", WALL, STEP, yawed([0, 0, 0], 0.0, mirrored=True)),
        _chart("a mirrored new camera", TWO_PLANES, yawed([0.37, 0.0, 0.0], 0.0, mirrored=True), HERE),
    ]
    # max_history below, at and above h
    for mh in (3.0, HISTORY, 20.0):
        out.append(_chart(f"max_history {mh:g} against h = {HISTORY:g}", WALL, STEP, HERE, params=dict(max_history=mh)))
    # looser and tighter tests
    out.append(_chart("loose tests: depth 0.6, normal -1 (the panel's taps pass for the wall behind it)", TWO_PLANES, STEP, HERE, params=dict(depth_tolerance=0.6, min_normal_dot=-1.0)))
    # frames of 1 x 1, one row, one column, one workgroup -+ 1 pixel
    for (w, h) in ((1, 1), (40, 1), (1, 33), (15, 15), (16, 16), (17, 17)):
        kw = dict(aspect=w / h, vfov_degrees=2.0 if h == 1 else 40.0)             # (one row of 40: a field of view that keeps the 40 pixels in front of the camera)
        out.append(_chart(f"frame {w} x {h}", WALL, yawed([0.11, 0.07, 0.0] if w > 1 else [0.004, 0.05, 0.0], 0.0, **kw), yawed([0, 0, 0], 0.0, **kw), width=w, height=h))
    return {c.name: c for c in out}


# special values, written over a step across the wall (every pixel's four taps carry weight): a class rewrites one pixel of the history planes or of the current sums
def _t(index, value):
    def write(p):
        p["T"][index] = value
    return write


def _g(index, value):
    def write(p):
        p["G"][index] = value
    return write


def _both(*writers):
    def write(p):
        for w in writers:
            w(p)
    return write


def _current_depth(value):
    def write(p):
        p["AC"][3], p["ND"][3] = F32(1.0), value              # (one hit among the samples: z = the value itself)
    return write


SPECIAL_CLASSES = {
    "history colour NaN at a valid tap": _t(1, NAN),
    "history colour +inf at a valid tap": _t(0, INF),
    "history colour -inf at a valid tap": _t(2, -INF),
    "history colour NaN at a tap invalid by its depth": _both(_t(slice(0, 3), NAN), _g(3, F32(50.0))),
    "history colour inf at a tap invalid by its count": _both(_t(slice(0, 3), INF), _t(3, F32(0.0))),
    "history colour NaN at a tap invalid by its normal": _both(_t(slice(0, 3), NAN), _g(slice(0, 3), np.array([1.0, 0.0, 0.0], F32))),
    "h = 0": _t(3, F32(0.0)),
    "h = -0": _t(3, F32(-0.0)),
    "h negative": _t(3, F32(-8.0)),
    "h denormal": _t(3, A_DENORMAL),
    "h = +inf": _t(3, INF),
    "h NaN": _t(3, NAN),
    "h huge": _t(3, F32(3e38)),
    "G'.z denormal": _g(3, A_DENORMAL),
    "G'.z +inf": _g(3, INF),
    "G'.z NaN": _g(3, NAN),
    "G'.z = 0 (background)": _g(3, F32(0.0)),
    "G' normal NaN": _g(0, NAN),
    "current z denormal": _current_depth(A_DENORMAL),
    "current z 3e38": _current_depth(F32(3e38)),
    "current z +inf": _current_depth(INF),
}


@functools.lru_cache(maxsize=None)
def special_chart():
    """The classes on a lattice of pitch 3 (so every special tap has ordinary taps beside it), over "a step across the wall" -> Chart with .cls / .names"""
    S, AC, ND, _ = view_sums(WALL, STEP, W, H, 11)
    hist = view_history(WALL, HERE, W, H)
    names = list(SPECIAL_CLASSES)
    cls = np.full((H, W), -1, np.int64)
    for k, (y, x) in enumerate((y, x) for y in range(0, H, 3) for x in range(0, W, 3)):
        name = names[k % len(names)]
        SPECIAL_CLASSES[name](dict(T=hist["color"][y, x], G=hist["geometry"][y, x], AC=AC[y, x], ND=ND[y, x]))
        cls[y, x] = names.index(name)
    chart = Chart("special values", S, AC, ND, STEP, hist, {}, finite=False)
    chart.cls, chart.names = cls, names
    return chart


@functools.lru_cache(maxsize=None)
def degenerate_camera_chart():
    """An old camera whose horizontal is zero: Nn = 0, dot(Nn, Nn) = 0 -- den is 0 and the first guard refuses; and one whose horizontal is a denormal, so that den is
    > 0 for some pixels while a, b, fx and fy overflow or are NaN: the guard in front of the conversion is what is tested"""
    out = {}
    for label, scale in (("zero horizontal", 0.0), ("denormal horizontal", 1e-42), ("huge horizontal", 1e30)):
        old = HERE.copy()
        old[6:9] = (old[6:9].astype(np.float64) * scale).astype(F32) if scale < 1 else old[6:9] * F32(scale)
        S, AC, ND, _ = view_sums(WALL, STEP, W, H, 13)
        hist = view_history(WALL, HERE, W, H)
        hist["camera"] = old
        out[label] = Chart("degenerate old camera: " + label, S, AC, ND, STEP, hist, {}, finite=False)
    return out


def all_charts():
    out = dict(finite_charts())
    out["special values"] = special_chart()
    out.update({c.name: c for c in degenerate_camera_chart().values()})
    return out


# ---------------------------------------------------------------------------------- references, computed once and shared
_references = {}


def reference(chart):
    """The restatement's (T, G, details) of a chart, read-only"""
    import temporal_restatement as tr
    if chart.name not in _references:
        with np.errstate(all="ignore"):
            T, G, info = tr.reproject(chart.S, chart.AC, chart.ND, chart.samples, chart.camera, chart.history, details=True, **dict(tr.DEFAULTS, **chart.params))
        for a in (T, G):
            a.setflags(write=False)
        _references[chart.name] = (T, G, info)
    return _references[chart.name]


def expected_bgra(T, exposure):
    """The display texels of T.rgb: the oracle's tonemap of {T.rgb, 1} with one accumulated sample; a NaN level is 0"""
    from oracle import orc
    rgba = np.concatenate([T[..., :3], np.ones(T.shape[:2] + (1,), F32)], -1).astype(F32)
    with np.errstate(all="ignore"):
        return orc.tonemap_bgra8(rgba, 1, exposure).reshape(T.shape[:2])


def mismatches(got, want, what=None, limit=5):
    """f32 results match where their bits are equal or both are NaN -> up to `limit` reports (what, (y, x, channel), got, want)"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return [(what, tuple(int(k) for k in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in np.argwhere(~same)[:limit]]
