"""Crafted inputs for the a-trous denoisers (rf_denoise_images, rf_denoise_tiles, rf_denoise_split_images, rf_denoise_split_tiles): frames of smooth foreground
pixels with special values -- denormals, signed zeros, overflowing and underflowing sums, NaN, infinities, background by every rule of prep -- written over them, and
the checks that these charts are not vacuous.  Shared by tests/test_denoise_charts.py (CPU: the charts reach the states they are built for, and the restatements
agree with an independent f64 evaluation) and tests/test_gpu_denoise_edges.py (the device against the restatements on the same inputs).  Deterministic, in memory.

The frame is 33 rows x 40 columns: 3 x 3 workgroups of 16 x 16 with a last column 8 wide and a last row 1 high, and 2 x 2 tiles of 32 x 32 with borders at
x = 32 and y = 32.  Ordinary pixels: one normal, one albedo, depth 3 + U(0, 0.05), irradiance 1 + U(0, 0.3) per channel, 6 samples, all of them hits; D = 0.6 S.

finite_chart: specials on a lattice of pitch 3 (offsets 1, 2 and 4 from a lattice pixel are never on the lattice, so every special has ordinary neighbours at the first
three steps) plus the frame's last row's corners and the seam pixels the lattice misses.  Every class leaves the reference finite everywhere.
poison_chart: one class at two pixels, (16, 20) and (0, 0), whose infinity or NaN reaches every pixel within 2 (2^L - 1): shallow filters only.

A chart with per-tile counts holds the ordinary sums times count / 6 per tile; a special is written after that scaling, from the pixel's scaled ordinary sums and its
tile's count, so a class that says "times 1e-20" or "1.2 S" means the same thing in every tile and one that names a value holds that value.  One class cannot do
either: the colour sum 3e38 stands for "e finite, its sum l infinite", which needs c = 5e37 -- with 1 or 3 samples 3e38 itself makes e infinite and poisons the frame,
so the class writes 3e38 count / 6 up to 6 samples and 3e38 above (where c is merely large)."""
import functools

import numpy as np

import denoise_restatement as dr
import split_restatement as sr
from denoise_tiles_restatement import denoise_tiles, pixel_counts, prep_tiles
from split_tiles_restatement import denoise_split_tiles, split_prep_tiles

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
A_DENORMAL = F32(1e-40)
H, W, N = 33, 40, 6
SIX = (6, 6, 6, 6)
NORMAL = np.array([0.48, 0.6, 0.64], F32)                # 0.2304 + 0.36 + 0.4096 = 1
ALBEDO = np.array([0.5, 0.35, 0.25], F32)                # 5e37 / (a + εa) is finite per channel and overflows when added up
POISON_AT = ((16, 20), (0, 0))
TILE_COUNTS = ((1, 3, 2 ** 24 + 1, 2 ** 32 - 1), (6, 6, 6, 2 ** 24 + 3))
SAMPLE_COUNTS = (1, 3, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 - 1)


# ---------------------------------------------------------------------------------- classes
# a class rewrites the sums of one pixel: p is a dict of its four float4 rows (S, D, AC, ND; views into the chart) holding the pixel's ordinary sums, nf its count
def _colour(value):
    def write(p, nf):
        p["S"][:3] = value
    return write


def _colour_l_overflows(p, nf):
    p["S"][:3] = F32(3e38) if nf >= 6 else F32(3e38) * (F32(nf) / F32(6))


def _negated_colour(p, nf):
    p["S"][:3] = -p["S"][:3]


def _albedo(value):
    def write(p, nf):
        p["AC"][:3] = value
    return write


def _normal_times(k):
    def write(p, nf):
        with np.errstate(all="ignore"):
            p["ND"][:3] = p["ND"][:3] * F32(k)
    return write


def _normal_nan(p, nf):
    p["ND"][1] = NAN


def _coverage_depth(coverage=None, depth=None):
    def write(p, nf):
        if coverage is not None:
            p["AC"][3] = coverage
        if depth is not None:
            p["ND"][3] = depth
    return write


def _direct(fn):
    def write(p, nf):
        p["D"][:3] = fn(p["S"][:3])
    return write


# name -> (writer, the state prep must show: see _promised)
FINITE_CLASSES = {
    "colour denormal": (_colour(A_DENORMAL), "e denormal"),
    "colour -0": (_colour(F32(-0.0)), "e -0"),
    "colour negative": (_negated_colour, "e negative"),
    "colour 1e30": (_colour(F32(1e30)), "e large"),
    "colour 3e38: l = inf, e finite": (_colour_l_overflows, "l inf"),
    "albedo 0": (_albedo(F32(0.0)), "a_eps == eps"),
    "albedo denormal (a plain special value: absorbed by + eps_a)": (_albedo(A_DENORMAL), "a_eps == eps"),
    "normal x 1e-20: d denormal": (_normal_times(1e-20), "d denormal"),
    "normal x 1e-25: d underflows to 0": (_normal_times(1e-25), "n == 0"),
    "normal x 1e20: d = inf": (_normal_times(1e20), "n == 0"),
    "normal with one NaN component": (_normal_nan, "n == 0"),
    "normal x -1": (_normal_times(-1.0), "n flipped"),
    "coverage 0, depth sum 1": (_coverage_depth(F32(0.0), F32(1.0)), "bg"),
    "coverage 0, depth sum 0": (_coverage_depth(F32(0.0), F32(0.0)), "bg"),
    "coverage NaN": (_coverage_depth(NAN, None), "bg"),
    "depth sum 0": (_coverage_depth(None, F32(0.0)), "bg"),
    "depth negative": (_coverage_depth(None, F32(-18.0)), "bg"),
    "depth NaN": (_coverage_depth(None, NAN), "bg"),
    "depth denormal": (_coverage_depth(None, A_DENORMAL), "z denormal"),
    "depth +inf": (_coverage_depth(None, INF), "z inf"),
    "depth 3e38": (_coverage_depth(None, F32(3e38)), "z large"),
}
SPLIT_CLASSES = {
    "D = S": (_direct(lambda s: s.copy()), "eI == 0"),
    "D = 0": (_direct(lambda s: F32(0.0)), "eD == 0"),
    "D = -0": (_direct(lambda s: F32(-0.0)), "eD -0"),
    "D denormal": (_direct(lambda s: A_DENORMAL), "eD denormal"),
    "D = 1.2 S": (_direct(lambda s: s * F32(1.2)), "eI negative"),
}
# what a build that flushes denormals to zero would see in place of a denormal class: the class whose output must differ from it
FLUSHED = {
    "colour denormal": _colour(F32(0.0)),
    "albedo denormal (a plain special value: absorbed by + eps_a)": _albedo(F32(0.0)),
    "normal x 1e-20: d denormal": _normal_times(0.0),          # (d itself is the denormal: flushed, the normal is (0, 0, 0))
    "depth denormal": _coverage_depth(None, F32(0.0)),
    "D denormal": _direct(lambda s: F32(0.0)),
}
MUST_BE_OBSERVABLE = ("colour denormal", "normal x 1e-20: d denormal", "depth denormal")


def _s_channel(value):
    def write(p, nf):
        p["S"][1] = value
    return write


def _albedo_cancels_eps(p, nf):
    p["AC"][0] = -F32(nf) * F32(2.0 ** -8)


def _both(value):
    def write(p, nf):
        p["S"][:3] = value
        p["D"][:3] = value
    return write


POISON_CLASSES = {
    "S with one +inf channel": _s_channel(INF),
    "S with one NaN channel": _s_channel(NAN),
    "S = -inf": _colour(-INF),
    "albedo sum = -N 2^-8 in one channel": _albedo_cancels_eps,
    "albedo NaN": _albedo(NAN),
    "albedo +inf": _albedo(INF),
}
SPLIT_POISON_CLASSES = {
    "D = +inf, S finite": _direct(lambda s: INF),
    "D NaN": _direct(lambda s: NAN),
    "S = D = +inf": _both(INF),
}


# ---------------------------------------------------------------------------------- the charts
class Chart:
    """S, D, AC, ND: (H, W, 4) f32 sums, read-only; counts: the four tiles' sample counts; cls[y, x]: index into names, -1 for an ordinary pixel."""

    def __init__(self, key, S, D, AC, ND, counts, cls, names):
        self.key, self.counts, self.cls, self.names = key, tuple(int(c) for c in counts), cls, list(names)
        self.S, self.D, self.AC, self.ND = S, D, AC, ND
        for a in (S, D, AC, ND, cls):
            a.setflags(write=False)
        self.tile_samples = np.array(self.counts, np.uint32)

    def label(self, y, x):
        return self.names[self.cls[y, x]] if self.cls[y, x] >= 0 else "ordinary"

    def pixels_of(self, name):
        return np.argwhere(self.cls == self.names.index(name))


def _ordinary(counts):
    rng = np.random.default_rng(3340)
    depth = F32(3.0) + rng.random((H, W)).astype(F32) * F32(0.05)
    irr = F32(1.0) + rng.random((H, W, 3)).astype(F32) * F32(0.3)
    S = np.zeros((H, W, 4), F32)
    S[..., :3] = irr * ALBEDO * F32(N)
    S[..., 3] = rng.random((H, W)).astype(F32)                                # (ignored)
    D = (S * F32(0.6)).astype(F32)
    AC = np.broadcast_to(np.concatenate([ALBEDO * F32(N), [F32(N)]]).astype(F32), (H, W, 4)).copy()
    ND = np.concatenate([np.broadcast_to(NORMAL * F32(N), (H, W, 3)), (depth * F32(N))[..., None]], -1).astype(F32)
    nf = pixel_counts(np.array(counts, np.uint64), H, W)                       # float(count), rounded as the device's conversion rounds it
    scale = (nf / F32(N))[..., None]
    return [(a * scale).astype(F32) for a in (S, D, AC, ND)], nf


def lattice():
    """The special pixels of finite_chart, in placement order: the pitch-3 lattice row by row, then the pixels the issue names that it misses."""
    at = [(y, x) for y in range(0, H, 3) for x in range(0, W, 3)]
    at += [(32, 0), (32, 39), (16, 16), (31, 32), (32, 31)]
    assert {(0, 0), (0, 39), (32, 0), (32, 39), (15, 15), (16, 16), (31, 32), (32, 31)} <= set(at) and len(set(at)) == len(at)
    return at


def _build(key, counts, writers, placements):
    """writers: {name: writer}; placements: [((y, x), name)]"""
    (S, D, AC, ND), nf = _ordinary(counts)
    names = list(writers)
    cls = np.full((H, W), -1, np.int64)
    for (y, x), name in placements:
        writers[name](dict(S=S[y, x], D=D[y, x], AC=AC[y, x], ND=ND[y, x]), float(nf[y, x]))
        cls[y, x] = names.index(name)
    return Chart(key, S, D, AC, ND, counts, cls, names)


@functools.lru_cache(maxsize=None)
def finite_chart(split=False, counts=SIX, flushed=None):
    """flushed: the name of a denormal class to write as a flushing build would see it (FLUSHED), for the observability check"""
    writers = {k: v[0] for k, v in FINITE_CLASSES.items()}
    if split:
        writers.update({k: v[0] for k, v in SPLIT_CLASSES.items()})
    names = list(writers)
    if flushed is not None:
        writers[flushed] = FLUSHED[flushed]
    return _build(("finite", split, tuple(counts), flushed), counts, writers, [(at, names[i % len(names)]) for i, at in enumerate(lattice())])


@functools.lru_cache(maxsize=None)
def poison_chart(cls, split=False, counts=SIX):
    writers = dict(POISON_CLASSES, **(SPLIT_POISON_CLASSES if split else {}))
    return _build(("poison", cls, split, tuple(counts)), counts, {cls: writers[cls]}, [(at, cls) for at in POISON_AT])


def poison_classes(split):
    return list(POISON_CLASSES) + (list(SPLIT_POISON_CLASSES) if split else [])


# ---------------------------------------------------------------------------------- the cases of the GPU tests (the CPU checks run over the same)
SIGMAS = (dict(), dict(sigma_color=3.5, sigma_normal=0.4, sigma_depth=0.02))
PAIRS = ((0, 0), (0, 3), (3, 0), (1, 5), (5, 5), (8, 2), (2, 8))
EXTREMES = ([dict(sigma_color=s) for s in (FLT_MAX, 2e19, 1e-23, 1e-45)] + [dict(sigma_depth=s) for s in (FLT_MAX, 2e36, FLT_MIN, 1e-45)]
            + [dict(sigma_normal=s) for s in (FLT_MAX, 2.0 ** -20)])
FINITE_CASES = [dict(sig, iterations=L) for sig in SIGMAS for L in range(9)] + [dict(sig, iterations=L) for sig in EXTREMES for L in (1, 5, 8)]
SPLIT_SIGMAS = ((SIGMAS[0], SIGMAS[0]), (SIGMAS[1], SIGMAS[1]), (SIGMAS[0], SIGMAS[1]), (SIGMAS[1], SIGMAS[0]))
SPLIT_CASES = [(dict(sd, iterations=ld), dict(si, iterations=li)) for sd, si in SPLIT_SIGMAS for ld, li in PAIRS]
SPLIT_EXTREMES = [(dict(sigma_color=FLT_MAX, iterations=2), dict(iterations=3)), (dict(sigma_color=1e-45, iterations=3), dict(iterations=2)),
                  (dict(iterations=2), dict(sigma_color=FLT_MAX, iterations=3)), (dict(iterations=3), dict(sigma_color=1e-45, iterations=2))]
POISON_CASES = [dict(sig, iterations=L) for sig in SIGMAS for L in (0, 1, 2)]
POISON_SPLIT_CASES = [(dict(sd, iterations=ld), dict(si, iterations=li)) for sd, si in SPLIT_SIGMAS[:3:2] for ld, li in ((1, 2), (2, 1), (0, 2), (2, 0), (1, 1))]
COUNT_CASES = [dict(sig, iterations=L) for sig in SIGMAS for L in (0, 1, 5)]             # the sample-count charts: every count at three depths
COUNT_SPLIT_CASES = [(dict(SIGMAS[0], iterations=1), dict(SIGMAS[1], iterations=5)), (dict(SIGMAS[1], iterations=2), dict(SIGMAS[1], iterations=2))]


def split_instantiations(direct, indirect):
    """The kDenoiseAtrousSplit<DIRECT, INDIRECT, SHARED> of every pass of one call, by enqueueDenoiseSplit's rule: a component is active while the pass index is
    below its own iteration count; two active components share the guide terms when their sigma_normal and their sigma_depth * step are equal floats."""
    pd, pi = sr._params(direct, sr.DIRECT_DEFAULTS), sr._params(indirect, sr.INDIRECT_DEFAULTS)
    out = []
    for i in range(max(pd["iterations"], pi["iterations"])):
        act_d, act_i = i < pd["iterations"], i < pi["iterations"]
        with np.errstate(over="ignore"):
            same = F32(pd["sigma_normal"]) == F32(pi["sigma_normal"]) and F32(pd["sigma_depth"]) * F32(1 << i) == F32(pi["sigma_depth"]) * F32(1 << i)
        out.append((act_d, act_i, bool(act_d and act_i and same)))
    return out


# ---------------------------------------------------------------------------------- references, computed once and shared
def _freeze(p):
    return tuple(sorted(p.items()))


_references = {}


def reference(chart, params, tiles=False):
    """The restatement's mean (H, W, 3) of one case, read-only: params is a dict (the one filter) or a (direct, indirect) pair (the split filter); tiles: through the
    per-tile restatements with chart.counts, else through the one-count ones with chart.counts[0] (the chart's counts are then all equal)."""
    split = isinstance(params, tuple)
    key = (chart.key, tiles, tuple(_freeze(p) for p in params) if split else _freeze(params))
    if key not in _references:
        assert tiles or len(set(chart.counts)) == 1
        n = chart.tile_samples if tiles else chart.counts[0]
        with np.errstate(all="ignore"):
            if split:
                fn = denoise_split_tiles if tiles else sr.denoise_split
                out = fn(chart.S, chart.D, chart.AC, chart.ND, n, direct=params[0], indirect=params[1])
            else:
                out = (denoise_tiles if tiles else dr.denoise)(chart.S, chart.AC, chart.ND, n, **params)
        out.setflags(write=False)
        _references[key] = out
    return _references[key]


def reach(params):
    """How far a pixel's value travels: 2 (2^L - 1), L the longer chain's of a split case"""
    return dr.radius(max(p["iterations"] for p in params) if isinstance(params, tuple) else params["iterations"])


def expected_bgra(mean, exposure):
    """The display texels of a mean image (H, W, 3): the oracle's tonemap of {mean, 1} with one accumulated sample; a NaN level is 0"""
    from oracle import orc
    rgba = np.concatenate([mean, np.ones(mean.shape[:2] + (1,), F32)], -1).astype(F32)
    with np.errstate(all="ignore"):
        return orc.tonemap_bgra8(rgba, 1, exposure).reshape(mean.shape[:2])


def mismatches(got, want, chart=None, what=None, limit=5):
    """The comparison rule: f32 results match where their bits are equal or both are NaN (a NaN's sign and payload are not compared; +-inf, +-0 and denormals are).
    -> a list of up to `limit` reports (what, class, (y, x, channel), got, want), empty when everything matches."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return [(what, chart.label(i[0], i[1]) if chart is not None else None, tuple(int(k) for k in i), float(got[tuple(i)]), float(want[tuple(i)]))
            for i in np.argwhere(~same)[:limit]]


# ---------------------------------------------------------------------------------- the checks
def _prep(chart, split):
    """The restatements' own prep of the chart: the one-count ones' where the chart has one count, the per-tile ones' otherwise"""
    one = len(set(chart.counts)) == 1
    with np.errstate(all="ignore"):
        if split:
            c, eD, eI, n, z, a_eps, bg = (sr.split_prep(chart.S, chart.D, chart.AC, chart.ND, chart.counts[0]) if one else
                                          split_prep_tiles(chart.S, chart.D, chart.AC, chart.ND, chart.tile_samples))
            return dict(c=c, eD=eD, eI=eI, n=n, z=z, a_eps=a_eps, bg=bg)
        c, e, lum, n, z, a_eps, bg = dr.prep(chart.S, chart.AC, chart.ND, chart.counts[0]) if one else prep_tiles(chart.S, chart.AC, chart.ND, chart.tile_samples)
        nf = pixel_counts(chart.tile_samples, H, W)[..., None]
        m = chart.ND[..., :3] / nf
        d = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
    return dict(c=c, e=e, lum=lum, n=n, z=z, a_eps=a_eps, bg=bg, d=d)


def _promised(state, s, at):
    """Does prep's output s show `state` at pixel `at`?"""
    y, x = at
    with np.errstate(all="ignore"):
        length = float(np.sqrt((s["n"][y, x].astype(np.float64) ** 2).sum()))
        if state == "bg":
            return bool(s["bg"][y, x])
        if s["bg"][y, x]:
            return False
        return {"e denormal": lambda: (np.abs(s["e"][y, x]) > 0).all() and (np.abs(s["e"][y, x]) < FLT_MIN).all(),
                "e -0": lambda: (s["e"][y, x] == 0).all() and np.signbit(s["e"][y, x]).all(),
                "e negative": lambda: (s["e"][y, x] < 0).all(),
                "e large": lambda: (s["e"][y, x] > 1e29).all() and np.isfinite(s["lum"][y, x]),
                "l inf": lambda: np.isfinite(s["e"][y, x]).all() and s["lum"][y, x] == INF,
                "a_eps == eps": lambda: (s["a_eps"][y, x] == dr.EPS_A).all(),
                "d denormal": lambda: 0 < abs(s["d"][y, x]) < FLT_MIN and abs(length - 1) < 1e-5,
                "n == 0": lambda: (s["n"][y, x] == 0).all(),
                "n flipped": lambda: np.array_equal(s["n"][y, x], -s["n"][1, 1]) and abs(length - 1) < 1e-5,
                "z denormal": lambda: 0 < s["z"][y, x] < FLT_MIN,
                "z inf": lambda: s["z"][y, x] == INF,
                "z large": lambda: 1e37 < s["z"][y, x] < INF,
                "eI == 0": lambda: (s["eI"][y, x] == 0).all() and (s["eD"][y, x] > 0).all(),
                "eD == 0": lambda: (s["eD"][y, x] == 0).all() and not np.signbit(s["eD"][y, x]).any(),
                "eD -0": lambda: (s["eD"][y, x] == 0).all() and np.signbit(s["eD"][y, x]).all(),
                "eD denormal": lambda: (s["eD"][y, x] > 0).all() and (s["eD"][y, x] < FLT_MIN).all(),
                "eI negative": lambda: (s["eI"][y, x] < 0).all()}[state]()


def denormal_observability():
    """{denormal class: does the one filter's output differ, in some pixel's bits at L = 1 or 3, when the class is written as a flushing build would see it?}
    ("D denormal": the split filter's.)  A build that flushes denormals computes the flushed chart's result on the real chart: it cannot match where this is True."""
    out = {}
    for name in FLUSHED:
        split = name in SPLIT_CLASSES
        a, b = finite_chart(split), finite_chart(split, SIX, name)
        cases = [(dict(iterations=L), dict(iterations=L)) if split else dict(iterations=L) for L in (1, 3)]
        out[name] = any(bool(mismatches(reference(a, p), reference(b, p))) for p in cases)
    return out


def check_finite_chart(chart, cases, tiles=False):
    """The non-vacuity conditions of a finite chart; -> {class: pixels}, plus the observability of the denormal classes for the 6-sample charts."""
    split = "D = S" in chart.names
    counts = {name: int((chart.cls == i).sum()) for i, name in enumerate(chart.names)}
    assert min(counts.values()) >= 2, counts
    for at in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (15, 15), (16, 16), (31, 32), (32, 31)]:
        assert chart.cls[at] >= 0, at
    s = _prep(chart, False)
    ordinary_fg = (chart.cls < 0) & ~s["bg"]
    assert ordinary_fg[chart.cls < 0].all()
    for y, x in np.argwhere((chart.cls >= 0) & ~s["bg"]):
        for step in (1, 2, 4):
            near = [(y + dy, x + dx) for dy, dx in ((step, 0), (-step, 0), (0, step), (0, -step)) if 0 <= y + dy < H and 0 <= x + dx < W]
            assert any(ordinary_fg[q] for q in near), (chart.label(y, x), (y, x), step)
    if chart.counts == SIX:
        states = dict({k: v[1] for k, v in FINITE_CLASSES.items()}, **{k: v[1] for k, v in SPLIT_CLASSES.items()})
        ss = _prep(chart, True) if split else None
        for name in chart.names:
            for at in chart.pixels_of(name):
                assert _promised(states[name], ss if name in SPLIT_CLASSES else s, tuple(at)), (name, tuple(at), states[name])
        seen = denormal_observability()
        assert all(seen[k] for k in MUST_BE_OBSERVABLE), seen
        counts["observable denormal classes"] = sorted(k for k, v in seen.items() if v)
    for p in cases:
        ref = reference(chart, p, tiles)
        assert np.isfinite(ref).all(), (chart.key, p, [chart.label(y, x) for y, x in np.argwhere(~np.isfinite(ref).all(-1))[:5]])
    return counts


def check_poison_chart(chart, cases, tiles=False):
    """The non-vacuity conditions of a poison chart; -> {L (or (L_D, L_I)): non-finite pixels}.  With no pass at all the output is c = S / Nf by definition, so only a
    poisoned S shows; with one pass or more the poison must show somewhere, and nowhere beyond its reach."""
    at = np.argwhere(chart.cls >= 0)
    assert [tuple(a) for a in at] == sorted(POISON_AT) and len(chart.names) == 1
    ys, xs = np.mgrid[0:H, 0:W]
    distance = np.min([np.maximum(np.abs(ys - y), np.abs(xs - x)) for y, x in POISON_AT], 0)
    name = chart.names[0]
    if name == "albedo sum = -N 2^-8 in one channel":
        assert (_prep(chart, False)["a_eps"][tuple(at.T)][:, 0] == 0).all()
    out = {}
    for p in cases:
        ref = reference(chart, p, tiles)
        bad = ~np.isfinite(ref).all(-1)
        r = reach(p)
        depth = tuple(q["iterations"] for q in p) if isinstance(p, tuple) else p["iterations"]
        assert bad.mean() <= 0.25, (name, p, bad.mean())
        assert not bad[distance > r].any(), (name, p)
        if r > 0:
            assert bad.any(), (name, p)
        else:
            with np.errstate(all="ignore"):
                assert np.array_equal(bad, ~np.isfinite(chart.S[..., :3] / pixel_counts(chart.tile_samples, H, W)[..., None]).all(-1)), (name, p)
        out[depth] = max(out.get(depth, 0), int(bad.sum()))
    return out
