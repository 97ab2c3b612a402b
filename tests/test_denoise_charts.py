"""CPU: the charts of tests/denoise_charts.py are not vacuous (every special class occurs, prep puts it in the state its name promises, every denormal class that
counts is observable, the finite charts stay finite and the poison charts stay mostly finite under every case the GPU tests run), and the f32 restatements the
GPU tests compare with agree with a plain f64 evaluation written from include/rayfinder_amd.h alone.  tests/test_gpu_denoise_edges.py runs the device on the same
inputs."""
import numpy as np
import pytest

import denoise_charts as dc
import denoise_restatement as dr
import split_restatement as sr
from denoise_tiles_restatement import pixel_counts
from test_gpu_split import _synthetic

FINITE_CHARTS = [(dc.SIX, False), (dc.SIX, True), (dc.TILE_COUNTS[0], True), (dc.TILE_COUNTS[1], True)]     # (counts, through the per-tile restatement)


# ---------------------------------------------------------------------------------- the charts
@pytest.mark.parametrize("split", [False, True], ids=["one filter", "split"])
def test_finite_charts_reach_every_class_and_stay_finite(split):
    cases = (dc.SPLIT_CASES + dc.SPLIT_EXTREMES) if split else dc.FINITE_CASES
    for counts, tiles in FINITE_CHARTS:
        got = dc.check_finite_chart(dc.finite_chart(split, counts), cases, tiles)
        print(f"finite chart, split {split}, counts {counts}, per tile {tiles}: {len(cases)} cases finite;", got)
    # the sample-count charts of the one-count entry points
    for n in dc.SAMPLE_COUNTS:
        dc.check_finite_chart(dc.finite_chart(split, (n,) * 4), dc.COUNT_SPLIT_CASES if split else dc.COUNT_CASES)
    all_equal = dc.finite_chart(split, (2 ** 24 + 1,) * 4)
    dc.check_finite_chart(all_equal, dc.COUNT_SPLIT_CASES if split else dc.COUNT_CASES, tiles=True)
    if split:
        seen = {inst for pd, pi in dc.SPLIT_CASES for inst in dc.split_instantiations(pd, pi)}
        assert seen == {(True, True, True), (True, True, False), (True, False, False), (False, True, False)}, seen


@pytest.mark.parametrize("split", [False, True], ids=["one filter", "split"])
def test_poison_charts_show_the_poison_and_keep_it_within_reach(split):
    cases = dc.POISON_SPLIT_CASES if split else dc.POISON_CASES
    assert max(dc.reach(p) for p in cases) == 6                              # at most two passes (of either component)
    for name in dc.poison_classes(split):
        for counts, tiles in ((dc.SIX, False), (dc.TILE_COUNTS[1], True)):
            got = dc.check_poison_chart(dc.poison_chart(name, split, counts), cases, tiles)
            print(f"poison chart '{name}', split {split}, counts {counts}: non-finite pixels of {dc.H * dc.W} by depth", got)
            assert max(got.values()) <= 218                                   # both pixels' whole reach at two passes: 13 x 13 + 7 x 7


def test_the_denormal_classes_are_observable():
    """A build that flushes denormals would compute, on the real chart, what the restatement computes on the flushed one: where the two differ it cannot pass."""
    seen = dc.denormal_observability()
    print("output changes when the class is flushed:", seen)
    assert all(seen[k] for k in dc.MUST_BE_OBSERVABLE) and sum(seen.values()) >= 3, seen


def test_the_comparison_rule():
    f = np.float32
    a = np.array([[[f(np.nan), f(0.0), f(np.inf)], [f(1e-40), f(1.0), f(-1.0)]]], f)
    b = a.copy()
    b.view(np.uint32)[0, 0, 0] ^= 0x80000001                                   # another NaN: sign and payload are not compared
    assert np.isnan(b[0, 0, 0]) and not dc.mismatches(a, b)
    for at, value in (((0, 0, 0), f(0.0)), ((0, 0, 1), f(-0.0)), ((0, 0, 2), f(-np.inf)), ((0, 1, 0), f(0.0)), ((0, 1, 1), f(np.nan)), ((0, 1, 2), np.nextafter(f(-1), f(0)))):
        c = a.copy()
        c[at] = value
        got = dc.mismatches(c, a, what="L")
        assert len(got) == 1 and got[0][0] == "L" and got[0][2] == at, (at, got)


def test_sample_counts_round_as_the_devices_conversion():
    want = {2 ** 24 + 1: 16777216.0, 2 ** 24 + 3: 16777220.0, 2 ** 32 - 1: 4294967296.0, 1: 1.0, 3: 3.0}
    for n, nf in want.items():
        assert float(pixel_counts(np.array([n], np.uint32), 1, 1)[0, 0]) == nf
        # prep divides by F(samples): S = Nf gives c = 1 exactly, and the neighbouring floats do not
        S = np.zeros((1, 3, 4), np.float32)
        S[0, :, :3] = np.array([np.nextafter(np.float32(nf), 0), nf, np.nextafter(np.float32(nf), np.inf)], np.float32)[:, None]
        c = dr.prep(S, np.ones((1, 3, 4), np.float32), np.ones((1, 3, 4), np.float32), n)[0]
        assert (c[0, 1] == 1).all() and ((c[0, 0] < 1).all() or nf == 1) and (c[0, 2] > 1).all(), (n, c)
    assert set(dc.SAMPLE_COUNTS) <= set(want) and set(dc.TILE_COUNTS[0]) | set(dc.TILE_COUNTS[1]) <= set(want) | {6}


def test_smallest_sigma_normal_that_keeps_the_finite_chart_finite():
    """Recorded, not a property of the kernels: 1 - n.n' of two equal unit normals is slightly negative, so a tiny sigma_normal makes the Tukey weight overflow.  The
    GPU cases use 2^-20 and larger."""
    chart = dc.finite_chart()
    finite = lambda k: bool(np.isfinite(dc.reference(chart, dict(iterations=8, sigma_normal=2.0 ** -k))).all())    # noqa: E731
    k = 1
    while k < 126 and finite(k + 1):
        k += 1
    print(f"the finite chart's reference at L = 8 is all finite down to sigma_normal = 2^-{k}, and not at 2^-{k + 1}")
    assert k >= 20


# ---------------------------------------------------------------------------------- the restatements against f64
# Written from the header's text ("Edge-aware a-trous denoiser", "Split-component denoiser"): Python floats, loops over pixels and taps, two ping-pong images.
EPS_A = EPS_L = 2.0 ** -8
KERNEL = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def _tukey(x):
    return (1 - x) * (1 - x) if x < 1 else 0.0


def _f64_prep(S, AC, ND, N):
    """-> per pixel: c, background, n, z, a + eps_a (lists of rows of tuples / floats)"""
    H, W = len(S), len(S[0])
    c = [[tuple(S[y][x][k] / N for k in range(3)) for x in range(W)] for y in range(H)]
    bg = [[True] * W for _ in range(H)]
    n = [[(0.0, 0.0, 0.0)] * W for _ in range(H)]
    z = [[0.0] * W for _ in range(H)]
    ae = [[(0.0, 0.0, 0.0)] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if AC[y][x][3] == 0 or not ND[y][x][3] / AC[y][x][3] > 0:
                continue
            bg[y][x] = False
            z[y][x] = ND[y][x][3] / AC[y][x][3]
            m = [ND[y][x][k] / N for k in range(3)]
            d = m[0] * m[0] + m[1] * m[1] + m[2] * m[2]
            n[y][x] = tuple(v / d ** 0.5 for v in m) if d != 0 else (0.0, 0.0, 0.0)
            ae[y][x] = tuple(AC[y][x][k] / N + EPS_A for k in range(3))
    return c, bg, n, z, ae


def _f64_passes(e, bg, n, z, L, sc, sn, sz):
    """L iterations over the image e (rows of 3-tuples); background pixels keep e"""
    H, W = len(e), len(e[0])
    for i in range(L):
        s = 2 ** i
        out = [row[:] for row in e]
        for y in range(H):
            for x in range(W):
                if bg[y][x]:
                    continue
                ep, lp = e[y][x], sum(e[y][x])
                sum_w, sum_e = 0.0, [0.0, 0.0, 0.0]
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qy, qx = y + s * dy, x + s * dx
                        if not (0 <= qy < H and 0 <= qx < W) or bg[qy][qx]:
                            continue
                        eq = e[qy][qx]
                        w = KERNEL[dx + 2] * KERNEL[dy + 2]
                        if dx or dy:
                            xc = sum((eq[k] - ep[k]) ** 2 for k in range(3)) / (sc * sc * 2.0 ** -i * (lp * lp + EPS_L))
                            xn = (1 - sum(n[y][x][k] * n[qy][qx][k] for k in range(3))) / sn
                            xz = abs(z[qy][qx] - z[y][x]) / (sz * s * z[y][x])
                            w = w * _tukey(xc) * _tukey(xn) * _tukey(xz)
                        sum_w += w
                        for k in range(3):
                            sum_e[k] += w * eq[k]
                out[y][x] = tuple(v / sum_w for v in sum_e)
        e = out
    return e


def _lists(*arrays):
    return [np.asarray(a, np.float64).tolist() for a in arrays]


def f64_denoise(S, AC, ND, N, iterations, sigma_color, sigma_normal, sigma_depth):
    S, AC, ND = _lists(S, AC, ND)
    H, W = len(S), len(S[0])
    c, bg, n, z, ae = _f64_prep(S, AC, ND, N)
    if iterations == 0:
        return np.array(c)
    e = [[c[y][x] if bg[y][x] else tuple(c[y][x][k] / ae[y][x][k] for k in range(3)) for x in range(W)] for y in range(H)]
    e = _f64_passes(e, bg, n, z, iterations, sigma_color, sigma_normal, sigma_depth)
    return np.array([[c[y][x] if bg[y][x] else tuple(e[y][x][k] * ae[y][x][k] for k in range(3)) for x in range(W)] for y in range(H)])


def f64_denoise_split(S, D, AC, ND, N, direct, indirect):
    S, D, AC, ND = _lists(S, D, AC, ND)
    H, W = len(S), len(S[0])
    c, bg, n, z, ae = _f64_prep(S, AC, ND, N)
    if direct["iterations"] == 0 and indirect["iterations"] == 0:
        return np.array(c)
    eD = [[c[y][x] if bg[y][x] else tuple(D[y][x][k] / N / ae[y][x][k] for k in range(3)) for x in range(W)] for y in range(H)]
    eI = [[(0.0, 0.0, 0.0) if bg[y][x] else tuple((S[y][x][k] - D[y][x][k]) / N / ae[y][x][k] for k in range(3)) for x in range(W)] for y in range(H)]
    eD = _f64_passes(eD, bg, n, z, direct["iterations"], direct["sigma_color"], direct["sigma_normal"], direct["sigma_depth"])
    eI = _f64_passes(eI, bg, n, z, indirect["iterations"], indirect["sigma_color"], indirect["sigma_normal"], indirect["sigma_depth"])
    return np.array([[c[y][x] if bg[y][x] else tuple((eD[y][x][k] + eI[y][x][k]) * ae[y][x][k] for k in range(3)) for x in range(W)] for y in range(H)])


# The largest error of the f32 restatements against the f64 evaluation over the cases below, relative to |ref| + 2^-8 over covered pixels, measured with
# numpy 2.x on x86-64: MEASURED_F32_ERROR.  The tolerance is 8 times that, rounded up to one significant digit (other numpy builds keep the order of every
# sum; their sqrt may differ).
MEASURED_F32_ERROR = 1.114e-05                            # (the one filter, L = 1, the custom sigmas; the other seven cases: 1.1e-06 .. 5.3e-06)
F32_TOLERANCE = 9e-05


def test_restatements_agree_with_an_independent_f64_evaluation():
    Hh, Ww, N = 17, 20, 6
    S, D, AC, ND = _synthetic(Hh, Ww, N, 1720)
    covered = AC[..., 3] > 0
    edges = lambda a: len(np.unique(np.round(a[covered], 1), axis=0)) > 1     # noqa: E731
    with np.errstate(invalid="ignore"):
        assert covered.any() and not covered.all() and edges(ND[..., :3] / AC[..., 3:]) and edges(ND[..., 3] / AC[..., 3]) and edges(AC[..., :3] / AC[..., 3:])
    worst = 0.0

    def error(got, ref, what):
        nonlocal worst
        err = float((np.abs(got.astype(np.float64) - ref) / (np.abs(ref) + 2.0 ** -8))[covered].max())
        print(f"{what}: f32 restatement against f64, largest relative error {err:.3e}")
        worst = max(worst, err)
        assert err <= F32_TOLERANCE, (what, err)

    for sig in dc.SIGMAS:
        full = dict(dr.DEFAULTS, **sig)
        for L in (1, 3):
            p = dict(full, iterations=L)
            error(dr.denoise(S, AC, ND, N, **p), f64_denoise(S, AC, ND, N, **p), ("one filter", L, sig))
        for ld, li in ((1, 3), (3, 1)):
            pd, pi = dict(sr.DIRECT_DEFAULTS, **sig, iterations=ld), dict(sr.INDIRECT_DEFAULTS, **sig, iterations=li)
            error(sr.denoise_split(S, D, AC, ND, N, direct=pd, indirect=pi), f64_denoise_split(S, D, AC, ND, N, pd, pi), ("split", ld, li, sig))
    print(f"largest over all cases: {worst:.3e} (recorded {MEASURED_F32_ERROR:.3e}, tolerance {F32_TOLERANCE:.0e})")
