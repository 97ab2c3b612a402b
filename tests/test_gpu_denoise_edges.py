"""The a-trous denoisers on crafted special values and frame edges (-m gpu): rf_denoise_images, rf_denoise_tiles, rf_denoise_split_images and rf_denoise_split_tiles
against the numpy restatements on the charts of tests/denoise_charts.py (tests/test_denoise_charts.py shows on the CPU that the charts reach what they are built
for) -- denormals, signed zeros, sums that overflow or underflow on the way, every rule that makes a pixel background, NaN and infinities within reach of a
shallow filter, sample counts that float() rounds, sigmas whose squares and products leave the f32 range -- and on ordinary inputs in frames of one row, one
column, exactly one workgroup and one pixel more or less.  Every comparison is bit for bit, NaN against NaN, and the display texels are the oracle's tonemap of
the restatement's mean."""
import numpy as np
import pytest

import denoise_charts as dc
import rayfinder_amd as rf
from denoise_restatement import denoise
from denoise_tiles_restatement import denoise_tiles, pixel_counts
from split_restatement import denoise_split
from split_tiles_restatement import denoise_split_tiles
from test_gpu_split import _synthetic

pytestmark = pytest.mark.gpu
EXPOSURES = (0.25, 1.0)


def _device(chart, params, tiles, exposure):
    if isinstance(params, tuple):
        if tiles:
            return rf.denoise_split_tiles(chart.S, chart.D, chart.AC, chart.ND, chart.tile_samples, exposure=exposure, direct=params[0], indirect=params[1])
        return rf.denoise_split_images(chart.S, chart.D, chart.AC, chart.ND, chart.counts[0], exposure=exposure, direct=params[0], indirect=params[1])
    if tiles:
        return rf.denoise_tiles(chart.S, chart.AC, chart.ND, chart.tile_samples, exposure=exposure, **params)
    return rf.denoise_images(chart.S, chart.AC, chart.ND, chart.counts[0], exposure=exposure, **params)


def _compare(chart, cases, tiles):
    """Every case through the entry point and through the restatement: the mean by the comparison rule, finite wherever the reference is, and the display texels"""
    for k, params in enumerate(cases):
        exposure = EXPOSURES[k % 2]
        rgb, bgra = _device(chart, params, tiles, exposure)
        want = dc.reference(chart, params, tiles)
        bad = dc.mismatches(rgb, want, chart, (params, "per tile" if tiles else "one count", chart.counts))
        assert not bad, bad
        assert np.isfinite(rgb[np.isfinite(want)]).all()
        texels = dc.expected_bgra(want, exposure)
        off = np.argwhere(bgra != texels)
        assert off.size == 0, (params, exposure, [(chart.label(y, x), (int(y), int(x)), hex(bgra[y, x]), hex(texels[y, x]), want[y, x].tolist()) for y, x in off[:5]])


# ---------------------------------------------------------------------------------- a. the finite charts
ENTRIES = [(dc.SIX, False), (dc.SIX, True), (dc.TILE_COUNTS[0], True), (dc.TILE_COUNTS[1], True)]
ENTRY_IDS = ["one count", "per tile, all 6", "per tile, 1 3 2^24+1 2^32-1", "per tile, 6 6 6 2^24+3"]


@pytest.mark.parametrize("counts,tiles", ENTRIES, ids=ENTRY_IDS)
def test_finite_chart_through_the_one_filter(counts, tiles):
    chart = dc.finite_chart(False, counts)
    assert np.isfinite(dc.reference(chart, dc.FINITE_CASES[8], tiles)).all() and len(dc.FINITE_CASES) == 18 + 10 * 3
    _compare(chart, dc.FINITE_CASES, tiles)


@pytest.mark.parametrize("counts,tiles", ENTRIES, ids=ENTRY_IDS)
def test_finite_chart_through_the_split_filter(counts, tiles):
    chart = dc.finite_chart(True, counts)
    reached = {inst for pd, pi in dc.SPLIT_CASES for inst in dc.split_instantiations(pd, pi)}
    assert reached == {(True, True, True), (True, True, False), (True, False, False), (False, True, False)}, reached      # <DIRECT, INDIRECT, SHARED>
    assert set(dc.split_instantiations(*dc.SPLIT_CASES[3])) == {(True, True, True), (False, True, False)}                  # (1, 5), the same sigmas
    assert set(dc.split_instantiations(*dc.SPLIT_CASES[2 * len(dc.PAIRS) + 4])) == {(True, True, False)}                   # (5, 5), mixed sigmas
    _compare(chart, dc.SPLIT_CASES + dc.SPLIT_EXTREMES, tiles)


# ---------------------------------------------------------------------------------- b. the poison charts
@pytest.mark.parametrize("cls", dc.poison_classes(False))
def test_poison_chart_through_the_one_filter(cls):
    for counts, tiles in ((dc.SIX, False), (dc.TILE_COUNTS[1], True)):
        chart = dc.poison_chart(cls, False, counts)
        assert max(dc.check_poison_chart(chart, dc.POISON_CASES, tiles).values()) > 0
        _compare(chart, dc.POISON_CASES, tiles)


@pytest.mark.parametrize("cls", dc.poison_classes(True))
def test_poison_chart_through_the_split_filter(cls):
    for counts, tiles in ((dc.SIX, False), (dc.TILE_COUNTS[1], True)):
        chart = dc.poison_chart(cls, True, counts)
        assert max(dc.check_poison_chart(chart, dc.POISON_SPLIT_CASES, tiles).values()) > 0
        _compare(chart, dc.POISON_SPLIT_CASES, tiles)


# ---------------------------------------------------------------------------------- c. the sample counts
@pytest.mark.parametrize("samples", dc.SAMPLE_COUNTS)
def test_finite_chart_at_sample_counts_the_conversion_rounds(samples):
    for split, cases in ((False, dc.COUNT_CASES), (True, dc.COUNT_SPLIT_CASES)):
        _compare(dc.finite_chart(split, (samples,) * 4), cases, False)


def test_equal_tile_counts_of_2_to_the_24_plus_1_give_the_one_count_bits():
    n = 2 ** 24 + 1
    for split, cases in ((False, dc.COUNT_CASES), (True, dc.COUNT_SPLIT_CASES)):
        chart = dc.finite_chart(split, (n,) * 4)
        for params in cases:
            one, per_tile = _device(chart, params, False, 0.25), _device(chart, params, True, 0.25)
            assert not dc.mismatches(per_tile[0], one[0], chart, params) and np.array_equal(per_tile[1], one[1])
            assert not dc.mismatches(one[0], dc.reference(chart, params, False), chart, params)


# ---------------------------------------------------------------------------------- d. the frame shapes
SHAPES = [(1, 40), (33, 1), (2, 2), (5, 3), (16, 16), (15, 17), (17, 15), (32, 32), (33, 31), (1, 300), (300, 1)]
TILED_SHAPES = [(33, 31), (1, 300), (300, 1)]
SHAPE_PAIRS = ((1, 5), (5, 5), (8, 2))


def _same(got, want, what):
    bad = dc.mismatches(got, want, None, what)
    assert not bad, bad


@pytest.mark.parametrize("h,w", SHAPES)
def test_frame_shapes(h, w):
    n = 6
    S, D, AC, ND = _synthetic(h, w, n, h * 1000 + w)
    for sig in dc.SIGMAS:
        for L in range(9):                                                    # the step passes the frame's size in one or both dimensions
            rgb, _ = rf.denoise_images(S, AC, ND, n, exposure=0.25, iterations=L, **sig)
            _same(rgb, denoise(S, AC, ND, n, iterations=L, **sig), (h, w, L, sig))
    for sd, si in dc.SPLIT_SIGMAS[:3:2]:
        for ld, li in SHAPE_PAIRS:
            pd, pi = dict(sd, iterations=ld), dict(si, iterations=li)
            rgb, _ = rf.denoise_split_images(S, D, AC, ND, n, exposure=0.25, direct=pd, indirect=pi)
            _same(rgb, denoise_split(S, D, AC, ND, n, direct=pd, indirect=pi), (h, w, pd, pi))


@pytest.mark.parametrize("h,w", TILED_SHAPES)
def test_frame_shapes_with_one_count_per_tile(h, w):
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    counts = (np.arange(tiles) % 9 + 1).astype(np.uint32)                     # 1 .. 9, cycling
    scale = (pixel_counts(counts, h, w) / np.float32(6))[..., None]
    S, D, AC, ND = ((a * scale).astype(np.float32) for a in _synthetic(h, w, 6, h * 1000 + w))
    for sig in dc.SIGMAS:
        for L in range(9):
            rgb, _ = rf.denoise_tiles(S, AC, ND, counts, exposure=0.25, iterations=L, **sig)
            _same(rgb, denoise_tiles(S, AC, ND, counts, iterations=L, **sig), (h, w, L, sig))
    for sd, si in dc.SPLIT_SIGMAS[:3:2]:
        for ld, li in SHAPE_PAIRS:
            pd, pi = dict(sd, iterations=ld), dict(si, iterations=li)
            rgb, _ = rf.denoise_split_tiles(S, D, AC, ND, counts, exposure=0.25, direct=pd, indirect=pi)
            _same(rgb, denoise_split_tiles(S, D, AC, ND, counts, direct=pd, indirect=pi), (h, w, pd, pi))
