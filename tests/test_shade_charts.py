"""CPU: the charts of tests/shade_charts.py are not vacuous (every edge class they are built for occurs among the oracle's own first-hit samples, NaN pixels
stay a minority), and a restatement of the texel index in plain numpy agrees with the oracle's textureLookup on every one of those samples.
tests/test_gpu_shade_edges.py runs the device on the same inputs."""
import numpy as np
import pytest

import shade_charts as sc
from oracle import orc


@pytest.mark.parametrize("layout", ["A", "B"])
def test_independent_texel_index_equals_the_oracles_lookup(layout):
    chart = sc.uv_chart(layout)
    n = 0
    for fa in sc.first_hits(chart):
        at = sc.texel_index(chart, fa["tex"], fa["uvx"], fa["uvy"])[0]
        bad = np.flatnonzero(at != fa["texel"])
        assert bad.size == 0, (layout, [(chart.names[fa["quad"][b]], fa["uvx"][b], fa["uvy"][b], int(at[b]), int(fa["texel"][b])) for b in bad[:5]])
        n += at.size
    print(f"layout {layout}: {n} first-hit samples, texel index == oracle on all")
    assert n > 0.7 * 2 * sc.FRAME[0] * sc.FRAME[1]


@pytest.mark.parametrize("layout", ["A", "B"])
def test_uv_chart_reaches_every_class(layout):
    chart = sc.uv_chart(layout)
    assert len(chart.names) == 77 and (np.bincount(chart.tri_quad[chart.tri_quad >= 0]) == 2).all() and (chart.tri_quad < 0).sum() == 4
    counts = sc.check_uv_classes(chart, layout)
    img = sc.oracle_render(chart)[0]
    counts["NaN pixel share"] = sc.check_nan_share(img)
    print(f"UV chart, layout {layout}:", counts)
    # every texture of the set is read
    used = {chart.quad_tex[q] for fa in sc.first_hits(chart) for q in np.unique(fa["quad"]) if q >= 0}
    assert used == set(sc.TEXTURE_SIZES)


def test_normal_chart_reaches_every_class():
    chart = sc.normal_chart()
    counts = sc.check_normal_classes(chart)
    print("normal chart:", counts)
    # every quad is seen by at least 6 x 6 pixels' worth of samples in each frame
    for fa in sc.first_hits(chart, sc.NORMAL_BOUNCES):
        assert (np.bincount(fa["quad"][fa["quad"] >= 0], minlength=len(chart.names)) >= 36).all()


def test_uv_chart_quads_cover_six_by_six_pixels():
    chart = sc.uv_chart("A")
    for fa in sc.first_hits(chart):
        assert (np.bincount(fa["quad"][fa["quad"] >= 0], minlength=len(chart.names)) >= 36).all()
        assert (fa["quad"] < 0).sum() >= 36                  # floor and fin are in the frame
    # the sums the GPU tests compare with (built from the attributes above) are aov_restatement.aov_sums
    from aov_restatement import aov_sums
    from conftest import bits
    want = aov_sums(chart.scene, chart.render_params(sc.N_FRAMES, 3)[1], range(sc.N_FRAMES))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(sc.expected_aov_sums(chart), want))


@pytest.mark.parametrize("pair", range(len(sc.TONEMAP_PAIRS)))
def test_tonemap_list_covers_every_level_and_sits_on_the_flip_points(pair):
    rows, samples, exposure = sc.tonemap_inputs(pair)
    flips = sc.flip_points(samples, exposure)
    k = np.arange(1, 256)
    assert (sc.oracle_levels(flips, samples, exposure) == k).all()
    below = np.array([sc.step(f, -1) for f in flips], np.float32)
    assert (sc.oracle_levels(below, samples, exposure) == k - 1).all()
    bgra = orc.tonemap_bgra8(rows, samples, exposure)
    levels = np.unique(np.concatenate([(bgra >> s) & 255 for s in (0, 8, 16)]))
    assert np.array_equal(levels, np.arange(256)) and ((bgra >> 24) == 255).all()
    print(f"tonemap list for (samples, exposure) = ({samples}, {exposure}): {len(rows)} entries")
    assert np.isnan(rows[:, :3]).any() and np.isinf(rows[:, :3]).any() and np.isnan(rows[:, 3]).any()
    # .w does not matter to the reference either
    other = rows.copy()
    other[:, 3] = 1.0
    assert np.array_equal(orc.tonemap_bgra8(other, samples, exposure), bgra)
    for n in sc.TONEMAP_LENGTHS:
        assert sc.tonemap_inputs(pair, n)[0].shape == (n, 4)


def test_documented_choices_for_nan():
    """A NaN or infinite uv reads texel (0,0) of its texture; a NaN display value is level 0."""
    chart = sc.uv_chart("B")
    for name, (idx, w, h, off) in chart.textures.items():
        for uv in ((np.nan, 0.3), (0.3, np.inf), (-np.inf, np.nan)):
            got = sc.decode_texel(orc.texture_lookup(chart.scene, idx, *uv)[None])[0]
            j = int(np.float32(uv[0]) * np.float32(w)) if np.isfinite(uv[0]) else 0
            i = int(np.float32(uv[1]) * np.float32(h)) if np.isfinite(uv[1]) else 0
            assert got == off + i * w + j, (name, uv, got)
    assert np.array_equal(orc.quantise_unorm8(np.array([np.nan, 0.0, 1.0, 0.5], np.float32)), [0, 0, 255, 128])
