"""GPU: the shading kernels on the crafted inputs of tests/shade_charts.py -- UVs on the edges of textureLookup's index arithmetic (fract() * w rounding up to w: the
row wrap, the next texture, the clamp at the end of the texel array; NaN, infinite and huge UVs; column and row boundaries; texture sizes from 1x1 to 2048x2048),
vertex normals on the edges of normalize and of the orthonormal basis (|n|^2 zero, denormal, overflowing, NaN; n.z = -1 and -0.0; cancelling and back-facing normals),
and pixel sums on the flip points of the display transform.  Every comparison is bit or integer equality against the oracle, the restatement of the first-hit AOVs
(tests/aov_restatement.py) or the independent index arithmetic (shade_charts.texel_index); there is no tolerance.  tests/test_shade_charts.py shows on the CPU that
the charts reach the classes they are built for; the same conditions are asserted here on the oracle-side values that the device is compared with."""
import numpy as np
import pytest

import rayfinder_amd as rf
import shade_charts as sc
from conftest import bits
from oracle import orc

pytestmark = pytest.mark.gpu


def _aov_sums(r):
    s = r.read_aovs()
    return np.concatenate([s["albedo"], s["coverage"][..., None]], -1), np.concatenate([s["normal"], s["depth"][..., None]], -1), s["samples"]


def _render_and_compare(chart, bounces, options, batching, label):
    params, _ = chart.render_params(sc.N_FRAMES, bounces)
    want_img, want_stats = sc.oracle_render(chart, bounces)
    want_ac, want_nd = sc.expected_aov_sums(chart, bounces)
    sc.check_nan_share(want_img)
    r = rf.ReferencePathTracer(params, chart.pt.scene())
    for k, v in options.items():
        r.set_option(k, v)
    r.set_aovs(True)
    for n in batching:
        r.render(n)
    img, acc = r.read_accumulation()
    ac, nd, n_aov = _aov_sums(r)
    s = r.stats()
    r.close()
    assert acc == sc.N_FRAMES and n_aov == sc.N_FRAMES, label
    for name, got, want in (("albedo / coverage", ac, want_ac), ("normal / depth", nd, want_nd)):
        bad = np.argwhere((bits(got) != bits(want)).any(-1))
        assert bad.size == 0, (label, name, len(bad), [(int(x), int(y), got[y, x], want[y, x]) for y, x in bad[:4]])
    g, c = img[..., :3], want_img[..., :3]
    assert np.array_equal(np.isnan(g), np.isnan(c)), (label, "NaN pixels differ", int(np.isnan(g).sum()), int(np.isnan(c).sum()))
    bad = np.argwhere(((bits(g) != bits(c)) & ~np.isnan(g)).any(-1))
    assert bad.size == 0, (label, "radiance", len(bad), [(int(x), int(y), g[y, x], c[y, x]) for y, x in bad[:4]])
    assert s["closest_rays"] == want_stats["closestRays"] and s["shadow_rays"] == want_stats["shadowRays"], (label, s["closest_rays"], s["shadow_rays"], want_stats)
    assert s["abandoned_rays"] == 0, label


@pytest.mark.parametrize("layout", ["A", "B"])
def test_uv_chart_aovs_image_and_ray_counts_equal_the_oracle(layout):
    chart = sc.uv_chart(layout)
    print(f"UV chart, layout {layout}:", sc.check_uv_classes(chart, layout))
    # the albedo sums this test compares with come from texels that the independent index arithmetic names too
    for fa in sc.first_hits(chart):
        assert np.array_equal(sc.texel_index(chart, fa["tex"], fa["uvx"], fa["uvy"])[0], fa["texel"])
    for options in ({}, dict(shade_sort_from_bounce=0), dict(accumulate_runs=0)):
        for batching in ((2,), (1, 1)):
            _render_and_compare(chart, 3, options, batching, (layout, options, batching))


def test_uv_chart_through_the_deferred_variant():
    chart = sc.uv_chart("A")
    W, H = sc.FRAME
    params, rp = chart.render_params(1, 2)
    r = rf.ReferencePathTracer(params, chart.pt.scene())
    r.reset_deferred()
    r.render_deferred(1)
    sample, accum, bgra, n = r.read_deferred()
    s = r.stats()
    r.close()
    assert n == 1
    with np.errstate(all="ignore"):
        ws, wa, wsrgb, st = orc.deferred_frames(chart.scene, rp, 1)
    assert sc.check_nan_share(ws) == 0.0                  # (the UV chart has ordinary normals: the compare below is over every pixel)
    assert st.texelOobClamps > 0                          # the clamp case is among the G-buffer's texels
    assert np.array_equal(bits(sample), bits(ws))
    assert np.array_equal(bits(accum), bits(wa))
    want = orc.quantise_unorm8(wsrgb)
    got = np.stack([(bgra >> 16) & 255, (bgra >> 8) & 255, bgra & 255], axis=-1)
    assert np.array_equal(got, want) and ((bgra >> 24) == 255).all()
    assert s["closest_rays"] == st.closestRays and s["shadow_rays"] == st.shadowRays and s["abandoned_rays"] == 0


@pytest.mark.parametrize("options", [{}, dict(shadow_self_test=0, quad_from_bounce=0)], ids=["default", "no_self_test_no_quad"])
def test_normal_chart_aovs_image_and_ray_counts_equal_the_oracle(options):
    chart = sc.normal_chart()
    print("normal chart:", sc.check_normal_classes(chart))
    _render_and_compare(chart, sc.NORMAL_BOUNCES, options, (2,), ("normal chart", options))


@pytest.mark.parametrize("pair", range(len(sc.TONEMAP_PAIRS)))
def test_tonemap_on_flip_points_and_special_values(pair):
    import torch
    samples, exposure = sc.TONEMAP_PAIRS[pair]
    chart = sc.normal_chart()                              # (any renderer: tonemap_device_image uses its exposure and nothing else)
    W, H = sc.FRAME
    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, chart.camera, 1, 1, rf.make_sky(), exposure), chart.pt.scene())
    for n in sc.TONEMAP_LENGTHS:
        rows, _, _ = sc.tonemap_inputs(pair, n)
        want = orc.tonemap_bgra8(rows, samples, exposure)
        if n >= 807:
            assert np.array_equal(np.unique(np.concatenate([(want >> s) & 255 for s in (0, 8, 16)])), np.arange(256))    # every level, oracle side
        t = torch.from_numpy(rows).to("cuda")
        got = r.tonemap_device_image(t.data_ptr(), n, 1, samples).reshape(-1)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (samples, exposure, n, len(bad), [(rows[b], hex(got[b]), hex(want[b])) for b in bad[:5]])
        assert np.array_equal(t.cpu().numpy().view(np.uint32), rows.view(np.uint32)), "the input tensor changed"
    r.close()
