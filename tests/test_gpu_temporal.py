"""The temporal history on the GPU (-m gpu).  Every comparison is bits equal or both NaN; texels are the oracle's tonemap of the restatement's T.rgb.
rf_temporal_images over the crafted charts of tests/temporal_charts.py (row-major planes: kTemporalReproject<false>), and the handle over the Duck at 96 x 64 (its own
tile-major sums: kTemporalReproject<true>) through two commits and three views, against rf_temporal_images and tests/temporal_restatement.py over the handle's own reads."""
import json
import os

import numpy as np
import pytest

import rayfinder_amd as rf
import temporal_charts as tc
import temporal_restatement as tr
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
W, H, SPP, CAP, BOUNCES, EXPOSURE = 96, 64, 4, 64, 2, 0.25
MAX_PATHS = 8 * 6 * 1024                                                      # a batch of 8 samples of the frame's 6 tiles
VIEWS = (dict(position=(0.75, 1.0, -0.75), yaw_degrees=129.64, pitch_degrees=-13.73),
         dict(position=(0.62, 1.02, -0.86), yaw_degrees=123.0, pitch_degrees=-13.0),             # tests/test_temporal_restatement.py's step: every decision is taken
         dict(position=(0.5, 1.0, -0.95), yaw_degrees=116.0, pitch_degrees=-13.0))


# ---------------------------------------------------------------------------------- rf_temporal_images on the charts
@pytest.mark.parametrize("name", list(tc.all_charts()))
def test_temporal_images_equals_the_restatement_on_a_chart(name):
    chart = tc.all_charts()[name]
    T, G, info = tc.reference(chart)
    got = rf.temporal_images(chart.S, chart.AC, chart.ND, chart.samples, chart.camera, history=chart.history, exposure=EXPOSURE, **chart.params)
    assert got["samples"] == chart.samples and got["color"].shape == (chart.height, chart.width, 4)
    assert tc.mismatches(got["geometry"], G, "G") == []
    assert tc.mismatches(got["color"], T, "T") == []
    assert np.array_equal(got["bgra8"], tc.expected_bgra(T, EXPOSURE))
    if chart.finite:
        assert np.isfinite(got["color"]).all()


def test_outputs_may_be_null_and_no_history_is_the_plain_mean():
    import ctypes as C
    chart = tc.finite_charts()["no history"]
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    S, AC, ND = (np.ascontiguousarray(a) for a in (chart.S, chart.AC, chart.ND))
    cam = rf.camera_from_array(chart.camera)
    assert rf._ffi.lib.rf_temporal_images(0, tc.W, tc.H, tc.N, P(S), P(AC), P(ND), C.byref(cam), None, None, None, None, 1.0, None, None, None) == rf._ffi.RF_OK
    got = rf.temporal_images(chart.S, chart.AC, chart.ND, tc.N, chart.camera)
    assert np.array_equal(bits(got["color"][..., :3]), bits(chart.S[..., :3] / np.float32(tc.N))) and (got["color"][..., 3] == tc.N).all()


# ---------------------------------------------------------------------------------- the handle
def _params(view, w=W, h=H, exposure=EXPOSURE):
    return rf.make_render_parameters(w, h, rf.fly_camera(w, h, **VIEWS[view]), CAP, BOUNCES, rf.make_sky(), exposure)


def _camera(view, w=W, h=H):
    return rf.camera_to_array(rf.fly_camera(w, h, **VIEWS[view]))


def _renderer(pt, view=0, aovs=True, **kw):
    r = rf.ReferencePathTracer(_params(view), pt.scene(), max_paths_in_flight=MAX_PATHS, **kw)
    if aovs:
        r.set_aovs(True)
    return r


def _sums(r):
    """The handle's own reads as the restatement takes them: S, AC, ND (H, W, 4) and the count"""
    S, n = r.read_accumulation()
    a = r.read_aovs()
    return S, np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), n


def _state(r, denoised=True):
    """Everything the temporal calls must leave exactly as it was"""
    S, AC, ND, n = _sums(r)
    st = r.stats()
    out = dict(S=bits(S), AC=bits(AC), ND=bits(ND), n=n, aov_samples=r.read_aovs()["samples"], tonemapped=r.read_tonemapped(), digest=r.state_digest(), tiles=r.read_tile_samples(),
               rays=(st["primary_rays"], st["closest_rays"], st["shadow_rays"], st["batches_traced"]))
    if denoised:
        rgb, bgra, m = r.read_denoised()
        out.update(denoised=bits(rgb), denoised_bgra=bgra, denoised_n=m)
    return out


def _same(a, b):
    return [k for k in a if not (np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k])]


def _refused(call, *words):
    with pytest.raises(rf.RayfinderError) as e:
        call()
    assert e.value.status == INVALID, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def _check(got, want_T, want_G, samples, what):
    assert got["samples"] == samples, what
    assert tc.mismatches(got["geometry"], want_G, what + ": G") == []
    assert tc.mismatches(got["color"], want_T, what + ": T") == []
    assert np.array_equal(got["bgra8"], tc.expected_bgra(want_T, EXPOSURE)), what


@pytest.fixture(scope="module")
def flight(duck_pt):
    """One handle through three views and two commits; every step's reads, computed once"""
    r = _renderer(duck_pt)
    out = dict(memory_before=r.memory_info())
    r.render(SPP)
    r.denoise(iterations=2)                                                   # an earlier denoise snapshot, to be left alone
    out["memory_rendered"] = r.memory_info()
    before = _state(r)
    _refused(r.read_temporal, "no temporal result")
    _refused(r.temporal_commit, "no temporal result")
    # view A: no history yet
    r.temporal_accumulate()
    out["memory_after"] = r.memory_info()
    out["a"] = dict(sums=_sums(r), got=r.read_temporal(), untouched=_same(before, _state(r)))
    r.temporal_commit()
    _refused(r.read_temporal, "no temporal result")
    out["a"]["untouched"] += _same(before, _state(r))
    # view B over A's frame
    r.set_render_parameters(_params(1))
    r.render(SPP)
    before = _state(r, denoised=False)
    r.temporal_accumulate()
    out["b"] = dict(sums=_sums(r), got=r.read_temporal(), untouched=_same(before, _state(r, denoised=False)))
    # four more samples: the same history again, not the result just made
    r.render(SPP)
    r.denoise(iterations=1)
    before = _state(r)
    r.temporal_accumulate(max_history=3.0)
    out["b8_capped"] = dict(sums=_sums(r), got=r.read_temporal())
    r.temporal_accumulate()
    out["b8"] = dict(sums=_sums(r), got=r.read_temporal(), untouched=_same(before, _state(r)))
    r.temporal_commit()
    # view C over B's 8-sample result
    r.set_render_parameters(_params(2))
    r.render(SPP)
    before = _state(r, denoised=False)
    r.temporal_accumulate()
    out["c"] = dict(sums=_sums(r), got=r.read_temporal(), untouched=_same(before, _state(r, denoised=False)))
    r.denoise_temporal(temporal=dict(depth_tolerance=0.1), iterations=3, sigma_color=2.0)
    out["c_denoised"] = dict(got=r.read_temporal(), denoised=r.read_denoised())
    out["c"]["untouched"] += _same(before, _state(r, denoised=False))
    r.close()
    return out


def test_the_first_view_has_no_history(flight):
    S, AC, ND, n = flight["a"]["sums"]
    T, G = tr.reproject(S, AC, ND, n, _camera(0))
    _check(flight["a"]["got"], T, G, SPP, "view A")
    assert (T[..., 3] == SPP).all() and np.array_equal(bits(T[..., :3]), bits(S[..., :3] / np.float32(SPP)))
    assert flight["a"]["untouched"] == []


def test_the_second_view_takes_the_firsts_frame(flight):
    S, AC, ND, n = flight["b"]["sums"]
    hist = dict(color=flight["a"]["got"]["color"], geometry=flight["a"]["got"]["geometry"], camera=_camera(0))
    T, G, info = tr.reproject(S, AC, ND, n, _camera(1), hist, details=True)
    counts = dict(took=int(info["took"].sum()), depth=int(info["depth_rejected"].sum()), normal=int(info["normal_rejected"].sum()),
                  left=int((~info["bg"] & ~info["inside"]).sum()), background=int(info["bg"].sum()))
    assert min(counts.values()) >= 16, counts                                  # every decision is taken on the way
    _check(flight["b"]["got"], T, G, SPP, "view B")
    images = rf.temporal_images(S, AC, ND, n, _camera(1), history=hist, exposure=EXPOSURE)
    _check(images, T, G, SPP, "view B through rf_temporal_images")            # row-major and tile-major sources: the same bits
    assert flight["b"]["untouched"] == []


def test_more_samples_recompute_from_the_same_history(flight):
    S, AC, ND, n = flight["b8"]["sums"]
    assert n == 2 * SPP
    hist = dict(color=flight["a"]["got"]["color"], geometry=flight["a"]["got"]["geometry"], camera=_camera(0))
    T, G, info = tr.reproject(S, AC, ND, n, _camera(1), hist, details=True)
    _check(flight["b8"]["got"], T, G, 2 * SPP, "view B at 8 samples")
    # the count is 8 + he with he <= 4, A's own count: the first result (4 + he) was not counted again
    assert info["took"].sum() >= 1000 and float(T[..., 3].max()) <= 2 * SPP + SPP * (1 + 1e-6) and float(T[info["took"], 3].min()) > 2 * SPP
    T3, G3 = tr.reproject(S, AC, ND, n, _camera(1), hist, max_history=3.0)
    _check(flight["b8_capped"]["got"], T3, G3, 2 * SPP, "view B at 8 samples, max_history 3")
    assert (T3[info["took"], 3] == 2 * SPP + 3).all()
    assert flight["b8"]["untouched"] == []


def test_a_third_view_after_a_second_commit(flight):
    S, AC, ND, n = flight["c"]["sums"]
    hist = dict(color=flight["b8"]["got"]["color"], geometry=flight["b8"]["got"]["geometry"], camera=_camera(1))
    T, G, info = tr.reproject(S, AC, ND, n, _camera(2), hist, details=True)
    _check(flight["c"]["got"], T, G, SPP, "view C")
    assert info["took"].sum() >= 1000 and float(T[..., 3].max()) > SPP + 2 * SPP                     # B's history counts for more than its own 8 samples
    assert flight["c"]["untouched"] == []


def test_denoise_temporal_filters_the_temporal_result(flight):
    S, AC, ND, n = flight["c"]["sums"]
    hist = dict(color=flight["b8"]["got"]["color"], geometry=flight["b8"]["got"]["geometry"], camera=_camera(1))
    T, G = tr.reproject(S, AC, ND, n, _camera(2), hist, depth_tolerance=0.1)
    _check(flight["c_denoised"]["got"], T, G, SPP, "the snapshot denoise_temporal leaves")
    rgb, bgra, m = flight["c_denoised"]["denoised"]
    want = tr.denoise_temporal(T, AC, ND, n, iterations=3, sigma_color=2.0)
    assert m == SPP and np.array_equal(bits(rgb), bits(want))
    assert np.array_equal(bgra, tc.expected_bgra(want, EXPOSURE))
    assert not np.array_equal(bits(want), bits(T[..., :3]))


def test_a_handle_that_never_calls_the_entry_points_allocates_nothing_more(flight):
    """memory_info of the same handle -- Duck, 96 x 64, AOVs on, 4 samples in one batch, max_paths_in_flight given -- as the parent commit reported it
    (tests/golden/temporal_memory_parent.json), and what the first temporal_accumulate adds: two pairs of float4 planes and one u32 plane"""
    with open(os.path.join(GOLDEN, "temporal_memory_parent.json")) as f:
        parent = json.load(f)
    assert flight["memory_before"] == parent["created"] and flight["memory_rendered"] == parent["rendered"]
    grown = dict(flight["memory_rendered"], path_state_bytes=flight["memory_rendered"]["path_state_bytes"] + W * H * (4 * 16 + 4))
    assert flight["memory_after"] == grown


def _nonuniform(pt):
    """A handle in the non-uniform state with the AOVs kept per tile count.  A twin handle renders the same first four samples and its estimate gives the six tiles'
    errors at the one check that matters; the target lies between the third and the fourth of them, so three tiles stop at 4 samples and three go on to 8."""
    def fresh():
        r = _renderer(pt, aovs=False)
        r.set_moments(True)
        r.set_aovs(True, tile_counts=True)
        return r

    twin = fresh()
    twin.render(SPP)
    errors = np.sort((twin.noise_estimate()["tile_sum"] / np.float32(1024)).astype(np.float32))
    twin.close()
    assert errors.size == 6 and errors[2] < errors[3], errors
    r = fresh()
    r.render_adaptive(float((np.float64(errors[2]) + np.float64(errors[3])) / 2), SPP, 0, 2 * SPP)
    assert sorted(r.read_tile_samples().reshape(-1).tolist()) == [SPP] * 3 + [2 * SPP] * 3 and not r.tile_samples_uniform()
    return r


def test_each_refusal_keeps_the_state(duck_pt):
    # bad parameters, before the handle's state is looked at (this handle has the AOVs off)
    r = _renderer(duck_pt, aovs=False)
    for bad, word in ((dict(max_history=0.0), "max_history"), (dict(max_history=float("inf")), "max_history"), (dict(depth_tolerance=-1.0), "depth_tolerance"),
                      (dict(min_normal_dot=1.5), "min_normal_dot"), (dict(min_normal_dot=float("nan")), "min_normal_dot")):
        _refused(lambda: r.temporal_accumulate(**bad), word)
        _refused(lambda: r.denoise_temporal(temporal=bad), word)
    _refused(lambda: r.denoise_temporal(iterations=9), "iterations")
    # the AOVs off
    r.render(SPP)
    before = _state(r, denoised=False)
    _refused(r.temporal_accumulate, "temporal_accumulate needs the first-hit AOVs")
    _refused(r.denoise_temporal, "denoise_temporal needs the first-hit AOVs")
    # the AOVs turned on partway
    assert _same(before, _state(r, denoised=False)) == []
    r.set_aovs(True)
    r.render(SPP)
    before = _state(r, denoised=False)
    assert (before["n"], before["aov_samples"]) == (2 * SPP, SPP)
    _refused(r.temporal_accumulate, "the AOV sample count (4) differs from the accumulated sample count (8)")
    _refused(r.denoise_temporal, "differs")
    assert _same(before, _state(r, denoised=False)) == []
    # no sample
    r.set_render_parameters(_params(1))
    _refused(r.temporal_accumulate, "no sample has been accumulated")
    # a tile shard
    r.set_tile_shard(0, 2)
    r.render(SPP)
    before = _state(r, denoised=False)
    _refused(r.temporal_accumulate, "needs the whole frame: a tile shard is set", "rf_temporal_images")
    _refused(r.denoise_temporal, "tile shard")
    assert _same(before, _state(r, denoised=False)) == []
    _refused(r.read_temporal, "no temporal result")
    r.close()
    # the non-uniform state
    r = _nonuniform(duck_pt)
    before = _state(r, denoised=False)
    _refused(r.temporal_accumulate, "rf_renderer_temporal_accumulate: the tiles hold different sample counts")
    _refused(r.denoise_temporal, "rf_renderer_denoise_temporal: the tiles hold different sample counts")
    assert _same(before, _state(r, denoised=False)) == []
    r.close()


def test_a_refused_call_keeps_the_history_and_the_result(duck_pt):
    r = _renderer(duck_pt)
    r.render(SPP)
    r.temporal_accumulate()
    first = r.read_temporal()
    _refused(lambda: r.temporal_accumulate(max_history=-1.0), "max_history")
    again = r.read_temporal()
    assert all(np.array_equal(bits(first[k]) if first[k].dtype == np.float32 else first[k], bits(again[k]) if again[k].dtype == np.float32 else again[k])
               for k in ("color", "geometry", "bgra8"))
    r.temporal_commit()
    r.set_render_parameters(_params(1))
    r.render(SPP)
    _refused(lambda: r.temporal_accumulate(depth_tolerance=0.0), "depth_tolerance")
    _refused(r.temporal_commit, "no temporal result")
    r.temporal_accumulate()
    S, AC, ND, n = _sums(r)
    T, G = tr.reproject(S, AC, ND, n, _camera(1), dict(color=first["color"], geometry=first["geometry"], camera=_camera(0)))
    _check(r.read_temporal(), T, G, SPP, "after the refusals")
    assert float(T[..., 3].max()) > SPP                                        # (the history was still there)
    r.close()


def test_a_new_frame_size_a_shard_and_a_reset_drop_the_history(duck_pt):
    r = _renderer(duck_pt, max_width=128, max_height=96)

    def view_with_history():
        r.render(SPP)
        r.temporal_accumulate()
        r.temporal_commit()
        r.set_render_parameters(_params(1))
        r.render(SPP)
        r.temporal_accumulate()
        assert float(r.read_temporal()["color"][..., 3].max()) > SPP           # the history is in use

    def no_history(camera, w=W, h=H):
        got = r.read_temporal()
        S, n = r.read_accumulation()
        assert got["color"].shape == (h, w, 4) and got["samples"] == n == SPP
        assert (got["color"][..., 3] == SPP).all() and np.array_equal(bits(got["color"][..., :3]), bits(S[..., :3] / np.float32(SPP)))

    # a reset
    view_with_history()
    r.temporal_reset()
    _refused(r.read_temporal, "no temporal result")
    r.temporal_accumulate()
    no_history(_camera(1))
    # a tile shard, set and lifted again
    r.temporal_commit()
    r.set_render_parameters(_params(0))
    view_with_history()
    r.temporal_commit()
    r.set_tile_shard(0, 2)
    r.set_tile_shard(0, 1)
    r.render(SPP)
    r.temporal_accumulate()
    no_history(_camera(1))
    # a new frame size (and back: the planes are allocated anew either way)
    r.temporal_commit()
    r.set_render_parameters(_params(0))
    view_with_history()
    r.temporal_commit()
    for (w, h) in ((80, 48), (W, H)):
        r.set_render_parameters(rf.make_render_parameters(w, h, rf.fly_camera(w, h, **VIEWS[2]), CAP, BOUNCES, rf.make_sky(), EXPOSURE))
        r.render(SPP)
        r.temporal_accumulate()
        no_history(_camera(2, w, h), w, h)
        S, AC, ND, n = _sums(r)
        T, G = tr.reproject(S, AC, ND, n, _camera(2, w, h))
        _check(r.read_temporal(), T, G, SPP, f"{w} x {h}")
        r.temporal_commit()
        r.set_render_parameters(rf.make_render_parameters(w, h, rf.fly_camera(w, h, **VIEWS[1]), CAP, BOUNCES, rf.make_sky(), EXPOSURE))
        r.render(SPP)
        r.temporal_accumulate()
        assert float(r.read_temporal()["color"][..., 3].max()) > SPP           # a history of the new size works as ever
        r.temporal_commit()
    r.close()
