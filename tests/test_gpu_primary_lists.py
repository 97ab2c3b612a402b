"""Bounce 1 over per-pixel leaf lists (-m gpu): option primary_lists off against on, on the same build, bit for bit -- the accumulation and the first-hit AOV sums
(they carry t and the normal of the first hit, so they carry the hit itself) -- over the cases in which the lists take another path: ragged tiles and waves that
straddle pixels, batches below the threshold, pixels whose directions change sign, lists that overflow, a leaf with a table-encoded count, a scene far from the origin,
a thin lens, a tile list, and two coincident triangles in different leaves (the tie in t goes to the reference's winner).  One case against the oracle."""
import functools

import numpy as np
import pytest

import rayfinder_amd as rf
import scale_scenes
from conftest import DUCK, bits, oracle_scene_from_pt
from oracle import orc

pytestmark = pytest.mark.gpu
AOV_KEYS = ("albedo", "normal", "depth", "coverage")


@functools.lru_cache(maxsize=None)
def _duck():
    return rf.PtFormat.from_gltf(DUCK)


def _render(scene, w, h, cam, steps, on, bounces=3, options=()):
    """One handle, the AOVs on, render(n) for n in steps -> dict(img, aov sums, stats), all as bit patterns / integers"""
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, cam, 4096, bounces, rf.make_sky(), 0.25), scene)
    r.set_option("primary_lists", 1 if on else 0)
    for k, v in options:
        r.set_option(k, v)
    r.set_aovs(True)
    for n in steps:
        r.render(n)
    img, acc = r.read_accumulation()
    a = r.read_aovs()
    s = r.stats()
    r.close()
    assert acc == sum(steps) == a["samples"]
    return dict(img=bits(img), aov={k: bits(a[k]) for k in AOV_KEYS}, stats=s)


def _same(a, b):
    return [k for k in ("img",) if not np.array_equal(a[k], b[k])] + [k for k in AOV_KEYS if not np.array_equal(a["aov"][k], b["aov"][k])]


def _off_on(scene, w, h, cam, steps, **kw):
    off, on = _render(scene, w, h, cam, steps, False, **kw), _render(scene, w, h, cam, steps, True, **kw)
    s = on["stats"]
    print(f"{w}x{h} steps {steps}: list rays {s['primary_list_rays']}, handed on {s['primary_fallback_rays']}, closest rays {s['closest_rays']}, scalar redo {s['scalar_redo_rays']}")
    assert off["stats"]["primary_list_rays"] == 0 and off["stats"]["primary_fallback_rays"] == 0
    assert _same(off, on) == []
    for k in ("primary_rays", "closest_rays", "shadow_rays", "shadow_rays_self_answered", "abandoned_rays"):
        assert off["stats"][k] == s[k], k
    return off, on


def test_ragged_frame_odd_batch_depth_and_a_batch_below_the_threshold():
    """33 x 40: two ragged tiles.  70 samples in one batch (waves of 64 straddle pixels), then 3 samples (below primary_list_min_samples: the old launch)"""
    w, h = 33, 40
    _, on = _off_on(_duck().scene(), w, h, rf.fly_camera(w, h), (70, 3))
    assert on["stats"]["primary_list_rays"] == w * h * 70               # the batch of 70, whole; the batch of 3 not at all
    _, alone = _off_on(_duck().scene(), w, h, rf.fly_camera(w, h), (3,))
    assert alone["stats"]["primary_list_rays"] == 0


def _axis_camera(w, h):
    """Looks exactly along -z at the Duck: the pixel columns and rows through the middle of the frame hold directions whose x / y change sign"""
    a = _duck().arrays()
    lo, hi = np.array(a["bvhNodes"][0]["min"]), np.array(a["bvhNodes"][0]["max"])
    c = np.round(0.5 * (lo + hi) * 8) / 8                                # (exactly representable: eye - target is exactly (0, 0, d))
    d = float(np.ceil(2.0 * np.max(hi - lo)))
    return rf.create_camera(c + np.array([0.0, 0.0, d]), c, 0.0, d, float(orc.degrees_to_radians(40.0)), w / h)


@pytest.mark.parametrize("w,h", [(32, 24), (33, 25)])
def test_pixels_whose_directions_change_sign_fall_back(w, h):
    _, on = _off_on(_duck().scene(), w, h, _axis_camera(w, h), (40,))
    s = on["stats"]
    assert s["primary_list_rays"] == w * h * 40
    assert 0 < s["primary_fallback_rays"] < s["primary_list_rays"]
    assert s["primary_fallback_rays"] >= 40 * (w + h - 2)                 # at least one column and one row of pixels


def test_lists_that_overflow_fall_back():
    w, h = 40, 33
    _, on = _off_on(_duck().scene(), w, h, rf.fly_camera(w, h), (64,), options=(("primary_list_capacity", 2),))
    _, roomy = _off_on(_duck().scene(), w, h, rf.fly_camera(w, h), (64,))
    assert on["stats"]["primary_list_rays"] == roomy["stats"]["primary_list_rays"] == w * h * 64
    assert on["stats"]["primary_fallback_rays"] > roomy["stats"]["primary_fallback_rays"]
    assert 0 < on["stats"]["primary_fallback_rays"] < on["stats"]["primary_list_rays"]


def _soup(P, colours=(0xFFB4A0C8,), tex_index=None):
    n = P.shape[0]
    N = np.tile(np.array([0, 1, 0], np.float32), (n, 3))
    UV = np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (n, 1))
    return rf.PtFormat.from_triangles(P.reshape(n, 9).astype(np.float32), N, UV, np.zeros(n, np.uint32) if tex_index is None else tex_index,
                                      [(np.array([c], np.uint32), 1, 1) for c in colours])


def test_a_big_leaf_falls_back():
    """Eight coincident triangles (one centroid, one box) cannot be split: one leaf of eight, a count that lives in the big-leaf table.  Around it, ordinary leaves."""
    rng = np.random.default_rng(5)
    big = np.tile(np.array([[[-0.5, -0.4, 0.05], [0.5, -0.35, -0.1], [0.05, 0.45, 0.15]]]), (8, 1, 1))
    rest = rng.uniform(-1.5, 1.5, (60, 1, 3)) + rng.normal(0, 0.25, (60, 3, 3))
    pt = _soup(np.concatenate([big, rest]))
    a = pt.arrays()
    assert int(a["bvhNodes"]["triangleCount"].max()) >= 8
    w, h = 48, 40
    cam = rf.create_camera((0.3, 0.4, 3.5), (0.0, 0.0, 0.0), 0.0, 3.5, float(orc.degrees_to_radians(50.0)), w / h)
    _, on = _off_on(pt.scene(), w, h, cam, (32,))
    assert 0 < on["stats"]["primary_fallback_rays"] < on["stats"]["primary_list_rays"] == w * h * 32


@pytest.mark.parametrize("row", ["unit_at_1e3", "unit_at_6e4"])
def test_a_scene_far_from_the_origin(row):
    pt = scale_scenes.soup_pt(scale_scenes.triangles(row))
    w, h = scale_scenes.FRAME
    label, cam, inside = scale_scenes.cameras(pt.arrays()["bvhNodes"], w, h)[0]
    assert label == "near" and inside
    _, on = _off_on(pt.scene(), w, h, cam, (24,))
    assert on["stats"]["primary_list_rays"] == w * h * 24


def test_a_thin_lens_keeps_the_old_launches():
    w, h = 40, 33
    cam = rf.fly_camera(w, h, aperture=0.1, focus_distance=2.0)
    _, on = _off_on(_duck().scene(), w, h, cam, (48,))
    assert on["stats"]["primary_list_rays"] == 0 and on["stats"]["primary_fallback_rays"] == 0


def _adaptive(pt, w, h, on, target, every):
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, rf.fly_camera(w, h), 2 * every, 3, rf.make_sky(), 0.25), pt.scene())
    r.set_option("primary_lists", 1 if on else 0)
    r.set_moments(True)
    r.set_aovs(True, tile_counts=True)
    res = r.render_adaptive(target, every, every)
    img, _ = r.read_accumulation()
    a = r.read_aovs()
    out = dict(img=bits(img), aov={k: bits(a[k]) for k in AOV_KEYS}, stats=r.stats(), counts=r.read_tile_samples().reshape(-1).tolist(), moments=bits(r.read_moments()[0]), res=res)
    r.close()
    return out


def test_a_batch_over_a_tile_list():
    """render_adaptive: 32 samples of all four tiles, then 32 more of the two noisiest (a batch over a tile list of two).  The target only picks the scenario: it lies
    between the second and the third largest tile error of the first check, as the handle with the option OFF reports them."""
    pt, w, h, every = _duck(), 64, 64, 32
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, rf.fly_camera(w, h), 2 * every, 3, rf.make_sky(), 0.25), pt.scene())
    r.set_option("primary_lists", 0)
    r.set_moments(True)
    r.render(every)
    est = r.noise_estimate()
    r.close()
    err = np.sort(est["tile_sum"].astype(np.float64) / 1024.0)[::-1]
    assert len(err) == 4 and err[1] > err[2]
    target = float(np.float32(0.5 * (err[1] + err[2])))
    off, on = _adaptive(pt, w, h, False, target, every), _adaptive(pt, w, h, True, target, every)
    print("tile counts", on["counts"], "list rays", on["stats"]["primary_list_rays"], "handed on", on["stats"]["primary_fallback_rays"])
    assert sorted(off["counts"]) == [every, every, 2 * every, 2 * every]        # the scenario: two active tiles in the second batch
    assert on["counts"] == off["counts"] and on["res"] == off["res"]
    assert _same(off, on) == [] and np.array_equal(off["moments"], on["moments"])
    assert on["stats"]["primary_list_rays"] == (4 + 2) * 1024 * every and off["stats"]["primary_list_rays"] == 0


def _tie_scene():
    """Two coincident triangles with different albedo, each in a leaf of its own under one root that splits along x -- a hand-made tree (the builder would put them
    into one leaf).  -> (rf scene, oracle scene, keep-alive)"""
    tri = np.array([[-1.0, -0.8, 0.1], [1.0, -0.7, -0.2], [0.1, 0.9, 0.3]])
    pt = _soup(np.stack([tri, tri]), colours=(0xFF2020E0, 0xFF20E020), tex_index=np.array([0, 1], np.uint32))
    a = pt.arrays()
    lo, hi = tri.min(0).astype(np.float32), tri.max(0).astype(np.float32)
    nodes = np.zeros(3, rf.NODE_DTYPE)
    for i in range(3):
        nodes[i]["min"], nodes[i]["max"] = lo, hi
    nodes[0]["secondChildOffset"], nodes[0]["splitAxis"] = 2, 0
    nodes[1]["trianglesOffset"], nodes[1]["triangleCount"] = 0, 1
    nodes[2]["trianglesOffset"], nodes[2]["triangleCount"] = 1, 1
    tex = [(px, tw, th) for (px, tw, th) in a["baseColorTextures"]]
    sc = rf.scene_from_arrays(nodes, a["trianglePositionAttributes"], a["triangleVertexAttributes"], tex)
    descs = np.array([[1, 1, 0], [1, 1, 1]], np.uint32)
    osc = orc.OracleScene(nodes, a["trianglePositionAttributes"], a["triangleVertexAttributes"], descs, np.concatenate([px for (px, _, _) in tex]))
    return sc, osc, (pt, nodes, a)


def test_a_tie_between_coincident_triangles_goes_to_the_references_winner():
    """Both triangles give the same t; the reference keeps the first one it tests (the second fails t < rayTMax), and which leaf comes first depends on the sign of
    the direction's x.  From either side: the lists on == off == the oracle, bit for bit, and the two sides see different triangles."""
    sc, osc, keep = _tie_scene()
    w, h, spp, bounces = 24, 20, 32, 2
    albedo = []
    for eye in ((2.5, 0.3, 2.0), (-2.5, 0.3, 2.0)):
        cam = rf.create_camera(eye, (0.0, 0.0, 0.0), 0.0, 3.0, float(orc.degrees_to_radians(45.0)), w / h)
        off, on = _off_on(sc, w, h, cam, (spp,), bounces=bounces)
        assert on["stats"]["primary_list_rays"] == w * h * spp and on["stats"]["primary_fallback_rays"] < on["stats"]["primary_list_rays"]
        ref, _ = orc.render(osc, orc.make_render_params(w, h, rf.camera_to_array(cam), 4096, bounces, 0.25, rf.aligned_sky_state(rf.make_sky())), 0, spp)
        assert np.array_equal(on["img"][..., :3], bits(ref[..., :3]))
        centre = on["aov"]["albedo"].view(np.float32)[h // 2, w // 2]
        assert on["aov"]["coverage"].view(np.float32)[h // 2, w // 2] == spp
        albedo.append(centre / spp)
    print("albedo at the centre from +x / -x:", albedo)
    assert not np.allclose(albedo[0], albedo[1])                                  # another winner from the other side


def test_duck_with_the_lists_is_bit_identical_to_the_oracle():
    pt = _duck()
    w, h, spp, bounces = 64, 48, 64, 2
    cam = rf.fly_camera(w, h)
    on = _render(pt.scene(), w, h, cam, (spp,), True, bounces=bounces)
    assert on["stats"]["primary_list_rays"] == w * h * spp
    sc, _ = oracle_scene_from_pt(pt)
    ref, st = orc.render(sc, orc.make_render_params(w, h, rf.camera_to_array(cam), 4096, bounces, 0.25, rf.aligned_sky_state(rf.make_sky())), 0, spp)
    assert on["stats"]["closest_rays"] == st.closestRays
    assert np.array_equal(on["img"][..., :3], bits(ref[..., :3]))
