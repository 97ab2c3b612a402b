"""Bounce 1 generated, intersected and shaded by one kernel (-m gpu): option primary_fused off against on, on the same build, the first-hit AOVs OFF (with them on the
mode is not selected) -- the accumulation bit for bit, the ray counts, and primary_fused_rays saying which launches ran.  The cases are those in which the fused kernel
takes another path: ragged tiles and waves that straddle pixels, a batch below the lists' threshold, sky pixels (kSky on fused misses), lists that overflow (most rays
through the listed kShade, both append paths in one batch), pixels whose directions change sign, bounce 1 as the last bounce, a leaf with a table-encoded count, two
coincident triangles, a scene far from the origin, a tile list, a tile shard, the direct sums and the moments, the two settings under which the three launches stay,
and one case against the oracle.  Scenes and cameras: tests/test_gpu_primary_lists.py."""
import numpy as np
import pytest

import rayfinder_amd as rf
import scale_scenes
import test_gpu_primary_lists as lists
from conftest import bits, oracle_scene_from_pt
from oracle import orc

pytestmark = pytest.mark.gpu
COUNTS = ("primary_rays", "closest_rays", "shadow_rays", "shadow_rays_self_answered", "abandoned_rays", "primary_list_rays", "primary_fallback_rays")


def _render(scene, w, h, cam, steps, fused, bounces=3, options=(), aovs=False, sums=False, shard=None):
    """One handle, render(n) for n in steps -> dict(img, stats, per-bounce ray counts[, direct, moments]) as bit patterns / integers"""
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, cam, 4096, bounces, rf.make_sky(), 0.25), scene)
    r.set_option("primary_fused", 1 if fused else 0)
    for k, v in options:
        r.set_option(k, v)
    if shard is not None:
        r.set_tile_shard(*shard)
    if aovs:
        r.set_aovs(True)
    if sums:
        r.set_direct(True)
        r.set_moments(True)
    for n in steps:
        r.render(n)
    img, acc = r.read_accumulation()
    assert acc == sum(steps)
    b = r.bounce_stats()
    out = dict(img=bits(img), stats=r.stats(), closest=b["closest_rays"].tolist(), hits=b["shadow_rays"].tolist())
    if sums:
        (d, nd), (q, nq) = r.read_direct(), r.read_moments()
        assert nd == nq == acc
        out["direct"], out["moments"] = bits(d), bits(q)
    if aovs:
        a = r.read_aovs()
        out["aov"] = {k: bits(a[k]) for k in lists.AOV_KEYS}
    r.close()
    return out


def _off_on(scene, w, h, cam, steps, selected=True, **kw):
    """Both settings; everything equal but primary_fused_rays: 0 with the option off, with it on primary_list_rays -- or 0 where the mode is not selected"""
    off, on = _render(scene, w, h, cam, steps, False, **kw), _render(scene, w, h, cam, steps, True, **kw)
    s = on["stats"]
    print(f"{w}x{h} steps {steps}: fused rays {s['primary_fused_rays']}, list rays {s['primary_list_rays']}, handed on {s['primary_fallback_rays']}, bounce-1 rays {on['closest'][:1]}, "
          f"bounce-1 hits {on['hits'][:1]}, shadow rays {s['shadow_rays']}, self answered {s['shadow_rays_self_answered']}")
    assert np.array_equal(off["img"], on["img"])
    for k in ("direct", "moments"):
        assert (k in off) == (k in on) and (k not in off or np.array_equal(off[k], on[k])), k
    if "aov" in off:
        assert all(np.array_equal(off["aov"][k], on["aov"][k]) for k in lists.AOV_KEYS)
    for k in COUNTS:
        assert off["stats"][k] == s[k], k
    assert off["closest"] == on["closest"] and off["hits"] == on["hits"]
    assert off["stats"]["primary_fused_rays"] == 0
    assert s["primary_fused_rays"] == (s["primary_list_rays"] if selected else 0)
    return off, on


def test_ragged_frame_straddling_waves_a_small_batch_and_sky_pixels():
    """33 x 40: two ragged tiles; 70 samples (waves of 64 straddle pixels), then a batch of 3, which stays unfused.  The frame shows sky: kSky runs on fused misses"""
    w, h = 33, 40
    _, on = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (70, 3))
    assert on["stats"]["primary_fused_rays"] == w * h * 70
    assert on["closest"][0] == w * h * 73 and 0 < on["hits"][0] < on["closest"][0]      # bounce 1: rays that hit, and rays that left for the sky


def test_lists_that_overflow_and_the_default_capacity():
    """capacity 2: most rays are handed on -- kTraceWide and the listed kShade -- while the rest are shaded by the fused kernel, both appending to the same queues"""
    w, h = 40, 33
    _, tight = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (64,), options=(("primary_list_capacity", 2),))
    _, roomy = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (64,))
    assert tight["stats"]["primary_fused_rays"] == roomy["stats"]["primary_fused_rays"] == w * h * 64
    assert roomy["stats"]["primary_fallback_rays"] < tight["stats"]["primary_fallback_rays"] < w * h * 64
    assert np.array_equal(tight["img"], roomy["img"])


@pytest.mark.parametrize("w,h", [(32, 24), (33, 25)])
def test_pixels_whose_directions_change_sign(w, h):
    _, on = _off_on(lists._duck().scene(), w, h, lists._axis_camera(w, h), (40,))
    assert on["stats"]["primary_fused_rays"] == w * h * 40
    assert 40 * (w + h - 2) <= on["stats"]["primary_fallback_rays"] < w * h * 40


@pytest.mark.parametrize("bounces", [1, 2])
def test_bounce_one_as_the_last_bounce(bounces):
    """bounces = 1: the fused kernel shades with kShadeLastBounce and writes no next direction or throughput"""
    w, h = 40, 33
    _, on = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (32,), bounces=bounces)
    assert on["stats"]["primary_fused_rays"] == w * h * 32 and 0 < on["hits"][0] < on["closest"][0] == w * h * 32


def test_a_big_leaf_is_handed_on():
    rng = np.random.default_rng(5)
    big = np.tile(np.array([[[-0.5, -0.4, 0.05], [0.5, -0.35, -0.1], [0.05, 0.45, 0.15]]]), (8, 1, 1))
    rest = rng.uniform(-1.5, 1.5, (60, 1, 3)) + rng.normal(0, 0.25, (60, 3, 3))
    pt = lists._soup(np.concatenate([big, rest]))
    assert int(pt.arrays()["bvhNodes"]["triangleCount"].max()) >= 8
    w, h = 48, 40
    cam = rf.create_camera((0.3, 0.4, 3.5), (0.0, 0.0, 0.0), 0.0, 3.5, float(orc.degrees_to_radians(50.0)), w / h)
    _, on = _off_on(pt.scene(), w, h, cam, (32,))
    assert 0 < on["stats"]["primary_fallback_rays"] < on["stats"]["primary_fused_rays"] == w * h * 32


def test_a_tie_between_coincident_triangles():
    """Two coincident triangles in two leaves: the fused walk keeps the reference's winner from either side -- fused == unfused == the oracle"""
    sc, osc, keep = lists._tie_scene()
    w, h, spp, bounces = 24, 20, 32, 2
    for eye in ((2.5, 0.3, 2.0), (-2.5, 0.3, 2.0)):
        cam = rf.create_camera(eye, (0.0, 0.0, 0.0), 0.0, 3.0, float(orc.degrees_to_radians(45.0)), w / h)
        _, on = _off_on(sc, w, h, cam, (spp,), bounces=bounces)
        assert on["stats"]["primary_fused_rays"] == w * h * spp
        ref, _ = orc.render(osc, orc.make_render_params(w, h, rf.camera_to_array(cam), 4096, bounces, 0.25, rf.aligned_sky_state(rf.make_sky())), 0, spp)
        assert np.array_equal(on["img"][..., :3], bits(ref[..., :3]))


def test_a_scene_far_from_the_origin():
    pt = scale_scenes.soup_pt(scale_scenes.triangles("unit_at_6e4"))
    w, h = scale_scenes.FRAME
    label, cam, inside = scale_scenes.cameras(pt.arrays()["bvhNodes"], w, h)[0]
    assert label == "near" and inside
    _, on = _off_on(pt.scene(), w, h, cam, (24,))
    assert on["stats"]["primary_fused_rays"] == w * h * 24


def _adaptive(pt, w, h, fused, target, every):
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, rf.fly_camera(w, h), 2 * every, 3, rf.make_sky(), 0.25), pt.scene())
    r.set_option("primary_fused", 1 if fused else 0)
    r.set_moments(True)
    res = r.render_adaptive(target, every, every)
    img, _ = r.read_accumulation()
    out = dict(img=bits(img), stats=r.stats(), counts=r.read_tile_samples().reshape(-1).tolist(), moments=bits(r.read_moments()[0]), res=res)
    r.close()
    return out


def test_a_batch_over_a_tile_list():
    """render_adaptive: 32 samples of all four tiles, then 32 more of the two noisiest -- a fused batch over a tile list that drops two tiles.  The target only picks
    the scenario (between the second and the third largest tile error of the first check, from a handle with the option off)"""
    pt, w, h, every = lists._duck(), 64, 64, 32
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, rf.fly_camera(w, h), 2 * every, 3, rf.make_sky(), 0.25), pt.scene())
    r.set_option("primary_fused", 0)
    r.set_moments(True)
    r.render(every)
    est = r.noise_estimate()
    r.close()
    err = np.sort(est["tile_sum"].astype(np.float64) / 1024.0)[::-1]
    assert len(err) == 4 and err[1] > err[2]
    target = float(np.float32(0.5 * (err[1] + err[2])))
    off, on = _adaptive(pt, w, h, False, target, every), _adaptive(pt, w, h, True, target, every)
    assert sorted(off["counts"]) == [every, every, 2 * every, 2 * every]
    assert on["counts"] == off["counts"] and on["res"] == off["res"]
    assert np.array_equal(off["img"], on["img"]) and np.array_equal(off["moments"], on["moments"])
    for k in COUNTS:
        assert off["stats"][k] == on["stats"][k], k
    assert off["stats"]["primary_fused_rays"] == 0 and on["stats"]["primary_fused_rays"] == on["stats"]["primary_list_rays"] == (4 + 2) * 1024 * every


@pytest.mark.parametrize("rank", [0, 1])
def test_a_tile_shard_of_two(rank):
    """70 x 40: three tiles dealt to two ranks; each rank's own tiles, fused against unfused"""
    w, h = 70, 40
    _, on = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (48,), shard=(rank, 2))
    assert 0 < on["stats"]["primary_fused_rays"] < w * h * 48


def test_the_direct_sums_and_the_moments():
    """D is summed right behind bounce 1's launch groups, from what the fused kernel and kSky have left in the radiance stream; Q at the end of the batch"""
    w, h = 40, 33
    off, on = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (32, 20), sums=True)
    assert on["stats"]["primary_fused_rays"] == w * h * 52
    assert off["direct"].any() and off["moments"].any()


def test_the_modes_that_keep_the_three_launches():
    """The AOVs on, then `transcendentals` 1: the fused kernel is not selected (the stat stays 0) and the image is the option-off image"""
    w, h = 40, 33
    _, on = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (32,), selected=False, aovs=True)
    assert on["stats"]["primary_list_rays"] == w * h * 32
    _, on = _off_on(lists._duck().scene(), w, h, rf.fly_camera(w, h), (32,), selected=False, options=(("transcendentals", 1),))
    assert on["stats"]["primary_list_rays"] == w * h * 32


def test_duck_fused_is_bit_identical_to_the_oracle():
    pt = lists._duck()
    w, h, spp, bounces = 24, 16, 32, 3
    cam = rf.fly_camera(w, h)
    on = _render(pt.scene(), w, h, cam, (spp,), True, bounces=bounces)
    assert on["stats"]["primary_fused_rays"] == w * h * spp
    sc, _ = oracle_scene_from_pt(pt)
    ref, st = orc.render(sc, orc.make_render_params(w, h, rf.camera_to_array(cam), 4096, bounces, 0.25, rf.aligned_sky_state(rf.make_sky())), 0, spp)
    assert on["stats"]["closest_rays"] == st.closestRays
    assert np.array_equal(on["img"][..., :3], bits(ref[..., :3]))
