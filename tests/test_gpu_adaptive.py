"""Tile-adaptive sampling on the GPU (-m gpu): rf_renderer_render_adaptive follows the schedule of the numpy restatement (tests/adaptive_restatement.py) fed with the
oracle's per-sample radiance, every tile's sums are bit for bit the sums of a uniform render of that tile's count, no scheduling choice shows, and the handle keeps the
books include/rayfinder_amd.h states.  Targets come from the restatement alone, never from the code under test."""
import functools

import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import estimate_tiles, play, prefix_sums, tile_errors, tile_slices
from conftest import DUCK, bits, oracle_scene_from_pt
from noise_restatement import estimate, oracle_samples, same_estimate
from oracle import orc

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
W, H, SPP, BOUNCES, EVERY, EXPOSURE = 150, 90, 32, 3, 4, 0.25           # 5 x 3 tiles, ragged right (150 = 4 x 32 + 22) and bottom (90 = 2 x 32 + 26)
TILES = 15


def _camera(w, h, aperture=0.0):
    return rf.fly_camera(w, h, aperture=aperture, focus_distance=2.0) if aperture else rf.fly_camera(w, h)


def _renderer(pt, w=W, h=H, spp=SPP, aperture=0.0, opts=(), moments=True, **kw):
    params = rf.make_render_parameters(w, h, _camera(w, h, aperture), spp, BOUNCES, rf.make_sky(), EXPOSURE)
    r = rf.ReferencePathTracer(params, pt.scene(), **kw)
    for k, v in dict(opts).items():
        r.set_option(k, v)
    if moments:
        r.set_moments(True)
    return r


@functools.lru_cache(maxsize=None)
def _oracle(w, h, spp, aperture=0.0):
    """The oracle's per-sample radiance of Duck as prefix sums (computed once per frame size; read-only), and the tile errors at the first check (L = 4)"""
    pt = rf.PtFormat.from_gltf(DUCK)
    sc, _ = oracle_scene_from_pt(pt)
    cam = _camera(w, h, aperture)
    rp = orc.make_render_params(w, h, rf.camera_to_array(cam), spp, BOUNCES, EXPOSURE, rf.aligned_sky_state(rf.make_sky()))
    S, Q = prefix_sums(list(oracle_samples(orc, sc, rp, range(spp))))
    for a in S + Q:
        a.setflags(write=False)
    return S, Q, tile_errors(estimate(S[EVERY], Q[EVERY], EVERY))


def _target(aperture=0.0):
    """The median of the restatement's per-tile errors at the first check"""
    return float(np.float32(np.median(_oracle(W, H, SPP, aperture)[2])))


@functools.lru_cache(maxsize=None)
def _want(aperture=0.0):
    S, Q, _ = _oracle(W, H, SPP, aperture)
    want = play(S, Q, W, H, _target(aperture), EVERY, min_samples=EVERY)
    counts = want["counts"]
    # before looking at the GPU: the schedule is a real one
    assert len(set(counts.tolist())) >= 3 and (counts == EVERY).any() and (counts == SPP).any(), counts
    return want


def _reads(r):
    """Everything the handle reports, as bit patterns / integers"""
    img, acc = r.read_accumulation()
    q, n = r.read_moments()
    return dict(counts=r.read_tile_samples().reshape(-1).astype(np.int64), S=bits(img), Q=bits(q), mean=bits(r.read_mean()), bgra=r.read_tonemapped(), acc=acc, n=n)


def _same_reads(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def _run(pt, target, aperture=0.0, opts=(), every=EVERY, min_samples=EVERY, **kw):
    r = _renderer(pt, aperture=aperture, opts=opts, **kw)
    res = r.render_adaptive(target, every, min_samples)
    return r, res


@functools.lru_cache(maxsize=None)
def _uniform_snapshots(aperture=0.0):
    """A second, uniform handle stepped in fours: (S, Q) bit patterns after 4, 8, ..., 32 samples"""
    pt = rf.PtFormat.from_gltf(DUCK)
    r = _renderer(pt, aperture=aperture)
    snaps = {}
    for n in range(EVERY, SPP + 1, EVERY):
        r.render(EVERY)
        snaps[n] = (bits(r.read_accumulation()[0]), bits(r.read_moments()[0]), r.read_tonemapped())
    r.close()
    return snaps


def _refused(call, *words):
    with pytest.raises(rf.RayfinderError) as err:
        call()
    return err.value.status == INVALID and all(w in str(err.value) for w in words)


def test_schedule_and_sums_match_the_restatement(duck_pt):
    want = _want()
    r, res = _run(duck_pt, _target())
    got = _reads(r)
    print("tile counts:", got["counts"].tolist(), "passes:", res["estimate_passes"], "pixel samples:", res["pixel_samples"], "of", W * H * SPP)
    assert got["counts"].tolist() == want["counts"].tolist()
    assert got["acc"] == SPP and got["n"] == SPP                             # the reads report the leading count
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"]))
    assert np.array_equal(got["mean"], bits(want["mean"]))
    assert np.array_equal(got["bgra"].reshape(-1), orc.tonemap_bgra8(want["mean"].reshape(-1, 4), 1, EXPOSURE))
    # the result struct
    for k in ("estimate_passes", "stopped_tiles", "min_tile_samples", "max_tile_samples", "pixel_samples"):
        assert res[k] == want[k], k
    assert res["tiles"] == TILES
    last = dict(res["last"], error_map=0, tile_sum=0, tile_max=0)
    assert same_estimate(last, dict(want["last"], error_map=0, tile_sum=0, tile_max=0)) == []
    assert r.stats()["primary_rays"] == want["pixel_samples"] < W * H * SPP
    # the estimate with every tile's own count, from the handle and from the host-sums twin
    ref = estimate_tiles(want["S"], want["Q"], want["counts"], W, H)
    assert same_estimate(r.noise_estimate(), ref) == []
    assert same_estimate(rf.noise_estimate_tiles(r.read_accumulation()[0], r.read_moments()[0], want["counts"]), ref) == []
    assert ref["samples"] == SPP
    r.close()
    # separately: every tile's sums are those of a uniform render(tile_samples[t]) on a second handle
    snaps = _uniform_snapshots()
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        s, q, _ = snaps[int(want["counts"][t])]
        assert np.array_equal(got["S"][rows, cols], s[rows, cols]) and np.array_equal(got["Q"][rows, cols], q[rows, cols]), t


@pytest.fixture(scope="module")
def baseline(duck_pt):
    r, res = _run(duck_pt, _target())
    got = _reads(r)
    r.close()
    assert got["counts"].tolist() == _want()["counts"].tolist()
    return got, res


@pytest.mark.parametrize("name,opts,paths", [
    ("one sample of the frame per batch", {}, 1 * TILES * 1024),
    ("five samples of the frame per batch", {}, 5 * TILES * 1024),
    ("sample-major slots", dict(slot_group_shift=-1), 0),
    ("groups of 4 pixels", dict(slot_group_shift=2), 0),
    ("groups of 64 pixels", dict(slot_group_shift=6), 0),
    ("unsorted samples", dict(sample_sort=0), 0),
    ("no LDS-staged accumulation", dict(accumulate_runs=0), 0),
])
def test_scheduling_is_invisible(duck_pt, baseline, name, opts, paths):
    r, res = _run(duck_pt, _target(), opts=opts, max_paths_in_flight=paths)
    got = _reads(r)
    r.close()
    assert _same_reads(got, baseline[0]) == [], name
    assert res == baseline[1], name


@pytest.mark.parametrize("every", [8, 16])
def test_longer_steps_take_the_lds_staged_kernel_and_leave_the_same_sums(duck_pt, every):
    """check_every > 4 with pixel-major slots: kSumRuns<RadianceMomentSum, true> (steps of 4 take the one-lane-per-pixel kernel).  The schedule is the restatement's for that step."""
    S, Q, _ = _oracle(W, H, SPP)
    want = play(S, Q, W, H, _target(), every, min_samples=every)
    assert len(set(want["counts"].tolist())) >= 2
    r, res = _run(duck_pt, _target(), every=every, min_samples=every)
    got = _reads(r)
    r.close()
    assert got["counts"].tolist() == want["counts"].tolist()
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"]))
    snaps = _uniform_snapshots()
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        s, q, _ = snaps[int(want["counts"][t])]
        assert np.array_equal(got["S"][rows, cols], s[rows, cols]) and np.array_equal(got["Q"][rows, cols], q[rows, cols]), t
    for opts in (dict(accumulate_runs=0), dict(sample_sort=0), dict(slot_group_shift=2)):
        r, res2 = _run(duck_pt, _target(), every=every, min_samples=every, opts=opts)
        assert _same_reads(_reads(r), got) == [] and res2 == res, opts
        r.close()


def test_an_aperture_changes_nothing_about_the_contract(duck_pt):
    aperture = 0.15
    want = _want(aperture)
    r, res = _run(duck_pt, _target(aperture), aperture=aperture)
    got = _reads(r)
    r.close()
    assert got["counts"].tolist() == want["counts"].tolist()
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"])) and np.array_equal(got["mean"], bits(want["mean"]))
    r, res2 = _run(duck_pt, _target(aperture), aperture=aperture, opts=dict(slot_group_shift=2), max_paths_in_flight=5 * TILES * 1024)
    assert _same_reads(_reads(r), got) == [] and res2 == res
    r.close()


def test_target_zero_runs_every_tile_to_the_cap_and_leaves_the_ordinary_state(duck_pt):
    r, res = _run(duck_pt, 0.0)
    got = _reads(r)
    assert got["counts"].tolist() == [SPP] * TILES and res["stopped_tiles"] == 0 and res["estimate_passes"] == SPP // EVERY
    assert res["pixel_samples"] == W * H * SPP and res["last"]["samples"] == SPP and res["last"]["pixels"] == W * H
    s, q, bgra = _uniform_snapshots()[SPP]
    assert np.array_equal(got["S"], s) and np.array_equal(got["Q"], q) and np.array_equal(got["bgra"], bgra)
    # the ordinary state: the estimate is kNoiseEstimate's, and render / render_until run (into the full accumulation: nothing is traced)
    S, Q, _ = _oracle(W, H, SPP)
    assert same_estimate(r.noise_estimate(), estimate(S[SPP], Q[SPP], SPP)) == []
    r.render(2)
    assert r.render_until(0.0, 4) == (0, None)
    assert _same_reads(_reads(r), got) == []
    assert _refused(r.denoise, "AOV")                                        # denoise's own check, as before: the AOVs are off
    r.close()


def test_a_huge_target_stops_every_tile_at_the_first_check_and_render_continues(duck_pt):
    r, res = _run(duck_pt, 1e30)
    assert r.read_tile_samples().reshape(-1).tolist() == [EVERY] * TILES
    assert res["stopped_tiles"] == 0 and res["estimate_passes"] == 1 and res["pixel_samples"] == W * H * EVERY
    snaps = _uniform_snapshots()
    assert np.array_equal(bits(r.read_accumulation()[0]), snaps[EVERY][0]) and np.array_equal(r.read_tonemapped(), snaps[EVERY][2])
    # frameCount continuity: the uniform state at L = 4, then render(8), is render(12)
    r.render(8)
    assert r.read_accumulation()[1] == 12 and r.read_tile_samples().reshape(-1).tolist() == [12] * TILES
    assert np.array_equal(bits(r.read_accumulation()[0]), snaps[12][0]) and np.array_equal(bits(r.read_moments()[0]), snaps[12][1])
    frames, last = r.render_until(0.0, 4, 4)
    assert frames == 4 and last["samples"] == 16 and np.array_equal(bits(r.read_accumulation()[0]), snaps[16][0])
    # ... and a render_adaptive after uniform renders continues from there
    res = r.render_adaptive(0.0, EVERY, EVERY, 24)
    assert res["min_tile_samples"] == res["max_tile_samples"] == 24 and np.array_equal(bits(r.read_moments()[0]), snaps[24][1])
    r.close()


@pytest.mark.parametrize("w,h,spp,every", [(20, 12, 32, 4), (64, 64, 32, 4), (W, H, 32, 3), (64, 64, 48, 40)])
def test_sizes_and_a_shorter_last_step(duck_pt, w, h, spp, every):
    """Smaller than one tile; exact tiles; a step that does not divide the cap (3: 3, 6, ..., 30, 32); a step longer than one LDS chunk of 32 samples (40, then 8)."""
    S, Q, _ = _oracle(w, h, spp)
    first = max(every, 2)
    errors = tile_errors(estimate(S[first], Q[first], first))
    target = float(np.float32(np.median(errors)))
    want = play(S, Q, w, h, target, every, min_samples=0)
    r = _renderer(duck_pt, w, h, spp)
    res = r.render_adaptive(target, every)
    got = _reads(r)
    print((w, h, spp, every), "counts:", got["counts"].tolist())
    assert got["counts"].tolist() == want["counts"].tolist()
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"])) and np.array_equal(got["mean"], bits(want["mean"]))
    assert res["estimate_passes"] == want["estimate_passes"] and res["pixel_samples"] == want["pixel_samples"] == r.stats()["primary_rays"]
    if want["stopped_tiles"]:
        assert same_estimate(r.noise_estimate(), estimate_tiles(want["S"], want["Q"], want["counts"], w, h)) == []
    r.close()


def test_refusals_and_the_non_uniform_state(duck_pt):
    # arguments and preconditions
    r = _renderer(duck_pt, moments=False)
    assert _refused(lambda: r.render_adaptive(0.1, 4), "moments")
    r.render(2)
    r.set_moments(True)
    assert _refused(lambda: r.render_adaptive(0.1, 4), "cover")               # turned on partway through
    r.set_render_parameters(rf.make_render_parameters(W, H, _camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
    assert _refused(lambda: r.render_adaptive(0.1, 0), "check_every")
    for bad in (-1e-3, float("nan"), float("inf")):
        assert _refused(lambda: r.render_adaptive(bad, 4), "target")
    r.set_aovs(rf._ffi.RF_AOV_FIRST_HIT)
    assert _refused(lambda: r.render_adaptive(0.1, 4), "AOV")
    r.set_aovs(0)
    r.set_tile_shard(0, 2)
    assert _refused(lambda: r.render_adaptive(0.1, 4), "shard")
    r.set_tile_shard(0, 1)
    assert r.read_accumulation()[1] == 0 and r.read_tile_samples().reshape(-1).tolist() == [0] * TILES
    r.close()
    # the non-uniform state (a fresh handle: the restatement's schedule): everything that assumes one count says why it refuses
    r = _renderer(duck_pt)
    res = r.render_adaptive(_target(), EVERY, EVERY)
    assert res["stopped_tiles"] > 0
    before = _reads(r)
    why = "different sample counts"
    assert _refused(lambda: r.render(1), why) and _refused(lambda: r.render_until(0.1, 4), why) and _refused(r.denoise, why) and _refused(lambda: r.set_tile_shard(0, 2), why)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert _refused(lambda: r.gather_frame(comm, root=0, loopback=True), why)
    assert _same_reads(_reads(r), before) == []
    # set_render_parameters with a change (here the exposure; unchanged parameters are a no-op, as they always were) clears the counts
    r.set_render_parameters(rf.make_render_parameters(W, H, _camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
    assert r.read_tile_samples().reshape(-1).tolist() == [0] * TILES and not r.read_mean()[..., :3].any()
    r.render(8)
    assert r.read_tile_samples().reshape(-1).tolist() == [8] * TILES
    assert r.gather_frame(comm, root=0, loopback=True)                         # the ordinary state again: nothing refuses
    r.close()
    comm.close()


def test_a_second_call_moves_only_the_leading_tiles(duck_pt):
    S, Q, _ = _oracle(W, H, SPP)
    first = play(S, Q, W, H, _target(), EVERY, min_samples=EVERY, max_samples=16)
    assert first["stopped_tiles"] > 0
    lower = float(np.float32(np.sort(_oracle(W, H, SPP)[2])[3]))               # below the median: were stopped tiles revived, some of them would move
    second = play(S, Q, W, H, lower, EVERY, min_samples=EVERY, counts=first["counts"])
    r = _renderer(duck_pt)
    res1 = r.render_adaptive(_target(), EVERY, EVERY, 16)
    assert r.read_tile_samples().reshape(-1).tolist() == first["counts"].tolist() and res1["max_tile_samples"] == 16
    rays = r.stats()["primary_rays"]
    res2 = r.render_adaptive(lower, EVERY, EVERY)
    got = _reads(r)
    assert got["counts"].tolist() == second["counts"].tolist()
    stopped = first["counts"] != 16
    assert (got["counts"][stopped] == first["counts"][stopped]).all() and (got["counts"][~stopped] > 16).all()
    assert np.array_equal(got["S"][..., :3], bits(second["S"])[..., :3]) and np.array_equal(got["Q"], bits(second["Q"]))
    assert res2["pixel_samples"] == second["pixel_samples"] == r.stats()["primary_rays"] and rays == first["pixel_samples"]
    assert res2["estimate_passes"] == second["estimate_passes"]
    # a third call at the cap does nothing
    res3 = r.render_adaptive(0.0, EVERY)
    assert res3["estimate_passes"] == 0 and res3["last"] is None and _same_reads(_reads(r), got) == []
    r.close()


def test_set_render_parameters_clears_and_a_uniform_render_equals_a_fresh_handles(duck_pt):
    r = _renderer(duck_pt)
    res = r.render_adaptive(_target(), EVERY, EVERY)
    assert res["stopped_tiles"] > 0
    r.set_render_parameters(rf.make_render_parameters(W, H, _camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
    assert r.read_tile_samples().reshape(-1).tolist() == [0] * TILES and r.read_accumulation()[1] == 0
    r.render(4)
    img, acc = r.read_accumulation()
    q, n = r.read_moments()
    r.close()
    # frames SPP .. SPP + 3 of the sequence: what a fresh handle traces after SPP frames that its accumulation drops
    fresh = _renderer(duck_pt)
    fresh.render(SPP)
    fresh.set_render_parameters(rf.make_render_parameters(W, H, _camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
    fresh.render(4)
    assert acc == 4 and n == 4 and np.array_equal(bits(fresh.read_accumulation()[0]), bits(img)) and np.array_equal(bits(fresh.read_moments()[0]), bits(q))
    assert fresh.read_tile_samples().reshape(-1).tolist() == [4] * TILES
    fresh.close()


def _read_pfm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    kind, (w, h) = parts[0], map(int, parts[1].split())
    assert kind == b"Pf" and parts[2] == b"-1.0"
    return np.frombuffer(parts[3], "<f4").reshape(h, w)[::-1]


def test_rf_render_adaptive_writes_the_sample_map_of_the_api(duck_pt, tmp_path):
    import os
    import subprocess

    from conftest import ROOT
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    base = [exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(SPP), "--bounces", str(BOUNCES), "--out", str(tmp_path / "a.png")]
    target = _target()                                                        # rf-render's defaults are this file's camera and sky; %.9g round-trips an f32
    txt = subprocess.check_output(base + ["--adaptive", "%.9g" % target, "--adaptive-min", str(EVERY), "--adaptive-every", str(EVERY), "--sample-map",
                                          str(tmp_path / "s.pfm")], timeout=120).decode()
    want = _want()
    assert f"{want['stopped_tiles']} of {TILES} tiles stopped early" in txt and f"{want['pixel_samples']} of {W * H * SPP} pixel-samples" in txt, txt
    got = _read_pfm(tmp_path / "s.pfm")
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        assert (got[rows, cols] == want["counts"][t]).all(), t
    bad = subprocess.run(base + ["--adaptive", "0.1", "--gpus", "2"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--adaptive needs --gpus 1" in bad.stderr
