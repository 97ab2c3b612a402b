"""The per-pixel sums in sample order on the GPU (-m gpu), every kernel that keeps them at the smallest shape that runs all of its code: a characterisation written
against the commit before the kernels were folded into rf_sums.hip, which passes on that commit's library and on this one.

The frame is 72 x 40: 3 x 2 tiles whose right column (72 = 2 x 32 + 8) and bottom row (40 = 32 + 8) reach past the frame, so the in-frame test decides on both edges.
One batch of 70 samples is two full 32-sample chunks of the LDS-staged kernels plus a partial one of 6; a tile-list step of 35 is one chunk plus 3.  The radiance sum S
and the second moments Q are held to the oracle's per-sample radiance (tests/noise_restatement.py), the two first-hit AOV sums to tests/aov_restatement.py, bit for
bit; every other way of scheduling the same samples -- the one-lane-per-pixel kernels, other slot orders, shorter steps, the tile-list kernels of render_adaptive --
must leave the same bits."""
import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import play, prefix_sums, tile_errors, tile_slices
from aov_restatement import aov_sums
from conftest import bits, oracle_scene_from_pt
from noise_restatement import estimate, oracle_samples
from oracle import orc

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES, EXPOSURE = 72, 40, 70, 3, 0.25
TILES = 6
SLOTS = SPP * TILES * 1024                                                     # one batch: 70 samples of 6 tiles of 1024 path slots
SUMS = ("S", "Q", "AC", "ND")


def _renderer(pt, opts=()):
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), EXPOSURE)
    r = rf.ReferencePathTracer(params, pt.scene(), max_paths_in_flight=SLOTS)
    for k, v in dict(opts).items():
        r.set_option(k, v)
    r.set_moments(True)
    r.set_aovs(True, tile_counts=True)
    return r


def _reads(r):
    """The four sums as bit patterns, and every count the handle reports"""
    img, acc = r.read_accumulation()
    q, n = r.read_moments()
    a = r.read_aovs()
    ac = np.concatenate([a["albedo"], a["coverage"][..., None]], -1)
    nd = np.concatenate([a["normal"], a["depth"][..., None]], -1)
    return dict(S=bits(img), Q=bits(q), AC=bits(ac), ND=bits(nd), counts=(acc, n, a["samples"], r.read_tile_samples().reshape(-1).tolist()))


def _differing(a, b):
    return [k for k in SUMS if not np.array_equal(a[k], b[k])] + ([] if a["counts"] == b["counts"] else ["counts"])


def _uniform(pt, opts=(), steps=(SPP,), snapshots=False):
    r = _renderer(pt, opts)
    snaps = {}
    for n in steps:
        r.render(n)
        if snapshots:
            got = _reads(r)
            snaps[got["counts"][0]] = got
    got = _reads(r)
    batches = r.stats()["batches_traced"]
    r.close()
    return (got, batches, snaps) if snapshots else (got, batches)


@pytest.fixture(scope="module")
def oracle(duck_pt):
    """The oracle's per-sample radiance of the frame as prefix sums, and its AOV sums of the 70 samples (computed once; read-only)"""
    sc, _ = oracle_scene_from_pt(duck_pt)
    rp = orc.make_render_params(W, H, rf.camera_to_array(rf.fly_camera(W, H)), SPP, BOUNCES, EXPOSURE, rf.aligned_sky_state(rf.make_sky()))
    S, Q = prefix_sums(list(oracle_samples(orc, sc, rp, range(SPP))))
    ac, nd = aov_sums(sc, rp, range(SPP))
    for a in S + Q + [ac, nd]:
        a.setflags(write=False)
    return dict(S=S, Q=Q, AC=ac, ND=nd)


@pytest.fixture(scope="module")
def baseline(duck_pt):
    """render(70) with the default options: one batch, the LDS-staged kernels for all four sums"""
    r = _renderer(duck_pt)
    plan = r.launch_plan(1, SPP)
    assert plan["runs"] == 1 and plan["tile_list"] == 0 and (plan["accumulate_kernel"], plan["accumulate_pixels"]) == (1, 4), plan
    assert plan["aov_pixels"] == 8 and plan["moment_pixels"] == 16, plan
    r.render(SPP)
    got = _reads(r)
    assert r.stats()["batches_traced"] == 1
    r.close()
    return got


def test_the_staged_kernels_equal_the_restatements(oracle, baseline):
    assert baseline["counts"] == (SPP, SPP, SPP, [SPP] * TILES)
    assert oracle["S"][SPP][..., :3].any() and 0.1 < float((oracle["AC"][..., 3] > 0).mean()) < 1.0       # radiance everywhere, first hits and misses both
    assert np.array_equal(baseline["S"][..., :3], bits(oracle["S"][SPP])[..., :3]), "S"
    assert np.array_equal(baseline["Q"], bits(oracle["Q"][SPP])), "Q"
    assert np.array_equal(baseline["AC"], bits(oracle["AC"])), "albedo / coverage"
    assert np.array_equal(baseline["ND"], bits(oracle["ND"])), "normal / depth"


@pytest.mark.parametrize("name,opts,steps", [
    ("one lane per pixel", dict(accumulate_runs=0), (SPP,)),
    ("unsorted samples", dict(sample_sort=0), (SPP,)),
    ("groups of 4 pixels", dict(slot_group_shift=2), (SPP,)),
    ("sample-major slots", dict(slot_group_shift=-1), (SPP,)),
    ("render(35); render(35)", {}, (35, 35)),
    ("render(64); render(6)", {}, (64, 6)),
])
def test_uniform_variants_leave_the_same_bits(duck_pt, baseline, name, opts, steps):
    got, batches = _uniform(duck_pt, opts, steps)
    assert batches == len(steps)
    assert _differing(got, baseline) == [], name


@pytest.mark.parametrize("every", [70, 35])
@pytest.mark.parametrize("opts", [{}, dict(accumulate_runs=0)], ids=["staged", "one lane per pixel"])
def test_the_tile_list_kernels_with_every_tile_active(duck_pt, baseline, every, opts):
    """render_adaptive enqueues through the tile-list kernels even while the list is the whole frame: a target of 0 stops no tile"""
    r = _renderer(duck_pt, opts)
    res = r.render_adaptive(0.0, every)
    got = _reads(r)
    assert res["stopped_tiles"] == 0 and res["estimate_passes"] == SPP // every and res["pixel_samples"] == W * H * SPP
    assert r.stats()["batches_traced"] == SPP // every
    assert _differing(got, baseline) == []
    # the uniform state: render and render_until are not refused (the accumulation is full: nothing is traced)
    assert r.tile_samples_uniform()
    r.render(2)
    assert r.render_until(0.0, 4) == (0, None)
    assert _differing(_reads(r), baseline) == []
    r.close()


def test_a_schedule_with_stopped_tiles_leaves_each_tile_a_uniform_renders_sums(duck_pt, oracle, baseline):
    every = 35
    target = float(np.float32(np.median(tile_errors(estimate(oracle["S"][every], oracle["Q"][every], every)))))
    want = play(oracle["S"], oracle["Q"], W, H, target, every, min_samples=every)
    counts = want["counts"].tolist()
    assert set(counts) == {every, SPP}, counts                                # before the GPU is looked at: tiles stop, tiles go on (a list of part of the frame)
    last, _, snaps = _uniform(duck_pt, steps=(every, SPP - every), snapshots=True)
    assert sorted(snaps) == [every, SPP] and _differing(last, baseline) == []
    r = _renderer(duck_pt)
    res = r.render_adaptive(target, every, every)
    got = _reads(r)
    r.close()
    assert got["counts"][3] == counts and res["stopped_tiles"] == want["stopped_tiles"] > 0 and res["pixel_samples"] == want["pixel_samples"]
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"]))
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        for k in SUMS:
            assert np.array_equal(got[k][rows, cols], snaps[counts[t]][k][rows, cols]), (k, t, counts[t])


@pytest.mark.parametrize("spp,pixels", [(8, 4), (200, 2), (700, 1)])
def test_whole_runs_in_lds_by_batch_depth(duck_pt, spp, pixels):
    """kAccumulateRuns<4 / 2 / 1>: a 32 x 32 frame, one batch; the image is the one-lane-per-pixel kernel's"""
    images = []
    for runs in (1, 0):
        params = rf.make_render_parameters(32, 32, rf.fly_camera(32, 32), spp, BOUNCES, rf.make_sky(), EXPOSURE)
        r = rf.ReferencePathTracer(params, duck_pt.scene(), max_paths_in_flight=spp * 1024)
        r.set_option("accumulate_runs", runs)
        plan = r.launch_plan(1, spp)
        assert (plan["accumulate_kernel"], plan["accumulate_pixels"]) == ((1, pixels) if runs else (0, 256)), plan
        r.render(spp)
        img, acc = r.read_accumulation()
        assert acc == spp and r.stats()["batches_traced"] == 1
        images.append(bits(img))
        r.close()
    assert images[0][..., :3].any() and np.array_equal(images[0], images[1])
