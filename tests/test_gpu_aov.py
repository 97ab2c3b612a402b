"""First-hit AOVs on the GPU (-m gpu): the sums kShade<false, true> + the AOV sum kernels (rf_sums.hip) keep are bit-identical to the restatement built on the
oracle's primitives (tests/aov_restatement.py), leave the image and the ray counts alone, do not depend on any scheduling choice, and follow the
bookkeeping include/rayfinder_amd.h states."""
import os
import subprocess

import numpy as np
import pytest

import rayfinder_amd as rf
from aov_restatement import aov_sums
from conftest import ROOT, bits, oracle_scene_from_pt
from oracle import orc

pytestmark = pytest.mark.gpu


def _renderer(pt, w, h, spp, bounces, cam=None, **kw):
    cam = cam if cam is not None else rf.fly_camera(w, h)
    params = rf.make_render_parameters(w, h, cam, spp, bounces, rf.make_sky(), 0.25)
    return rf.ReferencePathTracer(params, pt.scene(), **kw), params


def _rp(params):
    return orc.make_render_params(params.width, params.height, rf.camera_to_array(params.camera), params.num_samples_per_pixel, params.num_bounces, 0.25,
                                  rf.aligned_sky_state(params.sky))


def _sums(r):
    s = r.read_aovs()
    ac = np.concatenate([s["albedo"], s["coverage"][..., None]], -1)
    nd = np.concatenate([s["normal"], s["depth"][..., None]], -1)
    return ac, nd, s["samples"]


def _same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[:2], b[:2])) and a[2] == b[2]


@pytest.fixture(scope="module")
def atrium():
    from rayfinder_amd import scenes
    pt, _ = scenes.atrium()
    return pt


@pytest.mark.parametrize("aperture", [0.0, 0.15])
def test_duck_aov_sums_bit_identical_to_the_restatement(duck_pt, aperture):
    W, H, spp = 64, 48, 16
    cam = rf.fly_camera(W, H, aperture=aperture, focus_distance=2.0) if aperture else rf.fly_camera(W, H)
    r, params = _renderer(duck_pt, W, H, spp, 3, cam=cam)
    r.set_aovs(True)
    r.render(spp)
    ac, nd, n = _sums(r)
    r.close()
    assert n == spp
    sc, _ = oracle_scene_from_pt(duck_pt)
    want_ac, want_nd = aov_sums(sc, _rp(params), range(spp))
    assert 0.2 < float((want_ac[..., 3] > 0).mean()) < 1.0            # hits and misses both
    assert np.array_equal(bits(ac), bits(want_ac)), "albedo / coverage"
    assert np.array_equal(bits(nd), bits(want_nd)), "normal / depth"


def test_atrium_1080p_one_batch_crops_and_the_image_is_unchanged(atrium):
    """32 spp of a 1080p frame in ONE batch: the LDS-staged accumulation (pixel-major slots, permuted samples); three 32x32 crops bit-identical to the
    restatement.  The same frame without the AOVs: the same image and the same ray counts, bit for bit."""
    W, H, spp, bounces = 1920, 1080, 32, 2
    tiles = ((W + 31) // 32) * ((H + 31) // 32)
    out = {}
    for aov in (True, False):
        r, params = _renderer(atrium, W, H, spp, bounces, max_paths_in_flight=spp * tiles * 1024)
        if aov:
            r.set_aovs(True)
        r.render(spp)
        img, acc = r.read_accumulation()
        s = r.stats()
        assert acc == spp and s["batches_traced"] == 1
        out[aov] = (img, {k: s[k] for k in ("primary_rays", "closest_rays", "shadow_rays", "shadow_rays_self_answered")}, _sums(r) if aov else None)
        r.close()
    assert np.array_equal(bits(out[True][0]), bits(out[False][0]))
    assert out[True][1] == out[False][1]
    ac, nd, n = out[True][2]
    assert n == spp
    sc, _ = oracle_scene_from_pt(atrium)
    rp = _rp(params)
    for (x0, y0) in [(928, 508), (64, 64), (1500, 300)]:
        want_ac, want_nd = aov_sums(sc, rp, range(spp), x0, y0, x0 + 32, y0 + 32)
        assert np.array_equal(bits(ac[y0:y0 + 32, x0:x0 + 32]), bits(want_ac)), (x0, y0)
        assert np.array_equal(bits(nd[y0:y0 + 32, x0:x0 + 32]), bits(want_nd)), (x0, y0)


def test_duck_image_and_ray_counts_unchanged_with_the_aovs(duck_pt):
    W, H, spp, bounces = 150, 90, 12, 4
    res = []
    for aov in (False, True):
        r, _ = _renderer(duck_pt, W, H, spp, bounces)
        r.set_timing(True)
        if aov:
            r.set_aovs(True)
        r.render(spp)
        s = r.stats()
        res.append((r.read_accumulation()[0], [s[k] for k in ("primary_rays", "closest_rays", "shadow_rays", "shadow_rays_self_answered", "launches_shade",
                                                              "launches_accumulate", "batches_traced")]))
        r.close()
    assert np.array_equal(bits(res[0][0]), bits(res[1][0]))
    assert res[0][1] == res[1][1]


def test_batching_slot_orders_and_kernels_are_invisible_to_the_aovs(duck_pt):
    W, H, spp, bounces = 150, 90, 23, 3
    tiles = ((W + 31) // 32) * ((H + 31) // 32)

    def run(opts=(), counting=False, max_paths=0, shard=None):
        r, _ = _renderer(duck_pt, W, H, spp, bounces, max_paths_in_flight=max_paths)
        for k, v in dict(opts).items():
            r.set_option(k, v)
        r.set_counting(counting)
        if shard is not None:
            r.set_tile_shard(*shard)
        r.set_aovs(True)
        r.render(spp)
        got = _sums(r)
        r.close()
        return got

    want = run()
    assert want[2] == spp
    assert _same(run(max_paths=tiles * 1024), want), "one sample per batch"
    for opts in (dict(slot_group_shift=-1), dict(slot_group_shift=2), dict(slot_group_shift=6, sample_sort=0), dict(slot_group_shift=10, accumulate_runs=0),
                 dict(sample_sort=0), dict(accumulate_runs=0), dict(shade_sort_from_bounce=1), dict(shade_sort_from_bounce=0), dict(traversal_variant=0)):
        for max_paths in (0, 5 * tiles * 1024):
            assert _same(run(opts, max_paths=max_paths), want), (opts, max_paths)
    assert _same(run(counting=True), want), "counting build"
    union = [np.zeros_like(want[0]), np.zeros_like(want[1])]
    for rank in range(3):
        part = run(shard=(rank, 3))
        assert part[2] == spp
        union[0] += part[0]
        union[1] += part[1]
    assert np.array_equal(bits(union[0]), bits(want[0])) and np.array_equal(bits(union[1]), bits(want[1])), "union of 3 tile shards"


def test_aov_bookkeeping(duck_pt):
    W, H, spp = 64, 48, 12
    r, params = _renderer(duck_pt, W, H, spp, 2)
    # off by default: nothing to read
    r.render(5)
    ac, nd, n = _sums(r)
    assert n == 0 and not ac.any() and not nd.any()
    mem_off = r.memory_info()
    # on after 5 frames: the sums cover frames 5.. only
    r.set_aovs(True)
    r.render(4)
    ac, nd, n = _sums(r)
    assert n == 4 and r.read_accumulation()[1] == 9
    sc, _ = oracle_scene_from_pt(duck_pt)
    rp = _rp(params)
    want_ac, want_nd = aov_sums(sc, rp, range(5, 9))
    assert np.array_equal(bits(ac), bits(want_ac)) and np.array_equal(bits(nd), bits(want_nd))
    mem_on = r.memory_info()
    assert mem_on["path_state_bytes"] == mem_on["paths_allocated"] * 180 and mem_off["path_state_bytes"] == mem_off["paths_allocated"] * 148
    # frames past spp change nothing
    r.render(100)
    ac2, nd2, n2 = _sums(r)
    assert n2 == spp - 5
    r.render(3)
    assert _same(_sums(r), (ac2, nd2, n2))
    # set_render_parameters with a change resets; sample indices continue from frameCount = 112
    r.set_render_parameters(rf.make_render_parameters(W, H, params.camera, spp, 2, params.sky, 0.5))
    ac, nd, n = _sums(r)
    assert n == 0 and not ac.any() and not nd.any()
    r.render(2)
    ac, nd, n = _sums(r)
    assert n == 2
    want_ac, want_nd = aov_sums(sc, rp, (112, 113))
    assert np.array_equal(bits(ac), bits(want_ac)) and np.array_equal(bits(nd), bits(want_nd))
    # the flags changing resets too; off frees the per-path records
    r.set_aovs(False)
    assert _sums(r)[2] == 0 and r.memory_info()["path_state_bytes"] == r.memory_info()["paths_allocated"] * 148
    r.set_aovs(True)
    r.render(1)
    assert _sums(r)[2] == 1
    m = r.aov_means()
    cov = m["coverage"] > 0
    assert np.allclose(np.linalg.norm(m["normal"][cov], axis=-1), 1.0, atol=1e-5) and (m["depth"][~cov] == 0).all() and (m["depth"][cov] > 0).all()
    assert rf._ffi.lib.rf_renderer_set_aovs(r._h, 2) == rf._ffi.RF_ERROR_INVALID_ARGUMENT and _sums(r)[2] == 1   # refused, state kept
    r.close()


def _read_pfm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    kind, (w, h) = parts[0], map(int, parts[1].split())
    assert parts[2] == b"-1.0"
    ch = 3 if kind == b"PF" else 1
    img = np.frombuffer(parts[3], "<f4").reshape(h, w, ch)[::-1]
    return img if ch == 3 else img[..., 0]


def test_rf_render_aov_pfms_equal_aov_means_and_do_not_depend_on_the_rank_count(duck_pt, tmp_path):
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    W, H, spp, bounces = 200, 150, 4, 3
    files = {}
    for gpus in (1, 2):
        names = [tmp_path / f"g{gpus}_{k}.pfm" for k in ("albedo", "normal", "depth")]
        env = dict(os.environ, RF_COMM_TRANSPORT="local", RF_COMM_TIMEOUT_S="120")
        txt = subprocess.check_output([exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces), "--out", str(tmp_path / f"g{gpus}.png"),
                                       "--aov-albedo", str(names[0]), "--aov-normal", str(names[1]), "--aov-depth", str(names[2]), "--gpus", str(gpus)], env=env, timeout=300).decode()
        assert f"on {gpus} GPU(s)" in txt
        files[gpus] = [open(p, "rb").read() for p in names]
        if gpus == 1:
            albedo, normal, depth = (_read_pfm(p) for p in names)
    assert files[2] == files[1]
    assert files[1][2].startswith(b"Pf\n")
    r, _ = _renderer(duck_pt, W, H, spp, bounces)          # rf-render's defaults: fly camera, default sky
    r.set_aovs(True)
    r.render(spp)
    m = r.aov_means()
    r.close()
    assert np.array_equal(bits(albedo), bits(m["albedo"])) and np.array_equal(bits(normal), bits(m["normal"])) and np.array_equal(bits(depth), bits(m["depth"]))
