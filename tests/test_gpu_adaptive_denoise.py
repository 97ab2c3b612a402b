"""Tile-adaptive sampling with the first-hit AOVs and the denoiser on the GPU (-m gpu): with RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS rf_renderer_render_adaptive keeps
its schedule and its radiance sums, every tile's AOV sums are bit for bit those of a uniform render of that tile's count (the path tests/test_gpu_aov.py holds to the
oracle), whatever accumulate kernel and slot order ran, and rf_renderer_denoise / rf_denoise_tiles equal the numpy restatement with one count per tile
(tests/denoise_tiles_restatement.py).  Targets and expected schedules come from the restatements alone, never from the code under test."""
import functools
import os
import subprocess

import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import play, tile_errors, tile_slices
from aov_restatement import aov_sums
from conftest import DUCK, ROOT, bits, oracle_scene_from_pt
from denoise_restatement import denoise
from denoise_tiles_restatement import denoise_tiles, pixel_counts
from noise_restatement import estimate, same_estimate
from oracle import orc
from test_gpu_adaptive import BOUNCES, EVERY, EXPOSURE, H, SPP, TILES, W, _camera, _oracle, _reads, _refused, _renderer, _same_reads, _target, _want
from test_gpu_denoise import SIGMAS, _synthetic, _tonemap

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT


def _aov_renderer(pt, w=W, h=H, spp=SPP, aperture=0.0, opts=(), tile_counts=True, **kw):
    r = _renderer(pt, w, h, spp, aperture, opts, **kw)
    r.set_aovs(True, tile_counts=tile_counts)
    return r


def _aovs(r):
    """The AOV sums as the denoiser takes them: ({albedo.rgb, coverage}, {normal.xyz, depth}) (H, W, 4) f32, and the AOV sample count"""
    s = r.read_aovs()
    return np.concatenate([s["albedo"], s["coverage"][..., None]], -1), np.concatenate([s["normal"], s["depth"][..., None]], -1), s["samples"]


@functools.lru_cache(maxsize=None)
def _uniform_aovs(w=W, h=H, spp=SPP, aperture=0.0, step=EVERY):
    """A second, UNIFORM handle with set_aovs(True) stepped in `step`s (the last step shorter): (AC, ND, S) bit patterns after step, 2 step, ..., spp samples"""
    pt = rf.PtFormat.from_gltf(DUCK)
    r = _renderer(pt, w, h, spp, aperture, moments=False)
    r.set_aovs(True)
    snaps, n = {}, 0
    while n < spp:
        r.render(min(step, spp - n))
        n += min(step, spp - n)
        ac, nd, m = _aovs(r)
        assert m == n
        snaps[n] = (bits(ac), bits(nd), bits(r.read_accumulation()[0]))
    r.close()
    return snaps


def _tiles_equal_the_uniform_handles(ac, nd, counts, snaps, w, h):
    for t, (rows, cols) in enumerate(tile_slices(w, h)):
        want_ac, want_nd, _ = snaps[int(counts[t])]
        assert np.array_equal(bits(ac)[rows, cols], want_ac[rows, cols]), ("albedo / coverage of tile", t, int(counts[t]))
        assert np.array_equal(bits(nd)[rows, cols], want_nd[rows, cols]), ("normal / depth of tile", t, int(counts[t]))


@pytest.fixture(scope="module")
def frame(duck_pt):
    """The adaptive tests' frame with the AOVs kept per tile count, in the non-uniform state; read-only for the tests that share it"""
    want = _want()                                                            # (asserts, before the GPU is looked at, >= 3 distinct counts with tiles at 4 and at 32)
    r = _aov_renderer(duck_pt)
    r.set_timing(False)
    res = r.render_adaptive(_target(), EVERY, EVERY)
    ac, nd, n = _aovs(r)
    out = dict(r=r, res=res, reads=_reads(r), ac=ac, nd=nd, n=n, S=r.read_accumulation()[0], counts=r.read_tile_samples().reshape(-1), want=want)
    yield out
    r.close()


def test_schedule_and_radiance_are_untouched_by_the_aovs(duck_pt, frame):
    want, got, res = frame["want"], frame["reads"], frame["res"]
    assert got["counts"].tolist() == want["counts"].tolist()
    assert got["acc"] == SPP and got["n"] == SPP
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"]))
    assert np.array_equal(got["mean"], bits(want["mean"]))
    assert np.array_equal(got["bgra"].reshape(-1), orc.tonemap_bgra8(want["mean"].reshape(-1, 4), 1, EXPOSURE))
    for k in ("estimate_passes", "stopped_tiles", "min_tile_samples", "max_tile_samples", "pixel_samples"):
        assert res[k] == want[k], k
    assert res["tiles"] == TILES
    assert same_estimate(dict(res["last"], error_map=0, tile_sum=0, tile_max=0), dict(want["last"], error_map=0, tile_sum=0, tile_max=0)) == []
    assert frame["r"].stats()["primary_rays"] == want["pixel_samples"] < W * H * SPP
    # the same values as with the AOVs off, result struct included
    off = _renderer(duck_pt)
    res_off = off.render_adaptive(_target(), EVERY, EVERY)
    assert _same_reads(_reads(off), got) == [] and res_off == res
    off.close()


def test_every_tiles_aov_sums_are_a_uniform_renders_at_its_count(duck_pt, frame):
    counts = frame["want"]["counts"]
    assert frame["n"] == SPP                                                  # the AOV sample count advances with L
    _tiles_equal_the_uniform_handles(frame["ac"], frame["nd"], counts, _uniform_aovs(), W, H)
    # pixels outside every tile's in-frame part do not exist in a row-major read; inside, nothing but the tiles: the whole frame is covered by the comparison above
    # ... and two tiles against the oracle directly: an interior one and the ragged bottom-right corner (22 x 26 pixels)
    sc, _ = oracle_scene_from_pt(duck_pt)
    rp = orc.make_render_params(W, H, rf.camera_to_array(_camera(W, H)), SPP, BOUNCES, EXPOSURE, rf.aligned_sky_state(rf.make_sky()))
    slices = tile_slices(W, H)
    for t in (6, TILES - 1):
        rows, cols = slices[t]
        want_ac, want_nd = aov_sums(sc, rp, range(int(counts[t])), cols.start, rows.start, cols.stop, rows.stop)
        assert np.array_equal(bits(frame["ac"][rows, cols]), bits(want_ac)) and np.array_equal(bits(frame["nd"][rows, cols]), bits(want_nd)), (t, int(counts[t]))
    # aov_means divides every pixel by its own tile's count
    means = frame["r"].aov_means()
    nf = pixel_counts(counts, H, W)
    assert means["samples"] == SPP and np.array_equal(bits(means["albedo"]), bits(frame["ac"][..., :3] / nf[..., None]))
    assert np.array_equal(bits(means["coverage"]), bits(frame["ac"][..., 3] / nf)) and float(means["coverage"].max()) == 1.0


@pytest.mark.parametrize("name,w,h,spp,every,aperture,opts", [
    ("one thread per pixel", 64, 64, 32, 4, 0.0, {}),
    ("runs kernel, one chunk", 64, 64, 32, 8, 0.0, {}),
    ("runs kernel, two chunks: 32 + 8", 64, 64, 48, 40, 0.0, {}),
    ("a last step that is shorter", 64, 64, 32, 3, 0.0, {}),
    ("a last step that is shorter, runs kernel", 64, 64, 32, 5, 0.0, {}),
    ("sample-major slots", 64, 64, 32, 8, 0.0, dict(slot_group_shift=-1)),
    ("groups of 4 pixels", 64, 64, 32, 8, 0.0, dict(slot_group_shift=2)),
    ("no sample permutation", 64, 64, 32, 8, 0.0, dict(sample_sort=0)),
    ("runs kernels off", 64, 64, 32, 8, 0.0, dict(accumulate_runs=0)),
    ("a thin lens: sample permutation with real keys", 64, 64, 32, 8, 0.15, {}),
    ("a thin lens, one thread per pixel", 64, 64, 32, 4, 0.15, {}),
    ("smaller than one tile", 20, 12, 32, 4, 0.0, {}),
    ("ragged tiles, runs kernel", W, H, SPP, 8, 0.0, {}),
])
def test_every_accumulate_path_leaves_the_uniform_sums(duck_pt, name, w, h, spp, every, aperture, opts):
    S, Q, _ = _oracle(w, h, spp, aperture)
    first = max(every, 2)
    target = float(np.float32(np.median(tile_errors(estimate(S[first], Q[first], first)))))
    want = play(S, Q, w, h, target, every, min_samples=0)
    if w * h > 1024:
        assert want["stopped_tiles"] > 0, want["counts"]                      # a real schedule: the batches after the first check cover a tile LIST
    r = _aov_renderer(duck_pt, w, h, spp, aperture, opts)
    res = r.render_adaptive(target, every)
    got = _reads(r)
    ac, nd, n = _aovs(r)
    r.close()
    print(name, "counts:", got["counts"].tolist())
    assert got["counts"].tolist() == want["counts"].tolist() and n == want["leading"]
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"]))
    assert res["estimate_passes"] == want["estimate_passes"] and res["pixel_samples"] == want["pixel_samples"]
    _tiles_equal_the_uniform_handles(ac, nd, want["counts"], _uniform_aovs(w, h, spp, aperture, every), w, h)


@pytest.mark.parametrize("L", [0, 1, 5])
def test_the_handles_denoise_equals_the_restatement_and_leaves_the_state(frame, L):
    r = frame["r"]
    before, stats = _reads(r), r.stats()
    for sig in SIGMAS:
        r.denoise(iterations=L, **sig)
        rgb, bgra, m = r.read_denoised()
        assert m == SPP                                                       # the snapshot's count is the leading count
        want = denoise_tiles(frame["S"], frame["ac"], frame["nd"], frame["counts"], iterations=L, **sig)
        assert np.array_equal(bits(rgb), bits(want)), (L, sig)
        assert np.array_equal(bgra, _tonemap(r, rgb))
    # (the per-tile counts do show in this frame: the one-count filter at L gives another image)
    assert not np.array_equal(bits(rgb), bits(denoise(frame["S"], frame["ac"], frame["nd"], SPP, iterations=L, **SIGMAS[-1])))
    ac, nd, n = _aovs(r)
    assert _same_reads(_reads(r), before) == [] and n == SPP
    assert np.array_equal(bits(ac), bits(frame["ac"])) and np.array_equal(bits(nd), bits(frame["nd"]))
    after = r.stats()
    assert all(after[k] == stats[k] for k in ("primary_rays", "closest_rays", "shadow_rays", "batches_traced", "launches_accumulate")), (stats, after)


def test_denoise_tiles_on_the_handles_reads_gives_the_handles_bits(frame):
    r = frame["r"]
    for sig in SIGMAS:
        for L in (0, 5):
            r.denoise(iterations=L, **sig)
            rgb, bgra, _ = r.read_denoised()
            rgb2, bgra2 = rf.denoise_tiles(frame["S"], frame["ac"], frame["nd"], frame["counts"], exposure=EXPOSURE, iterations=L, **sig)
            assert np.array_equal(bits(rgb), bits(rgb2)) and np.array_equal(bgra, bgra2), (L, sig)


@pytest.mark.parametrize("h,w", [(23, 37), (144, 256)])
def test_denoise_tiles_bit_identical_to_the_restatement_on_synthetic_sums(h, w):
    """Random per-tile counts in 1 .. 9; the sums of a tile with n samples are n / 9 of the 9-sample synthetic sums."""
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    counts = np.random.default_rng(h * 1000 + w).integers(1, 10, tiles).astype(np.uint32)
    assert tiles == 2 or len(set(counts.tolist())) >= 5
    scale = (pixel_counts(counts, h, w) / np.float32(9))[..., None]
    S, AC, ND = ((a * scale).astype(np.float32) for a in _synthetic(h, w, 9, h * 1000 + w))
    assert (AC[..., 3] == 0).any() and (AC[..., 3] > 0).any()
    for sig in SIGMAS:
        for L in range(9):
            rgb, bgra = rf.denoise_tiles(S, AC, ND, counts, exposure=0.25, iterations=L, **sig)
            assert np.array_equal(bits(rgb), bits(denoise_tiles(S, AC, ND, counts, iterations=L, **sig))), (h, w, L, sig)
    # all counts equal: rf_denoise_images, bit for bit
    for n in (1, 6):
        same = np.full(tiles, n, np.uint32)
        for L in (0, 5):
            a, b = rf.denoise_tiles(S, AC, ND, same, exposure=0.25, iterations=L), rf.denoise_images(S, AC, ND, n, exposure=0.25, iterations=L)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (n, L)


def test_the_mode_bit_changes_nothing_before_an_adaptive_call_and_the_flags_keep_their_books(duck_pt):
    lib = rf._ffi.lib
    a, b = _aov_renderer(duck_pt, tile_counts=True), _aov_renderer(duck_pt, tile_counts=False)
    for r in (a, b):
        r.render(8)
    ra, rb = _reads(a), _reads(b)
    assert _same_reads(ra, rb) == [] and a.stats()["primary_rays"] == b.stats()["primary_rays"] == W * H * 8
    sa, sb = _aovs(a), _aovs(b)
    assert sa[2] == sb[2] == 8 and np.array_equal(bits(sa[0]), bits(sb[0])) and np.array_equal(bits(sa[1]), bits(sb[1])) and sa[0].any()
    snaps = _uniform_aovs()
    assert np.array_equal(bits(sa[0]), snaps[8][0]) and np.array_equal(bits(sa[1]), snaps[8][1])
    # 0x100 alone and 2: refused, the state kept (sums, count, and -- below -- the mode bit)
    for r in (a, b):
        for flags in (0x100, 2):
            assert lib.rf_renderer_set_aovs(r._h, flags) == INVALID
        assert _aovs(r)[2] == 8
    assert _refused(lambda: a.set_aovs(False, tile_counts=True), "RF_AOV_FIRST_HIT")
    a.set_aovs(True, tile_counts=True)                                        # the value it has: nothing restarts
    assert _aovs(a)[2] == 8
    # 1 <-> 0x101: the AOV sums restart (count 0, zeros), the image stays
    b.set_aovs(True, tile_counts=True)
    ac, nd, n = _aovs(b)
    assert n == 0 and not ac.any() and not nd.any() and _same_reads(_reads(b), rb) == []
    assert _refused(lambda: b.render_adaptive(0.1, 4), "cover", "AOV")        # on (with the bit) partway through: 0 of 8 samples
    assert _refused(b.denoise, "AOV")
    b.set_aovs(True, tile_counts=False)
    assert _refused(lambda: b.render_adaptive(0.1, 4), "AOV", "RF_AOV_TILE_COUNTS")   # without the bit: as ever, and the message names the bit
    b.render(4)
    assert _aovs(b)[2] == 4 and b.read_accumulation()[1] == 12
    b.set_aovs(True, tile_counts=True)
    assert _aovs(b)[2] == 0 and b.read_accumulation()[1] == 12
    b.close()
    # a kept the bit through the refusals: render_adaptive continues from the uniform 8 samples
    res = a.render_adaptive(0.0, EVERY, EVERY, 16)
    ac, nd, n = _aovs(a)
    assert res["min_tile_samples"] == res["max_tile_samples"] == 16 and n == 16
    assert np.array_equal(bits(ac), snaps[16][0]) and np.array_equal(bits(nd), snaps[16][1])
    a.close()
    # the AOVs (mode bit) turned on after 2 samples of a fresh accumulation
    r = _renderer(duck_pt)
    r.render(2)
    r.set_aovs(True, tile_counts=True)
    assert _refused(lambda: r.render_adaptive(0.1, 4), "cover", "AOV")
    r.close()


def test_the_non_uniform_state_without_covering_aovs_refuses_denoise(duck_pt):
    why = "different sample counts"
    r = _renderer(duck_pt)                                                    # the AOVs never on
    assert r.render_adaptive(_target(), EVERY, EVERY)["stopped_tiles"] > 0
    assert _refused(r.denoise, why, "RF_AOV_TILE_COUNTS")
    r.set_aovs(True, tile_counts=True)                                        # on now: they cover nothing of the accumulation
    assert _refused(r.denoise, why) and _refused(lambda: r.render_adaptive(0.0, 4), "cover")
    r.set_aovs(True, tile_counts=False)
    assert _refused(r.denoise, why)
    with pytest.raises(rf.RayfinderError):
        r.read_denoised()
    r.close()


def test_target_zero_leaves_the_ordinary_state_aovs_included(duck_pt):
    r = _aov_renderer(duck_pt)
    res = r.render_adaptive(0.0, EVERY, EVERY)
    assert res["stopped_tiles"] == 0 and r.read_tile_samples().reshape(-1).tolist() == [SPP] * TILES
    ac, nd, n = _aovs(r)
    snaps = _uniform_aovs()
    assert n == SPP and np.array_equal(bits(ac), snaps[SPP][0]) and np.array_equal(bits(nd), snaps[SPP][1])
    assert np.array_equal(bits(r.read_accumulation()[0]), snaps[SPP][2])
    # render and render_until run (into the full accumulation: nothing is traced), and denoise is the uniform handle's
    r.render(2)
    assert r.render_until(0.0, 4) == (0, None)
    r.denoise()
    rgb, bgra, m = r.read_denoised()
    assert m == SPP and np.array_equal(bits(rgb), bits(denoise(r.read_accumulation()[0], ac, nd, SPP)))
    u = _renderer(duck_pt, moments=False)
    u.set_aovs(True)
    u.render(SPP)
    u.denoise()
    rgb_u, bgra_u, m_u = u.read_denoised()
    assert m_u == SPP and np.array_equal(bits(rgb), bits(rgb_u)) and np.array_equal(bgra, bgra_u)
    u.close()
    r.close()


def test_a_second_call_moves_only_the_leading_tiles_aov_sums_included(duck_pt):
    S, Q, errors = _oracle(W, H, SPP)
    first = play(S, Q, W, H, _target(), EVERY, min_samples=EVERY, max_samples=16)
    assert first["stopped_tiles"] > 0
    lower = float(np.float32(np.sort(errors)[3]))                             # below the median: were stopped tiles revived, some of them would move
    second = play(S, Q, W, H, lower, EVERY, min_samples=EVERY, counts=first["counts"])
    snaps = _uniform_aovs()
    r = _aov_renderer(duck_pt)
    r.render_adaptive(_target(), EVERY, EVERY, 16)
    ac, nd, n = _aovs(r)
    assert r.read_tile_samples().reshape(-1).tolist() == first["counts"].tolist() and n == 16
    _tiles_equal_the_uniform_handles(ac, nd, first["counts"], snaps, W, H)
    r.denoise()
    stopped = first["counts"] != 16
    r.render_adaptive(lower, EVERY, EVERY)
    ac2, nd2, n2 = _aovs(r)
    counts = r.read_tile_samples().reshape(-1)
    assert counts.tolist() == second["counts"].tolist() and n2 == second["leading"]
    assert (counts[stopped] == first["counts"][stopped]).all() and (counts[~stopped] > 16).all()
    _tiles_equal_the_uniform_handles(ac2, nd2, second["counts"], snaps, W, H)
    for t, (rows, cols) in enumerate(tile_slices(W, H)):                      # a stopped tile's AOV sums were not touched
        if stopped[t]:
            assert np.array_equal(bits(ac2[rows, cols]), bits(ac[rows, cols])) and np.array_equal(bits(nd2[rows, cols]), bits(nd[rows, cols])), t
    assert r.read_denoised()[2] == 16                                         # the snapshot stays as it was until denoise runs again
    # set_render_parameters with a change clears the counts, the image and the AOVs together, and drops the snapshot
    r.set_render_parameters(rf.make_render_parameters(W, H, _camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
    ac3, nd3, n3 = _aovs(r)
    assert r.read_tile_samples().reshape(-1).tolist() == [0] * TILES and r.read_accumulation()[1] == 0 and n3 == 0 and not ac3.any() and not nd3.any()
    assert not r.read_accumulation()[0].any()
    assert _refused(r.read_denoised, "no denoised image") and _refused(r.denoise, "no sample")
    r.close()


def _read_pfm3(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    kind, (w, h) = parts[0], map(int, parts[1].split())
    assert kind == b"PF" and parts[2] == b"-1.0"
    return np.frombuffer(parts[3], "<f4").reshape(h, w, 3)[::-1]


def test_rf_render_adaptive_with_the_denoiser_and_the_aovs(duck_pt, frame, tmp_path):
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    base = [exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(SPP), "--bounces", str(BOUNCES), "--out", str(tmp_path / "o.png")]
    target = _target()                                                        # rf-render's defaults are this file's camera, sky and exposure; %.9g round-trips an f32
    txt = subprocess.check_output(base + ["--adaptive", "%.9g" % target, "--adaptive-min", str(EVERY), "--adaptive-every", str(EVERY), "--denoise", str(tmp_path / "d.png"),
                                          "--denoise-pfm", str(tmp_path / "d.pfm"), "--aov-albedo", str(tmp_path / "a.pfm"), "--sample-map", str(tmp_path / "s.pfm")],
                                  timeout=120).decode()
    want = frame["want"]
    assert f"{want['stopped_tiles']} of {TILES} tiles stopped early" in txt and f"{want['pixel_samples']} of {W * H * SPP} pixel-samples" in txt, txt
    r = frame["r"]
    r.denoise()
    rgb, _, _ = r.read_denoised()
    assert _read_pfm3(tmp_path / "d.pfm").tobytes() == np.ascontiguousarray(rgb, np.float32).tobytes()
    nf = pixel_counts(frame["counts"], H, W)
    assert _read_pfm3(tmp_path / "a.pfm").tobytes() == np.ascontiguousarray(frame["ac"][..., :3] / nf[..., None], np.float32).tobytes()
    assert os.path.getsize(tmp_path / "d.png") > 0
    bad = subprocess.run(base + ["--adaptive", "0.1", "--gpus", "2"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--adaptive needs --gpus 1" in bad.stderr
    bad = subprocess.run(base + ["--adaptive", "0.1", "--noise-target", "0.1"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--adaptive needs --gpus 1" in bad.stderr
