"""The bucket sums under tile-adaptive sampling and the robust mean with one count per tile, on the GPU (-m gpu): with K | RF_BUCKETS_TILE_COUNTS
rf_renderer_render_adaptive keeps its schedule and its other sums, the K planes of every tile are bit for bit tests/robust_restatement.py's bucket sums of the oracle's
first tile_samples[t] samples -- whatever accumulate kernel, slot order or batching ran --, and rf_renderer_robust_mean / rf_robust_mean_tiles /
rf_renderer_denoise_robust equal tests/robust_tiles_restatement.py.  Every comparison is exact.  Targets and expected schedules come from the restatements alone, never
from the code under test; the conditions a frame is chosen for are asserted from the restatement before the GPU is looked at."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import play, prefix_sums, tile_errors, tile_slices
from conftest import DUCK, ROOT, bits, oracle_scene_from_pt
from noise_restatement import estimate, oracle_samples
from oracle import orc
from robust_restatement import bucket_sizes, bucket_sums, robust_mean
from robust_tiles_restatement import denoise_robust_tiles, robust_mean_tiles
from test_gpu_adaptive import BOUNCES, EXPOSURE, H, SPP, TILES, W, _camera, _reads, _renderer, _same_reads

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
K, EVERY, MIN = 9, 4, 12                                                      # frames A and B: 150 x 90 (5 x 3 tiles, ragged right and bottom), 32 spp
COUNTS_A = [12, 32, 32, 12, 12, 12, 32, 32, 32, 12, 12, 32, 32, 12, 12]
COUNTS_B = [12, 32, 32, 16, 16, 12, 32, 32, 32, 12, 12, 32, 32, 20, 12]
LENS = 0.15


def _refused(call, *words):
    with pytest.raises(rf.RayfinderError) as e:
        call()
    assert e.value.status == INVALID, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@functools.lru_cache(maxsize=None)
def _samples(w=W, h=H, spp=SPP, aperture=0.0):
    """The oracle's per-sample radiance of Duck and its prefix sums (computed once per shape; read-only)"""
    pt = rf.PtFormat.from_gltf(DUCK)
    sc, _ = oracle_scene_from_pt(pt)
    rp = orc.make_render_params(w, h, rf.camera_to_array(_camera(w, h, aperture)), spp, BOUNCES, EXPOSURE, rf.aligned_sky_state(rf.make_sky()))
    samples = list(oracle_samples(orc, sc, rp, range(spp)))
    S, Q = prefix_sums(samples)
    for a in samples + S + Q:
        a.setflags(write=False)
    return samples, S, Q


def _tile_planes(samples, counts, k, w, h):
    """The defining property: the K planes of tile t are bucket_sums of its first counts[t] samples"""
    per_n = {int(n): bucket_sums(samples[:int(n)], k) if n else np.zeros((k, h, w, 4), np.float32) for n in np.unique(counts)}
    B = np.zeros((k, h, w, 4), np.float32)
    for t, (rows, cols) in enumerate(tile_slices(w, h)):
        B[:, rows, cols] = per_n[int(counts[t])][:, rows, cols]
    return B


def _target(aperture=0.0):
    """Frame A: the median of the restatement's tile errors at L = 12; frame B (the thin lens): their 0.3 quantile"""
    _, S, Q = _samples(aperture=aperture)
    errors = tile_errors(estimate(S[MIN], Q[MIN], MIN))
    return float(np.float32(np.median(errors) if aperture == 0.0 else np.quantile(errors, 0.3)))


@functools.lru_cache(maxsize=None)
def _want(aperture=0.0):
    """The restatement's frame: the schedule, the planes, the combine -- and the conditions it was chosen for, before the GPU is looked at"""
    samples, S, Q = _samples(aperture=aperture)
    want = play(S, Q, W, H, _target(aperture), EVERY, min_samples=MIN)
    counts = want["counts"]
    assert counts.tolist() == (COUNTS_A if aperture == 0.0 else COUNTS_B), counts.tolist()
    want["B"] = _tile_planes(samples, counts, K, W, H)
    want["M"], want["trim"] = robust_mean_tiles(want["B"], counts, W, H)
    nf = np.zeros((H, W), np.int64)
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        nf[rows, cols] = counts[t]
    want["pixel_counts"] = nf
    trimmed = {int(n): int((want["trim"][nf == n] > 0).sum()) for n in np.unique(counts)}
    pixels = {int(n): int((nf == n).sum()) for n in np.unique(counts)}
    print("frame", "A" if aperture == 0.0 else "B", "counts", counts.tolist(), "trimmed of pixels per count", trimmed, pixels, "max trim", int(want["trim"].max()))
    assert len(trimmed) >= 2
    if aperture == 0.0:                                                       # tiles at two counts, trimmed and untrimmed pixels at each
        assert trimmed == {12: 26, 32: 265} and pixels == {12: 6716, 32: 6784} and int(want["trim"].max()) == 3
        assert bucket_sizes(K, 12) == [2, 2, 2, 1, 1, 1, 1, 1, 1]
    else:                                                                     # four distinct counts, trimmed pixels at 20 and at 32
        assert len(trimmed) == 4 and trimmed[20] > 0 and trimmed[32] > 0
    assert all(0 < trimmed[n] < pixels[n] for n in (12, 32) if aperture == 0.0)
    return want


def _bucket_renderer(pt, k=K, tile_counts=True, aovs=False, **kw):
    r = _renderer(pt, **kw)
    if aovs:
        r.set_aovs(True, tile_counts=True)
    if k:
        r.set_buckets(k, tile_counts=tile_counts)
    return r


def _aovs(r):
    s = r.read_aovs()
    return np.concatenate([s["albedo"], s["coverage"][..., None]], -1), np.concatenate([s["normal"], s["depth"][..., None]], -1), s["samples"]


def _rays(r):
    st = r.stats()
    return st["primary_rays"], st["closest_rays"], st["shadow_rays"]


def _frame(pt, aperture, aovs):
    want = _want(aperture)
    r = _bucket_renderer(pt, aovs=aovs, aperture=aperture)
    res = r.render_adaptive(_target(aperture), EVERY, MIN)
    B, n = r.read_buckets()
    return dict(r=r, res=res, reads=_reads(r), rays=_rays(r), B=B, n=n, counts=r.read_tile_samples().reshape(-1), want=want, aperture=aperture)


@pytest.fixture(scope="module")
def frame_a(duck_pt):
    """Frame A with K = 9 | the bit and the AOVs kept per tile count, in the non-uniform state; read-only for the tests that share it"""
    f = _frame(duck_pt, 0.0, True)
    yield f
    f["r"].close()


@pytest.fixture(scope="module")
def frame_b(duck_pt):
    f = _frame(duck_pt, LENS, False)
    yield f
    f["r"].close()


@pytest.fixture(params=["A", "B"])
def frame(request):
    return request.getfixturevalue("frame_a" if request.param == "A" else "frame_b")


# ---- 1. the planes
def test_every_tiles_planes_are_the_bucket_sums_of_its_own_samples(duck_pt, frame):
    want, aperture = frame["want"], frame["aperture"]
    assert frame["counts"].tolist() == want["counts"].tolist()
    assert frame["n"] == SPP and frame["B"].shape == (K, H, W, 4)             # the bucket sample count advances with L; K is reported without the bit
    assert np.array_equal(bits(frame["B"]), bits(want["B"]))
    # S, Q, the counts, the mean, the texels, *result and the ray counts: a run with the buckets off
    off = _renderer(duck_pt, aperture=aperture)
    res_off = off.render_adaptive(_target(aperture), EVERY, MIN)
    assert _same_reads(_reads(off), frame["reads"]) == [] and res_off == frame["res"] and _rays(off) == frame["rays"]
    assert frame["rays"][0] == want["pixel_samples"] < W * H * SPP
    off.close()
    assert np.array_equal(frame["reads"]["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(frame["reads"]["Q"], bits(want["Q"]))
    # a second handle with set_buckets(9) WITHOUT the bit, stepped uniformly in fours: the same planes per tile at the tile's count
    u = _bucket_renderer(duck_pt, tile_counts=False, aperture=aperture, moments=False)
    snaps = {}
    for n in range(EVERY, SPP + 1, EVERY):
        u.render(EVERY)
        snaps[n], m = u.read_buckets()
        assert m == n
    u.close()
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        assert np.array_equal(bits(frame["B"][:, rows, cols]), bits(snaps[int(want["counts"][t])][:, rows, cols])), t


# ---- 2. every accumulate path
@pytest.mark.parametrize("name,w,h,spp,every,aperture,opts,counts,trimmed_tiles", [
    ("defaults: runs kernel, one chunk", 64, 64, 32, 8, 0.0, {}, [16, 8, 8, 16], 3),
    ("runs kernels off", 64, 64, 32, 8, 0.0, dict(accumulate_runs=0), [16, 8, 8, 16], 3),
    ("sample-major slots", 64, 64, 32, 8, 0.0, dict(slot_group_shift=-1), [16, 8, 8, 16], 3),
    ("groups of 4 pixels", 64, 64, 32, 8, 0.0, dict(slot_group_shift=2), [16, 8, 8, 16], 3),
    ("no sample permutation", 64, 64, 32, 8, 0.0, dict(sample_sort=0), [16, 8, 8, 16], 3),
    ("a thin lens: sample permutation with real keys", 64, 64, 32, 8, LENS, {}, None, None),
    ("runs kernel, two chunks: 32 + 8", 64, 64, 48, 40, 0.0, {}, None, None),
    ("a last step that is shorter, runs kernel", 64, 64, 32, 5, 0.0, {}, None, None),
    ("batches shorter than K whose phase wraps", 64, 64, 32, 3, 0.0, {}, None, None),
    ("smaller than one tile", 20, 12, 32, 8, 0.0, {}, [8], 1),
])
def test_every_accumulate_path_leaves_the_bucket_sums(duck_pt, name, w, h, spp, every, aperture, opts, counts, trimmed_tiles):
    k = 5
    samples, S, Q = _samples(w, h, spp, aperture)
    first = max(every, 2)
    target = float(np.float32(np.median(tile_errors(estimate(S[first], Q[first], first)))))
    want = play(S, Q, w, h, target, every, min_samples=0)
    if counts is not None:
        assert want["counts"].tolist() == counts, want["counts"].tolist()
        _, trim = robust_mean_tiles(_tile_planes(samples, want["counts"], k, w, h), want["counts"], w, h)
        assert sum(bool((trim[rows, cols] > 0).any()) for rows, cols in tile_slices(w, h)) == trimmed_tiles
        if w * h < 1024:
            assert int((trim > 0).sum()) == 2
    elif w * h > 1024:
        assert want["stopped_tiles"] > 0, want["counts"]                      # a real schedule: the batches after the first check cover a tile LIST
    r = _bucket_renderer(duck_pt, k=k, w=w, h=h, spp=spp, aperture=aperture, opts=opts)
    res = r.render_adaptive(target, every)
    got = _reads(r)
    B, n = r.read_buckets()
    r.close()
    print(name, "counts:", got["counts"].tolist())
    assert got["counts"].tolist() == want["counts"].tolist() and n == want["leading"]
    assert np.array_equal(got["S"][..., :3], bits(want["S"])[..., :3]) and np.array_equal(got["Q"], bits(want["Q"]))
    assert res["estimate_passes"] == want["estimate_passes"] and res["pixel_samples"] == want["pixel_samples"]
    assert np.array_equal(bits(B), bits(_tile_planes(samples, want["counts"], k, w, h))), name


# ---- 3. a later call continues
def test_a_second_call_continues_the_planes(duck_pt, frame_a):
    samples, S, Q = _samples()
    first = play(S, Q, W, H, _target(), EVERY, min_samples=MIN, max_samples=16)
    second = play(S, Q, W, H, _target(), EVERY, min_samples=MIN, counts=first["counts"])
    assert first["stopped_tiles"] > 0 and second["counts"].tolist() == COUNTS_A
    r = _bucket_renderer(duck_pt)
    r.render_adaptive(_target(), EVERY, MIN, 16)
    B, n = r.read_buckets()
    assert r.read_tile_samples().reshape(-1).tolist() == first["counts"].tolist() and n == 16
    assert np.array_equal(bits(B), bits(_tile_planes(samples, first["counts"], K, W, H)))
    r.render_adaptive(_target(), EVERY, MIN)
    B, n = r.read_buckets()
    assert r.read_tile_samples().reshape(-1).tolist() == COUNTS_A and n == SPP
    r.close()
    assert np.array_equal(bits(B), bits(frame_a["B"])) and np.array_equal(bits(B), bits(frame_a["want"]["B"]))


# ---- 4. the combine
def test_the_combine_takes_every_tiles_own_count(frame):
    r, want = frame["r"], frame["want"]
    before = _reads(r)
    r.robust_mean()
    got = r.read_robust_mean()
    assert got["samples"] == SPP                                              # the snapshot's count is the leading count
    assert np.array_equal(got["trim"], want["trim"]) and np.array_equal(bits(got["mean"]), bits(want["M"]))
    texels = orc.tonemap_bgra8(np.concatenate([want["M"], np.ones((H, W, 1), np.float32)], -1).reshape(-1, 4), 1, EXPOSURE)
    assert np.array_equal(got["bgra8"].reshape(-1), texels)
    assert _same_reads(_reads(r), before) == [] and np.array_equal(bits(r.read_buckets()[0]), bits(frame["B"]))
    # the host twin over the row-major reads: the tile-major and the row-major forms agree
    twin = rf.robust_mean_tiles(frame["B"], frame["counts"], exposure=EXPOSURE)
    assert all(np.array_equal(twin[k], got[k]) for k in ("trim", "bgra8")) and np.array_equal(bits(twin["mean"]), bits(got["mean"]))
    # (the per-tile counts do show: the one-count combine at L gives another image)
    one = rf.robust_mean_images(frame["B"], SPP, exposure=EXPOSURE)
    assert not np.array_equal(bits(one["mean"]), bits(got["mean"]))
    # with all counts equal to 32 the tiles form is the one-count form
    same = rf.robust_mean_tiles(frame["B"], np.full(TILES, SPP, np.uint32), exposure=EXPOSURE)
    assert all(np.array_equal(same[k], one[k]) for k in ("trim", "bgra8")) and np.array_equal(bits(same["mean"]), bits(one["mean"]))


# ---- 5. crafted planes
def _crafted_tile(k, n, h, w, rng):
    """tests/test_gpu_robust.py's crafted frame at the size of one tile: ordinary pixels and the special rows"""
    B = np.zeros((k, h, w, 4), np.float32)
    B[..., :3] = (rng.random((k, h, w, 3)) * n / k).astype(np.float32)
    B[:, 0, :, :3] = B[0, 0, :, :3][None]                                     # row 0: all buckets equal SUMS (unequal means when k does not divide n)
    for x in range(w):                                                        # row 1: one outlier, in every bucket in turn
        B[x % k, 1, x, :3] = 1000.0 * n
    B[:, 2, :, :3] = 0                                                        # row 2: all zero (den = 0)
    B[:, 3, :, :3] = np.float32(0.5) * np.float32(n // k)                     # row 3: tied keys wherever the bucket sizes are equal ...
    B[:, 3, :, 0] += (np.arange(k) % 2).astype(np.float32)[:, None]          # ... with different channels: r + 1 ...
    B[:, 3, :, 1] -= (np.arange(k) % 2).astype(np.float32)[:, None]          # ... g - 1
    for x in range(w):                                                        # rows 4 - 6: x % (k + 1) buckets with a NaN / +inf / both
        bad = rng.permutation(k)[:x % (k + 1)]
        B[bad, 4, x, rng.integers(0, 3)] = np.nan
        B[bad, 5, x, rng.integers(0, 3)] = np.inf
        B[bad[::2], 6, x, 0] = np.nan
        B[bad[1::2], 6, x, 2] = np.inf
    return B


def test_crafted_planes_with_one_count_per_tile():
    w, h, k = 72, 40, 9                                                       # 3 x 2 tiles, ragged
    counts = np.array([9, 10, 17, 18, 70, 1000], np.uint32)                   # K divides the count, or not
    rng = np.random.default_rng(9)
    B = np.zeros((k, h, w, 4), np.float32)
    for t, (rows, cols) in enumerate(tile_slices(w, h)):
        B[:, rows, cols] = _crafted_tile(k, int(counts[t]), rows.stop - rows.start, cols.stop - cols.start, rng)
    got = rf.robust_mean_tiles(B, counts, exposure=1.0)
    M, trim = robust_mean_tiles(B, counts, w, h)
    assert np.array_equal(got["trim"], trim) and np.array_equal(bits(got["mean"]), bits(M))
    half = (k - 1) // 2
    for rows, cols in tile_slices(w, h):                                      # the special rows did what they are there for, in every tile
        y = rows.start
        assert (trim[y + 1, cols] > 0).all() and (M[y + 1, cols] < 10).all() and (trim[y + 2, cols] == 0).all() and not M[y + 2, cols].any()
    nonfinite = (~np.isfinite(B[..., :3])).any(axis=3).sum(axis=0)
    assert (trim[(nonfinite > 0) & (nonfinite <= half)] == half).all() and np.isfinite(got["mean"][nonfinite <= half]).all()
    assert (~np.isfinite(got["mean"])).any()
    # a tile's result does not depend on its neighbours' counts
    other = counts.copy()
    other[1:] = 500
    again = rf.robust_mean_tiles(B, other, exposure=1.0)
    rows, cols = tile_slices(w, h)[0]
    assert np.array_equal(bits(again["mean"][rows, cols]), bits(got["mean"][rows, cols])) and np.array_equal(again["trim"][rows, cols], trim[rows, cols])


# ---- 6. the robust denoise
def test_the_robust_denoise_divides_the_guides_by_the_tiles_count(duck_pt, frame_a):
    r, want = frame_a["r"], frame_a["want"]
    before = _reads(r)
    ac, nd, n = _aovs(r)
    assert n == SPP
    r.denoise_robust()
    rgb, bgra, m = r.read_denoised()
    assert m == SPP and np.array_equal(bits(rgb), bits(denoise_robust_tiles(want["M"], ac, nd, want["counts"])))
    snap = r.read_robust_mean()                                               # the snapshot denoise_robust leaves is the tiles combine
    assert np.array_equal(bits(snap["mean"]), bits(want["M"])) and np.array_equal(snap["trim"], want["trim"]) and snap["samples"] == SPP
    r.denoise_robust(iterations=0)                                            # L = 0 returns M, with the combine's texels
    rgb0, bgra0, _ = r.read_denoised()
    assert np.array_equal(bits(rgb0), bits(want["M"])) and np.array_equal(bgra0, snap["bgra8"])
    # rf_renderer_denoise on the same handle: the handle without the buckets
    r.denoise()
    plain = _renderer(duck_pt)
    plain.set_aovs(True, tile_counts=True)
    plain.render_adaptive(_target(), EVERY, MIN)
    plain.denoise()
    for a, b in zip(r.read_denoised(), plain.read_denoised()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.array_equal(bits(r.read_denoised()[0]), bits(plain.read_denoised()[0]))
    plain.close()
    assert _same_reads(_reads(r), before) == []


# ---- 7. back to uniform
def test_no_tile_stopping_leaves_the_uniform_state(duck_pt):
    samples, _, _ = _samples()
    r = _bucket_renderer(duck_pt, aovs=True)
    res = r.render_adaptive(0.0, EVERY, SPP)                                  # min_samples equal to the cap: no tile can stop
    assert res["stopped_tiles"] == 0 and r.read_tile_samples().reshape(-1).tolist() == [SPP] * TILES
    u = _renderer(duck_pt, moments=False)
    u.set_aovs(True)
    u.set_buckets(K)
    u.render(SPP)
    (B, n), (Bu, nu) = r.read_buckets(), u.read_buckets()
    assert n == nu == SPP and np.array_equal(bits(B), bits(Bu)) and np.array_equal(bits(B), bits(bucket_sums(samples, K)))
    for h in (r, u):
        h.robust_mean()
    a, b = r.read_robust_mean(), u.read_robust_mean()
    M, trim = robust_mean(B, SPP)
    assert a["samples"] == b["samples"] == SPP and all(np.array_equal(a[k], b[k]) for k in ("trim", "bgra8")) and np.array_equal(bits(a["mean"]), bits(b["mean"]))
    assert np.array_equal(bits(a["mean"]), bits(M)) and np.array_equal(a["trim"], trim)
    for h in (r, u):
        h.denoise_robust()
    (rgb, bgra, m), (rgb_u, bgra_u, m_u) = r.read_denoised(), u.read_denoised()
    assert m == m_u == SPP and np.array_equal(bits(rgb), bits(rgb_u)) and np.array_equal(bgra, bgra_u)
    r.render(2)                                                               # (the ordinary calls run: into the full accumulation, nothing is traced)
    u.close()
    r.close()


# ---- 8. the refusals
def test_the_switch_and_its_refusals(duck_pt):
    lib = rf._ffi.lib
    BIT = rf._ffi.RF_BUCKETS_TILE_COUNTS
    assert BIT == 0x100
    r = _renderer(duck_pt)
    for word in (BIT, BIT | 4, 0x200 | K, 0x10000 | K, BIT | 17):             # the bit with K = 0, a bad K under it, unknown bits
        assert lib.rf_renderer_set_buckets(r._h, word) == INVALID and "K must be" in lib.rf_last_error_message().decode(), hex(word)
    _refused(lambda: r.set_buckets(0, tile_counts=True), "K must be")
    assert r.read_buckets()[0].shape[0] == 0
    # until render_adaptive is called a handle with the bit is the handle without it; a change of the bit alone clears the sums, the same word again does not
    b = _bucket_renderer(duck_pt, tile_counts=False)
    r.set_buckets(K, tile_counts=True)
    for h in (r, b):
        h.render(8)
    (Br, nr), (Bb, nb) = r.read_buckets(), b.read_buckets()
    assert nr == nb == 8 and np.array_equal(bits(Br), bits(Bb)) and Br.any() and _same_reads(_reads(r), _reads(b)) == []
    assert r.memory_info() == b.memory_info() and _rays(r) == _rays(b)
    assert r.launch_plan(1, 8) == b.launch_plan(1, 8)
    r.set_buckets(K, tile_counts=True)
    assert r.read_buckets()[1] == 8
    _refused(lambda: b.render_adaptive(0.1, 4), "bucket", "ONE sample count")  # without the bit: today's refusal
    b.set_buckets(K, tile_counts=True)
    B, n = b.read_buckets()
    assert B.shape == (K, H, W, 4) and n == 0 and not B.any() and b.read_accumulation()[1] == 8
    # ... and now the buckets (with the bit) were turned on partway through
    before = b.stats()["batches_traced"]
    _refused(lambda: b.render_adaptive(0.1, 4), "restart the accumulation first", "bucket")
    assert b.stats()["batches_traced"] == before
    b.close()
    r.close()
    # a tile below K: the planes still follow the counts, the combine and the robust denoise are refused
    k = 5
    samples, S, Q = _samples(64, 64, 32)
    target = float(np.float32(np.median(tile_errors(estimate(S[4], Q[4], 4)))))
    want = play(S, Q, 64, 64, target, 4, min_samples=0)
    assert want["counts"].tolist() == [8, 4, 4, 8]
    r = _bucket_renderer(duck_pt, k=k, aovs=True, w=64, h=64)
    r.render_adaptive(target, 4)
    B, n = r.read_buckets()
    assert r.read_tile_samples().reshape(-1).tolist() == [8, 4, 4, 8] and n == 8
    assert np.array_equal(bits(B), bits(_tile_planes(samples, want["counts"], k, 64, 64)))
    for t, (rows, cols) in enumerate(tile_slices(64, 64)):
        assert bool(B[4, rows, cols].any()) == (want["counts"][t] == 8) and B[3, rows, cols].any()
    _refused(r.robust_mean, "5 buckets", "smallest tile count is 4")
    _refused(r.denoise_robust, "5 buckets", "smallest tile count is 4")
    _refused(r.read_robust_mean)
    _refused(lambda: r.set_buckets(k, tile_counts=True), "different sample counts")   # K > 0 in the non-uniform state: refused, with or without the bit
    _refused(lambda: r.set_buckets(3), "different sample counts")
    r.denoise()                                                               # (rf_renderer_denoise is unchanged: it runs)
    r.close()
    # denoise_robust in the non-uniform state without the AOVs' tile counts
    r = _bucket_renderer(duck_pt)
    assert r.render_adaptive(_target(), EVERY, MIN)["stopped_tiles"] > 0
    _refused(r.denoise_robust, "different sample counts", "RF_AOV_TILE_COUNTS")
    r.robust_mean()                                                           # (the combine itself runs)
    r.set_buckets(0)
    _refused(r.robust_mean, "different sample counts")                        # the buckets off in the non-uniform state: as ever
    r.close()


def test_the_sharded_adaptive_call_refuses_the_bit_before_any_exchange(duck_pt, monkeypatch):
    """rf_comm_render_adaptive with K | RF_BUCKETS_TILE_COUNTS, two ranks of the local test transport in this process: both are refused with a message that names
    the buckets, nothing is traced, and the communicator serves the next collective"""
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "120")
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _bucket_renderer(duck_pt)
            r.set_tile_shard(rank, 2)
            comm = rf.TileComm(uid, rank, 2, 0)
            _refused(lambda: comm.render_adaptive(r, 0.1, 8), "bucket")
            out[rank] = (r.stats()["batches_traced"], r.read_accumulation()[1], comm.all_reduce_max(float(rank), r))
            comm.close()
            r.close()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads), "a rank hangs in an exchange"
    assert out == {0: (0, 0, 1.0), 1: (0, 0, 1.0)}


# ---- 9. the command line
def _read_pfm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    kind, (w, h) = parts[0], map(int, parts[1].split())
    assert parts[2] == b"-1.0"
    return np.frombuffer(parts[3], "<f4").reshape(h, w, 3 if kind == b"PF" else 1)[::-1]


def test_rf_render_writes_the_adaptive_frames_robust_mean(duck_pt, tmp_path):
    want = _want()
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    base = [exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(SPP), "--bounces", str(BOUNCES), "--out", str(tmp_path / "o.png")]
    # rf-render's defaults are this file's camera, sky and exposure; %.9g round-trips an f32
    adaptive = ["--adaptive", "%.9g" % _target(), "--adaptive-min", str(MIN), "--adaptive-every", str(EVERY), "--buckets", str(K)]
    txt = subprocess.check_output(base + adaptive + ["--buckets-tile-counts", "--robust-mean", str(tmp_path / "m.pfm"), "--trim-map", str(tmp_path / "t.pfm")],
                                  timeout=120).decode()
    assert f"{want['stopped_tiles']} of {TILES} tiles stopped early" in txt, txt
    rows = np.ascontiguousarray(want["M"][::-1], np.float32)                  # (a PFM's rows run bottom to top)
    assert open(tmp_path / "m.pfm", "rb").read() == b"PF\n%d %d\n-1.0\n" % (W, H) + rows.tobytes()
    assert np.array_equal(_read_pfm(tmp_path / "t.pfm")[..., 0], want["trim"].astype(np.float32))
    # the switch in another place of the line, and the robust denoise
    subprocess.check_output(base + ["--buckets-tile-counts"] + adaptive + ["--denoise-robust", str(tmp_path / "d.png")], timeout=120)
    assert os.path.getsize(tmp_path / "d.png") > 0
    # without the switch: today's message; several GPUs: refused as today
    bad = subprocess.run(base + adaptive, capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--buckets" in bad.stderr and b"need --gpus 1 and do not go with --adaptive" in bad.stderr
    bad = subprocess.run(base + ["--buckets", str(K), "--buckets-tile-counts", "--gpus", "2"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"need --gpus 1" in bad.stderr
    bad = subprocess.run(base + ["--buckets-tile-counts"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"needs --buckets" in bad.stderr
