"""The bucket sums and the robust mean on the GPU (-m gpu), at the shape of tests/test_gpu_sum_kernels.py: Duck, 72 x 40 (3 x 2 tiles, both edges ragged), 3 bounces,
K = 9, 70 samples -- buckets 0 .. 6 hold 8 samples and 7 .. 8 hold 7; one batch of 70 is two full 32-sample chunks of the LDS-staged kernel plus 6.  Every comparison is
exact: the bucket planes against tests/robust_restatement.py's sums of the oracle's per-sample radiance, the combine and the robust denoise against its restatements,
and every other way of scheduling the same samples against the same bits."""
import os
import subprocess
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import prefix_sums, tile_errors
from conftest import ROOT, bits, oracle_scene_from_pt
from noise_restatement import estimate, oracle_samples
from oracle import orc
from robust_restatement import bucket_sums, denoise_robust, robust_mean

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES, EXPOSURE, K = 72, 40, 70, 3, 0.25, 9
TILES = 6
SLOTS = SPP * TILES * 1024                                                     # one batch: 70 samples of 6 tiles of 1024 path slots
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
SUMS = ("S", "Q", "AC", "ND")


def _params(exposure=EXPOSURE):
    return rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), exposure)


def _renderer(pt, k=K, opts=(), max_paths=SLOTS, moments=True, aovs=True):
    r = rf.ReferencePathTracer(_params(), pt.scene(), max_paths_in_flight=max_paths)
    for name, v in dict(opts).items():
        r.set_option(name, v)
    if moments:
        r.set_moments(True)
    if aovs:
        r.set_aovs(True)
    if k:
        r.set_buckets(k)
    return r


def _reads(r):
    """The four ordinary sums as bit patterns, their counts and the ray counts"""
    img, acc = r.read_accumulation()
    q, n = r.read_moments()
    a = r.read_aovs()
    ac = np.concatenate([a["albedo"], a["coverage"][..., None]], -1)
    nd = np.concatenate([a["normal"], a["depth"][..., None]], -1)
    st = r.stats()
    return dict(S=bits(img), Q=bits(q), AC=bits(ac), ND=bits(nd), ac=ac, nd=nd, counts=(acc, n, a["samples"]),
                rays=(st["primary_rays"], st["closest_rays"], st["shadow_rays"]))


def _refused(call, *words):
    with pytest.raises(rf.RayfinderError) as e:
        call()
    assert e.value.status == INVALID, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.fixture(scope="module")
def samples(duck_pt):
    """The oracle's per-sample radiance of the 70 samples (computed once; read-only)"""
    sc, _ = oracle_scene_from_pt(duck_pt)
    rp = orc.make_render_params(W, H, rf.camera_to_array(rf.fly_camera(W, H)), SPP, BOUNCES, EXPOSURE, rf.aligned_sky_state(rf.make_sky()))
    out = list(oracle_samples(orc, sc, rp, range(SPP)))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def plain(duck_pt):
    """render(70) with the buckets off: the sums, the ray counts, the memory figures and the denoised image the buckets must not change"""
    r = _renderer(duck_pt, k=0)
    r.render(SPP)
    got = _reads(r)
    got["memory"] = r.memory_info()
    assert r.read_buckets()[0].shape == (0, H, W, 4) and r.read_buckets()[1] == 0
    _refused(r.robust_mean, "bucket")
    _refused(r.read_robust_mean)
    _refused(r.denoise_robust, "bucket")
    r.denoise()
    got["denoised"] = r.read_denoised()
    r.close()
    return got


@pytest.fixture(scope="module")
def baseline(duck_pt):
    """render(70) with K = 9 and the default options: one batch, the LDS-staged kernels; the planes, the combine and both denoised images"""
    r = _renderer(duck_pt)
    plan = r.launch_plan(1, SPP)
    assert plan["runs"] == 1 and plan["tile_list"] == 0, plan
    _refused(r.read_robust_mean)
    r.render(SPP)
    assert r.stats()["batches_traced"] == 1
    got = _reads(r)
    got["memory"] = r.memory_info()
    got["B"], got["n"] = r.read_buckets()
    r.robust_mean()
    got["robust"] = r.read_robust_mean()
    r.denoise()
    got["denoised"] = r.read_denoised()
    r.denoise_robust()
    got["denoised_robust"] = r.read_denoised()
    r.denoise_robust(iterations=0)
    got["denoised_robust_0"] = r.read_denoised()
    got["robust_after"] = r.read_robust_mean()
    r.close()
    return got


def test_bucket_sums_are_bit_exact_and_leave_the_other_sums_alone(samples, plain, baseline):
    want = bucket_sums(samples, K)
    assert baseline["n"] == SPP and baseline["B"].shape == (K, H, W, 4)
    assert want[..., :3].any() and all(want[b, ..., :3].any() for b in range(K))
    assert np.array_equal(bits(baseline["B"]), bits(want))
    assert baseline["counts"] == plain["counts"] == (SPP, SPP, SPP)
    for k in SUMS:
        assert np.array_equal(baseline[k], plain[k]), k
    assert baseline["rays"] == plain["rays"] and baseline["rays"][0] == W * H * SPP
    assert baseline["memory"] == plain["memory"]


@pytest.mark.parametrize("name,k,opts,steps,max_paths,batches", [
    ("render(35); render(35): the second batch starts at phase 8", 9, {}, (35, 35), SLOTS, 2),
    ("render(3); render(67): a batch shorter than K", 9, {}, (3, 67), SLOTS, 2),
    ("render(64); render(6)", 9, {}, (64, 6), SLOTS, 2),
    ("one lane per pixel", 9, dict(accumulate_runs=0), (SPP,), SLOTS, 1),
    ("one lane per pixel, two batches", 9, dict(accumulate_runs=0), (35, 35), SLOTS, 2),
    ("unsorted samples", 9, dict(sample_sort=0), (SPP,), SLOTS, 1),
    ("groups of 4 pixels", 9, dict(slot_group_shift=2), (SPP,), SLOTS, 1),
    ("sample-major slots", 9, dict(slot_group_shift=-1), (35, 35), SLOTS, 2),
    ("shallow batches of 10 samples", 9, {}, (SPP,), 10 * TILES * 1024, 7),
    ("shallow batches of 4 samples: one lane per pixel below 5", 9, {}, (SPP,), 4 * TILES * 1024, 18),
    ("K = 3", 3, {}, (35, 35), SLOTS, 2),
    ("K = 15", 15, {}, (35, 35), SLOTS, 2),
])
def test_every_schedule_leaves_the_same_bits(duck_pt, samples, plain, name, k, opts, steps, max_paths, batches):
    r = _renderer(duck_pt, k=k, opts=opts, max_paths=max_paths)
    for n in steps:
        r.render(n)
    got = _reads(r)
    B, count = r.read_buckets()
    assert r.stats()["batches_traced"] == batches, name
    r.close()
    assert count == SPP and np.array_equal(bits(B), bits(bucket_sums(samples, k))), name
    assert [s for s in SUMS if not np.array_equal(got[s], plain[s])] == [] and got["rays"] == plain["rays"], name


def test_the_combine_equals_the_restatement(baseline):
    M, trim = robust_mean(baseline["B"], SPP)
    got = baseline["robust"]
    assert got["samples"] == SPP and got["mean"].shape == (H, W, 3) and got["trim"].dtype == np.uint8
    assert np.isfinite(M).all() and M.any() and 0 < int((trim > 0).sum()) < W * H            # trimmed and untrimmed pixels both
    assert np.array_equal(got["trim"], trim)
    assert np.array_equal(bits(got["mean"]), bits(M))
    # the snapshot denoise_robust leaves is the same combine
    assert all(np.array_equal(baseline["robust_after"][k], got[k]) for k in ("mean", "bgra8", "trim"))


def test_denoising_the_robust_mean(baseline, plain):
    M = baseline["robust"]["mean"]
    rgb, bgra, n = baseline["denoised_robust"]
    want = denoise_robust(M, baseline["ac"], baseline["nd"], SPP)
    assert n == SPP and np.array_equal(bits(rgb), bits(want))
    assert not np.array_equal(bits(rgb), bits(baseline["denoised"][0]))                       # (it is another image than the plain denoise)
    # rf_renderer_denoise itself: bit for bit what it is with the buckets off
    for got, ref in zip(baseline["denoised"], plain["denoised"]):
        assert np.array_equal(np.asarray(got), np.asarray(ref))
    assert np.array_equal(bits(baseline["denoised"][0]), bits(plain["denoised"][0]))
    # L = 0 returns M, and its display texels are the robust mean's
    rgb0, bgra0, _ = baseline["denoised_robust_0"]
    assert np.array_equal(bits(rgb0), bits(M)) and np.array_equal(bgra0, baseline["robust"]["bgra8"])


def test_turned_on_partway_a_change_of_k_and_new_parameters(duck_pt, samples, plain):
    r = _renderer(duck_pt, k=0)
    r.render(10)
    before = r.memory_info()
    r.set_buckets(K)
    assert r.memory_info() == before
    r.render(SPP - 10)
    B, n = r.read_buckets()
    assert n == SPP - 10 and r.read_accumulation()[1] == SPP
    assert np.array_equal(bits(B), bits(bucket_sums(samples[10:], K)))                        # ordinal 0 is the first sample traced with the buckets on
    _refused(r.robust_mean, "differs", "60", "70")
    _refused(r.denoise_robust, "differs")
    assert [s for s in SUMS if not np.array_equal(_reads(r)[s], plain[s])] == []
    # the same K again changes nothing; another K clears the sums
    r.set_buckets(K)
    assert r.read_buckets()[1] == SPP - 10
    r.set_buckets(5)
    B, n = r.read_buckets()
    assert B.shape == (5, H, W, 4) and n == 0 and not B.any()
    # new parameters clear them with the image; they then cover the new accumulation from its first sample (the frame counter runs on: these are samples 70 .. 76,
    # which the oracle fixture does not hold -- the planes are held to the image instead: the same 7 non-negative values per channel in another order, each order
    # within 6 roundings of 2^-24 of the exact sum)
    r.set_render_parameters(_params(exposure=0.5))
    r.render(7)
    B, n = r.read_buckets()
    assert n == 7 and all(B[b, ..., :3].any() for b in range(5)) and not B[..., 3].any()
    assert np.allclose(B[..., :3].sum(axis=0, dtype=np.float64), r.read_accumulation()[0][..., :3], rtol=12 * 2.0 ** -24, atol=0)
    r.robust_mean()
    got = r.read_robust_mean()
    M, trim = robust_mean(B, 7)
    assert got["samples"] == 7 and np.array_equal(bits(got["mean"]), bits(M)) and np.array_equal(got["trim"], trim)
    # the snapshot goes with the sums
    r.set_render_parameters(_params())
    _refused(r.read_robust_mean)
    # a K that is refused keeps the state
    for bad in (1, 4, 17):
        _refused(lambda: r.set_buckets(bad), "K must be")
    assert r.read_buckets()[0].shape[0] == 5
    r.set_buckets(0)
    assert r.read_buckets()[0].shape[0] == 0
    r.close()


def test_the_refusals(duck_pt, samples):
    # fewer samples than buckets
    r = _renderer(duck_pt)
    r.render(K - 1)
    _refused(r.robust_mean, "9 buckets")
    _refused(r.denoise_robust, "9 buckets")
    r.render(1)
    r.robust_mean()
    assert r.read_robust_mean()["samples"] == K
    # render_adaptive with the buckets on: refused before anything is traced
    before = r.stats()["batches_traced"]
    _refused(lambda: r.render_adaptive(0.0, 8), "bucket")
    assert r.stats()["batches_traced"] == before and r.read_accumulation()[1] == K
    # a tile shard: the sums are kept (shard-compact), the combine is refused
    r.set_tile_shard(0, 2)
    r.render(K)
    assert r.read_buckets()[1] == K
    _refused(r.robust_mean, "shard")
    _refused(r.denoise_robust, "shard")
    r.close()
    # set_buckets in the non-uniform state: a target between the tiles' errors at 35 samples stops some of them there
    S, Q = prefix_sums(samples)
    target = float(np.float32(np.median(tile_errors(estimate(S[35], Q[35], 35)))))
    r = _renderer(duck_pt, k=0, aovs=False)
    res = r.render_adaptive(target, 35, 35)
    assert 0 < res["stopped_tiles"] < TILES and not r.tile_samples_uniform()
    _refused(lambda: r.set_buckets(K), "different sample counts")
    r.set_buckets(0)                                                           # (off is never refused)
    assert r.read_buckets()[0].shape[0] == 0
    r.close()


def test_the_sharded_adaptive_call_refuses_before_any_exchange(duck_pt, monkeypatch):
    """rf_comm_render_adaptive with the buckets on, two ranks of the local test transport in this process: both are refused with the buckets' message, nothing is
    traced, and the communicator serves the next collective (one all-reduce of the rank numbers)"""
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "120")
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _renderer(duck_pt, aovs=False)
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


def test_two_shards_add_up_to_the_frame(duck_pt, baseline):
    total = np.zeros((K, H, W, 4), np.float32)
    owned = np.zeros((H, W), np.int32)
    for rank in range(2):
        r = _renderer(duck_pt)
        r.set_tile_shard(rank, 2)
        r.render(SPP)
        B, n = r.read_buckets()
        r.close()
        assert n == SPP
        owned += B[..., :3].any(axis=(0, 3))
        total = total + B
    assert owned.max() == 1                                                    # no pixel comes from both ranks
    assert np.array_equal(bits(total), bits(baseline["B"]))
    got = rf.robust_mean_images(total, SPP, exposure=EXPOSURE)
    want = baseline["robust"]
    assert np.array_equal(bits(got["mean"]), bits(want["mean"])) and np.array_equal(got["trim"], want["trim"]) and np.array_equal(got["bgra8"], want["bgra8"])


@pytest.mark.parametrize("k,n", [(9, 70), (5, 5), (15, 1000)])
def test_crafted_planes(k, n):
    """robust_mean_images on a 40 x 33 frame (two blocks of 256 lanes and a ragged one) of ordinary pixels and the special ones"""
    rng = np.random.default_rng(k)
    h, w, half = 33, 40, (k - 1) // 2
    B = np.zeros((k, h, w, 4), np.float32)
    B[..., :3] = (rng.random((k, h, w, 3)) * n / k).astype(np.float32)
    B[:, 0, :, :3] = B[0, 0, :, :3][None]                                      # row 0: all buckets equal SUMS (unequal means when k does not divide n)
    for x in range(w):                                                         # row 1: one outlier, in every bucket in turn
        B[x % k, 1, x, :3] = 1000.0 * n
    B[:, 2, :, :3] = 0                                                         # row 2: all zero (den = 0)
    B[:, 3, :, :3] = np.float32(0.5) * np.float32(n // k)                      # row 3: tied keys wherever the bucket sizes are equal ...
    B[:, 3, :, 0] += (np.arange(k) % 2).astype(np.float32)[:, None]           # ... with different channels: r + 1 ...
    B[:, 3, :, 1] -= (np.arange(k) % 2).astype(np.float32)[:, None]           # ... g - 1
    for x in range(w):                                                         # rows 4 - 6: x % (k + 1) buckets with a NaN / +inf / both
        bad = rng.permutation(k)[:x % (k + 1)]
        B[bad, 4, x, rng.integers(0, 3)] = np.nan
        B[bad, 5, x, rng.integers(0, 3)] = np.inf
        B[bad[::2], 6, x, 0] = np.nan
        B[bad[1::2], 6, x, 2] = np.inf
    got = rf.robust_mean_images(B, n, exposure=1.0)
    M, trim = robust_mean(B, n)
    assert np.array_equal(got["trim"], trim)
    assert np.array_equal(bits(got["mean"]), bits(M))
    assert (trim[1] > 0).all() and (M[1] < 10).all() and (trim[2] == 0).all() and not M[2].any()
    nonfinite = (~np.isfinite(B[..., :3])).any(axis=3).sum(axis=0)            # buckets of the pixel with a non-finite channel
    assert (trim[(nonfinite > 0) & (nonfinite <= half)] == half).all()
    assert np.isfinite(got["mean"][nonfinite <= half]).all()
    assert (~np.isfinite(got["mean"])).any()                                   # (and the frame does hold pixels past saving)


def _read_pfm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    kind, (w, h) = parts[0], map(int, parts[1].split())
    assert parts[2] == b"-1.0"
    ch = 3 if kind == b"PF" else 1
    return np.frombuffer(parts[3], "<f4").reshape(h, w, ch)[::-1]


def test_rf_render_writes_the_robust_mean(duck_pt, baseline, tmp_path):
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    base = [exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(SPP), "--bounces", str(BOUNCES), "--out", str(tmp_path / "o.png")]
    # rf-render's defaults are this file's camera, sky and exposure
    subprocess.check_output(base + ["--buckets", str(K), "--robust-mean", str(tmp_path / "m.pfm"), "--trim-map", str(tmp_path / "t.pfm"),
                                    "--denoise-robust", str(tmp_path / "d.png")], timeout=120)
    want = baseline["robust"]
    rows = np.ascontiguousarray(want["mean"][::-1], np.float32)                # (a PFM's rows run bottom to top)
    assert open(tmp_path / "m.pfm", "rb").read() == b"PF\n%d %d\n-1.0\n" % (W, H) + rows.tobytes()
    assert np.array_equal(_read_pfm(tmp_path / "t.pfm")[..., 0], want["trim"].astype(np.float32))
    assert os.path.getsize(tmp_path / "d.png") > 0
    for extra in (["--gpus", "2"], ["--adaptive", "0.1"]):
        bad = subprocess.run(base + ["--buckets", str(K)] + extra, capture_output=True, timeout=120)
        assert bad.returncode != 0 and b"--buckets" in bad.stderr and b"need --gpus 1 and do not go with --adaptive" in bad.stderr, extra
    bad = subprocess.run(base + ["--robust-mean", str(tmp_path / "x.pfm")], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"need --buckets" in bad.stderr
