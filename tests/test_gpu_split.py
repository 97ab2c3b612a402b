"""The direct radiance sums and the split-component denoiser on the GPU (-m gpu): D is bit for bit the accumulation of a 1-bounce handle over the same samples
(and the oracle's 1-bounce render) whatever the batching, leaves every other sum alone and follows the bookkeeping include/rayfinder_amd.h states;
kDenoisePrepSplit + kDenoiseAtrousSplit are bit-identical to the numpy restatement (tests/split_restatement.py) on synthetic inputs and on rendered frames."""
import functools
import os
import subprocess

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import DUCK, ROOT, bits, oracle_scene_from_pt
from denoise_restatement import denoise
from oracle import orc
from split_restatement import denoise_split, denoise_split_window

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
SIGMAS = (dict(), dict(sigma_color=3.5, sigma_normal=0.4, sigma_depth=0.02))
W1, H1, SPP1, BOUNCES1 = 70, 45, 16, 3                                        # the sums' frame: ragged in both tile dimensions


def _renderer(pt, w, h, spp, bounces, **kw):
    params = rf.make_render_parameters(w, h, rf.fly_camera(w, h), spp, bounces, rf.make_sky(), 0.25)
    return rf.ReferencePathTracer(params, pt.scene(), **kw), params


def _refused(call, *words):
    with pytest.raises(rf.RayfinderError) as e:
        call()
    assert e.value.status == INVALID, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def _same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1]


@functools.lru_cache(maxsize=None)
def _one_bounce(w, h, spp, first=0, count=None):
    """read_accumulation of a fresh handle with num_bounces = 1 that renders samples [first, first + count) alone (computed once per shape; read-only)"""
    r, _ = _renderer(rf.PtFormat.from_gltf(DUCK), w, h, spp, 1)
    count = spp - first if count is None else count
    if first:
        r.render(first)                                                      # (the frame counter moves on; a change of the parameters then clears the image)
        r.set_render_parameters(rf.make_render_parameters(w, h, rf.fly_camera(w, h), spp, 1, rf.make_sky(), 0.5))
    r.render(count)
    img, n = r.read_accumulation()
    r.close()
    assert n == count
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------------------------ the sums
@pytest.mark.parametrize("max_paths", [3 * 6 * 1024, 0], ids=["per_pixel_kernel", "lds_staged_kernel"])
def test_direct_sums_equal_a_one_bounce_handle_and_the_oracle(duck_pt, max_paths):
    r, params = _renderer(duck_pt, W1, H1, SPP1, BOUNCES1, max_paths_in_flight=max_paths)
    r.set_direct(True)
    r.render(5)
    r.render(11)
    batches = r.stats()["batches_traced"]
    plan = r.launch_plan(1, 3 if max_paths else 11)
    D, n = r.read_direct()
    S, acc = r.read_accumulation()
    mem = r.memory_info()
    r.close()
    # 6 tiles: batches of <= 3 samples take the one-lane-per-pixel kernel (accumulate_kernel 0), 5 + 11 in two batches the LDS-staged one (1)
    assert (batches >= 6 and plan["accumulate_kernel"] == 0) if max_paths else (batches == 2 and plan["accumulate_kernel"] == 1), (batches, plan)
    assert n == acc == SPP1
    want = _one_bounce(W1, H1, SPP1)
    assert want[..., :3].any() and np.array_equal(bits(D), bits(want))
    assert not np.array_equal(bits(D), bits(S))                              # (three bounces: there is indirect light)
    sc, _ = oracle_scene_from_pt(duck_pt)
    rp = orc.make_render_params(W1, H1, rf.camera_to_array(params.camera), SPP1, 1, 0.25, rf.aligned_sky_state(params.sky))
    x0, y0, x1, y1 = 20, 8, 52, 40                                            # a crop across the tile border at x = 32 and y = 32
    ref, _ = orc.render(sc, rp, 0, SPP1, x0, y0, x1, y1)
    assert ref[y0:y1, x0:x1, :3].any() and np.array_equal(bits(D[y0:y1, x0:x1, :3]), bits(ref[y0:y1, x0:x1, :3]))
    assert mem["path_state_bytes"] >= 6 * 1024 * 16


def test_on_a_one_bounce_handle_direct_is_the_image(duck_pt):
    r, _ = _renderer(duck_pt, W1, H1, SPP1, 1)
    r.set_direct(True)
    r.render(SPP1)
    assert _same(r.read_direct(), r.read_accumulation()) and r.read_direct()[1] == SPP1
    r.close()


def _all_sums(r):
    a = r.read_aovs()
    return [r.read_accumulation(), (a["albedo"], a["samples"]), (a["coverage"], a["samples"]), (a["normal"], a["samples"]), (a["depth"], a["samples"]), r.read_moments()]


def test_direct_is_non_invasive(duck_pt):
    def run(direct):
        r, _ = _renderer(duck_pt, W1, H1, SPP1, BOUNCES1)
        r.set_aovs(True)
        r.set_moments(True)
        if direct is not None:
            r.set_direct(direct)
        r.set_timing(True)
        plans = [r.launch_plan(b, 8) for b in (1, 2, 3)]
        mem = r.memory_info()
        r.render(5)
        r.render(11)
        s = r.stats()
        out = _all_sums(r), {k: v for k, v in s.items() if k.startswith("launches_") or k.endswith("_rays") or k == "batches_traced"}, plans, mem, r.memory_info()
        r.close()
        return out

    never, off, on = run(None), run(False), run(True)
    for a, b in zip(never[0], on[0]):
        assert _same(a, b)
    for a, b in zip(never[0], off[0]):
        assert _same(a, b)
    assert never[1] == off[1] and never[2] == off[2] == on[2] and never[3:] == off[3:]
    # on: one more launch per batch, counted with the accumulation; 16 B per pixel of the 6 tiles
    assert on[1]["launches_accumulate"] == never[1]["launches_accumulate"] + on[1]["batches_traced"]
    assert {k: v for k, v in on[1].items() if k != "launches_accumulate"} == {k: v for k, v in never[1].items() if k != "launches_accumulate"}
    assert on[4]["path_state_bytes"] - never[4]["path_state_bytes"] == 6 * 1024 * 16 and on[3] == never[3]


def test_direct_counts_and_clearing(duck_pt):
    spp = 8
    r, params = _renderer(duck_pt, W1, H1, spp, BOUNCES1)
    r.render(3)
    r.set_direct(True)
    assert r.read_direct()[1] == 0 and not r.read_direct()[0].any()
    r.render(5)
    D, n = r.read_direct()
    assert n == 5 and r.read_accumulation()[1] == 8
    assert np.array_equal(bits(D), bits(_one_bounce(W1, H1, spp, 3, 5)))     # samples 3 .. 7 alone
    whole = _one_bounce(W1, H1, spp)

    def cleared():
        D, n = r.read_direct()
        return n == 0 and not D.any()

    r.set_render_parameters(rf.make_render_parameters(W1, H1, params.camera, spp, BOUNCES1, params.sky, 0.5))
    assert cleared()
    r.render(2)
    assert r.read_direct()[1] == 2
    r.set_tile_shard(0, 1)
    assert cleared()
    r.render(2)
    assert r.read_direct()[1] == 2
    import torch
    ptr, nbytes = r.accumulation_device_buffer()
    buf = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    r.bind_accumulation_buffer(buf.data_ptr(), nbytes)
    assert cleared()
    r.render(1)
    assert r.read_direct()[1] == 1
    r.set_direct(False)
    assert cleared()
    r.close()
    # render_adaptive is refused while direct is on, the state untouched
    r, _ = _renderer(duck_pt, W1, H1, spp, BOUNCES1)
    r.set_moments(True)
    r.set_direct(True)
    r.render(spp)
    before = [r.read_accumulation(), r.read_moments(), r.read_direct()]
    assert np.array_equal(bits(before[2][0]), bits(whole))
    _refused(lambda: r.render_adaptive(0.01, 4), "direct")
    after = [r.read_accumulation(), r.read_moments(), r.read_direct()]
    assert all(_same(a, b) for a, b in zip(before, after)) and r.tile_samples_uniform()
    r.close()


def test_set_direct_is_refused_in_the_non_uniform_state(duck_pt):
    W, H = 150, 90
    r, _ = _renderer(duck_pt, W, H, 12, BOUNCES1)
    r.set_moments(True)
    r.render(4)
    est = r.noise_estimate()
    tiles_x = (W + 31) // 32
    pixels = np.array([min(32, W - 32 * (t % tiles_x)) * min(32, H - 32 * (t // tiles_x)) for t in range(est["tile_sum"].size)], np.float64)
    errors = est["tile_sum"].reshape(-1) / pixels
    r.render_adaptive(float(np.median(errors) * 0.7), 4)
    assert not r.tile_samples_uniform()
    before = r.read_accumulation()
    _refused(lambda: r.set_direct(True), "different sample counts")
    _refused(lambda: r.denoise_split(), "different sample counts")            # (that state's message, before "AOVs" / "direct")
    r.set_direct(False)                                                       # (off stays allowed)
    assert _same(before, r.read_accumulation()) and r.read_direct()[1] == 0
    r.close()


def test_the_ranks_direct_reads_sum_to_the_frame(duck_pt):
    parts = []
    for rank in (0, 1):
        r, _ = _renderer(duck_pt, W1, H1, SPP1, BOUNCES1)
        r.set_tile_shard(rank, 2)
        r.set_direct(True)
        r.render(SPP1)
        D, n = r.read_direct()
        assert n == SPP1 and D.any()
        parts.append(D)
        r.close()
    assert not (parts[0].any(-1) & parts[1].any(-1)).any()                    # disjoint pixels
    assert np.array_equal(bits(parts[0] + parts[1]), bits(_one_bounce(W1, H1, SPP1)))


# ------------------------------------------------------------------------------------------------ the filter
def _synthetic(H, W, N, seed):
    """tests/test_gpu_denoise.py's recipe -- noisy colour, normal / depth / albedo edges, background holes, a background disc, zero normals, fireflies -- and
    D = S u with u in [0, 1.2] per pixel: indirect light goes negative somewhere."""
    rng = np.random.default_rng(seed)
    f = np.float32
    ys, xs = np.mgrid[0:H, 0:W]
    cov = rng.integers(1, N + 1, (H, W)).astype(f)
    cov[rng.random((H, W)) < 0.08] = 0                                          # holes
    cov[(xs - W // 3) ** 2 + (ys - H // 2) ** 2 < (min(W, H) // 6) ** 2] = 0    # a background disc
    normal = np.where((xs < W // 2)[..., None], np.array([1, 0, 0], f), np.array([0, 0.6, 0.8], f)).astype(f)
    normal += rng.normal(0, 0.05, (H, W, 3)).astype(f)
    depth = np.where(ys < H // 2, f(2.0), f(7.5)) + rng.random((H, W)).astype(f) * f(0.1)
    albedo = np.where(((xs // 5 + ys // 7) % 2 == 0)[..., None], np.array([0.8, 0.2, 0.1], f), np.array([0.05, 0.5, 0.9], f)).astype(f)
    irr = rng.gamma(1.0, 0.7, (H, W, 3)).astype(f)
    irr[rng.random((H, W)) < 0.01] *= f(500.0)                                  # fireflies
    S = np.zeros((H, W, 4), f)
    S[..., :3] = irr * albedo * f(N)
    S[..., 3] = rng.random((H, W)).astype(f)                                    # (ignored)
    AC = np.concatenate([albedo * cov[..., None], cov[..., None]], -1).astype(f)
    ND = np.concatenate([normal * cov[..., None], (depth * cov)[..., None]], -1).astype(f)
    ND[rng.random((H, W)) < 0.03, :3] = 0                                       # zero normals
    D = (S * rng.uniform(0.0, 1.2, (H, W, 1)).astype(f)).astype(f)
    return S, D, AC, ND


PAIRS = ((0, 0), (0, 3), (3, 0), (1, 5), (5, 5), (8, 2), (2, 8))


@pytest.mark.parametrize("H,W", [(1, 1), (23, 37), (45, 70)])
def test_denoise_split_images_bit_identical_to_the_restatement(H, W):
    N = 6
    S, D, AC, ND = _synthetic(H, W, N, H * 1000 + W)
    if H > 1:
        assert (AC[..., 3] == 0).any() and (AC[..., 3] > 0).any()
        assert ((S - D)[..., :3][AC[..., 3] > 0] < 0).any()
    for sd, si in ((SIGMAS[0], SIGMAS[0]), (SIGMAS[1], SIGMAS[1]), (SIGMAS[0], SIGMAS[1]), (SIGMAS[1], SIGMAS[0])):
        for ld, li in PAIRS:
            pd, pi = dict(sd, iterations=ld), dict(si, iterations=li)
            rgb, bgra = rf.denoise_split_images(S, D, AC, ND, N, exposure=0.25, direct=pd, indirect=pi)
            want = denoise_split(S, D, AC, ND, N, direct=pd, indirect=pi)
            assert np.array_equal(bits(rgb), bits(want)), (H, W, pd, pi)


def _inputs(r):
    S, n = r.read_accumulation()
    D, nd = r.read_direct()
    s = r.read_aovs()
    assert s["samples"] == n == nd
    AC = np.concatenate([s["albedo"], s["coverage"][..., None]], -1)
    ND = np.concatenate([s["normal"], s["depth"][..., None]], -1)
    return S, D, AC, ND, n


def _tonemap(r, rgb):
    import torch
    H, W = rgb.shape[:2]
    t = torch.from_numpy(np.ascontiguousarray(np.concatenate([rgb, np.ones((H, W, 1), np.float32)], -1))).cuda()
    torch.cuda.synchronize()
    return r.tonemap_device_image(t.data_ptr(), W, H, 1)


def _split_renderer(pt, w, h, spp, bounces):
    r, params = _renderer(pt, w, h, spp, bounces)
    r.set_aovs(True)
    r.set_direct(True)
    return r, params


def test_on_a_one_bounce_handle_the_split_filter_is_the_one_filter(duck_pt):
    W, H, spp = 64, 48, 16
    r, _ = _split_renderer(duck_pt, W, H, spp, 1)
    r.render(spp)
    for sig in SIGMAS:
        for L in (1, 5):
            p = dict(rf.denoise_defaults(), **sig, iterations=L)               # (every parameter said: the two calls fill a missing one from different defaults)
            r.denoise(**p)
            want = r.read_denoised()
            for other in (dict(iterations=0), dict(SIGMAS[1], iterations=7)):
                r.denoise_split(direct=p, indirect=other)
                got = r.read_denoised()
                assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2] == spp, (p, other)
    r.close()


def test_duck_denoise_split_bit_identical_to_the_restatement(duck_pt):
    W, H, spp = 64, 48, 16
    r, _ = _split_renderer(duck_pt, W, H, spp, 3)
    r.render(spp)
    S, D, AC, ND, n = _inputs(r)
    dd, di = rf.denoise_split_defaults()
    for pd, pi in ((None, None), (dict(SIGMAS[1], iterations=2), dict(iterations=5)), (dict(iterations=4), dict(SIGMAS[1], iterations=3))):
        r.denoise_split(direct=pd, indirect=pi)
        rgb, bgra, m = r.read_denoised()
        assert m == spp
        want = denoise_split(S, D, AC, ND, spp, direct=dict(dd, **(pd or {})), indirect=dict(di, **(pi or {})))
        assert np.array_equal(bits(rgb), bits(want)), (pd, pi)
        assert np.array_equal(bgra, _tonemap(r, rgb))
    r.close()


def test_atrium_1080p_denoise_split_crops_bit_identical_to_the_restatement():
    from rayfinder_amd import scenes
    pt, _ = scenes.atrium()
    W, H, spp = 1920, 1080, 4
    r, _ = _split_renderer(pt, W, H, spp, 2)
    r.render(spp)
    pd, pi = dict(iterations=3), dict(iterations=5, sigma_color=2.0)
    r.denoise_split(direct=pd, indirect=pi)
    rgb, bgra, m = r.read_denoised()
    S, D, AC, ND, n = _inputs(r)
    assert m == n == spp
    for (x0, y0) in [(0, 0), (928, 508), (1888, 1048), (1500, 300)]:          # (1888, 1048): the frame's last, partial tile
        want = denoise_split_window(S, D, AC, ND, spp, x0, y0, x0 + 32, y0 + 32, direct=pd, indirect=pi)
        assert np.array_equal(bits(rgb[y0:y0 + 32, x0:x0 + 32]), bits(want)), (x0, y0)
    assert np.array_equal(bgra, _tonemap(r, rgb))
    r.close()


def test_denoise_split_refusals_and_invalidation(duck_pt):
    W, H, spp = 64, 48, 8
    r, params = _renderer(duck_pt, W, H, spp, 2)
    r.render(2)
    _refused(r.denoise_split, "AOVs")                                         # AOVs off
    r.set_aovs(True)
    _refused(r.denoise_split, "direct")                                       # direct off
    r.set_direct(True)
    r.render(2)
    _refused(r.denoise_split, "differs")                                      # both on partway: 2 of 4
    r.set_render_parameters(rf.make_render_parameters(W, H, params.camera, spp, 2, params.sky, 0.5))
    _refused(r.denoise_split, "no sample")
    r.render(2)
    r.set_direct(False)
    r.set_direct(True)
    r.render(1)
    _refused(r.denoise_split, "direct sample count")                          # the AOVs cover the 3 samples, D has 1
    r.set_render_parameters(rf.make_render_parameters(W, H, params.camera, spp, 2, params.sky, 0.25))
    r.render(3)
    _refused(lambda: r.denoise_split(direct=dict(iterations=9)), "iterations")
    _refused(lambda: r.denoise_split(indirect=dict(sigma_color=0.0)), "sigma")
    r.denoise_split()
    assert r.read_denoised()[2] == 3
    # every clear of D drops the snapshot, as every clear of the AOV sums does
    r.set_direct(False)
    _refused(r.read_denoised, "no denoised image")
    r.set_direct(True)
    r.set_render_parameters(rf.make_render_parameters(W, H, params.camera, spp, 2, params.sky, 0.5))
    r.render(2)
    r.denoise_split()
    r.set_aovs(False)
    _refused(r.read_denoised, "no denoised image")
    r.set_aovs(True)
    r.set_tile_shard(0, 1)
    r.render(2)
    r.denoise_split()
    assert r.read_denoised()[2] == 2
    r.set_tile_shard(1, 2)
    _refused(r.read_denoised, "no denoised image")
    r.render(2)
    _refused(r.denoise_split, "tile shard")
    r.close()


def _quality(pt, W, H, bounces):
    """tests/test_gpu_denoise.py's recipe: 4 spp against 1024 spp of the same handle parameters, MSE over covered pixels, as a ratio to the noisy frame's"""
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), 1024, bounces, rf.make_sky(), 0.25)
    noisy = rf.ReferencePathTracer(params, pt.scene())
    noisy.set_aovs(True)
    noisy.set_direct(True)
    noisy.render(4)
    noisy.denoise_split()
    split, _, _ = noisy.read_denoised()
    noisy.denoise()
    one, _, _ = noisy.read_denoised()
    S, _, AC, _, _ = _inputs(noisy)
    noisy.close()
    ref = rf.ReferencePathTracer(params, pt.scene())
    ref.render(1024)
    truth = ref.read_accumulation()[0][..., :3] / np.float32(1024)
    ref.close()
    cov = AC[..., 3] > 0
    mse = lambda img: float(((img.astype(np.float64) - truth)[cov] ** 2).mean())   # noqa: E731
    base = mse(S[..., :3] / np.float32(4))
    return mse(split) / base, mse(one) / base


def test_split_quality_atrium_and_duck(duck_pt):
    from rayfinder_amd import scenes
    atrium, _ = scenes.atrium()
    a_split, a_one = _quality(atrium, 480, 270, 4)
    d_split, d_one = _quality(duck_pt, 160, 120, 4)
    print(f"denoised / noisy MSE: atrium split {a_split:.4f} (one filter {a_one:.4f}), duck split {d_split:.4f} (one filter {d_one:.4f})")
    assert a_split <= 0.5 and d_split <= 0.5


def _read_pfm(path, W, H):
    parts = open(path, "rb").read().split(b"\n", 3)
    assert parts[0] == b"PF" and parts[1] == f"{W} {H}".encode()
    return np.frombuffer(parts[3], "<f4").reshape(H, W, 3)[::-1]


def _decode_png(data, W, H):
    import struct
    import zlib
    pos, idat = 8, b""
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 4 * W)
    assert (raw[:, 0] == 0).all()                      # filter type 0 rows (cli_common.hpp's writer)
    return raw[:, 1:].reshape(H, W, 4)


def test_rf_render_direct_indirect_and_denoise_split_match_python(duck_pt, tmp_path):
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    W, H, spp, bounces = 200, 150, 4, 3
    common = [exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces), "--out", str(tmp_path / "o.png")]
    subprocess.check_output(common + ["--direct", str(tmp_path / "d.pfm"), "--indirect", str(tmp_path / "i.pfm"), "--denoise-split", str(tmp_path / "s.png")], timeout=300)
    r, _ = _split_renderer(duck_pt, W, H, spp, bounces)
    r.render(spp)
    S, D, _, _, n = _inputs(r)
    r.denoise_split()
    _, bgra, _ = r.read_denoised()
    r.close()
    nf = np.float32(n)
    assert np.array_equal(bits(_read_pfm(tmp_path / "d.pfm", W, H)), bits(D[..., :3] / nf))
    assert np.array_equal(bits(_read_pfm(tmp_path / "i.pfm", W, H)), bits((S[..., :3] - D[..., :3]) / nf))
    png = _decode_png(open(tmp_path / "s.png", "rb").read(), W, H)
    assert np.array_equal(png[..., :3], np.stack([(bgra >> 16) & 255, (bgra >> 8) & 255, bgra & 255], -1).astype(np.uint8))
    env = dict(os.environ, RF_COMM_TRANSPORT="local", RF_COMM_TIMEOUT_S="120")
    res = subprocess.run(common + ["--gpus", "2", "--direct", str(tmp_path / "d2.pfm")], env=env, capture_output=True, timeout=300)
    assert res.returncode != 0 and b"--gpus 1" in res.stderr and not os.path.exists(tmp_path / "d2.pfm")
