"""The edge-aware a-trous denoiser on the GPU (-m gpu): kDenoisePrep + kDenoiseAtrous are bit-identical to the numpy restatement
(tests/denoise_restatement.py) on synthetic inputs and on rendered frames, leave the renderer's own state alone, follow the bookkeeping
include/rayfinder_amd.h states, cut the error of a 4-spp frame at least in half, and give rf-render the same bytes on any rank count."""
import os
import subprocess

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import ROOT, bits
from denoise_restatement import denoise, denoise_window

pytestmark = pytest.mark.gpu

SIGMAS = (dict(), dict(sigma_color=3.5, sigma_normal=0.4, sigma_depth=0.02))


def _synthetic(H, W, N, seed):
    """Sums of N samples with noisy colour, normal / depth / albedo edges, background holes, zero normals and fireflies."""
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
    return S, AC, ND


@pytest.mark.parametrize("H,W", [(1, 1), (23, 37), (144, 256)])
def test_denoise_images_bit_identical_to_the_restatement(H, W):
    N = 6
    S, AC, ND = _synthetic(H, W, N, H * 1000 + W)
    for sig in SIGMAS:
        for L in range(9):
            rgb, bgra = rf.denoise_images(S, AC, ND, N, exposure=0.25, iterations=L, **sig)
            want = denoise(S, AC, ND, N, iterations=L, **sig)
            assert np.array_equal(bits(rgb), bits(want)), (H, W, L, sig)
    if H > 1:
        assert (AC[..., 3] == 0).any() and (AC[..., 3] > 0).any()


def _renderer(pt, w, h, spp, bounces, **kw):
    params = rf.make_render_parameters(w, h, rf.fly_camera(w, h), spp, bounces, rf.make_sky(), 0.25)
    return rf.ReferencePathTracer(params, pt.scene(), **kw), params


def _inputs(r):
    S, n = r.read_accumulation()
    s = r.read_aovs()
    assert s["samples"] == n
    AC = np.concatenate([s["albedo"], s["coverage"][..., None]], -1)
    ND = np.concatenate([s["normal"], s["depth"][..., None]], -1)
    return S, AC, ND, n


def _tonemap(r, rgb):
    import torch
    H, W = rgb.shape[:2]
    t = torch.from_numpy(np.ascontiguousarray(np.concatenate([rgb, np.ones((H, W, 1), np.float32)], -1))).cuda()
    torch.cuda.synchronize()
    return r.tonemap_device_image(t.data_ptr(), W, H, 1)


@pytest.fixture(scope="module")
def atrium():
    from rayfinder_amd import scenes
    pt, _ = scenes.atrium()
    return pt


def test_duck_denoise_bit_identical_to_the_restatement(duck_pt):
    W, H, spp = 64, 48, 16
    r, _ = _renderer(duck_pt, W, H, spp, 3)
    r.set_aovs(True)
    r.render(spp)
    S, AC, ND, n = _inputs(r)
    for sig in SIGMAS:
        r.denoise(**sig)
        rgb, bgra, m = r.read_denoised()
        assert m == spp
        assert np.array_equal(bits(rgb), bits(denoise(S, AC, ND, spp, **sig))), sig
        assert np.array_equal(bgra, _tonemap(r, rgb))
    r.close()


def test_atrium_1080p_denoise_crops_bit_identical_to_the_restatement(atrium):
    W, H, spp = 1920, 1080, 4
    r, _ = _renderer(atrium, W, H, spp, 2)
    r.set_aovs(True)
    r.render(spp)
    r.denoise()
    rgb, bgra, m = r.read_denoised()
    S, AC, ND, n = _inputs(r)
    assert m == n == spp
    for (x0, y0) in [(0, 0), (928, 508), (1888, 1048), (1500, 300)]:
        want = denoise_window(S, AC, ND, spp, x0, y0, x0 + 32, y0 + 32)
        assert np.array_equal(bits(rgb[y0:y0 + 32, x0:x0 + 32]), bits(want)), (x0, y0)
    assert np.array_equal(bgra, _tonemap(r, rgb))
    r.close()


def test_denoise_is_non_invasive_and_reproducible(duck_pt):
    W, H, bounces = 150, 90, 3

    def state(r):
        s = r.stats()
        return r.read_accumulation(), _inputs(r)[1:3], r.read_tonemapped(), [s[k] for k in ("primary_rays", "closest_rays", "shadow_rays")]

    a, _ = _renderer(duck_pt, W, H, 8, bounces)
    a.set_aovs(True)
    a.render(4)
    a.denoise()
    first = a.read_denoised()
    a.denoise()
    second = a.read_denoised()
    assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(first[1], second[1]) and first[2] == second[2] == 4
    a.render(4)
    b, _ = _renderer(duck_pt, W, H, 8, bounces)
    b.set_aovs(True)
    b.render(8)
    sa, sb = state(a), state(b)
    assert np.array_equal(bits(sa[0][0]), bits(sb[0][0])) and sa[0][1] == sb[0][1] == 8
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(sa[1], sb[1]))
    assert np.array_equal(sa[2], sb[2]) and sa[3] == sb[3]
    # the snapshot stays as it was (4 samples) until denoise runs again
    assert a.read_denoised()[2] == 4 and np.array_equal(bits(a.read_denoised()[0]), bits(first[0]))
    a.close()
    b.close()


def test_denoise_errors_and_invalidation(duck_pt):
    W, H, spp = 64, 48, 8
    INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT

    def refused(fn, match):
        with pytest.raises(rf.RayfinderError, match=match) as e:
            fn()
        assert e.value.status == INVALID

    r, params = _renderer(duck_pt, W, H, spp, 2)
    refused(r.read_denoised, "no denoised image")
    r.render(2)
    refused(r.denoise, "AOVs")                                   # off
    r.set_aovs(True)
    r.render(2)
    refused(r.denoise, "differs")                                # on partway: 2 AOV samples of 4
    r.set_render_parameters(rf.make_render_parameters(W, H, params.camera, spp, 2, params.sky, 0.5))
    refused(r.denoise, "no sample")
    r.render(3)
    refused(lambda: r.denoise(iterations=9), "iterations")
    r.denoise()
    assert r.read_denoised()[2] == 3
    # every clear of the AOV sums drops the snapshot
    r.set_render_parameters(rf.make_render_parameters(W, H, params.camera, spp, 2, params.sky, 0.25))
    refused(r.read_denoised, "no denoised image")
    r.render(3)
    r.denoise()
    r.set_aovs(False)
    refused(r.read_denoised, "no denoised image")
    r.set_aovs(True)
    r.render(1)
    refused(r.denoise, "differs")                                # the accumulation kept its 3 samples, the AOVs have 1
    r.set_tile_shard(0, 1)                                       # (clears both)
    r.render(1)
    r.denoise()
    r.set_tile_shard(0, 1)
    refused(r.read_denoised, "no denoised image")
    r.render(1)
    r.denoise()
    import ctypes as C
    import torch
    ptr, nbytes = C.c_void_p(), C.c_uint64(0)
    rf.check(rf._ffi.lib.rf_renderer_accumulation_device_buffer(r._h, C.byref(ptr), C.byref(nbytes)))
    buf = torch.zeros(nbytes.value // 4, dtype=torch.float32, device="cuda")
    r.bind_accumulation_buffer(buf.data_ptr(), nbytes.value)
    refused(r.read_denoised, "no denoised image")
    r.render(2)
    r.denoise()                                                  # (a caller-owned accumulation buffer works as well)
    assert r.read_denoised()[2] == 2
    r.set_tile_shard(1, 2)
    r.render(2)
    refused(r.denoise, "tile shard")
    r.close()


def _quality(pt, W, H, bounces):
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), 1024, bounces, rf.make_sky(), 0.25)
    noisy = rf.ReferencePathTracer(params, pt.scene())
    noisy.set_aovs(True)
    noisy.render(4)
    noisy.denoise()
    den, _, _ = noisy.read_denoised()
    S, AC, ND, _ = _inputs(noisy)
    noisy.close()
    ref = rf.ReferencePathTracer(params, pt.scene())
    ref.render(1024)
    truth = ref.read_accumulation()[0][..., :3] / np.float32(1024)
    ref.close()
    cov = AC[..., 3] > 0
    mse = lambda img: float(((img.astype(np.float64) - truth)[cov] ** 2).mean())   # noqa: E731
    return mse(den) / mse(S[..., :3] / np.float32(4))


def test_quality_atrium_and_duck(atrium, duck_pt):
    ratio_atrium = _quality(atrium, 480, 270, 4)
    ratio_duck = _quality(duck_pt, 160, 120, 4)
    print(f"denoised / noisy MSE: atrium {ratio_atrium:.4f}, duck {ratio_duck:.4f}")
    assert ratio_atrium <= 0.5 and ratio_duck <= 0.5


def test_rf_render_denoise_png_matches_python_and_any_rank_count(duck_pt, tmp_path):
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    W, H, spp, bounces = 200, 150, 4, 3
    files = {}
    for gpus in (1, 4, 3):
        env = dict(os.environ, RF_COMM_TRANSPORT="local", RF_COMM_TIMEOUT_S="120")
        txt = subprocess.check_output([exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces),
                                       "--out", str(tmp_path / f"g{gpus}.png"), "--denoise", str(tmp_path / f"d{gpus}.png"),
                                       "--denoise-pfm", str(tmp_path / f"d{gpus}.pfm"), "--gpus", str(gpus)], env=env, timeout=300).decode()
        assert f"on {gpus} GPU(s)" in txt
        files[gpus] = [open(tmp_path / f"d{gpus}.{ext}", "rb").read() for ext in ("png", "pfm")]
    assert files[4] == files[1] and files[3] == files[1]
    # the same frame through Python: rf-render uses exposure 2^-2 and the fly camera
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), spp, bounces, rf.make_sky(), 0.25)
    r = rf.ReferencePathTracer(params, duck_pt.scene())
    r.set_aovs(True)
    r.render(spp)
    r.denoise()
    rgb, bgra, _ = r.read_denoised()
    r.close()
    pfm = files[1][1]
    parts = pfm.split(b"\n", 3)
    assert parts[0] == b"PF" and parts[1] == f"{W} {H}".encode()
    assert np.array_equal(np.frombuffer(parts[3], "<f4").reshape(H, W, 3)[::-1].view(np.uint32), bits(rgb))
    png = _decode_png(files[1][0], W, H)
    want = np.stack([(bgra >> 16) & 255, (bgra >> 8) & 255, bgra & 255], -1).astype(np.uint8)
    assert np.array_equal(png[..., :3], want)


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
