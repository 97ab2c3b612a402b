"""The split-component denoiser with per-tile sample counts and RF_DIRECT_TILE_COUNTS, without a GPU: rf_denoise_split_tiles and the flag are declared, exported and
bound, rf_denoise_split_tiles refuses bad arguments before any device call, rf_renderer_set_direct checks its argument's domain, and the restatement the GPU tests
compare against (tests/split_tiles_restatement.py) is the one-count split restatement at equal counts and the one filter's per-tile restatement when D == S."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import rayfinder_amd as rf
from conftest import ROOT, bits
from denoise_tiles_restatement import denoise_tiles
from split_restatement import denoise_split, split_prep
from split_tiles_restatement import denoise_split_tiles, split_prep_tiles

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
NO_DEVICE = rf._ffi.RF_ERROR_NO_DEVICE
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
SIGMAS = (dict(), dict(sigma_color=3.5, sigma_normal=0.4, sigma_depth=0.02))


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _random_inputs(H, W, seed):
    """Random sums with background pixels (coverage 0, or a depth sum <= 0), zero normals and a D that leaves negative indirect light somewhere"""
    rng = np.random.default_rng(seed)
    f = np.float32
    cov = rng.integers(1, 7, (H, W)).astype(f)
    cov[rng.random((H, W)) < 0.15] = 0
    AC = np.concatenate([rng.random((H, W, 3)).astype(f) * cov[..., None], cov[..., None]], -1).astype(f)
    ND = np.concatenate([rng.normal(0, 1, (H, W, 3)).astype(f) * cov[..., None], (rng.uniform(0.5, 9.0, (H, W)).astype(f) * cov)[..., None]], -1).astype(f)
    ND[rng.random((H, W)) < 0.04, 3] *= f(-1)                                   # z <= 0: background too
    ND[rng.random((H, W)) < 0.03, :3] = 0
    S = np.concatenate([rng.gamma(1.0, 2.0, (H, W, 3)).astype(f), rng.random((H, W, 1)).astype(f)], -1).astype(f)
    D = (S * rng.uniform(0.0, 1.2, (H, W, 1)).astype(f)).astype(f)
    return S, D, AC, ND


def test_the_entry_point_and_the_flag_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    assert re.search(r"RF_API int rf_denoise_split_tiles\(", header)
    assert hasattr(lib, "rf_denoise_split_tiles") and "rf_denoise_split_tiles" in rf._ffi.SIGNATURES
    assert len(rf._ffi.SIGNATURES["rf_denoise_split_tiles"][1]) == 13
    assert re.search(r"#define RF_DIRECT_TILE_COUNTS 0x100u", header) and rf._ffi.RF_DIRECT_TILE_COUNTS == 0x100
    assert callable(rf.denoise_split_tiles)
    names = list(inspect.signature(rf.denoise_split_tiles).parameters)
    assert names == ["color_sum", "direct_sum", "albedo_coverage", "normal_depth", "tile_samples", "exposure", "device_ordinal", "direct", "indirect"]
    assert list(inspect.signature(rf.ReferencePathTracer.set_direct).parameters)[1:] == ["enabled", "tile_counts"]
    assert inspect.signature(rf.ReferencePathTracer.set_direct).parameters["tile_counts"].default is False


def test_set_direct_with_a_null_handle_is_invalid_whatever_the_word():
    lib = rf._ffi.lib
    for word in (0, 1, 0x101, 0x100, 0x102, 0x200, 0x301, 2):
        assert lib.rf_renderer_set_direct(None, word) == INVALID, hex(word)


def test_denoise_split_tiles_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    W, H = 40, 33                                   # 2 x 2 tiles
    s, d, ac, nd = (np.ones((H, W, 4), np.float32) for _ in range(4))
    ok = np.array([8, 4, 1, 8], np.uint32)
    good = rf._ffi.DenoiseParameters(5, 1.0, 0.1, 0.1)
    rgba = np.full((H, W, 4), -7.0, np.float32)
    bgra = np.full((H, W), 77, np.uint32)
    g = C.byref(good)
    cases = [
        (W, H, None, P(s), P(d), P(ac), P(nd), g, g),                         # NULL counts
        (W, H, P(ok), None, P(d), P(ac), P(nd), g, g),                        # each NULL input
        (W, H, P(ok), P(s), None, P(ac), P(nd), g, g),
        (W, H, P(ok), P(s), P(d), None, P(nd), g, g),
        (W, H, P(ok), P(s), P(d), P(ac), None, g, g),
        (0, H, P(ok), P(s), P(d), P(ac), P(nd), g, g),                        # zero width / height
        (W, 0, P(ok), P(s), P(d), P(ac), P(nd), g, g),
    ]
    for t in range(4):                                                        # a tile without a sample, wherever it sits
        keep = ok.copy()
        keep[t] = 0
        cases.append((W, H, P(keep), P(s), P(d), P(ac), P(nd), g, g, keep))
    for bad in ((9, 1.0, 0.1, 0.1), (5, 0.0, 0.1, 0.1), (5, 1.0, -0.1, 0.1), (5, 1.0, 0.1, float("nan")), (5, float("inf"), 0.1, 0.1)):   # either component's set
        keep = rf._ffi.DenoiseParameters(*bad)
        cases.append((W, H, P(ok), P(s), P(d), P(ac), P(nd), C.byref(keep), g, keep))
        cases.append((W, H, P(ok), P(s), P(d), P(ac), P(nd), g, C.byref(keep), keep))
    for case in cases:
        w, h, pc, ps, pd_, pa, pn, pdir, pind = case[:9]
        # device ordinal 1 << 20: were a device call made, the status would be NO_DEVICE (no GPU) or "ordinal out of range", never this message
        assert lib.rf_denoise_split_tiles(1 << 20, w, h, pc, ps, pd_, pa, pn, pdir, pind, 1.0, P(rgba), P(bgra)) == INVALID, case[:2]
        msg = lib.rf_last_error_message().decode()
        assert "ordinal" not in msg and "HIP" not in msg, msg
        assert (rgba == -7.0).all() and (bgra == 77).all()
    assert lib.rf_denoise_split_tiles(1 << 20, W, H, P(ok), P(s), P(d), P(ac), P(nd), g, g, float("nan"), P(rgba), P(bgra)) == INVALID
    assert "ordinal" not in lib.rf_last_error_message().decode()


def test_without_a_device_good_arguments_report_no_device():
    lib = rf._ffi.lib
    s = np.ones((33, 40, 4), np.float32)
    counts = np.array([8, 4, 1, 8], np.uint32)
    rgba = np.full((33, 40, 4), -7.0, np.float32)
    for params in (None, C.byref(rf._ffi.DenoiseParameters(0, 1.0, 0.1, 0.1))):   # NULL parameters: that component's defaults
        status = lib.rf_denoise_split_tiles(1 << 20, 40, 33, P(counts), P(s), P(s), P(s), P(s), params, params, 1.0, P(rgba), None)
        if _have_gpu():
            assert status == INVALID and "ordinal" in lib.rf_last_error_message().decode()
        else:
            assert status == NO_DEVICE and "no CPU fallback" in lib.rf_last_error_message().decode()
        assert (rgba == -7.0).all()


def test_python_wrapper_checks_the_shapes_and_the_number_of_counts():
    s = np.ones((33, 40, 4), np.float32)
    for counts in ([4, 4, 4], np.ones((3, 2), np.uint32)):
        try:
            rf.denoise_split_tiles(s, s, s, s, counts)
        except ValueError as e:
            assert "4 tile counts expected" in str(e)
        else:
            raise AssertionError("accepted")
    try:
        rf.denoise_split_tiles(s, s[:, :39], s, s, [4, 4, 4, 4])
    except ValueError as e:
        assert "one size" in str(e)
    else:
        raise AssertionError("accepted")


PAIRS = ((0, 0), (0, 3), (3, 0), (1, 2), (5, 5), (4, 1))


def test_equal_counts_are_the_one_count_split_restatement_bit_for_bit():
    H, W = 45, 70                                   # 3 x 2 tiles, ragged both ways
    for N in (1, 6):
        S, D, AC, ND = _random_inputs(H, W, 300 + N)
        assert (AC[..., 3] == 0).any() and (AC[..., 3] > 0).any()
        counts = np.full(6, N, np.uint32)
        for a, b in zip(split_prep_tiles(S, D, AC, ND, counts), split_prep(S, D, AC, ND, N)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        for sd, si in ((SIGMAS[0], SIGMAS[0]), (SIGMAS[0], SIGMAS[1]), (SIGMAS[1], SIGMAS[0])):
            for ld, li in PAIRS:
                pd, pi = dict(sd, iterations=ld), dict(si, iterations=li)
                assert np.array_equal(bits(denoise_split_tiles(S, D, AC, ND, counts, pd, pi)), bits(denoise_split(S, D, AC, ND, N, pd, pi))), (N, pd, pi)


def test_with_d_equal_to_s_it_is_the_one_filters_per_tile_restatement():
    """D == S and L_D >= 1: the indirect chain is +0 throughout, whatever its parameters, and the result is the one filter's with the direct parameters"""
    H, W = 45, 70
    S, _, AC, ND = _random_inputs(H, W, 77)
    assert (AC[..., 3] == 0).any() and (ND[..., 3][AC[..., 3] > 0] < 0).any()
    rng = np.random.default_rng(5)
    counts = rng.integers(1, 40, 6).astype(np.uint32)
    assert len(set(counts.tolist())) >= 4
    for sig in SIGMAS:
        for L in (1, 2, 5):
            p = dict(dict(sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1), **sig, iterations=L)
            want = denoise_tiles(S, AC, ND, counts, **p)
            for other in (dict(iterations=0), dict(SIGMAS[1], iterations=4)):
                assert np.array_equal(bits(denoise_split_tiles(S, S, AC, ND, counts, p, other)), bits(want)), (p, other)
    # ... and the counts do show: another count in one tile moves that tile's prep and no other pixel's
    _, D, _, _ = _random_inputs(H, W, 78)
    got = split_prep_tiles(S, D, AC, ND, counts)
    other = counts.copy()
    other[4] += 1
    moved = split_prep_tiles(S, D, AC, ND, other)
    tile4 = np.zeros((H, W), bool)
    tile4[32:45, 32:64] = True
    for k in (0, 1, 2):                                                       # c, eD, eI
        assert not np.array_equal(bits(moved[k][tile4]), bits(got[k][tile4])), k
    for a, b in zip(moved, got):
        assert np.array_equal(a[~tile4].view(np.uint8), b[~tile4].view(np.uint8))
