"""The denoiser with per-tile sample counts, without a GPU: rf_denoise_tiles and RF_AOV_TILE_COUNTS are declared, exported and bound, rf_denoise_tiles refuses bad
arguments before any device call, and the restatement the GPU tests compare against (tests/denoise_tiles_restatement.py) differs from the one-count restatement in
prep's divisor alone."""
import ctypes as C
import os
import re

import numpy as np

import rayfinder_amd as rf
from conftest import ROOT, bits
from denoise_restatement import denoise, prep
from denoise_tiles_restatement import denoise_tiles, pixel_counts, prep_tiles
from test_gpu_denoise import SIGMAS, _synthetic

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
NO_DEVICE = rf._ffi.RF_ERROR_NO_DEVICE
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_entry_point_and_the_mode_bit_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    assert re.search(r"RF_API int rf_denoise_tiles\(", header)
    assert hasattr(lib, "rf_denoise_tiles") and "rf_denoise_tiles" in rf._ffi.SIGNATURES
    assert len(rf._ffi.SIGNATURES["rf_denoise_tiles"][1]) == 11
    assert re.search(r"#define RF_AOV_TILE_COUNTS 0x100u", header) and rf._ffi.RF_AOV_TILE_COUNTS == 0x100 and rf._ffi.RF_AOV_FIRST_HIT == 1
    assert callable(rf.denoise_tiles)
    import inspect
    assert list(inspect.signature(rf.ReferencePathTracer.set_aovs).parameters)[1:] == ["enabled", "tile_counts"]
    assert inspect.signature(rf.ReferencePathTracer.set_aovs).parameters["tile_counts"].default is False


def test_set_aovs_checks_the_flags_before_the_handle():
    """With a NULL handle throughout (nothing here can dereference a bad pointer): good flags are refused for the handle, bad flags for the flags."""
    lib = rf._ffi.lib
    for flags in (0, 1, 0x101):
        assert lib.rf_renderer_set_aovs(None, flags) == INVALID and "null" in lib.rf_last_error_message().decode(), hex(flags)
    for flags in (0x100, 0x102, 0x200, 0x301, 2):
        assert lib.rf_renderer_set_aovs(None, flags) == INVALID, hex(flags)
        msg = lib.rf_last_error_message().decode()
        assert ("RF_AOV_FIRST_HIT" in msg) if flags == 0x100 else ("flag" in msg), msg


def test_denoise_tiles_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    W, H = 40, 33                                   # 2 x 2 tiles
    s, ac, nd = (np.ones((H, W, 4), np.float32) for _ in range(3))
    ok = np.array([8, 4, 1, 8], np.uint32)
    good = rf._ffi.DenoiseParameters(5, 1.0, 0.1, 0.1)
    rgba = np.full((H, W, 4), -7.0, np.float32)
    bgra = np.full((H, W), 77, np.uint32)
    g = C.byref(good)
    cases = [
        (W, H, None, P(s), P(ac), P(nd), g),                                  # NULL counts
        (W, H, P(ok), None, P(ac), P(nd), g),                                 # each NULL input
        (W, H, P(ok), P(s), None, P(nd), g),
        (W, H, P(ok), P(s), P(ac), None, g),
        (0, H, P(ok), P(s), P(ac), P(nd), g),                                 # zero width / height
        (W, 0, P(ok), P(s), P(ac), P(nd), g),
    ]
    for t in range(4):                                                        # a tile without a sample, wherever it sits
        keep = ok.copy()
        keep[t] = 0
        cases.append((W, H, P(keep), P(s), P(ac), P(nd), g, keep))
    for bad in ((9, 1.0, 0.1, 0.1), (5, 0.0, 0.1, 0.1), (5, 1.0, -0.1, 0.1), (5, 1.0, 0.1, float("nan")), (5, float("inf"), 0.1, 0.1)):   # rf_denoise_images' checks
        keep = rf._ffi.DenoiseParameters(*bad)
        cases.append((W, H, P(ok), P(s), P(ac), P(nd), C.byref(keep), keep))
    for case in cases:
        w, h, pc, ps, pa, pn, pp = case[:7]
        # device ordinal 1 << 20: were a device call made, the status would be NO_DEVICE (no GPU) or "ordinal out of range", never this message
        assert lib.rf_denoise_tiles(1 << 20, w, h, pc, ps, pa, pn, pp, 1.0, P(rgba), P(bgra)) == INVALID, case[:2]
        msg = lib.rf_last_error_message().decode()
        assert "ordinal" not in msg and "HIP" not in msg, msg
        assert (rgba == -7.0).all() and (bgra == 77).all()
    assert lib.rf_denoise_tiles(1 << 20, W, H, P(ok), P(s), P(ac), P(nd), g, float("nan"), P(rgba), P(bgra)) == INVALID   # (and rf_denoise_images' exposure check)
    assert "ordinal" not in lib.rf_last_error_message().decode()


def test_without_a_device_good_arguments_report_no_device():
    """Good arguments reach the device: without one the status is RF_ERROR_NO_DEVICE (with one, the ordinal is out of range)."""
    lib = rf._ffi.lib
    s = np.ones((33, 40, 4), np.float32)
    counts = np.array([8, 4, 1, 8], np.uint32)
    rgba = np.full((33, 40, 4), -7.0, np.float32)
    for params in (None, C.byref(rf._ffi.DenoiseParameters(0, 1.0, 0.1, 0.1))):   # NULL parameters: the defaults
        status = lib.rf_denoise_tiles(1 << 20, 40, 33, P(counts), P(s), P(s), P(s), params, 1.0, P(rgba), None)
        if _have_gpu():
            assert status == INVALID and "ordinal" in lib.rf_last_error_message().decode()
        else:
            assert status == NO_DEVICE and "no CPU fallback" in lib.rf_last_error_message().decode()
        assert (rgba == -7.0).all()


def test_python_wrapper_checks_the_number_of_counts():
    s = np.ones((33, 40, 4), np.float32)
    for counts in ([4, 4, 4], np.ones((3, 2), np.uint32)):
        try:
            rf.denoise_tiles(s, s, s, counts)
        except ValueError as e:
            assert "4 tile counts expected" in str(e)
        else:
            raise AssertionError("accepted")


def test_equal_counts_are_the_uniform_restatement_bit_for_bit():
    H, W = 37, 70                                   # 3 x 2 tiles, ragged both ways
    for N in (1, 6):
        S, AC, ND = _synthetic(H, W, N, 100 + N)
        counts = np.full(6, N, np.uint32)
        for sig in SIGMAS:
            for L in (0, 1, 3, 5):
                assert np.array_equal(bits(denoise_tiles(S, AC, ND, counts, iterations=L, **sig)), bits(denoise(S, AC, ND, N, iterations=L, **sig))), (N, L, sig)
        for a, b in zip(prep_tiles(S, AC, ND, counts), prep(S, AC, ND, N)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_a_pixels_prep_is_the_uniform_prep_at_its_own_tiles_count():
    """The synthetic sums scaled per tile (a tile with n samples holds n / 6 of the 6-sample sums): prep of a pixel depends on its own tile's count alone."""
    H, W = 70, 100                                  # 4 x 3 tiles
    S, AC, ND = _synthetic(H, W, 6, 7)
    rng = np.random.default_rng(11)
    counts = rng.integers(1, 10, 12).astype(np.uint32)
    assert len(set(counts.tolist())) >= 4
    nf = pixel_counts(counts, H, W)
    assert nf.shape == (H, W) and nf[0, 0] == counts[0] and nf[33, 65] == counts[1 * 4 + 2] and nf[69, 99] == counts[11]
    scale = (nf / np.float32(6))[..., None]
    S, AC, ND = (S * scale).astype(np.float32), (AC * scale).astype(np.float32), (ND * scale).astype(np.float32)
    got = prep_tiles(S, AC, ND, counts)
    assert got[6].any() and not got[6].all()                                 # background and surface pixels both
    for n in np.unique(counts):
        want = prep(S, AC, ND, int(n))
        here = nf == np.float32(n)
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a[here].view(np.uint8), b[here].view(np.uint8)), (int(n), k)
    # ... and the counts do show: with another count in one tile, that tile's prep changes and no other pixel's does
    other = counts.copy()
    other[5] += 1
    moved = prep_tiles(S, AC, ND, other)
    tile5 = np.zeros((H, W), bool)
    tile5[32:64, 32:64] = True
    assert not np.array_equal(bits(moved[0][tile5]), bits(got[0][tile5]))
    for a, b in zip(moved, got):
        assert np.array_equal(a[~tile5].view(np.uint8), b[~tile5].view(np.uint8))
