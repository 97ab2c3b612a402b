"""The robust mean with one count per tile without a GPU: rf_robust_mean_tiles' argument checks that are made before any device call, the switch's checks that come
before the handle, the declarations of the new entry point and flag, and the invariants of tests/robust_tiles_restatement.py itself."""
import ctypes as C
import os
import re

import numpy as np

import rayfinder_amd as rf
from adaptive_restatement import tile_slices
from conftest import ROOT, bits
from denoise_tiles_restatement import pixel_counts
from robust_restatement import denoise_robust, robust_mean
from robust_tiles_restatement import denoise_robust_tiles, robust_mean_tiles

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
PROTOTYPE = ("int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t K, const uint32_t* tile_samples, const float* buckets, float exposure, "
             "float* out_rgba, uint32_t* out_bgra8, uint8_t* out_trim")


def _planes(k, h, w, seed):
    rng = np.random.default_rng(seed)
    B = np.zeros((k, h, w, 4), np.float32)
    B[..., :3] = rng.random((k, h, w, 3)).astype(np.float32) * 8
    B[rng.integers(0, k, 40), rng.integers(0, h, 40), rng.integers(0, w, 40), :3] = 4000.0    # fireflies: trimmed pixels
    return B


def test_the_entry_point_and_the_flag_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    m = re.search(r"RF_API int rf_robust_mean_tiles\(([^)]*)\);", header)
    assert m and ", ".join(" ".join(p.split()) for p in m.group(1).split(",")) == PROTOTYPE
    assert hasattr(C.CDLL(rf._ffi.LIB_PATH), "rf_robust_mean_tiles")
    res, args = rf._ffi.SIGNATURES["rf_robust_mean_tiles"]
    assert res is C.c_int and len(args) == 10
    assert args[:4] == [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32] and args[6] is C.c_float and all(a is C.c_void_p for a in args[4:6] + args[7:])
    assert re.search(r"#define RF_BUCKETS_TILE_COUNTS 0x100u", header) and rf._ffi.RF_BUCKETS_TILE_COUNTS == 0x100
    assert callable(rf.robust_mean_tiles)
    assert "tile_counts" in rf.ReferencePathTracer.set_buckets.__code__.co_varnames


def test_robust_mean_tiles_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    b = np.ones((15, 40, 40, 4), np.float32)                                 # 40 x 40: 2 x 2 tiles
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = np.array([16, 9, 40, 1000], np.uint32)
    out = np.full((40, 40, 4), 3.0, np.float32)
    cases = [
        (40, 40, 9, P(good), None),                                           # NULL planes
        (40, 40, 9, None, P(b)),                                              # NULL counts
        (0, 40, 9, P(good), P(b)),                                            # zero width
        (40, 0, 9, P(good), P(b)),                                            # zero height
        (40, 40, 4, P(good), P(b)),                                           # K even
        (40, 40, 1, P(good), P(b)),                                           # K = 1
        (40, 40, 17, P(good), P(b)),                                          # K = 17
        (40, 40, 0, P(good), P(b)),                                           # K = 0
        (40, 40, 9 | 0x100, P(good), P(b)),                                   # (the bit belongs to rf_renderer_set_buckets alone)
        (40, 40, 11, P(good), P(b)),                                          # a count below K: the second tile
        (40, 40, 9, P(np.array([16, 9, 40, 8], np.uint32)), P(b)),            # ... the last tile
        (40, 40, 9, P(np.array([16, 0, 40, 9], np.uint32)), P(b)),            # ... a tile without a sample
    ]
    for w, h, K, pc, pb in cases:
        # device ordinal 1 << 20: were a device call made, the status would be NO_DEVICE (no GPU) or "ordinal out of range", never this message
        assert lib.rf_robust_mean_tiles(1 << 20, w, h, K, pc, pb, 1.0, P(out), None, None) == INVALID, (w, h, K)
        msg = lib.rf_last_error_message().decode()
        assert "ordinal" not in msg and "HIP" not in msg, msg
        assert (out == 3.0).all()
    assert "tile count" in msg
    # the wrapper counts the tiles itself
    try:
        rf.robust_mean_tiles(b[:9], good[:3])
    except ValueError as e:
        assert "4 tile counts expected" in str(e)
    else:
        raise AssertionError("three counts for four tiles were accepted")


def test_the_switch_is_checked_before_the_handle():
    lib = rf._ffi.lib
    for word in (0x100, 0x100 | 4, 0x100 | 1, 0x100 | 17, 0x200 | 9, 0x300 | 9, 0x10000 | 9, 0x80000000 | 9):
        assert lib.rf_renderer_set_buckets(None, word) == INVALID and "K must be" in lib.rf_last_error_message().decode(), hex(word)
    for word in (0x100 | 3, 0x100 | 9, 0x100 | 15):
        assert lib.rf_renderer_set_buckets(None, word) == INVALID and "null" in lib.rf_last_error_message().decode(), hex(word)


def test_equal_counts_are_the_one_count_combine():
    w, h, k = 72, 40, 9
    B = _planes(k, h, w, 1)
    for n in (9, 12, 70):
        M, trim = robust_mean_tiles(B, np.full(6, n), w, h)
        M1, trim1 = robust_mean(B, n)
        assert np.array_equal(bits(M), bits(M1)) and np.array_equal(trim, trim1) and 0 < int((trim > 0).sum()) < w * h


def test_a_tiles_result_does_not_depend_on_its_neighbours_counts():
    w, h, k = 72, 40, 5
    B = _planes(k, h, w, 2)
    a = robust_mean_tiles(B, [5, 6, 7, 8, 9, 10], w, h)
    b = robust_mean_tiles(B, [33, 6, 100, 5, 9, 31], w, h)
    for t, (rows, cols) in enumerate(tile_slices(w, h)):
        same = np.array_equal(bits(a[0][rows, cols]), bits(b[0][rows, cols])) and np.array_equal(a[1][rows, cols], b[1][rows, cols])
        assert same == (t in (1, 4)), t                                       # (counts that do not divide alike give other means: the tiles do differ)
    # every tile is the one-count combine at its own count, on its own pixels
    for t, (rows, cols) in enumerate(tile_slices(w, h)):
        M, trim = robust_mean(B[:, rows, cols], [5, 6, 7, 8, 9, 10][t])
        assert np.array_equal(bits(a[0][rows, cols]), bits(M)) and np.array_equal(a[1][rows, cols], trim)


def test_the_robust_denoise_with_equal_counts_is_the_one_count_form():
    rng = np.random.default_rng(3)
    h, w, n = 40, 72, 6
    M = rng.random((h, w, 3)).astype(np.float32)
    AC = np.zeros((h, w, 4), np.float32); AC[..., :3] = rng.random((h, w, 3)).astype(np.float32) * n; AC[..., 3] = n
    ND = np.zeros((h, w, 4), np.float32); ND[..., :3] = rng.standard_normal((h, w, 3)).astype(np.float32) * n; ND[..., 3] = (1 + rng.random((h, w)).astype(np.float32)) * n
    AC[:2, :, 3] = 0                                                          # background rows
    for L in (0, 2):
        assert np.array_equal(bits(denoise_robust_tiles(M, AC, ND, np.full(6, n), iterations=L)), bits(denoise_robust(M, AC, ND, n, iterations=L)))
    # other counts: another image (L > 0), and M itself for L = 0
    counts = [6, 3, 6, 12, 6, 2]
    assert np.array_equal(bits(denoise_robust_tiles(M, AC, ND, counts, iterations=0)), bits(M))
    other = denoise_robust_tiles(M, AC, ND, counts, iterations=2)
    assert not np.array_equal(bits(other), bits(denoise_robust(M, AC, ND, n, iterations=2)))
    assert pixel_counts(counts, h, w)[0, 32] == 3 and pixel_counts(counts, h, w)[39, 71] == 2
