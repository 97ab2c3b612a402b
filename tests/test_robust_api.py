"""The bucket sums and the robust mean without a GPU: the restatement's own worked cases (include/rayfinder_amd.h, "Bucket sums and the robust mean"), the C ABI's
argument checks that are made before any device call, and the declarations of the six entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import ROOT, bits
from robust_restatement import bucket_sizes, bucket_sums, denoise_robust, robust_mean

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
F = np.float32
# name -> the parameter list as the header writes it (whitespace folded)
PROTOTYPES = {
    "rf_renderer_set_buckets": "rf_renderer* r, uint32_t K",
    "rf_renderer_read_buckets": "rf_renderer* r, float* buckets, uint32_t* K, uint32_t* bucket_sample_count",
    "rf_renderer_robust_mean": "rf_renderer* r",
    "rf_renderer_read_robust_mean": "rf_renderer* r, float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* sample_count",
    "rf_robust_mean_images": "int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t K, uint32_t samples, const float* buckets, float exposure, "
                             "float* out_rgba, uint32_t* out_bgra8, uint8_t* out_trim",
    "rf_renderer_denoise_robust": "rf_renderer* r, const rf_denoise_parameters* params",
}
CTYPE = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}


def _pixel(keys, N=None):
    """One pixel whose K bucket MEANS have the given keys (grey: r = g = b = key / 3 would round, so the key sits in r alone): sums = mean * bucket size"""
    K = len(keys)
    N = K if N is None else N
    B = np.zeros((K, 1, 1, 4), np.float32)
    for b, (k, n) in enumerate(zip(keys, bucket_sizes(K, N))):
        B[b, 0, 0, 0] = F(k) * F(n)
    return B


def test_the_six_entry_points_are_declared_exported_and_bound_with_the_headers_signatures():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    for name, want in PROTOTYPES.items():
        m = re.search(r"RF_API int " + name + r"\(([^)]*)\);", header)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert ", ".join(params) == want, (name, params)
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES, name
        res, args = rf._ffi.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            base = p.rsplit(" ", 1)[0]
            if base.endswith("*"):
                pointee = CTYPE.get(base[:-1].replace("const ", "").strip())
                assert a is C.c_void_p or (pointee is not None and a is C.POINTER(pointee)), (name, p, a)
            else:
                assert a is CTYPE[base], (name, p, a)
    for name in ("set_buckets", "read_buckets", "robust_mean", "read_robust_mean", "denoise_robust"):
        assert callable(getattr(rf.ReferencePathTracer, name)), name
    assert callable(rf.robust_mean_images)


def test_bucket_sums_deal_the_samples_round_robin_from_the_first_ordinal():
    rng = np.random.default_rng(5)
    samples = rng.random((11, 2, 3, 4)).astype(np.float32)
    B = bucket_sums(samples, 3)
    for b in range(3):
        want = np.zeros((2, 3, 3), np.float32)
        for j in range(b, 11, 3):
            want = want + samples[j, ..., :3]
        assert np.array_equal(bits(B[b, ..., :3]), bits(want)) and not B[b, ..., 3].any()
    # two batches of 4 and 7 are one batch of 11; a first ordinal of 2 shifts every sample by two buckets
    two = bucket_sums(samples[4:], 3, first_ordinal=4, start=bucket_sums(samples[:4], 3))
    assert np.array_equal(bits(two), bits(B))
    shifted = bucket_sums(samples[:3], 3, first_ordinal=2)
    assert np.array_equal(bits(shifted[2, ..., :3]), bits(samples[0, ..., :3])) and np.array_equal(bits(shifted[0, ..., :3]), bits(samples[1, ..., :3]))
    assert bucket_sizes(9, 70) == [8] * 7 + [7] * 2 and bucket_sizes(5, 5) == [1] * 5


def test_all_buckets_equal_is_the_mean_of_the_means():
    for K in (3, 5, 9, 15):
        B = np.zeros((K, 1, 2, 4), np.float32)
        B[:, 0, 0, :3] = (0.25, 0.5, 0.125)
        B[:, 0, 1, :3] = (3.0, 0.0, 7.0)
        M, trim = robust_mean(B, K)
        assert trim.tolist() == [[0, 0]]
        assert np.array_equal(M, B[0, ..., :3])


def test_one_outlier_in_five_is_cut():
    M, trim = robust_mean(_pixel([1, 1, 1, 1, 1001]), 5)
    # num = -4 - 2 + 0 + 2 + 4004 = 4000, den = 5 * 1005 = 5025, G = 4000/5025, t = G * 2.5 = 1.99..., c = 1
    assert trim[0, 0] == 1 and M[0, 0, 0] == F(1)
    # the outlier's bucket index does not matter
    M, trim = robust_mean(_pixel([1001, 1, 1, 1, 1]), 5)
    assert trim[0, 0] == 1 and M[0, 0, 0] == F(1)


def test_two_outliers_in_nine_are_cut():
    M, trim = robust_mean(_pixel([1] * 7 + [1001] * 2), 9)
    # num = (-8 -6 -4 -2 +0 +2 +4) + (6 + 8) 1001 = 14000, den = 9 * 2009 = 18081, t = (14000 / 18081) * 4.5 = 3.48..., c = 3
    assert trim[0, 0] == 3 and M[0, 0, 0] == F(1)


def test_unequal_bucket_sizes_divide_each_sum_by_its_own_count():
    # N = 7, K = 3: sizes 3, 2, 2; every bucket's MEAN is 2
    M, trim = robust_mean(_pixel([2, 2, 2], N=7), 7)
    assert trim[0, 0] == 0 and M[0, 0, 0] == F(2)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nonfinite_bucket_takes_the_median_and_the_result_is_finite(bad):
    for K in (3, 9):
        keys = [float(i + 1) for i in range(K)]
        B = _pixel(keys)
        B[1, 0, 0, 1] = bad                                                  # one channel of one bucket
        M, trim = robust_mean(B, K)
        assert trim[0, 0] == (K - 1) // 2 and np.isfinite(M).all()
        # the bad bucket sorts last: the median is over the K - 1 good keys and the bad one
        assert M[0, 0, 0] == F(sorted(keys[:1] + keys[2:])[(K - 1) // 2])


def test_an_all_zero_pixel_is_zero_and_untrimmed():
    M, trim = robust_mean(np.zeros((7, 1, 1, 4), np.float32), 20)
    assert trim[0, 0] == 0 and not M.any() and not np.signbit(M).any()


def test_relabelling_buckets_with_distinct_keys_changes_nothing():
    rng = np.random.default_rng(11)
    K, N = 9, 9                                                              # equal sizes: a relabelling moves sums between equal divisors
    B = np.zeros((K, 6, 7, 4), np.float32)
    B[..., :3] = rng.random((K, 6, 7, 3)).astype(np.float32)
    B[3, 2, 2, :3] = 500.0                                                   # a firefly
    M, trim = robust_mean(B, N)
    m = B[..., :3] / F(1)
    key = (m[..., 0] + m[..., 1]) + m[..., 2]
    assert all(np.unique(key[:, y, x]).size == K for y in range(6) for x in range(7))
    assert trim[2, 2] > 0 and trim.min() == 0
    for perm in (np.arange(K)[::-1], rng.permutation(K)):
        M2, trim2 = robust_mean(B[perm], N)
        assert np.array_equal(bits(M2), bits(M)) and np.array_equal(trim2, trim)


def test_ties_keep_bucket_order():
    # three keys tie (1 + 2 == 2 + 1 == 0 + 3) while the channels differ: the stable order decides which of them the trim cuts.
    # keys 3, 3, 3, 1800, 1800: num = -12 - 6 + 0 + 3600 + 7200 = 10782, den = 5 * 3609, t = 1.49..., c = 1: ranks 1 .. 3 are kept
    B = np.zeros((5, 1, 1, 4), np.float32)
    B[0, 0, 0, :3] = (1, 2, 0)
    B[1, 0, 0, :3] = (2, 1, 0)
    B[2, 0, 0, :3] = (0, 3, 0)
    B[3:, 0, 0, :3] = (900, 900, 0)
    M, trim = robust_mean(B, 5)
    assert trim[0, 0] == 1 and M[0, 0].tolist() == [F(902) / F(3), F(904) / F(3), 0.0]     # order 0, 1, 2, 3, 4: bucket 0 is cut
    M, trim = robust_mean(B[[1, 0, 2, 3, 4]], 5)
    assert trim[0, 0] == 1 and M[0, 0].tolist() == [F(901) / F(3), F(905) / F(3), 0.0]     # now (2, 1, 0) comes first and is cut
    # (K = 3 never trims a bright outlier: G < 2/3 there, so t < 1)
    assert robust_mean(B[[0, 1, 3]], 3)[1][0, 0] == 0


def test_denoise_robust_with_the_plain_mean_is_the_denoiser():
    """The one change is prep's colour: handing in c = S / Nf must reproduce denoise_restatement.denoise bit for bit"""
    from denoise_restatement import denoise
    rng = np.random.default_rng(3)
    H, W, N = 12, 14, 6
    S = np.zeros((H, W, 4), np.float32); S[..., :3] = rng.random((H, W, 3)).astype(np.float32) * N
    AC = np.zeros((H, W, 4), np.float32); AC[..., :3] = rng.random((H, W, 3)).astype(np.float32) * N; AC[..., 3] = N
    ND = np.zeros((H, W, 4), np.float32); ND[..., :3] = rng.standard_normal((H, W, 3)).astype(np.float32) * N; ND[..., 3] = (1 + rng.random((H, W)).astype(np.float32)) * N
    AC[:2, :, 3] = 0                                                         # background rows
    c = S[..., :3] / F(N)
    for L in (0, 2):
        assert np.array_equal(bits(denoise_robust(c, AC, ND, N, iterations=L)), bits(denoise(S, AC, ND, N, iterations=L)))


def test_robust_mean_images_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    b = np.ones((15, 4, 4, 4), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full((4, 4, 4), 3.0, np.float32)
    cases = [
        (4, 4, 9, 16, None),          # NULL planes
        (0, 4, 9, 16, P(b)),          # zero width
        (4, 0, 9, 16, P(b)),          # zero height
        (4, 4, 4, 16, P(b)),          # K even
        (4, 4, 1, 16, P(b)),          # K = 1
        (4, 4, 17, 32, P(b)),         # K = 17
        (4, 4, 0, 16, P(b)),          # K = 0
        (4, 4, 9, 8, P(b)),           # samples < K
        (4, 4, 9, 0, P(b)),           # no sample
    ]
    for w, h, K, n, pb in cases:
        # device ordinal 1 << 20: were a device call made, the status would be NO_DEVICE (no GPU) or "ordinal out of range", never this message
        assert lib.rf_robust_mean_images(1 << 20, w, h, K, n, pb, 1.0, P(out), None, None) == INVALID, (w, h, K, n)
        msg = lib.rf_last_error_message().decode()
        assert "ordinal" not in msg and "HIP" not in msg, msg
        assert (out == 3.0).all()


def test_set_buckets_checks_k_before_the_handle_and_null_handles_are_invalid():
    lib = rf._ffi.lib
    for K in (1, 2, 4, 8, 16, 17, 0xFFFFFFFF):
        assert lib.rf_renderer_set_buckets(None, K) == INVALID and "K must be" in lib.rf_last_error_message().decode(), K
    for K in (0, 3, 9, 15):
        assert lib.rf_renderer_set_buckets(None, K) == INVALID and "null" in lib.rf_last_error_message().decode(), K
    k, n = C.c_uint32(7), C.c_uint32(7)
    assert lib.rf_renderer_read_buckets(None, None, C.byref(k), C.byref(n)) == INVALID and (k.value, n.value) == (7, 7)
    assert lib.rf_renderer_robust_mean(None) == INVALID
    assert lib.rf_renderer_read_robust_mean(None, None, None, None, C.byref(n)) == INVALID and n.value == 7
    assert lib.rf_renderer_denoise_robust(None, None) == INVALID and "null" in lib.rf_last_error_message().decode()
    bad = rf._ffi.DenoiseParameters(9, 1.0, 0.1, 0.1)
    assert lib.rf_renderer_denoise_robust(None, C.byref(bad)) == INVALID and "iterations" in lib.rf_last_error_message().decode()
