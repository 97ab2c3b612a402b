"""Radiance second moments, the noise estimate and render-to-a-noise-target without a GPU: the C ABI entry points exist and refuse bad arguments before any
device call, and the restatement the GPU tests compare against (tests/noise_restatement.py) computes what it says."""
import ctypes as C
import os
import re

import numpy as np

import rayfinder_amd as rf
from conftest import ROOT
from noise_restatement import estimate, moment_sums, pixel_errors, pixel_variance, tile_tree

ENTRY_POINTS = ("rf_renderer_set_moments", "rf_renderer_read_moments", "rf_renderer_noise_estimate", "rf_noise_estimate_images", "rf_renderer_render_until")
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT


def test_the_five_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"RF_API int " + name + r"\(", header), name
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES, name
    assert "typedef struct rf_noise_estimate" in header
    # {double; float; u32; u32; (pad); u64; u64}
    assert C.sizeof(rf._ffi.NoiseEstimate) == 40 and rf._ffi.NoiseEstimate.pixels.offset == 24
    for name in ("set_moments", "read_moments", "noise_estimate", "render_until"):
        assert callable(getattr(rf.ReferencePathTracer, name)), name
    assert callable(rf.noise_estimate_images)


def _sentinel_estimate():
    return rf._ffi.NoiseEstimate(-7.0, -7.0, 77, 77, 77, 77)


def _untouched(est):
    return (est.mean_error, est.max_error, est.worst_tile, est.samples, est.pixels, est.nonfinite_pixels) == (-7.0, -7.0, 77, 77, 77, 77)


def test_a_null_handle_is_an_invalid_argument_and_leaves_the_outputs_untouched():
    lib = rf._ffi.lib
    assert lib.rf_renderer_set_moments(None, 1) == INVALID
    assert lib.rf_renderer_set_moments(None, 0) == INVALID
    q = np.full(8, 3.0, np.float32)
    n = C.c_uint32(7)
    assert lib.rf_renderer_read_moments(None, q.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID
    assert n.value == 7 and (q == 3.0).all()
    est = _sentinel_estimate()
    emap = np.full(8, 3.0, np.float32)
    assert lib.rf_renderer_noise_estimate(None, C.byref(est), emap.ctypes.data_as(C.c_void_p), None, None) == INVALID
    assert _untouched(est) and (emap == 3.0).all()
    frames = C.c_uint32(7)
    assert lib.rf_renderer_render_until(None, 0.1, 4, 16, C.byref(frames), C.byref(est)) == INVALID
    assert frames.value == 7 and _untouched(est)
    assert "null" in lib.rf_last_error_message().decode()


def test_noise_estimate_images_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    s = np.ones((4, 4, 4), np.float32)
    q = np.ones((4, 4, 4), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    est = _sentinel_estimate()
    cases = [
        (4, 4, 8, None, P(q), C.byref(est)),      # NULL colour sums
        (4, 4, 8, P(s), None, C.byref(est)),      # NULL second moments
        (4, 4, 8, P(s), P(q), None),              # NULL out
        (0, 4, 8, P(s), P(q), C.byref(est)),      # zero width
        (4, 0, 8, P(s), P(q), C.byref(est)),      # zero height
        (4, 4, 0, P(s), P(q), C.byref(est)),      # no sample
        (4, 4, 1, P(s), P(q), C.byref(est)),      # one sample: no variance
    ]
    for w, h, n, ps, pq, pe in cases:
        # device ordinal 1 << 20: were a device call made, the status would be NO_DEVICE (no GPU) or "ordinal out of range", never this message
        assert lib.rf_noise_estimate_images(1 << 20, w, h, n, ps, pq, pe, None, None, None) == INVALID, (w, h, n)
        msg = lib.rf_last_error_message().decode()
        assert "ordinal" not in msg and "HIP" not in msg, msg
        assert _untouched(est)


def test_set_aovs_still_refuses_every_flag_bit_but_first_hit():
    lib = rf._ffi.lib
    bogus = C.c_void_p(16)                         # never dereferenced: the flags are checked first
    for flags in (2, 3, 0x80000000):
        assert lib.rf_renderer_set_aovs(bogus, flags) == INVALID
        assert "flag" in lib.rf_last_error_message().decode()


def test_restatement_variance_agrees_with_an_f64_two_pass_variance():
    """N = 256 synthetic samples per pixel, sigma / mu >= 0.5 per channel.  f32 ordered sums are off by at most ~N 2^-24 relative (1.5e-5), and the subtraction
    Q - S mu amplifies that by (mu^2 + sigma^2) / sigma^2 <= 5: agreement to 1e-3 relative."""
    rng = np.random.default_rng(20261017)
    N, H, W = 256, 24, 40
    shape_k = rng.uniform(0.5, 3.0, (H, W, 3))                              # gamma(k): sigma / mu = 1 / sqrt(k) in [0.58, 1.41]
    scale = rng.uniform(0.05, 20.0, (H, W, 3))
    samples = (rng.gamma(shape_k, scale, (N, H, W, 3))).astype(np.float32)
    x = samples.astype(np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).sum(0) / (N - 1)
    assert (np.sqrt(var) / mean >= 0.5).mean() > 0.9                        # the population's ratio is >= 0.5; the sample's with few exceptions
    keep = np.sqrt(var) / mean >= 0.5
    S = np.zeros((H, W, 4), np.float32)
    for r in samples:
        S[..., :3] = S[..., :3] + r
    Q = moment_sums(samples)
    assert Q.dtype == np.float32 and not Q[..., 3].any()
    mu, v = pixel_variance(S, Q, N)
    assert v.dtype == np.float32 and mu.dtype == np.float32
    rel = np.abs(v.astype(np.float64) - var) / var
    assert rel[keep].max() <= 1e-3, rel[keep].max()
    assert np.abs(mu.astype(np.float64) - mean).max() <= 1e-5 * mean.max()
    # and the per-pixel error is the standard error of the mean over the level
    e, bad = pixel_errors(S, Q, N)
    want = np.sqrt(var.sum(-1) / N) / (mean.sum(-1) + 2.0 ** -8)
    assert not bad.any() and np.allclose(e, want, rtol=2e-3)


def test_moment_sums_add_in_the_order_given_from_plus_zero():
    r = [np.full((2, 2, 4), v, np.float32) for v in (1e4, 1.0, 1.0, 1.0, -1e4)]
    q = moment_sums(r)
    want = np.float32(0)
    for v in (1e4, 1.0, 1.0, 1.0, -1e4):
        want = np.float32(want + np.float32(v) * np.float32(v))
    assert (q[..., :3] == want).all() and not q[..., 3].any()
    assert np.array_equal(moment_sums(r[2:], start=moment_sums(r[:2])), q)      # resumable: batching is invisible


def test_tile_tree_is_the_halving_tree_not_a_running_sum():
    a = np.zeros(1024, np.float32)
    a[0], a[512], a[1], a[513] = 1e8, 1.0, -1e8, 1.0
    # h = 512: a[0] = 1e8 + 1 = 1e8 (f32), a[1] = -1e8 + 1 = -1e8; ...; h = 1: a[0] = 1e8 + -1e8 = 0.  A running sum in index order gives 1 + 1 = 2 ... differently rounded.
    assert tile_tree(a) == 0.0
    b = np.arange(1024, dtype=np.float32)
    assert tile_tree(b) == 1023 * 1024 / 2


def test_ragged_frame_counts_only_in_frame_pixels():
    W, H, N = 70, 45, 8
    rng = np.random.default_rng(5)
    samples = rng.gamma(2.0, 1.0, (N, H, W, 3)).astype(np.float32)
    S = np.zeros((H, W, 4), np.float32)
    for r in samples:
        S[..., :3] = S[..., :3] + r
    out = estimate(S, moment_sums(samples), N)
    assert out["tile_pixels"].tolist() == [1024, 1024, 6 * 32, 13 * 32, 13 * 32, 6 * 13]        # 3 x 2 tiles; 70 = 64 + 6, 45 = 32 + 13
    assert out["pixels"] == W * H and out["nonfinite_pixels"] == 0 and out["samples"] == N
    e = out["error_map"]
    assert (e > 0).all()
    # entries outside the frame are zeros: each tile's tree sum is the sum of its in-frame errors up to rounding, and the mean is the map's mean
    for t, (y0, x0) in enumerate([(0, 0), (0, 32), (0, 64), (32, 0), (32, 32), (32, 64)]):
        part = e[y0:y0 + 32, x0:x0 + 32].astype(np.float64)
        assert abs(float(out["tile_sum"][t]) - part.sum()) <= 1e-5 * part.sum()
        assert out["tile_max"][t] == part.max()
    assert abs(out["mean_error"] - e.astype(np.float64).mean()) <= 1e-5 * out["mean_error"]
    assert out["max_error"] == e.max() and out["tile_max"][out["worst_tile"]] == e.max()


def test_nan_and_inf_inputs_are_counted_as_non_finite_with_zero_error():
    W, H, N = 40, 33, 4
    S = np.full((H, W, 4), 4.0, np.float32)
    Q = np.full((H, W, 4), 8.0, np.float32)          # mu = 1, v = (8 - 4) / 3 per channel: a finite error everywhere ...
    S[0, 0, 0] = np.nan                              # ... except: NaN sum
    Q[1, 1, 1] = np.inf                              # inf second moment: v = inf, e = inf
    S[2, 2, :3] = np.inf                             # inf sum: mu = inf, S mu = inf, Q - inf = -inf -> v = 0, e = 0 / inf = 0: finite
    S[32, 39, 2] = -np.inf                           # (second tile row, second tile column) l = -inf, v: (8 - inf) < 0 -> 0; e = 0 / -inf = -0: finite
    S[3, 3, :3] = 0.0
    Q[3, 3, :3] = 0.0                                # all-zero pixel: e = 0 / 2^-8 = 0
    Q[4, 4, :3] = 1.0                                # negative variance: (1 - 4) / 3 < 0 -> 0
    Q[6, 6, 0] = np.nan                              # NaN second moment: v > 0 is false -> that channel's v is 0, the pixel stays finite
    out = estimate(S, Q, N)
    e = out["error_map"]
    assert out["nonfinite_pixels"] == 2 and out["tile_nonfinite"].tolist() == [2, 0, 0, 0]
    assert e[0, 0] == 0 and e[1, 1] == 0 and e[2, 2] == 0 and e[3, 3] == 0 and e[4, 4] == 0 and e[32, 39] == 0
    assert 0 < e[6, 6] < e[10, 10]
    assert np.isfinite(e).all() and np.isfinite(out["tile_sum"]).all() and np.isfinite(out["mean_error"])
    plain = np.float32(np.sqrt(np.float32(np.float32(4.0) / np.float32(4.0))) / np.float32(3.0 + 2.0 ** -8))      # v = 4/3 per channel: s2 = ((v + v) + v) / 4
    assert np.isclose(e[10, 10], plain, rtol=1e-6) and out["max_error"] == e[10, 10]
    assert out["pixels"] == W * H
