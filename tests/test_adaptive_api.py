"""Tile-adaptive sampling without a GPU: the C ABI entry points exist and refuse bad arguments before any device call, and the restatement the GPU tests compare
against (tests/adaptive_restatement.py) plays the loop include/rayfinder_amd.h states."""
import ctypes as C
import os
import re

import numpy as np

import rayfinder_amd as rf
from adaptive_restatement import estimate_tiles, mean_image, play, prefix_sums, sums_for_counts, tile_errors
from conftest import ROOT
from noise_restatement import estimate

ENTRY_POINTS = ("rf_renderer_render_adaptive", "rf_renderer_read_tile_samples", "rf_renderer_read_mean", "rf_noise_estimate_tiles")
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
NO_DEVICE = rf._ffi.RF_ERROR_NO_DEVICE


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_four_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"RF_API int " + name + r"\(", header), name
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES, name
    assert "typedef struct rf_adaptive_parameters" in header and "typedef struct rf_adaptive_result" in header
    # {f32; u32 x 3} and {u32 x 6; u64; rf_noise_estimate}
    assert C.sizeof(rf._ffi.AdaptiveParameters) == 16
    assert C.sizeof(rf._ffi.AdaptiveResult) == 72 and rf._ffi.AdaptiveResult.pixel_samples.offset == 24 and rf._ffi.AdaptiveResult.last.offset == 32
    for name in ("render_adaptive", "read_tile_samples", "read_mean"):
        assert callable(getattr(rf.ReferencePathTracer, name)), name
    assert callable(rf.noise_estimate_tiles)


def test_a_null_handle_is_an_invalid_argument_and_leaves_the_outputs_untouched():
    lib = rf._ffi.lib
    p = rf._ffi.AdaptiveParameters(0.1, 4, 4, 0)
    res = rf._ffi.AdaptiveResult()
    res.tiles = 77
    assert lib.rf_renderer_render_adaptive(None, C.byref(p), C.byref(res)) == INVALID
    assert res.tiles == 77 and "null" in lib.rf_last_error_message().decode()
    bogus = C.c_void_p(16)                         # never dereferenced: the NULL parameters are refused first
    assert lib.rf_renderer_render_adaptive(bogus, None, C.byref(res)) == INVALID and res.tiles == 77
    counts = np.full(4, 7, np.uint32)
    n = C.c_uint32(7)
    assert lib.rf_renderer_read_tile_samples(None, counts.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID
    assert n.value == 7 and (counts == 7).all()
    assert lib.rf_renderer_read_tile_samples(bogus, counts.ctypes.data_as(C.c_void_p), None) == INVALID
    mean = np.full(8, 3.0, np.float32)
    assert lib.rf_renderer_read_mean(None, mean.ctypes.data_as(C.c_void_p)) == INVALID and (mean == 3.0).all()
    assert lib.rf_renderer_read_mean(bogus, None) == INVALID


def _sentinel_estimate():
    return rf._ffi.NoiseEstimate(-7.0, -7.0, 77, 77, 77, 77)


def _untouched(est):
    return (est.mean_error, est.max_error, est.worst_tile, est.samples, est.pixels, est.nonfinite_pixels) == (-7.0, -7.0, 77, 77, 77, 77)


def test_noise_estimate_tiles_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    W, H = 40, 33                                   # 2 x 2 tiles
    s = np.ones((H, W, 4), np.float32)
    q = np.ones((H, W, 4), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok = np.array([8, 4, 2, 8], np.uint32)
    est = _sentinel_estimate()
    cases = [
        (W, H, None, P(s), P(q), C.byref(est)),                               # NULL counts
        (W, H, P(ok), None, P(q), C.byref(est)),                              # NULL colour sums
        (W, H, P(ok), P(s), None, C.byref(est)),                              # NULL second moments
        (W, H, P(ok), P(s), P(q), None),                                      # NULL out
        (0, H, P(ok), P(s), P(q), C.byref(est)),                              # zero width
        (W, 0, P(ok), P(s), P(q), C.byref(est)),                              # zero height
    ]
    for bad in ([8, 4, 1, 8], [0, 4, 4, 4], [4, 4, 4, 1]):                    # a tile with fewer than 2 samples, wherever it sits
        keep = np.array(bad, np.uint32)
        cases.append((W, H, P(keep), P(s), P(q), C.byref(est)))
        cases[-1] += (keep,)
    for case in cases:
        w, h, pc, ps, pq, pe = case[:6]
        # device ordinal 1 << 20: were a device call made, the status would be NO_DEVICE (no GPU) or "ordinal out of range", never this message
        assert lib.rf_noise_estimate_tiles(1 << 20, w, h, pc, ps, pq, pe, None, None, None) == INVALID, case[:2]
        msg = lib.rf_last_error_message().decode()
        assert "ordinal" not in msg and "HIP" not in msg, msg
        assert _untouched(est)


def test_without_a_device_the_calls_report_no_device():
    """Good arguments reach the device: without one the status is RF_ERROR_NO_DEVICE (with one, the ordinal is out of range)."""
    lib = rf._ffi.lib
    s = np.ones((33, 40, 4), np.float32)
    counts = np.array([8, 4, 2, 8], np.uint32)
    est = _sentinel_estimate()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    status = lib.rf_noise_estimate_tiles(1 << 20, 40, 33, P(counts), P(s), P(s), C.byref(est), None, None, None)
    if _have_gpu():
        assert status == INVALID and "ordinal" in lib.rf_last_error_message().decode()
    else:
        assert status == NO_DEVICE and "no CPU fallback" in lib.rf_last_error_message().decode()
    assert _untouched(est)


def _synthetic(n, h, w, noisy, seed=11):
    """Per-sample radiance with a constant level everywhere and noise only inside the `noisy` slices"""
    rng = np.random.default_rng(seed)
    out = np.full((n, h, w, 4), 1.0, np.float32)
    out[..., 3] = 0
    rows, cols = noisy
    out[:, rows, cols, :3] = rng.gamma(0.5, 2.0, (n, rows.stop - rows.start, cols.stop - cols.start, 3)).astype(np.float32)
    return out


def test_play_stops_flat_tiles_at_the_first_check_and_runs_noisy_ones_to_the_cap():
    W, H, N = 70, 40, 16                            # 3 x 2 tiles, ragged right and bottom
    samples = _synthetic(N, H, W, (slice(0, 32), slice(32, 64)))            # tile 1 is noisy, the others are constant: error exactly 0
    S, Q = prefix_sums(samples)
    out = play(S, Q, W, H, target=1e-3, check_every=4, min_samples=4)
    assert out["counts"].tolist() == [4, 16, 4, 4, 4, 4]
    assert out["estimate_passes"] == 4 and [p["L"] for p in out["passes"]] == [4, 8, 12, 16]
    assert [p["active"] for p in out["passes"]] == [[0, 1, 2, 3, 4, 5], [1], [1], [1]]
    assert out["stopped_tiles"] == 5 and out["min_tile_samples"] == 4 and out["max_tile_samples"] == 16 and out["leading"] == 16
    assert out["pixel_samples"] == 1024 * 4 + 1024 * 16 + 6 * 32 * 4 + 32 * 8 * 4 + 32 * 8 * 4 + 6 * 8 * 4
    assert out["last"]["samples"] == 16 and out["last"]["pixels"] == 1024 and out["last"]["worst_tile"] == 1
    # the defining property: every tile holds the sums of its first counts[t] samples
    assert np.array_equal(out["S"][0:32, 0:32], S[4][0:32, 0:32]) and np.array_equal(out["S"][0:32, 32:64], S[16][0:32, 32:64])
    assert np.array_equal(out["Q"][32:40, 64:70], Q[4][32:40, 64:70])
    assert (out["mean"][..., 3] == 1).all() and np.array_equal(out["mean"][0:32, 0:32, :3], S[4][0:32, 0:32, :3] / np.float32(4))
    # min_samples delays the first check, the cap shortens the last step, and max_samples above spp is clamped
    late = play(S, Q, W, H, target=1e-3, check_every=3, min_samples=7)
    assert [p["L"] for p in late["passes"]] == [9, 12, 15, 16] and late["counts"].tolist() == [9, 16, 9, 9, 9, 9]
    assert play(S, Q, W, H, target=1e-3, check_every=4, max_samples=99)["counts"].tolist() == out["counts"].tolist()
    assert play(S, Q, W, H, target=1e-3, check_every=4, max_samples=6)["counts"].tolist() == [4, 6, 4, 4, 4, 4]


def test_play_ends_of_the_range_and_continuation():
    W, H, N = 40, 33, 12
    samples = _synthetic(N, H, W, (slice(0, 33), slice(0, 40)), seed=3)
    S, Q = prefix_sums(samples)
    assert play(S, Q, W, H, 0.0, 4)["counts"].tolist() == [12] * 4 and play(S, Q, W, H, 0.0, 4)["stopped_tiles"] == 0
    huge = play(S, Q, W, H, 1e30, 4, min_samples=4)
    assert huge["counts"].tolist() == [4] * 4 and huge["stopped_tiles"] == 0 and huge["estimate_passes"] == 1
    one = play(S, Q, W, H, 0.0, 1)                                          # a single sample makes no estimate: the first pass is at L = 2
    assert [p["L"] for p in one["passes"]] == list(range(2, 13))
    # a target between the tile errors at the first check, then a second call with a lower target: only the leading tiles move
    errors = tile_errors(estimate(S[4], Q[4], 4))
    first = play(S, Q, W, H, np.sort(errors)[1], 4, min_samples=4, max_samples=4)
    assert first["counts"].tolist() == [4] * 4
    mid = np.float32(np.sort(errors)[1])
    a = play(S, Q, W, H, mid, 4, min_samples=4, max_samples=8)
    stopped = [t for t in range(4) if errors[t] <= mid]
    assert len(stopped) == 2 and all(a["counts"][t] == 4 for t in stopped) and all(a["counts"][t] == 8 for t in range(4) if t not in stopped)
    b = play(S, Q, W, H, 0.0, 4, counts=a["counts"])
    assert all(b["counts"][t] == 4 for t in stopped) and all(b["counts"][t] == 12 for t in range(4) if t not in stopped)
    # a NaN tile error never stops a tile
    bad = samples.copy()
    bad[0, 0, 0, 0] = np.nan
    Sn, Qn = prefix_sums(bad)
    assert play(Sn, Qn, W, H, 1e30, 4, min_samples=4)["counts"].tolist() == [4] * 4     # (a NaN PIXEL is counted as non-finite with error 0: the tile's sum stays finite)


def test_estimate_tiles_uses_each_tiles_own_count():
    W, H, N = 70, 40, 8
    samples = _synthetic(N, H, W, (slice(0, 40), slice(0, 70)), seed=5)
    S, Q = prefix_sums(samples)
    counts = np.array([8, 4, 2, 4, 8, 6])
    s, q = sums_for_counts(S, Q, counts, W, H)
    got = estimate_tiles(s, q, counts, W, H)
    for t, n in enumerate(counts):
        want = estimate(S[n], Q[n], int(n))
        assert got["tile_sum"][t] == want["tile_sum"][t] and got["tile_max"][t] == want["tile_max"][t]
    assert got["samples"] == 8 and got["pixels"] == W * H
    assert got["max_error"] == got["tile_max"].max() and got["tile_max"][got["worst_tile"]] == got["max_error"]
    uniform = estimate_tiles(S[8], Q[8], np.full(6, 8), W, H)
    want = estimate(S[8], Q[8], 8)
    assert np.array_equal(uniform["error_map"], want["error_map"]) and uniform["mean_error"] == want["mean_error"]
    m = mean_image(s, np.array([8, 4, 0, 4, 8, 6]), W, H)
    assert not m[0:32, 64:70, :3].any() and (m[..., 3] == 1).all()
