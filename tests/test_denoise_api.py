"""The a-trous denoiser without a GPU: the C ABI entry points exist, carry the header's defaults and refuse bad arguments before any device call, and
the restatement the GPU tests compare against (tests/denoise_restatement.py) has the properties the header states."""
import ctypes as C
import math
import os

import numpy as np

import rayfinder_amd as rf
from conftest import ROOT, bits
from denoise_restatement import DEFAULTS, denoise, denoise_window

NAMES = ("rf_denoise_default_parameters", "rf_renderer_denoise", "rf_renderer_read_denoised", "rf_denoise_images")


def test_denoise_symbols_are_exported_and_declared():
    lib = C.CDLL(rf._ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES
        assert f"RF_API int {name}(" in header
    for name in ("denoise", "read_denoised"):
        assert callable(getattr(rf.ReferencePathTracer, name))
    assert callable(rf.denoise_images) and callable(rf.denoise_defaults)


def test_defaults_match_the_header_and_the_restatement():
    d = rf.denoise_defaults()
    assert d["iterations"] == DEFAULTS["iterations"] == 5
    for k in ("sigma_color", "sigma_normal", "sigma_depth"):
        assert np.float32(d[k]) == np.float32(DEFAULTS[k])
    assert (np.float32(d["sigma_color"]), np.float32(d["sigma_normal"]), np.float32(d["sigma_depth"])) == (1.0, np.float32(0.1), np.float32(0.1))
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    assert "defaults L = 5, σc = 1, σn = 0.1, σz = 0.1" in header
    assert rf._ffi.lib.rf_denoise_default_parameters(None) == rf._ffi.RF_ERROR_INVALID_ARGUMENT


BAD = [dict(iterations=9), dict(iterations=100), dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_depth=math.inf), dict(sigma_color=math.nan),
       dict(sigma_depth=-0.0)]


def _params(**kw):
    return rf._denoise_parameters(kw) if not kw else rf._ffi.DenoiseParameters(*(dict(rf.denoise_defaults(), **kw)[k] for k in DEFAULTS))


def test_bad_parameters_and_null_handles_are_refused_before_any_device_call():
    lib = rf._ffi.lib
    INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
    bogus = C.c_void_p(16)                  # never dereferenced: the parameters are checked first
    for kw in BAD:
        assert lib.rf_renderer_denoise(bogus, C.byref(_params(**kw))) == INVALID, kw
        msg = lib.rf_last_error_message().decode()
        assert ("iterations" in msg) if "iterations" in kw else ("sigma" in msg), (kw, msg)
    assert lib.rf_renderer_denoise(None, None) == INVALID
    assert lib.rf_renderer_denoise(None, C.byref(_params())) == INVALID
    n = C.c_uint32(7)
    assert lib.rf_renderer_read_denoised(None, None, None, C.byref(n)) == INVALID and n.value == 7


def test_denoise_images_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
    a = np.zeros((2, 3, 4), np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    good = C.byref(_params())
    out = np.full((2, 3, 4), 5.0, np.float32)
    o = out.ctypes.data_as(C.c_void_p)
    cases = [(0, 3, 2, 1, p, p, p, good), (0, 0, 2, 1, p, p, p, good), (0, 3, 0, 1, p, p, p, good), (0, 3, 2, 0, p, p, p, good),
             (0, 3, 2, 1, None, p, p, good), (0, 3, 2, 1, p, None, p, good), (0, 3, 2, 1, p, p, None, good), (0, 1 << 16, 1 << 15, 1, p, p, p, good)]
    cases += [(0, 3, 2, 1, p, p, p, C.byref(_params(**kw))) for kw in BAD]
    for i, args in enumerate(cases):
        if i == 0:
            continue                        # the valid call (it would need a device)
        assert lib.rf_denoise_images(*args, 1.0, o, None) == INVALID, args
    assert lib.rf_denoise_images(0, 3, 2, 1, p, p, p, good, math.inf, o, None) == INVALID
    assert (out == 5.0).all()               # nothing written


# ------------------------------------------------------------------------------------------------ restatement self-checks
def _inputs(H, W, N, seed, bg_frac=0.2):
    rng = np.random.default_rng(seed)
    cov = rng.integers(1, N + 1, (H, W)).astype(np.float32)
    cov[rng.random((H, W)) < bg_frac] = 0
    S = np.zeros((H, W, 4), np.float32)
    S[..., :3] = rng.gamma(1.0, 1.0, (H, W, 3)).astype(np.float32) * np.float32(N)
    AC = np.zeros((H, W, 4), np.float32)
    AC[..., :3] = rng.random((H, W, 3)).astype(np.float32) * cov[..., None]
    AC[..., 3] = cov
    ND = np.zeros((H, W, 4), np.float32)
    n = rng.normal(size=(H, W, 3)).astype(np.float32)
    ND[..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True).astype(np.float32) * cov[..., None]
    ND[..., 3] = (rng.random((H, W)).astype(np.float32) + np.float32(0.5)) * cov
    return S, AC, ND


def test_zero_iterations_give_the_mean_bit_for_bit():
    S, AC, ND = _inputs(13, 17, 6, 1)
    out = denoise(S, AC, ND, 6, iterations=0)
    assert np.array_equal(bits(out), bits(S[..., :3] / np.float32(6)))


def test_background_pixels_pass_through_bit_for_bit():
    S, AC, ND = _inputs(21, 19, 4, 2, bg_frac=0.4)
    bg = AC[..., 3] == 0
    for L in (1, 3, 5):
        out = denoise(S, AC, ND, 4, iterations=L)
        assert np.array_equal(bits(out[bg]), bits(S[..., :3][bg] / np.float32(4)))
        assert not np.array_equal(bits(out[~bg]), bits(S[..., :3][~bg] / np.float32(4)))   # the rest is filtered


def test_edge_isolation_across_a_normal_edge():
    """Left half faces +x, right half +z: 1 - dot = 1 >= σn across the edge.  Any change of colour on the right leaves the left's output alone."""
    H, W, N = 24, 40, 4
    S, AC, ND = _inputs(H, W, N, 3, bg_frac=0.0)
    ND[:, :20, :3] = np.float32(N) * np.array([1, 0, 0], np.float32)
    ND[:, 20:, :3] = np.float32(N) * np.array([0, 0, 1], np.float32)
    S2 = S.copy()
    S2[:, 20:, :3] = np.random.default_rng(9).gamma(2.0, 3.0, (H, 20, 3)).astype(np.float32)
    for kw in (dict(), dict(iterations=8, sigma_color=100.0, sigma_depth=1000.0), dict(sigma_normal=1.0)):
        a, b = denoise(S, AC, ND, N, **kw), denoise(S2, AC, ND, N, **kw)
        assert np.array_equal(bits(a[:, :20]), bits(b[:, :20])), kw
        assert not np.array_equal(bits(a[:, 20:]), bits(b[:, 20:]))


def test_window_with_margin_equals_the_whole_frame():
    S, AC, ND = _inputs(150, 160, 8, 4)
    whole = denoise(S, AC, ND, 8, iterations=5)
    part = denoise_window(S, AC, ND, 8, 70, 64, 102, 96, iterations=5)
    assert np.array_equal(bits(part), bits(whole[64:96, 70:102]))
