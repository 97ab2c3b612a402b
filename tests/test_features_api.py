"""The feature export without a GPU: the C ABI entry points exist, channel counts and order, every refusal rf_export_features_images makes before it touches a device
(on a machine without one a device call would answer RF_ERROR_NO_DEVICE, so RF_ERROR_INVALID_ARGUMENT is the proof), the Python wrappers' argument checks, the
restatement's own edge cases, and the request's host arithmetic under the sanitizers as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import features_restatement as fr
import rayfinder_amd as rf
from conftest import ROOT

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
lib = rf._ffi.lib


def _message():
    return lib.rf_last_error_message().decode()


def test_symbols_are_exported_and_declared():
    raw = C.CDLL(rf._ffi.LIB_PATH)
    for name in ("rf_feature_channel_count", "rf_renderer_export_features", "rf_comm_export_features", "rf_export_features_images"):
        assert hasattr(raw, name) and name in rf._ffi.SIGNATURES
    assert callable(rf.ReferencePathTracer.export_features) and callable(rf.TileComm.export_features)
    assert callable(rf.export_features_images) and callable(rf.feature_channels)
    assert C.sizeof(rf._ffi.FeatureRequest) == 16
    # the header's words
    with open(os.path.join(ROOT, "include", "rayfinder_amd.h")) as f:
        header = f.read()
    for name, bit, _ in rf._ffi.FEATURE_GROUPS:
        assert f"#define RF_FEATURE_{name.upper()} 0x{bit:03x}u" in header
    assert rf._ffi.FEATURE_GROUPS == fr.GROUPS


def test_channel_counts_and_order():
    n = C.c_uint32(99)
    for mask in range(1, 0x400):
        assert lib.rf_feature_channel_count(mask, C.byref(n)) == 0 and n.value == fr.channel_count(mask)
    assert n.value == 22
    for bad in (0, 0x400, 0x80000001, 0xFFFFFFFF):
        n.value = 77
        assert lib.rf_feature_channel_count(bad, C.byref(n)) == INVALID and n.value == 77
    assert lib.rf_feature_channel_count(1, None) == INVALID
    names, count = rf.feature_channels(("depth", "color"))       # the groups' bit order, whatever the order given
    assert names == ("color.r", "color.g", "color.b", "depth") and count == 4
    assert rf.feature_channels("normal") == (("normal.x", "normal.y", "normal.z"), 3)
    assert rf.feature_channels(0x3FF)[1] == 22 and rf.feature_channels(0x3FF)[0][-3:] == ("variance.b", "error", "samples")
    assert rf.feature_channels(0x208) == (("depth", "samples"), 2)
    assert rf.feature_channels([g for g, _, _ in rf._ffi.FEATURE_GROUPS]) == rf.feature_channels(0x3FF)
    for bad in ((), 0, 0x400, ("colour",), "rgb", -1):
        with pytest.raises(ValueError):
            rf.feature_channels(bad)


def _images(width=8, height=8, samples=4, counts=None, have=(1, 1, 1, 1, 1), request=(1, 0, 0, 0), out=True, req_null=False):
    big = width * height > 4096          # (a frame the library refuses for its size: nothing of that size is allocated here)
    plane = np.zeros((1, 1, 4) if big else (height or 1, width or 1, 4), np.float32)
    req = rf._ffi.FeatureRequest(*request)
    dst = np.full(22 if big else max(width * height, 1) * 22, 7.0, np.float32)
    status = lib.rf_export_features_images(0, width, height, samples, None if counts is None else np.asarray(counts, np.uint32).ctypes.data_as(C.c_void_p),
                                           *(plane.ctypes.data_as(C.c_void_p) if h else None for h in have), None if req_null else C.byref(req),
                                           dst.ctypes.data_as(C.c_void_p) if out else None)
    assert (dst == 7.0).all(), "a refused call wrote to the output"
    return status


def test_export_features_images_refuses_before_any_device_call():
    M = fr.mask_of
    # the request
    assert _images(req_null=True) == INVALID
    for request, word in (((0, 0, 0, 0), "empty"), ((0x400, 0, 0, 0), "unknown channel"), ((1, 2, 0, 0), "layout"), ((1, 0, 2, 0), "element type"), ((1, 0, 0, 1), "reserved")):
        assert _images(request=request) == INVALID and word in _message(), (request, _message())
    # sizes, the output, the counts
    assert _images(width=0) == INVALID and _images(height=0) == INVALID and "non-zero" in _message()
    assert _images(width=65536, height=32768, out=True, have=(0, 0, 0, 0, 0), request=(0x200, 0, 0, 0)) == INVALID and "too large" in _message()
    assert _images(out=False) == INVALID
    assert _images(samples=0) == INVALID and "sample count" in _message()
    assert _images(width=33, height=65, counts=[3, 3, 0, 3, 3, 3]) == INVALID and "every tile" in _message()
    # a NULL that a selected channel reads: S for COLOR / INDIRECT / VARIANCE / ERROR, Q for VARIANCE / ERROR, both AOV sums for the guides, D for DIRECT / INDIRECT
    needs = {"color": (0,), "albedo": (2, 3), "normal": (2, 3), "depth": (2, 3), "coverage": (2, 3), "direct": (4,), "indirect": (0, 4), "variance": (0, 1), "error": (0, 1)}
    for name, planes in needs.items():
        for missing in planes:
            have = [1] * 5
            have[missing] = 0
            assert _images(have=have, request=(M([name]), 0, 0, 0)) == INVALID and "null argument" in _message(), (name, missing)
    # VARIANCE / ERROR: any count below 2
    for name in ("variance", "error"):
        assert _images(samples=1, request=(M([name]), 0, 0, 0)) == INVALID and "at least 2" in _message()
        assert _images(width=33, height=65, counts=[3, 3, 3, 3, 1, 3], request=(M([name]), 1, 1, 0)) == INVALID and "at least 2" in _message()


def test_a_valid_call_reaches_the_device_check():
    """Everything above is refused with INVALID_ARGUMENT; the same call with valid arguments gets past the checks: without a GPU it answers NO_DEVICE (with one it runs)."""
    status = lib.rf_export_features_images(0, 8, 8, 4, None, np.zeros((8, 8, 4), np.float32).ctypes.data_as(C.c_void_p), None, None, None, None,
                                           C.byref(rf._ffi.FeatureRequest(1, 0, 0, 0)), np.zeros(192, np.float32).ctypes.data_as(C.c_void_p))
    assert status in (0, rf._ffi.RF_ERROR_NO_DEVICE), _message()
    # a counts-only request reads no sum at all
    status = lib.rf_export_features_images(0, 8, 8, 4, None, None, None, None, None, None, C.byref(rf._ffi.FeatureRequest(0x200, 1, 1, 0)),
                                           np.zeros(64, np.float16).ctypes.data_as(C.c_void_p))
    assert status in (0, rf._ffi.RF_ERROR_NO_DEVICE), _message()


def test_null_handles_are_refused():
    req = rf._ffi.FeatureRequest(1, 0, 0, 0)
    bogus = C.c_void_p(16)   # never dereferenced: the NULLs and the request are checked first
    n = C.c_uint32(5)
    assert lib.rf_renderer_export_features(None, C.byref(req), bogus, 64, C.byref(n)) == INVALID
    assert lib.rf_renderer_export_features(bogus, None, bogus, 64, C.byref(n)) == INVALID
    assert lib.rf_renderer_export_features(bogus, C.byref(req), None, 64, C.byref(n)) == INVALID
    assert lib.rf_comm_export_features(None, bogus, C.byref(req), bogus, 64, None) == INVALID
    assert lib.rf_comm_export_features(bogus, None, C.byref(req), bogus, 64, None) == INVALID
    assert lib.rf_comm_export_features(bogus, bogus, None, bogus, 64, None) == INVALID
    assert lib.rf_comm_export_features(bogus, bogus, C.byref(req), None, 64, None) == INVALID
    for request in ((0, 0, 0, 0), (0x800, 0, 0, 0), (1, 7, 0, 0), (1, 0, 7, 0), (1, 0, 0, 7)):
        assert lib.rf_renderer_export_features(bogus, C.byref(rf._ffi.FeatureRequest(*request)), bogus, 64, None) == INVALID, request
        assert lib.rf_comm_export_features(bogus, bogus, C.byref(rf._ffi.FeatureRequest(*request)), bogus, 64, None) == INVALID, request
    assert n.value == 5


def test_python_wrappers_check_their_arguments():
    import torch
    S = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(ValueError, match="layout"):
        rf.export_features_images(S, samples=4, channels=("color",), layout="nchw")
    with pytest.raises(ValueError, match="dtype"):
        rf.export_features_images(S, samples=4, channels=("color",), dtype="bf16")
    with pytest.raises(ValueError, match="unknown feature channels"):
        rf.export_features_images(S, samples=4, channels=("colour",))
    with pytest.raises(ValueError, match="no sum"):
        rf.export_features_images(samples=4, channels=("samples",))
    with pytest.raises(ValueError, match="one size"):
        rf.export_features_images(S, albedo_coverage=np.zeros((8, 9, 4), np.float32), samples=4)
    with pytest.raises(ValueError, match="tile counts expected"):
        rf.export_features_images(S, samples=4, tile_samples=[4, 4], channels=("color",))
    with pytest.raises(rf.RayfinderError) as e:      # the library's own refusal comes through as INVALID_ARGUMENT
        rf.export_features_images(S, samples=4, channels=("color", "albedo"))
    assert e.value.status == INVALID
    # the destination tensor: device, dtype, shape, contiguity -- checked before the library is called
    check = rf._feature_tensor
    with pytest.raises(TypeError):
        check("t", np.zeros((3, 8, 8), np.float32), (3, 8, 8), "f32", 0)
    with pytest.raises(ValueError, match="lies on cpu"):
        check("t", torch.zeros((3, 8, 8)), (3, 8, 8), "f32", 0)
    meta = dict(device="meta")     # a tensor without storage stands in for the device checks that need no GPU
    with pytest.raises(ValueError, match="lies on meta"):
        check("t", torch.zeros((3, 8, 8), **meta), (3, 8, 8), "f32", 0)


def test_the_restatement_on_its_own_edges():
    """What the GPU tests rely on: per-tile counts spread over the pixels, a count of 0 gives +0, the background rule, the clamped variance, one f16 conversion"""
    counts = fr.pixel_counts(40, 33, 0, [1, 2, 3, 4])
    assert counts.shape == (33, 40) and counts[0, 0] == 1 and counts[0, 32] == 2 and counts[32, 31] == 3 and counts[32, 39] == 4
    S = np.full((33, 40, 4), 6.0, np.float32)
    out = fr.features(0x201, 40, 33, S=S, tile_samples=[0, 2, 3, 4])
    assert out.shape == (4, 33, 40) and not out[:, :32, :32].any() and not np.signbit(out[:, :32, :32]).any()
    assert (out[0, 0, 32:] == 3.0).all() and (out[0, 32, :32] == 2.0).all() and (out[3, 32, 32:] == 4.0).all()
    AC = np.zeros((1, 4, 4), np.float32); ND = np.zeros((1, 4, 4), np.float32)
    AC[0, :, 3] = (0.0, 2.0, 2.0, 2.0); ND[0, :, 3] = (5.0, -1.0, np.nan, 3.0); ND[0, :, :3] = (0.0, 0.0, 4.0)
    g = fr.features(0x00C, 4, 1, AC=AC, ND=ND, samples=2, layout="hwc")
    assert not g[0, :3].any() and np.array_equal(g[0, 3], np.float32([0, 0, 1, 1.5]))
    Q = np.zeros((1, 1, 4), np.float32); S1 = np.full((1, 1, 4), 4.0, np.float32)
    assert not fr.features(0x080, 1, 1, S=S1, Q=Q, samples=2).any()              # Q < S mu: v clamped to 0
    h = fr.features(0x001, 1, 1, S=np.float32([[[65520.0, 2.0 ** -25, 1.5 * 2.0 ** -24, 0]]]), samples=1, dtype="f16")
    assert h.dtype == np.float16 and np.isinf(h[0, 0, 0]) and h[1, 0, 0] == 0 and h[2, 0, 0] == np.float16(2.0 ** -23)
    assert fr.same(np.float32([np.nan, 1]), np.float32([np.nan, 1])) and not fr.same(np.float32([0.0]), np.float32([-0.0]))


def test_the_request_arithmetic_alone_under_asan_and_ubsan(tmp_path):
    """tests/features_request_main.cpp over rf_feature_request.hpp, -fsanitize=address,undefined, run as a plain executable: exit 0 and no sanitizer report.  Nothing is
    preloaded and nothing is loaded into Python (the runtimes are linked statically, as tests/test_checkpoint_api.py explains)."""
    csrc = os.path.join(ROOT, "rayfinder_amd", "csrc")
    exe = str(tmp_path / "features_request_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I", csrc, os.path.join(ROOT, "tests", "features_request_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "1023 masks checked, 0 failures" in run.stdout, run.stdout
