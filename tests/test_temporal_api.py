"""The temporal history without a GPU: the declarations of the seven entry points, temporal_defaults(), the C ABI's argument checks that are made before any device
call -- rf_temporal_images' own, and the order "NULL handle, then bad parameters" of the handle's calls -- and the Python layer's own checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rayfinder_amd as rf
import temporal_charts as tc
from conftest import ROOT

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
PROTOTYPES = {
    "rf_temporal_default_parameters": "rf_temporal_parameters* params",
    "rf_renderer_temporal_accumulate": "rf_renderer* r, const rf_temporal_parameters* params",
    "rf_renderer_temporal_commit": "rf_renderer* r",
    "rf_renderer_temporal_reset": "rf_renderer* r",
    "rf_renderer_read_temporal": "rf_renderer* r, float* rgba, uint32_t* bgra8, float* geometry, uint32_t* sample_count",
    "rf_renderer_denoise_temporal": "rf_renderer* r, const rf_temporal_parameters* tparams, const rf_denoise_parameters* dparams",
    "rf_temporal_images": "int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* albedo_coverage4, "
                          "const float* normal_depth4, const rf_camera* camera, const float* history_color4, const float* history_geometry4, "
                          "const rf_camera* history_camera, const rf_temporal_parameters* params, float exposure, float* out_color4, float* out_geometry4, "
                          "uint32_t* out_bgra8",
}
CTYPE = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def test_the_entry_points_are_declared_exported_and_bound_with_the_headers_signatures():
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
    for name in ("temporal_accumulate", "temporal_commit", "temporal_reset", "read_temporal", "denoise_temporal"):
        assert callable(getattr(rf.ReferencePathTracer, name)), name
    assert callable(rf.temporal_images) and callable(rf.temporal_defaults)
    assert C.sizeof(rf._ffi.TemporalParameters) == 16


def test_the_defaults_are_the_headers_and_the_restatements():
    import temporal_restatement as tr
    d = rf.temporal_defaults()
    assert d == dict(max_history=64.0, depth_tolerance=np.float32(0.05), min_normal_dot=np.float32(0.9)) and set(d) == set(tr.DEFAULTS)
    assert all(np.float32(d[k]) == np.float32(tr.DEFAULTS[k]) for k in d)
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    assert "rf_temporal_default_parameters: max_history = 64, depth_tolerance = 0.05, min_normal_dot = 0.9" in header
    lib = rf._ffi.lib
    assert lib.rf_temporal_default_parameters(None) == INVALID and "null" in lib.rf_last_error_message().decode()


BAD_PARAMETERS = [((0.0, 0.05, 0.9, 0), "max_history"), ((-1.0, 0.05, 0.9, 0), "max_history"), ((np.inf, 0.05, 0.9, 0), "max_history"), ((np.nan, 0.05, 0.9, 0), "max_history"),
                  ((64.0, 0.0, 0.9, 0), "depth_tolerance"), ((64.0, -0.1, 0.9, 0), "depth_tolerance"), ((64.0, np.inf, 0.9, 0), "depth_tolerance"),
                  ((64.0, np.nan, 0.9, 0), "depth_tolerance"), ((64.0, 0.05, 1.5, 0), "min_normal_dot"), ((64.0, 0.05, -1.5, 0), "min_normal_dot"),
                  ((64.0, 0.05, np.nan, 0), "min_normal_dot"), ((64.0, 0.05, 0.9, 1), "reserved")]


def test_temporal_images_refuses_bad_arguments_before_any_device_call():
    lib = rf._ffi.lib
    chart = tc.finite_charts()["identical cameras"]
    S, AC, ND = (np.ascontiguousarray(a) for a in (chart.S, chart.AC, chart.ND))
    hc, hg = np.ascontiguousarray(chart.history["color"]), np.ascontiguousarray(chart.history["geometry"])
    cam, old = rf.camera_from_array(chart.camera), rf.camera_from_array(chart.history["camera"])
    out = np.full((tc.H, tc.W, 4), 3.0, np.float32)

    def call(w=tc.W, h=tc.H, n=tc.N, s=P(S), ac=P(AC), nd=P(ND), c=C.byref(cam), tcol=P(hc), tgeo=P(hg), tcam=C.byref(old), params=None, exposure=1.0):
        # device ordinal 1 << 20: were a device call made, the status would be NO_DEVICE (no GPU) or "ordinal out of range", never these messages
        return lib.rf_temporal_images(1 << 20, w, h, n, s, ac, nd, c, tcol, tgeo, tcam, params, exposure, P(out), None, None)

    cases = [dict(s=None), dict(ac=None), dict(nd=None), dict(c=None), dict(w=0), dict(h=0), dict(n=0), dict(w=1 << 16, h=1 << 15), dict(exposure=float("nan")),
             dict(tcol=None), dict(tgeo=None), dict(tcam=None), dict(tcol=None, tgeo=None), dict(tgeo=None, tcam=None)]
    for kw in cases:
        assert call(**kw) == INVALID, kw
        msg = lib.rf_last_error_message().decode()
        assert "ordinal" not in msg and "HIP" not in msg and "device" not in msg, (kw, msg)
        if any(k in kw for k in ("tcol", "tgeo", "tcam")):
            assert "history" in msg, msg
    for values, word in BAD_PARAMETERS:
        bad = rf._ffi.TemporalParameters(*values)
        assert call(params=C.byref(bad)) == INVALID and word in lib.rf_last_error_message().decode(), (values, lib.rf_last_error_message().decode())
    assert (out == 3.0).all()
    # with everything in order the call goes on to the device: on a machine without one that is where it ends, with another status
    if not _have_gpu():
        assert call() not in (rf._ffi.RF_OK, INVALID) or "ordinal" in lib.rf_last_error_message().decode()
        assert call(tcol=None, tgeo=None, tcam=None) not in (rf._ffi.RF_OK, INVALID) or "ordinal" in lib.rf_last_error_message().decode()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_a_null_handle_comes_before_bad_parameters_and_the_parameters_before_the_handles_state():
    lib = rf._ffi.lib
    bad = rf._ffi.TemporalParameters(0.0, 0.05, 0.9, 0)
    n = C.c_uint32(7)
    for status in (lib.rf_renderer_temporal_accumulate(None, None), lib.rf_renderer_temporal_accumulate(None, C.byref(bad)), lib.rf_renderer_temporal_commit(None),
                   lib.rf_renderer_temporal_reset(None), lib.rf_renderer_read_temporal(None, None, None, None, C.byref(n)),
                   lib.rf_renderer_denoise_temporal(None, C.byref(bad), None)):
        assert status == INVALID and "null" in lib.rf_last_error_message().decode()
    assert n.value == 7


def test_the_python_layer_refuses_unknown_parameters_and_mismatched_planes():
    chart = tc.finite_charts()["identical cameras"]
    with pytest.raises(TypeError, match="unknown temporal parameters"):
        rf.temporal_images(chart.S, chart.AC, chart.ND, tc.N, chart.camera, max_histroy=3)
    with pytest.raises(ValueError, match="one size"):
        rf.temporal_images(chart.S, chart.AC[:-1], chart.ND, tc.N, chart.camera)
    with pytest.raises(ValueError, match="one size"):
        rf.temporal_images(chart.S, chart.AC, chart.ND, tc.N, chart.camera, history=dict(color=chart.history["color"][:, :-1], geometry=chart.history["geometry"],
                                                                                         camera=chart.history["camera"]))
