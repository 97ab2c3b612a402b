"""rf_renderer_cast_rays without a GPU: the C ABI entry point exists and is declared, the request's host arithmetic (rf_ray_query_request.hpp) under the sanitizers as
a stand-alone program, the Python wrappers' argument checks (made before the library is called: a "meta" tensor stands in for the device checks), and the restatement
of the attribute arithmetic on its own edges."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cast_rays_restatement as cr
import rayfinder_amd as rf
from conftest import ROOT

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
lib = rf._ffi.lib


def test_the_symbol_is_exported_and_declared():
    raw = C.CDLL(rf._ffi.LIB_PATH)
    assert hasattr(raw, "rf_renderer_cast_rays") and "rf_renderer_cast_rays" in rf._ffi.SIGNATURES
    assert callable(rf.ReferencePathTracer.cast_rays) and callable(rf.ReferencePathTracer.cast_occlusion)
    # two pointers, two strides, the count, t_max, the kind, two reserved words, ten output pointers
    assert C.sizeof(rf._ffi.RayBatch) == 16 + 8 + 8 + 4 + 4 + 8 + 80
    assert rf._ffi.RayBatch.triangle.offset == 48 and rf._ffi.RayBatch.visibility.offset == 120
    with open(os.path.join(ROOT, "include", "rayfinder_amd.h")) as f:
        header = f.read()
    assert "#define RF_RAYS_CLOSEST 0u" in header and "#define RF_RAYS_ANY     1u" in header
    assert "RF_API int rf_renderer_cast_rays(rf_renderer* r, const rf_ray_batch* batch);" in header
    struct = header[header.index("typedef struct rf_ray_batch"):header.index("} rf_ray_batch;")]
    order = [struct.index(" " + name + ";") for name, _, _, _ in rf._ffi.RAY_OUTPUTS]
    assert order == sorted(order), "the header's outputs are not in RAY_OUTPUTS' order"
    assert "cast_chunk" in header


def test_null_arguments_are_refused_before_the_handle_is_touched():
    bogus = C.c_void_p(16)   # never dereferenced: the NULLs are checked first
    batch = rf._ffi.RayBatch()
    assert lib.rf_renderer_cast_rays(None, C.byref(batch)) == INVALID
    assert lib.rf_renderer_cast_rays(bogus, None) == INVALID
    assert lib.rf_renderer_cast_rays(None, None) == INVALID


def test_the_request_arithmetic_alone_under_asan_and_ubsan(tmp_path):
    """tests/ray_query_request_main.cpp over rf_ray_query_request.hpp, -fsanitize=address,undefined, run as a plain executable: exit 0 and no sanitizer report.  Nothing
    is preloaded and nothing is loaded into Python (the runtimes are linked statically, as tests/test_features_api.py does)."""
    csrc = os.path.join(ROOT, "rayfinder_amd", "csrc")
    exe = str(tmp_path / "ray_query_request_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I", csrc, os.path.join(ROOT, "tests", "ray_query_request_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert " checks, 0 failures" in run.stdout and not run.stdout.startswith("0 checks"), run.stdout


def test_python_wrappers_check_their_arguments():
    import torch
    meta = dict(device="meta")       # a tensor without storage: layouts are checked before devices, so it reaches every layout check without a GPU
    good = torch.zeros((5, 3), **meta)
    ray, out, batch, device = rf._ray_tensor, rf._ray_output, rf._ray_batch, rf._ray_device
    # an input: type, dtype, shape, strides
    with pytest.raises(TypeError):
        ray("t", "origins", np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match="float32"):
        ray("t", "origins", torch.zeros((5, 3), dtype=torch.float64, **meta))
    for shape in ((5,), (5, 4), (5, 3, 1), (3, 5)):
        with pytest.raises(ValueError, match="shape"):
            ray("t", "origins", torch.zeros(shape, **meta))
    with pytest.raises(ValueError, match="strides"):
        ray("t", "origins", torch.zeros((3, 5), **meta).t())                # columns, not rows
    with pytest.raises(ValueError, match="strides"):
        ray("t", "origins", torch.zeros((5, 6), **meta)[:, ::2])            # every second float
    with pytest.raises(ValueError, match="strides"):
        ray("t", "origins", torch.zeros((1, 3), **meta).expand(5, 3))       # row stride 0
    assert ray("t", "origins", good) == 3
    assert ray("t", "origins", torch.zeros((5, 6), **meta)[:, 3:]) == 6     # half of an (N, 6) tensor
    assert ray("t", "origins", torch.zeros((5, 8), **meta)[:, :3]) == 8     # rows with padding
    assert ray("t", "origins", torch.zeros((1, 3), **meta)) == 3 and ray("t", "origins", torch.zeros((0, 3), **meta)) == 3
    # its device
    with pytest.raises(ValueError, match="lies on cpu"):
        device("t", "origins", torch.zeros((5, 3)), 0)
    with pytest.raises(ValueError, match="lies on meta"):
        device("t", "origins", good, 0)
    # an output
    with pytest.raises(TypeError):
        out("t", "t", np.zeros(5, np.float32), 5)
    with pytest.raises(ValueError, match="torch.float32"):
        out("t", "t", torch.zeros(5, dtype=torch.float16, **meta), 5)
    with pytest.raises(ValueError, match="torch.int32"):
        out("t", "triangle", torch.zeros(5, **meta), 5)
    with pytest.raises(ValueError, match="shape"):
        out("t", "position", torch.zeros((5, 2), **meta), 5)
    with pytest.raises(ValueError, match="shape"):
        out("t", "t", torch.zeros((5, 1), **meta), 5)
    with pytest.raises(ValueError, match="contiguous"):
        out("t", "bary", torch.zeros((5, 4), **meta)[:, :2], 5)
    assert out("t", "albedo", None, 5) == (torch.float32, (5, 3)) and out("t", "texture", None, 5) == (torch.int32, (5,))
    assert out("t", "normal", torch.zeros((9, 3), **meta)[2:7], 5) == (torch.float32, (5, 3))      # a storage offset is fine
    # the call: names, counts, t_max, out -- and only then the devices
    o, d = good, torch.zeros((5, 3), **meta)
    CLOSEST, ANY = rf._ffi.RF_RAYS_CLOSEST, rf._ffi.RF_RAYS_ANY
    for names in ((), ("colour",), ("t", "t"), ("visibility",), "normals"):
        with pytest.raises(ValueError, match="outputs"):
            batch("t", o, d, 1.0, CLOSEST, names, None, 0)
    with pytest.raises(ValueError, match="outputs"):
        batch("t", o, d, 1.0, ANY, ("t",), None, 0)
    with pytest.raises(ValueError, match="5 origins, 4 directions"):
        batch("t", o, torch.zeros((4, 3), **meta), 1.0, CLOSEST, ("t",), None, 0)
    with pytest.raises(ValueError, match="NaN"):
        batch("t", o, d, float("nan"), CLOSEST, ("t",), None, 0)
    with pytest.raises(TypeError, match="dict"):
        batch("t", o, d, 1.0, CLOSEST, ("t",), [torch.zeros(5)], 0)
    with pytest.raises(ValueError, match="does not ask for"):
        batch("t", o, d, 1.0, CLOSEST, ("t",), {"bary": torch.zeros((5, 2), **meta)}, 0)
    with pytest.raises(ValueError, match="shape"):
        batch("t", o, d, 1.0, CLOSEST, ("t",), {"t": torch.zeros(6, **meta)}, 0)
    with pytest.raises(ValueError, match="origins lies on meta"):
        batch("t", o, d, 1.0, CLOSEST, ("t",), {"t": torch.zeros(5, **meta)}, 0)
    # the wrappers themselves refuse before the handle is used: an object without a handle is enough
    r = object.__new__(rf.ReferencePathTracer)
    r._h, r._device_ordinal = None, 0
    with pytest.raises(TypeError):
        r.cast_rays([[0, 0, 0]], [[0, 0, 1]])
    with pytest.raises(ValueError, match="lies on cpu"):
        r.cast_rays(torch.zeros((2, 3)), torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="outputs"):
        r.cast_rays(torch.zeros((2, 3)), torch.zeros((2, 3)), outputs=("depth",))
    with pytest.raises(ValueError, match="lies on cpu"):
        r.cast_occlusion(torch.zeros((2, 3)), torch.zeros((2, 3)))
    with pytest.raises(TypeError, match="torch.Tensor"):
        r.cast_occlusion(torch.zeros((2, 3)), torch.zeros((2, 3)), out={"visibility": None})


def test_the_restatement_on_its_own_edges():
    F = np.float32
    pos = np.zeros((4, 12), F)
    att = np.zeros((4, 20), F)
    # 0: a unit right triangle in the plane z = 1, normals along +z with different lengths, uvs outside [0, 1)
    pos[0, 0:3], pos[0, 4:7], pos[0, 8:11] = (0, 0, 1), (1, 0, 1), (0, 1, 1)
    att[0, 0:3], att[0, 4:7], att[0, 8:11] = (0, 0, 1), (0, 0, 2), (0, 0, 4)
    att[0, 12:18] = (-1.5, 2.25, 3.0, -0.5, 0.25, 7.0)
    att[0].view(np.uint32)[18] = 0
    # 1: a degenerate triangle (three points on a line): the cross product is 0, 1 / sqrt(0) = inf, 0 * inf = NaN
    pos[1, 0:3], pos[1, 4:7], pos[1, 8:11] = (0, 0, 0), (1, 1, 1), (2, 2, 2)
    att[1, 0:3] = att[1, 4:7] = att[1, 8:11] = (1, 0, 0)
    # 2: normals that cancel: n0 = -n1, n2 = 0 -> a zero sum at u = 0.5, v = 0
    pos[2] = pos[0]
    att[2, 0:3], att[2, 4:7] = (0, 1, 0), (0, -1, 0)
    # 3: a normal sum that overflows: dot(n, n) is not finite
    pos[3] = pos[0]
    att[3, 0:3] = att[3, 4:7] = att[3, 8:11] = (3e38, 3e38, 0)
    seen = []

    def lookup(i, u, v):
        seen.append((i, F(u), F(v)))
        return F([u, v, i])

    tri = np.array([0, 0, 0, 1, 2, 3, 0xFFFFFFFF], np.uint32)
    u = F([0.25, 1.0, 0.75, 0.25, 0.5, 0.25, 0.9])
    v = F([0.5, 0.0, 0.25, 0.25, 0.0, 0.25, 0.9])
    a = cr.attributes(pos, att, tri, u, v, lookup)
    assert set(a) == set(cr.NAMES) and all(a[k].dtype == (np.uint32 if k == "texture" else F) for k in a)
    # ray 0: b0 = 0.25: n = (0.25 * 1 + 0.25 * 2) + 0.5 * 4 = 2.75 along z -> unit; uv in the stated order, not wrapped
    assert np.array_equal(a["geometric_normal"][0], F([0, 0, 1])) and np.array_equal(a["normal"][0], F([0, 0, 1]))
    assert np.array_equal(a["texcoord"][0], F([(F(0.25) * F(-1.5) + F(0.25) * F(3.0)) + F(0.5) * F(0.25), (F(0.25) * F(2.25) + F(0.25) * F(-0.5)) + F(0.5) * F(7.0)]))
    assert a["texcoord"][0, 1] > 1 and np.array_equal(a["albedo"][0], F([a["texcoord"][0, 0], a["texcoord"][0, 1], 0]))
    # u + v == 1 (rays 1 and 2): b0 is exactly 0, the first vertex drops out with a +0 product
    assert np.array_equal(a["texcoord"][1], F([3.0, -0.5])) and np.array_equal(a["normal"][1], F([0, 0, 1]))
    assert np.array_equal(a["texcoord"][2], F([(F(0) * F(-1.5) + F(0.75) * F(3.0)) + F(0.25) * F(0.25), (F(0) * F(2.25) + F(0.75) * F(-0.5)) + F(0.25) * F(7.0)]))
    # the degenerate triangle: a NaN geometric normal, the shading normal still interpolated
    assert np.isnan(a["geometric_normal"][3]).all() and np.array_equal(a["normal"][3], F([1, 0, 0]))
    # a zero normal sum and a sum whose square overflows: (0, 0, 0), +0
    for k in (4, 5):
        assert not a["normal"][k].any() and not np.signbit(a["normal"][k]).any()
    # a miss: every float +0, the index all ones; the look-up is asked for hits only, with the unwrapped coordinates
    assert all(not a[k][6].any() and not np.signbit(a[k][6]).any() for k in ("geometric_normal", "normal", "texcoord", "albedo")) and a["texture"][6] == 0xFFFFFFFF
    assert len(seen) == 6 and seen[0] == (0, a["texcoord"][0, 0], a["texcoord"][0, 1])
    assert "albedo" not in cr.attributes(pos, att, tri, u, v)
    # the comparison: NaNs as NaNs, zeros by sign, words as words
    assert cr.same(F([np.nan, 1]), F([np.nan, 1])) and not cr.same(F([0.0]), F([-0.0])) and not cr.same(F([1, 2]), F([1, 2, 3]))
    assert cr.same(np.uint32([0xFFFFFFFF]), np.int32([-1])) and not cr.same(np.uint32([1]), np.uint32([2]))
    assert cr.first_difference(F([[1, 2], [3, 4]]), F([[1, 2], [3, 5]])).startswith("row 1")
