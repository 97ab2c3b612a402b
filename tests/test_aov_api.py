"""First-hit AOVs without a GPU: the C ABI entry points exist and refuse bad arguments, and the restatement the GPU tests compare
against (tests/aov_restatement.py) agrees with the product's own host query on the Duck."""
import ctypes as C

import numpy as np

import rayfinder_amd as rf
from aov_restatement import T_MAX, aov_sums, first_hit_samples, oracle_intersect
from conftest import bits, oracle_scene_from_pt
from oracle import orc


def test_aov_symbols_are_exported_and_declared():
    lib = C.CDLL(rf._ffi.LIB_PATH)
    for name in ("rf_renderer_set_aovs", "rf_renderer_read_aovs"):
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES
    assert rf._ffi.RF_AOV_FIRST_HIT == 1
    for name in ("set_aovs", "read_aovs", "aov_means"):
        assert callable(getattr(rf.ReferencePathTracer, name))


def test_null_handle_and_unknown_flags_are_invalid_arguments():
    lib = rf._ffi.lib
    n = C.c_uint32(7)
    assert lib.rf_renderer_set_aovs(None, 1) == rf._ffi.RF_ERROR_INVALID_ARGUMENT
    assert lib.rf_renderer_set_aovs(None, 0) == rf._ffi.RF_ERROR_INVALID_ARGUMENT
    assert lib.rf_renderer_read_aovs(None, None, None, C.byref(n)) == rf._ffi.RF_ERROR_INVALID_ARGUMENT
    assert n.value == 7
    # unknown flag bits are refused before the handle is used: a non-null handle that is never dereferenced
    bogus = C.c_void_p(16)
    for flags in (2, 0x80000000, 3):
        assert lib.rf_renderer_set_aovs(bogus, flags) == rf._ffi.RF_ERROR_INVALID_ARGUMENT
        assert "flag" in lib.rf_last_error_message().decode()


def _duck_rp(W, H, spp, aperture=0.0):
    cam = rf.fly_camera(W, H, aperture=aperture, focus_distance=2.0) if aperture else rf.fly_camera(W, H)
    return orc.make_render_params(W, H, rf.camera_to_array(cam), spp, 2, 0.25, rf.aligned_sky_state(rf.make_sky()))


def test_restatement_equals_the_products_host_query_plus_attribute_arithmetic(duck_pt):
    """The helper's per-sample values with the oracle's BVH walk == with the product's CPU query (rf_intersect_bvh_batch): same hits, same t, and the
    attribute arithmetic gives unit normals, texels in [0, 1] and coverage exactly where the product's query hits."""
    sc, a = oracle_scene_from_pt(duck_pt)
    W, H, spp = 64, 48, 16

    def product_intersect(scene, rays):
        return rf.intersect_bvh_batch(rays, scene.nodes, scene.positions.view(np.float32).reshape(-1, 12), T_MAX)

    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.ravel(), ys.ravel()
    for aperture in (0.0, 0.1):
        rp = _duck_rp(W, H, spp, aperture)
        hits = 0
        for f in (0, 5, 15):
            ac_o, nd_o = first_hit_samples(sc, rp, xs, ys, f, oracle_intersect)
            ac_p, nd_p = first_hit_samples(sc, rp, xs, ys, f, product_intersect)
            assert np.array_equal(bits(ac_o), bits(ac_p)) and np.array_equal(bits(nd_o), bits(nd_p)), (aperture, f)
            rays = np.stack([orc.wgsl_camera_ray(rp, int(x), int(y), f, sc.blue_noise) for x, y in zip(xs, ys)])
            h = product_intersect(sc, rays)
            hit = h["hit"] != 0
            hits += int(hit.sum())
            assert np.array_equal(ac_p[:, 3], hit.astype(np.float32))
            assert np.array_equal(bits(nd_p[hit, 3]), bits(h["t"][hit]))
            assert (ac_p[~hit] == 0).all() and (nd_p[~hit] == 0).all()
            assert ((ac_p[hit, :3] >= 0) & (ac_p[hit, :3] <= 1)).all()
            length = np.sqrt((nd_p[hit, :3].astype(np.float64) ** 2).sum(1))
            assert np.allclose(length, 1.0, atol=1e-5)
        assert hits > 0.2 * 3 * W * H                  # the duck fills a good part of the frame


def test_restatement_sums_in_frame_order():
    """aov_sums adds the per-sample values in the order of `frames`, in f32, starting from +0 (as the renderer's sums do)."""
    d = _tiny_scene()
    rp = orc.make_render_params(8, 8, rf.camera_to_array(rf.create_camera((0.0, 0.0, -3.0), (0.0, 0.0, 0.0), 0.0, 1.0, np.radians(40.0), 1.0)), 4, 1, 1.0,
                                rf.aligned_sky_state(rf.make_sky()))
    ac, nd = aov_sums(d, rp, range(4))
    ys, xs = np.mgrid[0:8, 0:8]
    want_ac = np.zeros((64, 4), np.float32)
    want_nd = np.zeros((64, 4), np.float32)
    for f in range(4):
        a, n = first_hit_samples(d, rp, xs.ravel(), ys.ravel(), f)
        want_ac, want_nd = want_ac + a, want_nd + n
    assert np.array_equal(bits(ac.reshape(-1, 4)), bits(want_ac)) and np.array_equal(bits(nd.reshape(-1, 4)), bits(want_nd))
    assert (ac[..., 3] == 4).all()                     # the quad covers the whole frame
    assert np.allclose(nd[..., :3] / 4, (0.0, 0.0, -1.0))


def _tiny_scene():
    """One big quad at z = 0 facing -z (normal (0, 0, -1)), white texture."""
    P = np.array([[-5, -5, 0, 5, -5, 0, 5, 5, 0], [-5, -5, 0, 5, 5, 0, -5, 5, 0]], np.float32)
    N = np.tile(np.array([0, 0, -1], np.float32), (2, 3))
    T = np.zeros((2, 6), np.float32)
    pt = rf.PtFormat.from_triangles(P, N, T, np.zeros(2, np.uint32), [(np.array([0xFFFFFFFF], np.uint32), 1, 1)])
    sc, _ = oracle_scene_from_pt(pt)
    return sc
