"""The BVH builders on the CPU: the host builder (rf.build_bvh) and the oracle's restatement of the reference's recursion
(orc.build_bvh) give the same node bytes and the same permutation on every soup of bvh_soups.py, and both trees pass
check_tree (bvh_invariants.py), which states what a valid tree is with no builder in it and is shown here to catch six
mutations of a good tree.  So two references agree on every input before the GPU builder is compared with them
(test_gpu_bvh_edges.py)."""
import numpy as np
import pytest

import bvh_soups as S
import rayfinder_amd as rf
from bvh_invariants import check_tree, node_ranges
from oracle import orc

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
FAMILIES = ("threshold", "unsplittable", "straddle", "partition", "signed_zero", "extent_overflow", "other_values")
# only where areas overflow may a leaf hold more than 255 splittable triangles ("no finite SAH cost -> leaf")
NONFINITE_AREA_OK = ("extent_overflow",)


def both_builders(name):
    _, tris = S.soup(name)
    hn, hi, hd = rf.build_bvh(tris)
    on, oi, od = orc.build_bvh(tris)
    assert hn.tobytes() == np.ascontiguousarray(on).tobytes(), name
    assert np.array_equal(hi, oi) and hd == od, name
    return tris, hn, hi, hd, on, oi, od


@pytest.mark.parametrize("name", [n for f in FAMILIES for n in S.names(f)])
def test_host_builder_equals_oracle_and_both_trees_are_valid(name):
    tris, hn, hi, hd, on, oi, od = both_builders(name)
    allow = name in [n for f in NONFINITE_AREA_OK for n in S.names(f)]
    check_tree(tris, hn, hi, hd, allow_nonfinite_area=allow)
    check_tree(tris, on, oi, od, allow_nonfinite_area=allow)


def test_extent_overflow_soups_reach_the_non_finite_quotients_and_terminate():
    """The inputs are what their names say (bvh_soups.py): finite vertices; an extent that is finite with 12 * (c - min)
    overflowing (q = +inf), or infinite through lo + hi (q = NaN).  The builders end (they returned) and their depth, which
    is the GPU builder's level count, is small."""
    for name in S.names("extent_overflow"):
        tris, hn, hi, hd, *_ = both_builders(name)
        assert np.isfinite(tris).all()
        t = tris.reshape(-1, 3, 3)
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.float32(0.5) * (t.min(1) + t.max(1))[:, 0]
            extent = c.max() - c.min()
            q = np.float32(12) * (c - c.min()) / extent
        if name in ("x_pm1.6e38", "x_pm4e37"):
            assert np.isfinite(extent) and np.isposinf(q).any() and not np.isnan(q).any(), name
        else:
            assert np.isinf(extent) and np.isnan(q).any(), name
        assert hd <= 64, (name, hd)


@pytest.mark.parametrize("name", S.names("scan_carry"))
def test_scan_carry_soups_host_tree_is_valid(name):
    """The two sizes past 1 024 scan blocks.  Measured on one CPU core: host builder 0.9 s and 2.5 s, oracle 0.8 s and 2.1 s
    (1 048 577 and 2 100 000 triangles), together under the 10 s the pair may cost, so the oracle is compared here, once;
    the GPU test compares with the host builder alone.  check_tree takes 1.5 s and 2.9 s on the 2.1 M and 4.2 M nodes."""
    tris, hn, hi, hd, *_ = both_builders(name)
    check_tree(tris, hn, hi, hd)


def test_partition_seeds_make_the_permutation_observable():
    """Every committed seed: enough multi-triangle leaves, and one at least whose source indices are not ascending, so a
    STABLE partition in place of libstdc++'s would change the bytes the GPU test compares."""
    for p in S.PARTITION_PATTERNS:
        for n in S.PARTITION_SIZES:
            tris = S.partition_soup(p, n, S.PARTITION_SEEDS[p, n])
            nodes, idx, _ = rf.build_bvh(tris)
            assert S.partition_ok(n, nodes, idx), (p, n, S.partition_condition(n, nodes, idx))
            # the first split is the pattern's own: cluster A on the left
            src = np.empty(n, np.int64); src[idx.astype(np.int64)] = np.arange(n)
            left = int(node_ranges(nodes)[1][1])
            assert np.all(tris[src[:left], 0] < 0) and np.all(tris[src[left:], 0] > 0), (p, n)


# ---------------------------------------------------------------------------------------------- check_tree catches
@pytest.fixture(scope="module")
def good():
    _, tris = S.soup("alternating_300")
    nodes, idx, depth = rf.build_bvh(tris)
    check_tree(tris, nodes, idx, depth)
    return tris, nodes, idx, depth


def _ulp(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


@pytest.mark.parametrize("what", ["leaf", "interior"])
@pytest.mark.parametrize("outward", [True, False])
def test_check_tree_catches_a_box_coordinate_one_ulp_off(good, what, outward):
    tris, nodes, idx, depth = good
    nodes = nodes.copy()
    i = np.nonzero((nodes["triangleCount"] > 0) if what == "leaf" else (nodes["triangleCount"] == 0))[0][3]
    nodes["max"][i, 1] = _ulp(nodes["max"][i, 1], outward)
    with pytest.raises(AssertionError):
        check_tree(tris, nodes, idx, depth)
    nodes["max"][i, 1] = good[1]["max"][i, 1]
    nodes["min"][i, 2] = _ulp(nodes["min"][i, 2], not outward)
    with pytest.raises(AssertionError):
        check_tree(tris, nodes, idx, depth)


def test_check_tree_catches_two_triangles_swapped_across_a_leaf_boundary(good):
    tris, nodes, idx, depth = good
    leaves = np.nonzero(nodes["triangleCount"] > 0)[0]
    a, b = leaves[4], leaves[5]
    pa = int(nodes["trianglesOffset"][a] + nodes["triangleCount"][a] - 1); pb = int(nodes["trianglesOffset"][b])
    idx = idx.copy()
    sa, sb = np.nonzero(idx == pa)[0][0], np.nonzero(idx == pb)[0][0]
    idx[sa], idx[sb] = pb, pa
    with pytest.raises(AssertionError):
        check_tree(tris, nodes, idx, depth)


@pytest.mark.parametrize("delta", [1, -1])
def test_check_tree_catches_a_second_child_offset_off_by_one(good, delta):
    tris, nodes, idx, depth = good
    nodes = nodes.copy()
    i = np.nonzero(nodes["triangleCount"] == 0)[0][2]
    nodes["secondChildOffset"][i] = int(nodes["secondChildOffset"][i]) + delta
    with pytest.raises(AssertionError):
        check_tree(tris, nodes, idx, depth)


def test_check_tree_catches_a_leaf_count_off_by_one_with_its_neighbour_compensated(good):
    tris, nodes, idx, depth = good
    leaves = np.nonzero(nodes["triangleCount"] > 0)[0]
    k = np.nonzero(nodes["triangleCount"][leaves[1:]] >= 2)[0][0]             # leaves[k], leaves[k + 1]: the second keeps one at least
    a, b = leaves[k], leaves[k + 1]
    nodes = nodes.copy()
    nodes["triangleCount"][a] += 1
    nodes["trianglesOffset"][b] += 1
    nodes["triangleCount"][b] -= 1
    with pytest.raises(AssertionError):
        check_tree(tris, nodes, idx, depth)


def test_check_tree_catches_a_depth_off_by_one(good):
    tris, nodes, idx, depth = good
    with pytest.raises(AssertionError):
        check_tree(tris, nodes, idx, depth + 1)


def test_check_tree_reports_a_big_leaf_of_non_finite_area_unless_told_to_expect_it():
    tris = (np.random.default_rng(12).uniform(-1, 1, (600, 9)) * 1e20).astype(np.float32)      # areas overflow: one leaf of 600
    nodes, idx, depth = rf.build_bvh(tris)
    assert len(nodes) == 1
    with pytest.raises(AssertionError, match="allow_nonfinite_area"):
        check_tree(tris, nodes, idx, depth)
    assert check_tree(tris, nodes, idx, depth, allow_nonfinite_area=True)["nonfinite_area_leaves"] == 1


def test_check_tree_is_quick_at_60k_triangles():
    import time
    tris = S.uniform(np.random.default_rng(13), 60000)
    nodes, idx, depth = rf.build_bvh(tris)
    t0 = time.perf_counter()
    check_tree(tris, nodes, idx, depth)
    assert time.perf_counter() - t0 < 1.0


# ---------------------------------------------------------------------------------------------- non-finite positions
@pytest.mark.parametrize("name", S.names("non_finite"))
def test_host_entry_points_refuse_non_finite_positions(name):
    """A NaN or infinite coordinate: rf_build_bvh and the bake refuse with RF_ERROR_INVALID_ARGUMENT and write nothing (with a
    NaN in play the boxes depend on the order of the fold, so no tree is defined; profiles/bvh_edges/README.md)."""
    _, tris = S.soup(name)
    bad = int(np.nonzero(~np.isfinite(tris).all(axis=1))[0][0])
    with pytest.raises(rf.RayfinderError) as e:
        rf.build_bvh(tris)
    assert e.value.status == INVALID and f"triangle {bad} " in str(e.value) and "non-finite" in str(e.value)
    n = len(tris)
    with pytest.raises(rf.RayfinderError) as e:
        rf.PtFormat.from_triangles(tris, np.zeros((n, 9), np.float32), np.zeros((n, 6), np.float32), np.zeros(n, np.uint32), [])
    assert e.value.status == INVALID and "non-finite" in str(e.value)
    # the GPU entry point decides the same on the host, before it looks for a device: the same refusal with or without one
    with pytest.raises(rf.RayfinderError) as e:
        rf.build_bvh_gpu(tris)
    assert e.value.status == INVALID and f"triangle {bad} " in str(e.value) and "non-finite" in str(e.value)
    # nothing written
    import ctypes as C
    nodes = np.full(2 * n, 0xAB, np.uint8).repeat(48).reshape(-1, 48); idx = np.full(n, 7, np.uint64); cnt = C.c_uint64(99); depth = C.c_int32(-5)
    rc = rf._ffi.lib.rf_build_bvh(tris.ctypes.data_as(C.c_void_p), n, nodes.ctypes.data_as(C.c_void_p), C.byref(cnt), idx.ctypes.data_as(C.c_void_p), C.byref(depth))
    assert rc == INVALID and (nodes == 0xAB).all() and (idx == 7).all() and cnt.value == 99 and depth.value == -5
    # and the finite rest of the soup builds
    ok = tris[np.isfinite(tris).all(axis=1)]
    nodes, idx, depth = rf.build_bvh(ok)
    check_tree(ok, nodes, idx, depth)
