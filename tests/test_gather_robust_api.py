"""The frame gather carrying the robust mean as plane 4, without a GPU: the C ABI declares RF_GATHER_ROBUST_MEAN and the two root-side calls, NULL handles are
refused before any device call, and rf_gather_plan_planes with the flag lists, for every rank of a world, the list without it plus the one-plane plan tagged
plane 4 -- receives of all planes first, then the sends in plane order -- while the lists of every older flag combination stay what they were."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import ROOT

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
WORLDS = (1, 2, 3, 4, 5, 8)
FRAMES = ((72, 40), (200, 150))
OLD_MASKS = tuple(itertools.product((False, True), repeat=2))        # (aovs, moments)


def test_the_header_declares_the_flag_and_the_two_calls():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    assert re.search(r"#define RF_GATHER_ROBUST_MEAN\s+16u", header)
    assert rf.RF_GATHER_ROBUST_MEAN == 16
    for name in ("rf_comm_read_robust_mean", "rf_comm_denoise_robust"):
        assert re.search(r"RF_API int\s+" + name + r"\(", header), name
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES, name
    assert re.search(r"rf_comm_read_robust_mean\(rf_comm\* c, rf_renderer\* r, float\* rgba, uint32_t\* bgra8, uint8_t\* trim, uint32_t\* K, uint32_t\* sample_count\)", header)
    # the older flags keep their values, and the defining property is stated
    for name, value in (("LOOPBACK", 1), ("AOVS", 2), ("MOMENTS", 4), ("TILE_COUNTS", 8)):
        assert re.search(r"#define RF_GATHER_" + name + r"\s+" + str(value) + "u", header), name
    flat = re.sub(r"[\s*]+", " ", header)
    assert "rf_comm_read_robust_mean on the root (mean, texels, trim, count) is bit for bit rf_renderer_read_robust_mean of one handle without a tile shard" in flat
    for name in ("read_robust_mean", "denoise_robust"):
        assert callable(getattr(rf.TileComm, name)), name


def test_null_handles_are_invalid_arguments_without_a_device():
    lib = rf._ffi.lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bogus = C.c_void_p(16)                       # never dereferenced: the NULL partner is found first
    buf = np.full(16, 3.0, np.float32)
    texels = np.full(4, 9, np.uint32)
    trim = np.full(4, 5, np.uint8)
    k, n = C.c_uint32(7), C.c_uint32(7)
    ptr = C.c_void_p(5)
    flag = rf.RF_GATHER_ROBUST_MEAN
    for flags in (flag, flag | rf.RF_GATHER_AOVS, flag | rf.RF_GATHER_AOVS | rf.RF_GATHER_MOMENTS | rf.RF_GATHER_TILE_COUNTS | rf.RF_GATHER_LOOPBACK):
        assert lib.rf_renderer_gather_frame(None, bogus, 0, flags, C.byref(ptr)) == INVALID
        assert lib.rf_renderer_gather_frame(bogus, None, 0, flags, C.byref(ptr)) == INVALID
    calls = [
        lambda c, r: lib.rf_comm_read_robust_mean(c, r, P(buf), P(texels), P(trim), C.byref(k), C.byref(n)),
        lambda c, r: lib.rf_comm_read_robust_mean(c, r, None, None, None, None, None),
        lambda c, r: lib.rf_comm_denoise_robust(c, r, None),
    ]
    for call in calls:
        for c, r in ((None, bogus), (bogus, None), (None, None)):
            assert call(c, r) == INVALID
            msg = lib.rf_last_error_message().decode()
            assert "null" in msg and "HIP" not in msg and "device" not in msg, msg
    assert ptr.value == 5 and (k.value, n.value) == (7, 7) and (buf == 3.0).all() and (texels == 9).all() and (trim == 5).all()
    # bad denoise parameters are refused as everywhere else, before the handles are looked at
    bad = rf._ffi.DenoiseParameters(9, 1.0, 0.1, 0.1)
    assert lib.rf_comm_denoise_robust(None, None, C.byref(bad)) == INVALID and "iterations" in lib.rf_last_error_message().decode()
    bad = rf._ffi.DenoiseParameters(5, 0.0, 0.1, 0.1)
    assert lib.rf_comm_denoise_robust(bogus, None, C.byref(bad)) == INVALID and "sigma" in lib.rf_last_error_message().decode()


@pytest.mark.parametrize("world", WORLDS)
def test_the_flag_adds_the_one_plane_plan_tagged_plane_four(world):
    for (W, H), root, loopback, (aovs, moments) in itertools.product(FRAMES, sorted({0, world - 1}), (False, True), OLD_MASKS):
        case = (W, H, world, root, loopback, aovs, moments)
        first, slot, owner = rf.gather_layout(W, H, world)
        total = int(first[world])
        for k in range(world):
            without = rf.gather_plan_planes(W, H, world, k, root, loopback, aovs, moments)
            with_flag = rf.gather_plan_planes(W, H, world, k, root, loopback, aovs, moments, robust_mean=True)
            one = rf.gather_plan(W, H, world, k, root, loopback)                                   # {is_send, peer, offset, count}
            tagged = np.insert(one, 2, 4, axis=1)                                                   # {is_send, peer, plane = 4, offset, count}
            # receives of all planes first (plane 4's behind plane 3's), then the sends in plane order (plane 4's last)
            want = np.concatenate([without[without[:, 0] == 0], tagged[tagged[:, 0] == 0], without[without[:, 0] == 1], tagged[tagged[:, 0] == 1]]).reshape(-1, 5)
            assert with_flag.dtype == without.dtype and np.array_equal(with_flag, want), (case, k)
            assert not (without[:, 2] == 4).any(), (case, k)
        # every send has its receive, per (source, destination) in the same plane order, plane 4 last
        plans = [rf.gather_plan_planes(W, H, world, k, root, loopback, aovs, moments, robust_mean=True) for k in range(world)]
        planes = [0] + ([1, 2] if aovs else []) + ([3] if moments else []) + [4]
        sends, recvs = {}, {}
        for k, plan in enumerate(plans):
            for is_send, peer, plane, offset, count in plan.tolist():
                assert count > 0
                if is_send:
                    assert peer == root and offset == 0 and count == int(first[k + 1] - first[k]), case
                    sends.setdefault((k, peer), []).append((plane, count))
                else:
                    assert k == root and offset == int(first[peer]), case
                    recvs.setdefault((peer, k), []).append((plane, count))
        assert sends == recvs, case
        for pair, ops in sends.items():
            assert [p for p, _ in ops] == planes, (case, pair)
        assert {src for src, _ in sends} == {k for k in range(world) if first[k + 1] > first[k] and (k != root or loopback)}, case
        # plane 4's receives tile its staging area exactly, without overlap (the root's own place stays free unless it loops back)
        covered = np.zeros(total, np.int32)
        for is_send, peer, plane, offset, count in plans[root].tolist():
            if not is_send and plane == 4:
                covered[offset:offset + count] += 1
        want = np.ones(total, np.int32)
        if not loopback:
            want[int(first[root]):int(first[root + 1])] = 0
        assert np.array_equal(covered, want), case


@pytest.mark.parametrize("world", WORLDS)
def test_the_lists_of_the_older_flags_are_unchanged(world):
    """Without the flag: the plain list is rf_gather_plan's with plane = 0, and a list with extra planes is that one-plane list once per carried plane of 0 .. 3 --
    receives first, then sends -- as tests/test_gather_sums_api.py computes it.  The count plan is the one-plane plan in words."""
    for (W, H), root, loopback, (aovs, moments) in itertools.product(FRAMES, sorted({0, world - 1}), (False, True), OLD_MASKS):
        planes = [0] + ([1, 2] if aovs else []) + ([3] if moments else [])
        for k in range(world):
            one = rf.gather_plan(W, H, world, k, root, loopback)
            got = rf.gather_plan_planes(W, H, world, k, root, loopback, aovs, moments)
            want = [[s, peer, p, off, cnt] for sends in (0, 1) for p in planes for s, peer, off, cnt in one.tolist() if s == sends]
            assert got.tolist() == want, (W, H, world, root, loopback, aovs, moments, k)
            assert np.array_equal(rf.gather_plan_counts(W, H, world, k, root, loopback), one)


def test_the_plan_call_counts_plane_four():
    lib = rf._ffi.lib
    n = C.c_uint32(0)
    flags = rf.RF_GATHER_AOVS | rf.RF_GATHER_MOMENTS | rf.RF_GATHER_ROBUST_MEAN
    assert lib.rf_gather_plan_planes(200, 150, 4, 0, 0, flags, None, C.byref(n)) == rf._ffi.RF_OK and n.value == 3 * 5    # the root: three receives for each of five planes
    assert lib.rf_gather_plan_planes(200, 150, 4, 1, 0, rf.RF_GATHER_ROBUST_MEAN, None, C.byref(n)) == rf._ffi.RF_OK and n.value == 2   # a sender: planes 0 and 4
