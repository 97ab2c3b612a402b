"""The frame gather with the direct sums (RF_GATHER_DIRECT, plane 5), without a GPU: the C ABI declares the flag and the two root-side calls, NULL handles are refused
before any device call, the plan of every rank of a world with the flag is the plan without it followed by the one-plane plan tagged plane 5 (pure host arithmetic:
rf_gather_plan_planes), and the NumPy restatement of rf_comm_read_split (tests/split_mean_restatement.py) gives the values worked out by hand."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import ROOT, bits
from split_mean_restatement import pixel_counts, read_split

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
WORLDS = (1, 2, 3, 4, 8)
FRAMES = ((200, 150), (72, 40))
NEW_CALLS = ("rf_comm_denoise_split", "rf_comm_read_split")


def test_the_header_the_library_and_the_package_export_the_flag_and_the_calls():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    for name in NEW_CALLS:
        assert re.search(r"RF_API int\s+" + name + r"\(", header), name
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES, name
    assert re.search(r"#define RF_GATHER_DIRECT\s+32u", header)
    assert rf.RF_GATHER_DIRECT == 32
    assert len({rf.RF_GATHER_LOOPBACK, rf.RF_GATHER_AOVS, rf.RF_GATHER_MOMENTS, rf.RF_GATHER_TILE_COUNTS, rf.RF_GATHER_ROBUST_MEAN, rf.RF_GATHER_DIRECT}) == 6
    for name in ("denoise_split", "read_split", "read_plane"):
        assert callable(getattr(rf.TileComm, name)), name
    # the older flags keep their values and the keyword comes last: positional callers keep working
    assert rf._gather_flags(True, True, True, True, True) == 31 and rf._gather_flags(direct=True) == 32
    assert np.array_equal(rf.gather_plan_planes(200, 150, 4, 1, 0, False, True, True, True), rf.gather_plan_planes(200, 150, 4, 1, 0, False, True, True, True, False))


def test_null_handles_are_invalid_arguments_without_a_device():
    lib = rf._ffi.lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bogus = C.c_void_p(16)                       # never dereferenced: the NULL partner is found first
    a, b = np.full(16, 3.0, np.float32), np.full(16, 4.0, np.float32)
    ptr = C.c_void_p(5)
    for flags in (rf.RF_GATHER_DIRECT, rf.RF_GATHER_DIRECT | rf.RF_GATHER_AOVS | rf.RF_GATHER_TILE_COUNTS | rf.RF_GATHER_LOOPBACK):
        assert lib.rf_renderer_gather_frame(None, bogus, 0, flags, C.byref(ptr)) == INVALID
        assert lib.rf_renderer_gather_frame(bogus, None, 0, flags, C.byref(ptr)) == INVALID
    calls = [
        lambda c, r: lib.rf_comm_denoise_split(c, r, None, None),
        lambda c, r: lib.rf_comm_read_split(c, r, P(a), P(b)),
        lambda c, r: lib.rf_comm_read_split(c, r, P(a), None),
        lambda c, r: lib.rf_comm_read_split(c, r, None, P(b)),
        lambda c, r: lib.rf_comm_read_plane(c, r, 5, P(a)),
    ]
    for call in calls:
        for c, r in ((None, bogus), (bogus, None), (None, None)):
            assert call(c, r) == INVALID
            msg = lib.rf_last_error_message().decode()
            assert "null" in msg and "HIP" not in msg and "device" not in msg, msg
    assert lib.rf_comm_plane_device(None, 5, C.byref(ptr)) == INVALID
    # both outputs NULL: nothing to write, refused before the handles are used
    assert lib.rf_comm_read_split(bogus, bogus, None, None) == INVALID and "null" in lib.rf_last_error_message().decode()
    assert ptr.value == 5 and (a == 3.0).all() and (b == 4.0).all()
    # bad parameters of either component are refused as everywhere else, before the handles are looked at
    good, bad = rf._ffi.DenoiseParameters(2, 1.0, 0.1, 0.1), rf._ffi.DenoiseParameters(9, 1.0, 0.1, 0.1)
    assert lib.rf_comm_denoise_split(None, None, C.byref(bad), C.byref(good)) == INVALID and "iterations" in lib.rf_last_error_message().decode()
    bad = rf._ffi.DenoiseParameters(5, 1.0, float("nan"), 0.1)
    assert lib.rf_comm_denoise_split(bogus, None, C.byref(good), C.byref(bad)) == INVALID and "sigma" in lib.rf_last_error_message().decode()


def _one_plane_tagged(W, H, world, rank, root, loopback, plane):
    one = rf.gather_plan(W, H, world, rank, root, loopback)
    return np.column_stack([one[:, 0], one[:, 1], np.full(len(one), plane, np.uint32), one[:, 2], one[:, 3]]).astype(np.uint32).reshape(-1, 5)


@pytest.mark.parametrize("world", WORLDS)
def test_the_plan_with_the_flag_is_the_plan_without_it_followed_by_plane_five(world):
    others = [dict(), dict(aovs=True), dict(moments=True), dict(robust_mean=True), dict(aovs=True, moments=True, robust_mean=True)]
    for (W, H), root, loopback, other in itertools.product(FRAMES, sorted({0, world - 1}), (False, True), others):
        case = (W, H, world, root, loopback, other)
        first, _, _ = rf.gather_layout(W, H, world)
        plans = []
        for rank in range(world):
            without = rf.gather_plan_planes(W, H, world, rank, root, loopback, **other)
            plan = rf.gather_plan_planes(W, H, world, rank, root, loopback, direct=True, **other)
            assert not (without[:, 2] == 5).any(), case
            assert np.array_equal(plan, np.concatenate([without, _one_plane_tagged(W, H, world, rank, root, loopback, 5)])), (case, rank)
            plans.append(plan)
        # sends and receives pair up across the world: the same planes with the same tile counts, in the same order on both sides of every (source, destination)
        sends, recvs = {}, {}
        for rank, plan in enumerate(plans):
            for is_send, peer, plane, offset, count in plan.tolist():
                assert count > 0, case
                if is_send:
                    assert peer == root and offset == 0 and count == int(first[rank + 1] - first[rank]), case
                    sends.setdefault((rank, peer), []).append((plane, count))
                else:
                    assert rank == root and offset == int(first[peer]), case
                    recvs.setdefault((peer, rank), []).append((plane, count))
        assert sends == recvs, case
        want = [0] + ([1, 2] if other.get("aovs") else []) + ([3] if other.get("moments") else []) + ([4] if other.get("robust_mean") else []) + [5]
        for pair, ops in sends.items():
            assert [p for p, _ in ops] == want, (case, pair)                  # plane 5 behind plane 4, behind everything
        assert {src for src, _ in sends} == {k for k in range(world) if first[k + 1] > first[k] and (k != root or loopback)}, case
        # plane 5's receives tile its staging area exactly (the root's own place stays free unless it loops back)
        covered = np.zeros(int(first[world]), np.int32)
        for is_send, peer, plane, offset, count in plans[root].tolist():
            if not is_send and plane == 5:
                covered[offset:offset + count] += 1
        free = np.ones_like(covered)
        if not loopback:
            free[int(first[root]):int(first[root + 1])] = 0
        assert np.array_equal(covered, free), case


def test_the_raw_plan_call_counts_six_planes_on_the_root_and_two_on_a_sender():
    lib = rf._ffi.lib
    n = C.c_uint32(0)
    assert lib.rf_gather_plan_planes(200, 150, 4, 0, 0, 2 | 4 | 16 | 32, None, C.byref(n)) == rf._ffi.RF_OK and n.value == 3 * 6   # three receives for each of six planes
    assert lib.rf_gather_plan_planes(200, 150, 4, 1, 0, 32, None, C.byref(n)) == rf._ffi.RF_OK and n.value == 2                    # rank 1 sends S and D
    ops = np.zeros((2, 5), np.uint32)
    assert lib.rf_gather_plan_planes(200, 150, 4, 1, 0, 32, ops.ctypes.data_as(C.c_void_p), C.byref(n)) == rf._ffi.RF_OK
    assert ops[:, 0].tolist() == [1, 1] and ops[:, 1].tolist() == [0, 0] and ops[:, 2].tolist() == [0, 5] and ops[0, 3:].tolist() == ops[1, 3:].tolist()
    small = np.zeros((1, 5), np.uint32)
    n = C.c_uint32(1)
    assert lib.rf_gather_plan_planes(200, 150, 4, 1, 0, 32, small.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID and not small.any()


def test_the_restatement_of_read_split_on_hand_made_sums():
    # 40 x 33: 2 x 2 tiles, ragged right (8 columns) and bottom (1 row); counts 4, 0, 3, 1
    W, H = 40, 33
    counts = np.array([[4, 0], [3, 1]], np.uint32)
    n = pixel_counts(counts, W, H)
    assert n.shape == (H, W) and n[0, 0] == 4 and n[0, 31] == 4 and n[0, 32] == 0 and n[31, 39] == 0 and n[32, 0] == 3 and n[32, 31] == 3 and n[32, 32] == 1
    assert (pixel_counts(7, W, H) == 7).all()
    S, D = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    S[..., :3], D[..., :3] = (8.0, 2.0, 1.0), (6.0, 3.0, 1.0)
    S[..., 3], D[..., 3] = 123.0, 0.0                                          # the sums' fourth float is not read
    S[32, 5, :3], D[32, 5, :3] = (1.0, 0.1, np.float32(1e30)), (np.float32(1.0) / np.float32(3.0), 0.3, np.float32(-1e30))
    direct, indirect = read_split(S, D, counts)
    assert direct.dtype == indirect.dtype == np.float32 and direct.shape == indirect.shape == (H, W, 4)
    assert (direct[..., 3] == 1.0).all() and (indirect[..., 3] == 1.0).all()
    assert direct[0, 0, :3].tolist() == [1.5, 0.75, 0.25] and indirect[0, 0, :3].tolist() == [0.5, -0.25, 0.0]        # count 4; indirect light may be negative
    assert direct[0, 32, :3].tolist() == [0.0, 0.0, 0.0] and indirect[5, 39, :3].tolist() == [0.0, 0.0, 0.0]           # a tile without a sample
    assert direct[32, 0, :3].tolist() == [2.0, 1.0, np.float32(1.0) / np.float32(3.0)]                                  # count 3
    assert indirect[32, 0, :3].tolist() == [np.float32(2.0) / np.float32(3.0), np.float32(-1.0) / np.float32(3.0), 0.0]
    assert direct[32, 39, :3].tolist() == [6.0, 3.0, 1.0] and indirect[32, 39, :3].tolist() == [2.0, -1.0, 0.0]         # count 1
    # the subtraction is an f32 operation of its own, before the division: 0.1f - 0.3f is rounded, then divided by 3; 1e30 - -1e30 stays finite, and so does its third
    third = np.float32(1.0) / np.float32(3.0)
    want = [(np.float32(1.0) - third) / np.float32(3.0), (np.float32(0.1) - np.float32(0.3)) / np.float32(3.0), (np.float32(1e30) - np.float32(-1e30)) / np.float32(3.0)]
    assert np.array_equal(bits(indirect[32, 5, :3]), bits(np.array(want, np.float32))) and np.isfinite(indirect[32, 5, :3]).all()
    assert np.array_equal(bits(direct[32, 5, :3]), bits(np.array([third / np.float32(3.0), np.float32(0.3) / np.float32(3.0), np.float32(-1e30) / np.float32(3.0)], np.float32)))
    # one count for the frame; D == S leaves an indirect component of exactly +0
    direct, indirect = read_split(S, S, 4)
    assert np.array_equal(bits(direct[..., :3]), bits(S[..., :3] / np.float32(4.0))) and not bits(indirect[..., :3]).any()
    direct, indirect = read_split(S, D, 0)
    assert not direct[..., :3].any() and not indirect[..., :3].any() and (direct[..., 3] == 1.0).all()
