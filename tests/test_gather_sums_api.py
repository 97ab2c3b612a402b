"""The frame gather with the AOV and moment sums, without a GPU: the C ABI declares the two flags, the plan call and the six root-side calls, the multi-plane plan
of every rank of a world is consistent (pure host arithmetic: rf_gather_plan_planes), and NULL handles are refused before any device call."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import ROOT

ROOT_SIDE_CALLS = ("rf_comm_gathered_planes", "rf_comm_read_plane", "rf_comm_plane_device", "rf_comm_denoise", "rf_comm_read_denoised", "rf_comm_noise_estimate")
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
WORLDS = (1, 2, 3, 4, 8)
FRAMES = ((200, 150), (333, 217))
MASKS = tuple(itertools.product((False, True), repeat=2))        # (aovs, moments)


def test_the_header_declares_the_calls_the_flags_and_the_plan():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    lib = C.CDLL(rf._ffi.LIB_PATH)
    for name in ROOT_SIDE_CALLS + ("rf_gather_plan_planes",):
        assert re.search(r"RF_API int\s+" + name + r"\(", header), name
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES, name
    assert re.search(r"#define RF_GATHER_AOVS\s+2u", header) and re.search(r"#define RF_GATHER_MOMENTS\s+4u", header)
    assert re.search(r"#define RF_GATHER_LOOPBACK\s+1u", header)
    assert (rf.RF_GATHER_LOOPBACK, rf.RF_GATHER_AOVS, rf.RF_GATHER_MOMENTS) == (1, 2, 4)
    assert re.search(r"typedef struct rf_gather_plane_op\s*\{\s*uint32_t is_send, peer, plane, offset_tiles, count_tiles;", header)
    assert "typedef struct rf_gather_op" in header and re.search(r"RF_API int rf_gather_plan\(", header)          # the one-plane call stays
    for name in ("gathered_planes", "read_plane", "denoise", "read_denoised", "noise_estimate"):
        assert callable(getattr(rf.TileComm, name)), name


def _planes_of(aovs, moments):
    return [0] + ([1, 2] if aovs else []) + ([3] if moments else [])


@pytest.mark.parametrize("world", WORLDS)
def test_every_rank_s_plane_plan_is_consistent(world):
    for (W, H), root, loopback, (aovs, moments) in itertools.product(FRAMES, sorted({0, world - 1}), (False, True), MASKS):
        first, slot, owner = rf.gather_layout(W, H, world)
        total = int(first[world])
        planes = _planes_of(aovs, moments)
        plans = [rf.gather_plan_planes(W, H, world, k, root, loopback, aovs, moments) for k in range(world)]
        case = (W, H, world, root, loopback, aovs, moments)
        # with no extra plane the list is rf_gather_plan's, plane = 0
        if not aovs and not moments:
            for k in range(world):
                old = rf.gather_plan(W, H, world, k, root, loopback)
                assert np.array_equal(plans[k][:, [0, 1, 3, 4]], old) and not plans[k][:, 2].any(), case
        sends = {}      # (source, destination) -> [(plane, count)] in posting order
        recvs = {}
        for k, plan in enumerate(plans):
            assert set(plan[:, 2].tolist()) <= set(planes), case
            for is_send, peer, plane, offset, count in plan.tolist():
                assert count > 0
                if is_send:
                    assert peer == root and offset == 0 and count == int(first[k + 1] - first[k]), case      # a rank sends its whole shard of that plane
                    sends.setdefault((k, peer), []).append((plane, count))
                else:
                    assert k == root, case                                                                  # only the root receives
                    assert offset == int(first[peer]), case                                                 # ... at the sender's place of THAT plane's area
                    recvs.setdefault((peer, k), []).append((plane, count))
        # every send has exactly one receive of the same plane and tile count; per (source, destination) both sides list the planes in the same order
        assert sends == recvs, case
        for pair, ops in sends.items():
            assert [p for p, _ in ops] == planes, (case, pair)
        # who takes part: every rank that owns a tile, the root only in loop-back
        senders = {k for k in range(world) if first[k + 1] > first[k] and (k != root or loopback)}
        assert {src for src, _ in sends} == senders, case
        # each plane's receives tile its staging area exactly, without overlap (the root's own place stays free unless it loops back)
        root_plan = plans[root]
        for plane in planes:
            covered = np.zeros(total, np.int32)
            for is_send, peer, p, offset, count in root_plan.tolist():
                if not is_send and p == plane:
                    covered[offset:offset + count] += 1
            want = np.ones(total, np.int32)
            if not loopback:
                want[int(first[root]):int(first[root + 1])] = 0
            assert np.array_equal(covered, want), (case, plane)
        # on the root: for each plane in order, the receives of that plane in rank order; then its sends in plane order
        order = [(int(s), int(p), int(peer)) for s, peer, p, _, _ in root_plan]
        assert order == sorted(order), case


def test_the_plan_call_refuses_bad_arguments_and_answers_a_count_query():
    lib = rf._ffi.lib
    n = C.c_uint32(0)
    assert lib.rf_gather_plan_planes(200, 150, 4, 0, 0, 6, None, None) == INVALID
    assert lib.rf_gather_plan_planes(0, 150, 4, 0, 0, 6, None, C.byref(n)) == INVALID
    assert lib.rf_gather_plan_planes(200, 150, 4, 4, 0, 6, None, C.byref(n)) == INVALID
    assert lib.rf_gather_plan_planes(200, 150, 4, 0, 4, 6, None, C.byref(n)) == INVALID
    assert lib.rf_gather_plan_planes(200, 150, 4, 0, 0, 6, None, C.byref(n)) == rf._ffi.RF_OK and n.value == 3 * 4     # the root: three receives for each of four planes
    small = np.zeros((2, 5), np.uint32)
    n = C.c_uint32(2)
    assert lib.rf_gather_plan_planes(200, 150, 4, 0, 0, 6, small.ctypes.data_as(C.c_void_p), C.byref(n)) == INVALID and not small.any()


def test_null_handles_are_invalid_arguments_without_a_device():
    lib = rf._ffi.lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bogus = C.c_void_p(16)                       # never dereferenced: the NULL partner is found first
    buf = np.full(16, 3.0, np.float32)
    words = [C.c_uint32(7) for _ in range(4)]
    ptr = C.c_void_p(5)
    est = rf._ffi.NoiseEstimate(-7.0, -7.0, 77, 77, 77, 77)
    for flags in (0, rf.RF_GATHER_AOVS, rf.RF_GATHER_MOMENTS, rf.RF_GATHER_AOVS | rf.RF_GATHER_MOMENTS | rf.RF_GATHER_LOOPBACK):
        assert lib.rf_renderer_gather_frame(None, bogus, 0, flags, C.byref(ptr)) == INVALID              # a NULL handle
        assert lib.rf_renderer_gather_frame(bogus, None, 0, flags, C.byref(ptr)) == INVALID
    calls = [
        lambda c, r: lib.rf_comm_gathered_planes(c, *[C.byref(w) for w in words]),
        lambda c, r: lib.rf_comm_read_plane(c, r, 0, P(buf)),
        lambda c, r: lib.rf_comm_plane_device(c, 1, C.byref(ptr)),
        lambda c, r: lib.rf_comm_denoise(c, r, None),
        lambda c, r: lib.rf_comm_read_denoised(c, r, P(buf), None, C.byref(words[0])),
        lambda c, r: lib.rf_comm_noise_estimate(c, r, C.byref(est), P(buf), None, None),
    ]
    for call in calls:
        assert call(None, bogus) == INVALID                                                               # a NULL communicator
        msg = lib.rf_last_error_message().decode()
        assert "null" in msg and "HIP" not in msg and "device" not in msg, msg
    for call in calls[1:2] + calls[3:]:
        assert call(bogus, None) == INVALID                                                               # a NULL handle (the calls that take one)
    assert ptr.value == 5 and all(w.value == 7 for w in words) and (buf == 3.0).all()
    assert (est.mean_error, est.samples, est.pixels) == (-7.0, 77, 77)
    # bad denoise parameters are refused as everywhere else, before the handles are looked at
    bad = rf._ffi.DenoiseParameters(9, 1.0, 0.1, 0.1)
    assert lib.rf_comm_denoise(None, None, C.byref(bad)) == INVALID and "iterations" in lib.rf_last_error_message().decode()
    bad = rf._ffi.DenoiseParameters(5, 0.0, 0.1, 0.1)
    assert lib.rf_comm_denoise(bogus, None, C.byref(bad)) == INVALID and "sigma" in lib.rf_last_error_message().decode()
