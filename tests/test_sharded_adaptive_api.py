"""Tile-adaptive sampling across ranks, the host-only part: the operations a gather posts for the per-tile counts (rf_gather_plan_counts), what the header declares,
and the argument checks that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import ROOT

FRAMES = ((150, 90), (70, 45), (64, 64), (200, 150))


@pytest.mark.parametrize("world", [2, 4, 8])
def test_every_count_send_has_its_receive_and_the_receives_tile_the_staging_area(world):
    for w, h in FRAMES:
        tiles = ((w + 31) // 32) * ((h + 31) // 32)
        first, _, _ = rf.gather_layout(w, h, world)
        for root in range(world):
            for loopback in (False, True):
                plans = [rf.gather_plan_counts(w, h, world, k, root, loopback) for k in range(world)]
                sends = {(k, int(op[1])): int(op[3]) for k in range(world) for op in plans[k] if op[0] == 1}
                recvs = [(int(op[1]), int(op[2]), int(op[3])) for op in plans[root] if op[0] == 0]
                assert all(not any(op[0] == 0 for op in plans[k]) for k in range(world) if k != root)      # only the root receives
                assert all(dst == root for (_, dst) in sends)
                # each send has its receive, of the same length, at the sender's place of the staging area; offsets of a send count from the rank's own first word
                assert sorted(sends) == sorted((peer, root) for peer, _, _ in recvs)
                for peer, offset, count in recvs:
                    assert count == sends[(peer, root)] == len(rf.tiles_for_rank(w, h, peer, world)) and offset == first[peer]
                assert all(int(op[2]) == 0 for k in range(world) for op in plans[k] if op[0] == 1)
                # the receives, with the root's own words (read in place without loop-back), tile [0, tiles) exactly
                covered = np.zeros(tiles, np.int64)
                for _, offset, count in recvs:
                    covered[offset:offset + count] += 1
                if not loopback:
                    covered[first[root]:first[root + 1]] += 1
                assert (covered == 1).all(), (w, h, world, root, loopback)
                # one word per tile: the list is the one-plane plan's, and the plans of the planes are what they were
                assert np.array_equal(plans[root], rf.gather_plan(w, h, world, root, root, loopback))


def test_the_header_declares_the_new_names():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    assert re.search(r"#define\s+RF_GATHER_TILE_COUNTS\s+8u\b", header)
    assert rf.RF_GATHER_TILE_COUNTS == 8
    for name in ("rf_comm_render_adaptive", "rf_comm_read_tile_samples", "rf_comm_read_mean", "rf_gather_plan_counts"):
        assert re.search(r"RF_API\s+int\s+" + name + r"\(", header), name
        assert name in rf._ffi.SIGNATURES and hasattr(rf._ffi.lib, name)
    for field in ("rf_adaptive_result rank;", "frame_leading_samples;", "frame_min_tile_samples;", "max_rank_pixel_samples;", "} rf_comm_adaptive_result;"):
        assert field in header, field
    # the struct as ctypes sees it: rf_adaptive_result, two words, one uint64
    assert C.sizeof(rf._ffi.CommAdaptiveResult) == C.sizeof(rf._ffi.AdaptiveResult) + 16
    assert rf._ffi.CommAdaptiveResult.max_rank_pixel_samples.offset == C.sizeof(rf._ffi.AdaptiveResult) + 8


def test_null_handles_are_invalid_arguments_without_a_device():
    lib, bad = rf._ffi.lib, rf._ffi.RF_ERROR_INVALID_ARGUMENT
    p = rf._ffi.AdaptiveParameters(0.1, 4, 0, 0)
    res = rf._ffi.CommAdaptiveResult()
    n = C.c_uint32(0)
    buf = np.zeros(16, np.float32)
    assert lib.rf_comm_render_adaptive(None, None, C.byref(p), C.byref(res)) == bad
    assert lib.rf_comm_render_adaptive(None, None, None, None) == bad
    assert lib.rf_comm_read_tile_samples(None, None, C.byref(n)) == bad
    assert lib.rf_comm_read_mean(None, None, buf.ctypes.data_as(C.c_void_p)) == bad
    assert lib.rf_gather_plan_counts(150, 90, 2, 0, 0, 0, None, None) == bad
    assert lib.rf_gather_plan_counts(150, 90, 2, 2, 0, 0, None, C.byref(n)) == bad                # rank out of range
    assert lib.rf_gather_plan_counts(0, 90, 2, 0, 0, 0, None, C.byref(n)) == bad
