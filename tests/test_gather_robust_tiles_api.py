"""RF_BUCKETS_SHARD_TILE_COUNTS without a GPU: the word checks of rf_renderer_set_buckets that come before the handle is used, and the declarations of the bit in the
header, the ffi module and the Python wrapper.  (The bit itself -- the bucket planes per tile count under a tile shard and through the frame gather -- is
tests/test_gpu_gather_robust_tiles.py's.)"""
import os
import re

import rayfinder_amd as rf
from conftest import ROOT

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT


def _set_buckets_without_a_handle(word):
    lib = rf._ffi.lib
    assert lib.rf_renderer_set_buckets(None, word) == INVALID, hex(word)
    return lib.rf_last_error_message().decode()


def test_the_bit_alone_or_without_the_tile_counts_bit_is_refused_before_the_handle_is_used():
    """0x400 is valid only together with RF_BUCKETS_TILE_COUNTS and K > 0, and 0x200 stays unknown: the K message, not the handle's"""
    for word in (0x400 | 9, 0x400, 0x600 | 9, 0x500 | 4, 0x500, 0x500 | 17, 0x700 | 9, 0xC00 | 9):
        assert "K must be" in _set_buckets_without_a_handle(word), hex(word)
    for word in (0x200 | 9, 0x300 | 9):                                      # as before the bit existed
        assert "K must be" in _set_buckets_without_a_handle(word), hex(word)


def test_the_valid_word_passes_the_argument_check_and_reaches_the_handle_check():
    for word in (0x500 | 9, 0x500 | 3, 0x500 | 15):
        msg = _set_buckets_without_a_handle(word)
        assert "null" in msg and "K must be" not in msg, (hex(word), msg)
    for word in (0x100 | 9, 9, 0):                                           # the words known before are what they were
        assert "null" in _set_buckets_without_a_handle(word), hex(word)


def test_the_ffi_constants_equal_the_header_s():
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    defines = {name: int(value, 16) for name, value in re.findall(r"#define (RF_BUCKETS_\w+) (0x[0-9a-fA-F]+)u", header)}
    assert defines == dict(RF_BUCKETS_TILE_COUNTS=0x100, RF_BUCKETS_SHARD_TILE_COUNTS=0x400)
    assert rf._ffi.RF_BUCKETS_TILE_COUNTS == defines["RF_BUCKETS_TILE_COUNTS"]
    assert rf._ffi.RF_BUCKETS_SHARD_TILE_COUNTS == defines["RF_BUCKETS_SHARD_TILE_COUNTS"]
    names = rf.ReferencePathTracer.set_buckets.__code__.co_varnames
    assert "tile_counts" in names and "shard" in names
