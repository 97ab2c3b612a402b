"""The checkpoint's host side: the C ABI's new symbols, the blob parser behind rf_checkpoint_info on blobs crafted in numpy (no device is touched), the digest's
restatement against hand-written integer arithmetic, and the parser alone under AddressSanitizer + UBSan as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rayfinder_amd as rf
import digest_restatement as dr
from checkpoint_blobs import HEADER, TILE_BYTES, field_boundaries, make_blob, patched, stored_planes
from conftest import ROOT

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
NAMES = ("rf_renderer_state_digest", "rf_renderer_save_checkpoint", "rf_checkpoint_info", "rf_renderer_load_checkpoint")


def _refused(blob, *words):
    with pytest.raises(rf.RayfinderError) as e:
        rf.checkpoint_info(blob)
    assert e.value.status == INVALID, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def _bad_blobs():
    """name -> (blob, words its refusal names)"""
    good = make_blob()
    n, planes = 6, len(stored_planes(1, 1, 0, 3, [[4, 0]] * 5))
    bad = {
        "bad_magic": (b"RFCKPT2\0" + good[8:], ("magic",)),
        "bad_version": (patched(good, "version", 2), ("version",)),
        "header_length": (patched(good, "header_bytes", 280), ("header length",)),
        "tile_count_up": (patched(good, "num_tiles", 5), ("tile count",)),        # one tile fewer than the length holds
        "tile_count_grid": (patched(good, "num_tiles", 7), ("grid",)),            # more than 3 x 2
        "short_by_one_texel": (patched(good[:-16], "total_bytes", len(good) - 16), ("tile count",)),
        "total_bytes": (good + b"\0" * 16, ("bytes",)),
        "zero_width": (patched(good, "width", 0), ("size",)),
        "aov_word": (patched(good, "aov_flags", 2), ("AOV",)),
        "buckets_word": (patched(good, "buckets_word", 4), ("buckets",)),
        "off_family_with_samples": (patched(good, "moments", 0), ("off",)),
        "tile_twice": (make_blob(tiles=(0, 1, 2, 2, 4, 5)), ("ascending",)),
        "tile_outside": (make_blob(tiles=(0, 1, 2, 3, 4, 6)), ("outside",)),
        "count_above": (make_blob(tile_samples=(4, 4, 5, 4, 4, 4)), ("more samples",)),
    }
    assert n * planes * TILE_BYTES < len(good)
    for at in field_boundaries():
        bad[f"truncated_{at:03d}"] = (good[:at], ("truncated",) if at < 288 else ("bytes",))
    return good, bad


def test_the_symbols_are_exported_and_declared():
    lib = C.CDLL(rf._ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rayfinder_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in rf._ffi.SIGNATURES, name
        assert f"RF_API int {name}(" in header, name
    assert "RF_ERROR_CORRUPT = 5" in header and rf._ffi.RF_ERROR_CORRUPT == 5
    for name in ("state_digest", "save_checkpoint", "load_checkpoint", "resume"):
        assert callable(getattr(rf.ReferencePathTracer, name)), name
    assert callable(rf.checkpoint_info)
    # the ctypes mirrors have the C structs' sizes (rf_state_digest: 21 u64 + 18 u32; rf_checkpoint_info: 24 u32, one u64, camera 76 B, sky 24 B, padded to 8)
    assert C.sizeof(rf._ffi.StateDigest) == 21 * 8 + 18 * 4 and C.sizeof(rf._ffi.CheckpointInfo) == 24 * 4 + 8 + 76 + 24 + 4


def test_info_reads_a_crafted_blob():
    blob = make_blob(tile_samples=(4, 2, 4, 3, 4, 4), direct_word=0x101, buckets_word=0x103)
    info = rf.checkpoint_info(blob)
    h = np.frombuffer(blob[:288], HEADER)[0]
    assert (info["width"], info["height"], info["num_tiles"], info["frame_count"], info["accumulated"]) == (70, 45, 6, 7, 4)
    assert (info["aov_flags"], info["moments_on"], info["direct_word"], info["buckets_word"]) == (1, 1, 0x101, 0x103)
    assert info["family_samples"] == [4] * 5 and info["family_restarted"] == [0] * 5
    assert info["stored_planes"] == 1 + 2 + 1 + 1 + 3 and info["total_bytes"] == len(blob) and info["num_bounces"] == 3
    assert bytes(info["camera"]) == h["camera"].tobytes() and bytes(info["sky"]) == h["sky"].tobytes()
    # nothing accumulated: every family restarted, no plane stored
    empty = make_blob(accumulated=0)
    assert len(empty) == 288 + 6 * 8 and rf.checkpoint_info(empty)["stored_planes"] == 0


def test_bad_blobs_are_refused_and_never_crash():
    good, bad = _bad_blobs()
    assert rf.checkpoint_info(good)["num_tiles"] == 6
    for name, (blob, words) in bad.items():
        _refused(blob, *words)
    _refused(b"")


def test_the_restatement_against_hand_written_integers():
    M = (1 << 64) - 1

    def mix(z):  # written out once more, on purpose
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M
        z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M
        return z ^ (z >> 31)

    assert dr.mix64(0) == 0 and dr.mix64(1) == mix(1) and dr.mix64(M) == mix(M)
    plane = np.array([[[1.0, -2.5, 0.0, 3.0], [0.25, 0.0, 7.0, 0.0], [0.0, 0.0, 0.0, 0.0]]], np.float32)  # 3 x 1 pixels
    w = plane.view(np.uint32)
    want = 0
    for i in range(3):
        k = mix((3 << 32) | i)
        want = (want + mix(k ^ (int(w[0, i, 1]) << 32 | int(w[0, i, 0]))) + mix(((k + 0x9E3779B97F4A7C15) & M) ^ (int(w[0, i, 3]) << 32 | int(w[0, i, 2])))) & M
    assert dr.plane_digest_ints(3, plane) == want == dr.plane_digest(3, plane)
    # -0.0 is not +0.0; two pixels swapped, or the same texels under another plane id, are another digest
    negative = plane.copy()
    negative[0, 2, 1] = -0.0
    assert dr.plane_digest(3, negative) != want
    assert dr.plane_digest(3, plane[:, [1, 0, 2]]) != want and dr.plane_digest(2, plane) != want
    # additivity over a split of the tiles, and the vectorised form against the integers, on a ragged 3 x 2 tile frame
    rng = np.random.default_rng(5)
    frame = rng.standard_normal((45, 70, 4)).astype(np.float32)
    whole = dr.plane_digest(0, frame)
    assert whole == dr.plane_digest_ints(0, frame)
    assert (dr.plane_digest(0, frame, [0, 3, 4]) + dr.plane_digest(0, frame, [1, 2, 5])) & M == whole
    assert dr.plane_digest_ints(0, frame, {1, 5}) == dr.plane_digest(0, frame, [1, 5])
    # two tiles swapped: the pixels keep their values and change their frame index
    swapped = frame.copy()
    swapped[0:32, 0:32], swapped[0:32, 32:64] = frame[0:32, 32:64], frame[0:32, 0:32]
    assert dr.plane_digest(0, swapped) != whole
    counts = [4, 2, 4, 3, 4, 4]
    assert (dr.counts_digest(counts, [0, 2, 4]) + dr.counts_digest(counts, [1, 3, 5])) & M == dr.counts_digest(counts, range(6))
    assert dr.counts_digest(counts, range(6)) != dr.counts_digest([2, 4, 4, 3, 4, 4], range(6))
    assert dr.counts_digest([4], [0]) == mix(mix(0xC0 << 32) ^ 4)


def test_the_parser_alone_under_asan_and_ubsan(tmp_path):
    """tests/checkpoint_parse_main.cpp + rf_checkpoint.cpp, -fsanitize=address,undefined, run as a plain executable on the crafted blobs and 256 seeded single-byte
    corruptions of a good header: exit 0 and no sanitizer report.  Nothing is preloaded and nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "rayfinder_amd", "csrc")
    exe = str(tmp_path / "checkpoint_parse_main")
    # -static-libasan / -static-libubsan: ASan's shared runtime refuses to start unless it is the first library the loader maps, which is not the program's to decide --
    # an environment that preloads any library of its own into every process (LD_PRELOAD, /etc/ld.so.preload) would turn this test into a failure that says nothing
    # about the parser.  With the runtimes linked into the executable there is no such order to keep; the instrumentation and the checks are the same.
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc,
                           os.path.join(ROOT, "tests", "checkpoint_parse_main.cpp"), os.path.join(csrc, "rf_checkpoint.cpp"), "-o", exe])
    good, bad = _bad_blobs()
    paths = []
    for name, blob in [("good", good)] + [(k, v[0]) for k, v in bad.items()]:
        paths.append(str(tmp_path / f"{name}.bin"))
        with open(paths[-1], "wb") as f:
            f.write(blob)
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert f"{len(bad)} bad refused" in run.stdout, run.stdout
