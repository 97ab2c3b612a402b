"""The books of the temporal history (rayfinder_amd/csrc/rf_books.cpp) on the CPU, through tests/temporal_books_main.cpp: every new refusal in the order the header
states, the result snapshot's drop rules, and the history's -- it survives a restart of the accumulation and goes with the frame size, a tile shard and a reset.  The
program links nothing of HIP, and runs once with the sanitizers and once with the flags that ship."""
import json
import os
import subprocess

import pytest

from conftest import ROOT
from test_scene_pack import COMMON, CSRC, SANITIZED, SHIPPED

SOURCES = [os.path.join(ROOT, "tests", "temporal_books_main.cpp"), os.path.join(CSRC, "rf_books.cpp")]
TILES, SPP = 6, 64


@pytest.fixture(scope="module", params=[SANITIZED, SHIPPED], ids=["asan_ubsan", "shipped_flags"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("temporal_books") / "temporal_books_main")
    link = COMMON + request.param + SOURCES + ["-o", path]
    assert not any("hip" in word.lower() for word in link if word.startswith(("-l", "-L"))), link      # nothing of HIP is linked
    subprocess.check_call(link)
    needed = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "amdhip" not in needed and "hsa-runtime" not in needed, needed
    return path


def play(exe, script):
    """script: calls as strings -> one row per call"""
    words = [f"tiles={TILES}", f"spp={SPP}"]
    for i, call in enumerate(script):
        words += (["--"] if i else []) + call.split()
    run = subprocess.run([exe] + words, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr                     # no sanitizer report either
    rows = [json.loads(line) for line in run.stdout.splitlines()]
    assert [r["call"] for r in rows] == [" ".join(c.split()) for c in script]
    return rows


def state(row):
    return {k: v for k, v in row.items() if k not in ("call", "outcome", "message")}


def refused(rows, *words):
    """the last call was refused with these words, and left the state as the call before it had"""
    last = rows[-1]
    assert last["outcome"] == "invalid_argument", last
    assert all(w in last["message"] for w in words), last["message"]
    assert all(r["outcome"] == "accepted" for r in rows[:-1]), rows
    if len(rows) > 1:
        assert state(last) == state(rows[-2]), (last, rows[-2])
    return last["message"]


UNIFORM = ",".join(["4"] * TILES)
RAGGED = ",".join(["4"] * (TILES - 1) + ["2"])


@pytest.mark.parametrize("call, api", [("temporal_accumulate", "rf_renderer_temporal_accumulate"), ("denoise_temporal", "rf_renderer_denoise_temporal")])
def test_each_refusal_in_its_stated_order(exe, call, api):
    """AOVs off; AOV count != accumulated count; no sample; a tile shard; the non-uniform state -- each script has the fault it names and every fault behind it in the
    list that the state can hold at once, and gets the message of the first."""
    what = call
    # the AOVs off -- also with nothing accumulated, under a shard and in the non-uniform state
    msg = refused(play(exe, [call]), what + " needs the first-hit AOVs", "rf_renderer_set_aovs")
    assert msg == refused(play(exe, ["set_tile_shard 0 2 tiles=3", call]))
    assert msg == refused(play(exe, ["render 4", f"tile_counts {RAGGED}", call]))
    # the AOVs turned on partway: the counts differ -- also under a shard
    msg = refused(play(exe, ["render 2", "set_aovs 1", "render 2", call]), what + ": the AOV sample count (2) differs from the accumulated sample count (4)")
    assert msg == refused(play(exe, ["set_tile_shard 1 2 tiles=3", "render 2", "set_aovs 1", "render 2", call]))
    # no sample -- also under a shard
    msg = refused(play(exe, ["set_aovs 1", call]), what + ": no sample has been accumulated")
    assert msg == refused(play(exe, ["set_aovs 1", "set_tile_shard 0 2 tiles=3", call]))
    assert msg == refused(play(exe, ["set_aovs 1", "render 4", "set_exposure 0.5", call]))                # (restarted: the counts agree again, at 0)
    # a tile shard
    refused(play(exe, ["set_aovs 1", "set_tile_shard 0 2 tiles=3", "render 4", call]), what + " needs the whole frame: a tile shard is set", "rf_temporal_images")
    # the non-uniform state
    refused(play(exe, ["set_aovs 257", "render 4", f"tile_counts {RAGGED}", call]), api + ": the tiles hold different sample counts after rf_renderer_render_adaptive")
    # and none of them
    rows = play(exe, ["set_aovs 1", "render 4", call])
    assert rows[-1]["outcome"] == "accepted" and rows[-1]["temporal"] == dict(valid=True, samples=4) and rows[-1]["history"] is False
    assert rows[-1]["denoised"]["valid"] == (call == "denoise_temporal")


def test_commit_and_read_are_refused_without_a_result(exe):
    for call in ("temporal_commit", "read_temporal"):
        refused(play(exe, ["set_aovs 1", "render 4", call]), "no temporal result", "rf_renderer_temporal_accumulate")
        refused(play(exe, ["set_aovs 1", "render 4", "temporal_accumulate", "temporal_commit", call]), "no temporal result")   # a commit takes the result
    assert play(exe, ["set_aovs 1", "render 4", "temporal_accumulate", "read_temporal"])[-1]["outcome"] == "accepted"


@pytest.mark.parametrize("drop", ["set_exposure 0.5", "bind", "set_aovs 0", "set_aovs 257", "resize", "set_tile_shard 0 1 tiles=6", "temporal_reset"])
def test_the_result_is_dropped_with_the_aov_sums(exe, drop):
    rows = play(exe, ["set_aovs 1", "render 4", "denoise", "temporal_accumulate", drop, "read_temporal"])
    assert rows[3]["temporal"] == dict(valid=True, samples=4)
    assert rows[4]["outcome"] == "accepted" and rows[4]["temporal"]["valid"] is False
    assert rows[5]["outcome"] == "invalid_argument"
    # (the denoise snapshot goes with the AOV sums as it always did, and a reset of the temporal history does not touch it)
    assert rows[4]["denoised"]["valid"] == (drop == "temporal_reset")


def test_later_samples_and_the_other_snapshot_leave_the_result(exe):
    rows = play(exe, ["set_aovs 1", "render 4", "temporal_accumulate", "render 4", "denoise", "read_temporal", "temporal_accumulate"])
    assert rows[5]["outcome"] == "accepted" and rows[5]["temporal"] == dict(valid=True, samples=4) and rows[5]["denoised"] == dict(valid=True, samples=8)
    assert rows[6]["temporal"] == dict(valid=True, samples=8)


def test_the_history_survives_a_restart(exe):
    rows = play(exe, ["set_aovs 1", "render 4", "temporal_accumulate", "temporal_commit", "set_exposure 0.5", "bind", "set_aovs 0", "set_aovs 1", "render 4", "temporal_accumulate",
                      "render 4", "temporal_accumulate", "temporal_commit"])
    assert [r["outcome"] for r in rows] == ["accepted"] * len(rows)
    assert [r["history"] for r in rows] == [False] * 3 + [True] * 10
    assert rows[3]["temporal"]["valid"] is False                                                          # the commit took the result
    assert rows[9]["temporal"] == dict(valid=True, samples=4) and rows[11]["temporal"] == dict(valid=True, samples=8)


@pytest.mark.parametrize("drop", ["resize", "set_tile_shard 0 2 tiles=3", "set_tile_shard 0 1 tiles=6", "temporal_reset"])
def test_the_history_goes_with_the_frame_size_a_shard_and_a_reset(exe, drop):
    rows = play(exe, ["set_aovs 1", "render 4", "temporal_accumulate", "temporal_commit", drop])
    assert rows[3]["history"] is True and rows[4]["outcome"] == "accepted" and rows[4]["history"] is False
