"""The accumulation's books (rayfinder_amd/csrc/rf_books.cpp) on the CPU, through tests/books_main.cpp: the shipped state machine walked against the handle model
(tests/handle_model.py) over all 16 seeded walks, and its refusals held, byte for byte, to what the library said before the books were taken out of the HIP driver
(tests/golden/refusals_parent.json, recorded by tools/record_refusals.py on a GPU).  The program links nothing of HIP, and runs once with the sanitizers and once with
the flags that ship.  The sums themselves stay with tests/test_gpu_handle_walk.py."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import books_cases as bc
import handle_walk as hw
from conftest import GOLDEN, ROOT
from test_scene_pack import COMMON, CSRC, SANITIZED, SHIPPED

SOURCES = [os.path.join(ROOT, "tests", "books_main.cpp"), os.path.join(CSRC, "rf_books.cpp")]
FAMILIES = ("image", "aovs", "moments", "direct", "buckets")


@pytest.fixture(scope="module", params=[SANITIZED, SHIPPED], ids=["asan_ubsan", "shipped_flags"])
def exe(request, tmp_path_factory):
    directory = tmp_path_factory.mktemp("books")
    path = str(directory / "books_main")
    link = COMMON + request.param + SOURCES + ["-o", path]
    assert not any("hip" in word.lower() for word in link if word.startswith(("-l", "-L"))), link      # nothing of HIP is linked
    subprocess.check_call(link)
    needed = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "amdhip" not in needed and "hsa-runtime" not in needed, needed
    return path


@functools.lru_cache(maxsize=None)
def recording():
    with open(os.path.join(GOLDEN, "refusals_parent.json")) as f:
        return json.load(f)


def number(a):
    return str(int(a)) if isinstance(a, (int, np.integer)) else repr(float(np.float32(a)))


def words(call, counts=None, frames=None, tiles=None):
    """One call as books_main's words; what the books cannot know rides on the line"""
    name, args = call[0], call[1:]
    if name == "export_features":
        reads, two = bc.feature_reads(args[0])
        return [name, str(reads), str(int(two))]
    out = [name] + [number(a) for a in args]
    if name == "render_adaptive":
        out.append("counts=" + ",".join(str(int(c)) for c in counts))
    if name == "render_until":
        out.append(f"frames={int(frames)}")
    if name == "set_tile_shard":
        out.append(f"tiles={int(tiles)}")
    return out


def shard_tiles(rank, world):
    import rayfinder_amd as rf                                # the tile deal: host arithmetic
    return len(rf.tiles_for_rank(hw.W, hw.H, rank, world)) if world and rank < world else 0


def play(exe, calls):
    """-> one row per call"""
    script = [f"tiles={hw.TILES}", f"spp={hw.SPP}"]
    for i, call in enumerate(calls):
        script += (["--"] if i else []) + call
    run = subprocess.run([exe] + script, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr and run.stderr == "", run.stderr          # no sanitizer report
    rows = [json.loads(line) for line in run.stdout.splitlines()]
    assert [r["call"] for r in rows] == [" ".join(c) for c in calls]
    return rows


def state(row):
    return {k: v for k, v in row.items() if k not in ("call", "outcome", "message")}


@functools.lru_cache(maxsize=None)
def walked(seed):
    """The walk through the model alone -> per call: (its words, the model's outcome, what the model holds afterwards)"""
    calls, _ = hw.walk(seed)
    m, out = hw.new_model(), []
    for call in calls:
        want = hw.apply(m, call)
        extra = {}
        if call[0] == "render_adaptive":
            extra["counts"] = [m.counts[t] for t in m.own]
        if call[0] == "render_until":
            extra["frames"] = want[1]["frames"] if want[0] == "ok" else 0
        if call[0] == "set_tile_shard":
            extra["tiles"] = shard_tiles(call[1], call[2])
        on = dict(aovs=m._aov_on(), moments=m.moments_on, buckets=bool(m.K))
        start = dict(aovs=m.a_start, moments=m.q_start, buckets=m.b_start)
        holds = dict(accumulated=m.L, frame_count=m.frame_count, tile_counts=[int(m.counts[t]) for t in m.own],
                     families={f: dict(on=on[f], samples=m._count(on[f], start[f]), covers=m._covers(on[f], start[f])) for f in on},
                     denoised=dict(valid=m.denoised is not None, samples=m.denoised["samples"] if m.denoised else 0),
                     robust=dict(valid=m.robust is not None, samples=m.robust["samples"] if m.robust else 0))
        out.append((words(call, **extra), want, holds))
    return out


@pytest.mark.parametrize("seed", hw.SEEDS)
def test_the_books_follow_the_model_through_a_seeded_walk(exe, seed):
    steps = walked(seed)
    assert len(steps) == hw.LENGTH                                                                       # every call of the walk, none skipped
    rows = play(exe, [w for w, _, _ in steps])
    before = None
    for i, (row, (call, want, holds)) in enumerate(zip(rows, steps)):
        where = f"seed {seed}, call {i} {' '.join(call)}: {row}"
        assert (row["outcome"] == "accepted") == (want[0] == "ok"), where
        if want[0] == "refused":
            assert row["outcome"] == "invalid_argument", where
            assert all(w in row["message"] for w in (want[1] or ())), where                              # (tests/test_gpu_handle_walk.py: the promised words)
            assert before is not None and state(row) == state(before), where                             # a refused call changes nothing
        for key in ("accumulated", "frame_count", "tile_counts", "denoised", "robust"):
            assert row[key] == holds[key], (key, where)
        assert row["families"]["image"]["samples"] == holds["accumulated"], where
        for f, want_f in holds["families"].items():
            got = row["families"][f]
            assert got["on"] == want_f["on"] and got["samples"] == want_f["samples"], (f, where)
            if holds["accumulated"]:                                                                     # (with nothing accumulated the model's "covers" is a promise, the books' a fact)
                assert got["covers"] == want_f["covers"], (f, where)
        before = row


def outcomes_of(status):
    """rf_c_api.cpp: std::invalid_argument is RF_ERROR_INVALID_ARGUMENT, every other exception of the books RF_ERROR_RUNTIME"""
    return ("invalid_argument",) if status == recording()["invalid_argument"] else ("logic_error", "runtime_error")


def test_the_recording_is_of_this_frame_and_these_cases():
    rec = recording()
    assert rec["frame"] == dict(width=hw.W, height=hw.H, spp=hw.SPP, tiles=hw.TILES)
    assert sorted(rec["walks"]) == sorted(str(s) for s in hw.SEEDS) and sorted(rec["cases"]) == sorted(bc.CASES)
    assert all(row["message"] for row in rec["cases"].values())


@pytest.mark.parametrize("seed", hw.SEEDS)
def test_a_walks_refusals_say_what_the_parent_said(exe, seed):
    steps = walked(seed)
    rows = play(exe, [w for w, _, _ in steps])
    want = {r["index"]: r for r in recording()["walks"][str(seed)]}
    assert sorted(want) == [i for i, row in enumerate(rows) if row["outcome"] != "accepted"]
    for i, ref in want.items():
        assert rows[i]["outcome"] in outcomes_of(ref["status"]) and rows[i]["message"] == ref["message"], (seed, i, rows[i]["call"], rows[i]["message"], ref["message"])


def test_the_word_checks_the_c_abi_shadows(exe):
    """Renderer::setDirect and Renderer::setTileShard check their arguments themselves; through the C ABI nobody sees it (rf_c_api.cpp refuses the same words first,
    in words of its own: the recording holds those).  The books' own check, as C++ callers meet it: the type and the text the renderer had."""
    rows = play(exe, [["set_direct_unchecked", "256"], ["set_direct_unchecked", "2"], ["set_tile_shard_unchecked", "2", "2"], ["set_tile_shard_unchecked", "0", "0"]])
    word = "set_direct: the word must be 0 (off), 1 (on) or 1 | RF_DIRECT_TILE_COUNTS (the bit says how D is kept: valid only together with 1)"
    assert [(r["outcome"], r["message"]) for r in rows] == [("invalid_argument", word)] * 2 + [("runtime_error", "invalid tile shard")] * 2
    assert all(state(r) == state(rows[0]) for r in rows)


def test_the_hand_written_refusals_say_what_the_parent_said(exe):
    wrong = []
    for name, calls in bc.CASES.items():
        ref = recording()["cases"][name]
        script = []
        for i, call in enumerate(calls):
            tiles = shard_tiles(call[1], call[2]) if call[0] == "set_tile_shard" else None
            script.append(words(call, counts=ref["counts"].get(str(i), [0] * hw.TILES), frames=ref["frames"].get(str(i), 0), tiles=tiles))
        rows = play(exe, script)
        assert [r["outcome"] for r in rows[:-1]] == ["accepted"] * (len(rows) - 1), (name, rows)
        assert state(rows[-1]) == (state(rows[-2]) if len(rows) > 1 else state(rows[-1])), name          # a refused call changes nothing
        if rows[-1]["outcome"] not in outcomes_of(ref["status"]) or rows[-1]["message"] != ref["message"]:
            wrong.append((name, rows[-1]["outcome"], rows[-1]["message"], ref["message"]))
    assert not wrong, wrong
