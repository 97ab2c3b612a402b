"""The scene packing (rayfinder_amd/csrc/rf_scene_pack.cpp, rf_wide_build.cpp) against the recording of the renderer's constructor it was taken out of: every packed
array, every derived fact and layout default and checkWideLayouts' flags, on the scenes of tests/scene_pack_scenes.py.  CPU only: the program links nothing of HIP."""
import json
import os
import subprocess

import pytest

import scene_pack_scenes as sp
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "rayfinder_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "scene_pack_main.cpp")] + [os.path.join(CSRC, f) for f in ("rf_scene_pack.cpp", "rf_wide_build.cpp", "rf_bvh.cpp")]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
COMMON = ["g++", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I", os.path.join(ROOT, "include")]
# -static-libasan / -static-libubsan: see tests/test_checkpoint_api.py -- the runtimes are linked into the executable, nothing is preloaded
SANITIZED = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SHIPPED = ["-O2"]                                             # the Makefile's host flags: the build that ships


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    return sp.write_all(tmp_path_factory.mktemp("scenes"))


@pytest.fixture(scope="module")
def recording():
    with open(os.path.join(GOLDEN, "scene_pack_parent.json")) as f:
        return json.load(f)["scenes"]


def test_the_recording_shows_every_branch(recording):
    """A scene that stops taking its branch must fail here, in the recording itself, not pass silently"""
    assert list(recording) == list(sp.SCENES)
    for name, wants in sp.BRANCH.items():
        row = recording[name]
        assert "error" not in row and "check.error" not in row, row
        for key, want in wants.items():
            assert want(row[key]) if callable(want) else row[key] == want, (name, key, row[key])


@pytest.mark.parametrize("flags", [SANITIZED, SHIPPED], ids=["asan_ubsan", "shipped_flags"])
def test_packed_scenes_equal_the_parents_recording(flags, scene_files, recording, tmp_path, monkeypatch):
    monkeypatch.delenv("RF_OCCLUDER_HINT_LEVELS", raising=False)
    exe = str(tmp_path / "scene_pack_main")
    # (one compiler per source, side by side: the sanitized builder alone takes a quarter of a minute)
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compilers = [subprocess.Popen(COMMON + flags + ["-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]
    assert [c.wait() for c in compilers] == [0] * len(SOURCES)
    subprocess.check_call(COMMON + flags + objects + ["-o", exe])
    run = subprocess.run([exe] + scene_files, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    rows = [json.loads(line) for line in run.stdout.splitlines()]
    assert [r["scene"] for r in rows] == list(recording)
    for row in rows:
        want = recording[row["scene"]]
        assert row.keys() == want.keys(), (row["scene"], sorted(row.keys() ^ want.keys()))
        assert {k: v for k, v in row.items() if v != want[k]} == {}, row["scene"]
    # the experiment override is read by the packing, with its clamp
    env = dict(os.environ, RF_OCCLUDER_HINT_LEVELS="11")
    run = subprocess.run([exe, scene_files[0]], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and json.loads(run.stdout)["facts.occluderHintLevels"] == 8, run.stdout + run.stderr
