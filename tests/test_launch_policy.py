"""The launch policy (rayfinder_amd/csrc/rf_launch_policy.cpp) against the recording of what the parent of planBatch / planBounce launched: the whole matrix of
tests/test_gpu_launch_plan.py (tests/launch_plan_cases.py) replayed through tests/launch_policy_main.cpp, every field of every cell equal to
tests/golden/launch_plan_parent.json.  CPU only: the program links nothing of HIP, and runs once with the sanitizers and once with the flags that ship."""
import json
import os
import subprocess

import pytest

import launch_plan_cases as lp
import scene_pack_scenes as sp
from conftest import ROOT
from test_scene_pack import COMMON, CSRC, SANITIZED, SHIPPED

SOURCES = [os.path.join(ROOT, "tests", "launch_policy_main.cpp")] + [os.path.join(CSRC, f) for f in ("rf_launch_policy.cpp", "rf_scene_pack.cpp", "rf_wide_build.cpp", "rf_bvh.cpp")]
ENVIRONMENT = ("RF_TRAVERSAL_VARIANT", "RF_PACKET_BOUNCES", "RF_PRIMARY_LIST_MIN_SAMPLES", "RF_PRIMARY_LIST_CAPACITY", "RF_OCCLUDER_HINT_LEVELS")   # what a new handle reads
FILES = [(scene, tree) for scene in lp.SCENES for tree in (None, "poke") if any(s == scene and lp.CASES[c].get("tree") == tree for s, c in lp.MATRIX)]


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    """one RFSCENE1 file per (scene, hand-made tree) of the matrix"""
    directory = tmp_path_factory.mktemp("scenes")
    paths = {}
    for scene, tree in FILES:
        paths[scene, tree] = str(directory / f"{scene}_{tree}.scene")
        sp.write_scene(paths[scene, tree], lp.scene_arrays(scene, tree))
    return paths


@pytest.fixture(scope="module")
def recording():
    with open(lp.RECORDING) as f:
        rec = json.load(f)
    fields = rec["batch_fields"] + rec["bounce_fields"]
    return {f"{cell}/{n}": [dict(zip(fields, rec["batch_rows"][batch] + rec["bounce_rows"][b])) for b in c["bounces"]] for cell, c in rec["cells"].items() for n, batch in c["batch"].items()}


def case_words(scene, case, state):
    c = lp.CASES[case]
    words = [f"case={scene}/{case}", f"state={state}", f"width={lp.W}", f"height={lp.H}", f"bounces={lp.BOUNCES}", "samples=" + ",".join(map(str, lp.SAMPLE_COUNTS)),
             "camera=" + bytes(lp.camera(scene, case)).hex()]
    words += [f"{name}={value}" for name, value in c["options"]] + [switch for switch in ("counting", "aovs", "moments") if c.get(switch)]
    return words


@pytest.mark.parametrize("flags", [SANITIZED, SHIPPED], ids=["asan_ubsan", "shipped_flags"])
def test_the_policy_plans_what_the_parent_launched(flags, scene_files, recording, tmp_path, monkeypatch):
    for name in ENVIRONMENT:
        monkeypatch.delenv(name, raising=False)
    exe = str(tmp_path / "launch_policy_main")
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compilers = [subprocess.Popen(COMMON + flags + ["-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]
    assert [c.wait() for c in compilers] == [0] * len(SOURCES)
    link = COMMON + flags + objects + ["-o", exe]
    print("link:", " ".join(link))
    assert not any("hip" in word.lower() for word in link if word.startswith(("-l", "-L"))), link      # nothing of HIP is linked
    subprocess.check_call(link)
    needed = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    assert "amdhip" not in needed and "hsa-runtime" not in needed, needed

    got = {}
    for (scene, tree), path in scene_files.items():
        cells = [(s, c, state) for s, c in lp.MATRIX if s == scene and lp.CASES[c].get("tree") == tree for state in lp.STATES]
        args = [path]
        for cell in cells:
            args += case_words(*cell) + ["--"]
        run = subprocess.run([exe] + args[:-1], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
        for line in run.stdout.splitlines():
            row = json.loads(line)
            got.setdefault(f"{row['case']}/{row['state']}/{row['plan']['num_samples']}", []).append(row)
    # every cell of the recording, no other, no cell skipped
    assert sorted(got) == sorted(recording) and len(got) == len(lp.MATRIX) * len(lp.STATES) * len(lp.SAMPLE_COUNTS)
    wrong = []
    for cell, want in recording.items():
        rows = got[cell]
        assert [r["bounce"] for r in rows] == list(range(1, lp.BOUNCES + 1)) and len(want) == lp.BOUNCES, cell
        for row, ref in zip(rows, want):
            assert row["plan"].keys() == ref.keys(), cell
            wrong += [(cell, row["bounce"], k, row["plan"][k], ref[k]) for k in ref if row["plan"][k] != ref[k]]
    assert not wrong, f"(cell, bounce, field, plan, parent's launch): {wrong[:12]} ... {len(wrong)} in all"

    # a name the options do not know: LaunchOptions::set says so (Renderer::setOption then throws "unknown option")
    run = subprocess.run([exe, scene_files["quad", None], "case=unknown", "no_such_option=1", "samples=2"], capture_output=True, text=True)
    assert run.returncode == 0 and [json.loads(line) for line in run.stdout.splitlines()] == [{"case": "unknown", "unknown_option": "no_such_option"}], run.stdout + run.stderr
