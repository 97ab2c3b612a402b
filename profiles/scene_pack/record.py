"""Write the scenes of tests/scene_pack_scenes.py, run a recorder built from record_parent.hip on them and keep its lines as tests/golden/scene_pack_parent.json.
Usage (from the repository root, after building the recorder as README.md says):  python profiles/scene_pack/record.py <recorder executable>"""
import json
import os
import pathlib
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import scene_pack_scenes as sp  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    paths = sp.write_all(pathlib.Path(d))
    env = {k: v for k, v in os.environ.items() if k != "RF_OCCLUDER_HINT_LEVELS"}
    out = subprocess.run([sys.argv[1]] + paths, capture_output=True, text=True, check=True, env=env).stdout
rows = [json.loads(line) for line in out.splitlines()]
assert [r["scene"] for r in rows] == list(sp.SCENES)
with open(os.path.join(ROOT, "tests", "golden", "scene_pack_parent.json"), "w") as f:
    f.write('{"recorded_from": "the parent commit\'s Renderer::Renderer, compiled as host code of a .hip file with the Makefile\'s HIPFLAGS (profiles/scene_pack/record_parent.hip)",\n "scenes": {\n')
    f.write(",\n".join(f'  {json.dumps(r["scene"])}: {json.dumps(r)}' for r in rows))
    f.write("\n }}\n")
print(len(rows), "scenes recorded")
