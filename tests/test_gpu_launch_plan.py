"""The launch plan (-m gpu): rf_renderer_launch_plan equals what the parent of the commit that introduced planBatch / planBounce LAUNCHED.

None of the host driver's choices shows in the image (the contract is "same image with any setting"), so the parity tests cannot see a slipped refill threshold,
exit vote, claim size or count word.  tests/golden/launch_plan_parent.json is a recording made at the launch sites of that parent commit (a throw-away patch that
printed one line per launch: profiles/plan/parent_capture.patch, run by profiles/plan/record_parent.py over the matrix below), reworded into the fields of
rf_launch_plan.  A characterisation: the recording is the reference and every field must EQUAL it.  rf_renderer_layout_info must say what the plan says, and two
counters that exist already tie the plan to what ran."""
import json
import os

import numpy as np
import pytest

import rayfinder_amd as rf
from rayfinder_amd import scenes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDING = os.path.join(GOLDEN, "launch_plan_parent.json")
W, H, BOUNCES, SPP = 64, 48, 4, 1024          # 2 x 2 tiles, the lower row half outside the frame
SAMPLE_COUNTS = (2, 8, 200, 700)              # per batch: across the <= 4 cutoff (no runs) and the 160 / 640 steps of the pixels per workgroup
STATES = ("cold", "warm")                     # before the handle's first batch / after one 2-sample render (the occluder grid is warm: first look is eligible)


def _case(*options, **kw):
    return dict(options=options, **kw)


CASES = {
    "nothing_set": _case(),
    "counting": _case(counting=True),
    "traversal_variant_0": _case(("traversal_variant", 0)),
    "aovs": _case(aovs=True),
    "moments": _case(moments=True),
    "shade_sort_from_bounce_0": _case(("shade_sort_from_bounce", 0)),
    "occluder_cache_bounces_0": _case(("occluder_cache_bounces", 0)),
    "shadow_self_test_0": _case(("shadow_self_test", 0)),
    "shadow_nearest_first_0": _case(("shadow_nearest_first", 0)),
    "shadow_sign_order_0": _case(("shadow_sign_order", 0)),
    "shadow_first_look_from_bounce_1": _case(("shadow_first_look_from_bounce", 1)),
    "shadow_first_look_from_bounce_0": _case(("shadow_first_look_from_bounce", 0)),
    "quad_half_from_bounce_1": _case(("quad_half_from_bounce", 1), ("quad_half_shadow_from_bounce", 1)),
    "quad_local_from_bounce_1": _case(("quad_local_from_bounce", 1), ("quad_local_shadow_from_bounce", 1)),
    "quad_from_bounce_0": _case(("quad_from_bounce", 0)),
    "quad_except_mask_2": _case(("quad_except_mask", 2)),
    "oct_from_bounce_2": _case(("oct_from_bounce", 2)),
    "dense_leaf_min_2": _case(("dense_leaf_min", 2)),
    "dense_leaf_from_bounce_3": _case(("dense_leaf_from_bounce", 3)),
    "uniform_fetch_m1": _case(("uniform_fetch", -1)),
    "uniform_fetch_0": _case(("uniform_fetch", 0)),
    "uniform_fetch_1": _case(("uniform_fetch", 1)),
    "refill_min_7": _case(("refill_min", 7)),
    "refill_min_deep_9": _case(("refill_min_deep", 9)),
    "refill_deep_from_bounce_3": _case(("refill_deep_from_bounce", 3)),
    "leaf_vote_11": _case(("leaf_vote", 11)),
    "chunk_64": _case(("chunk", 64)),
    "chunk_early_bounces_0": _case(("chunk_early_bounces", 0)),
    "slot_group_shift_m1": _case(("slot_group_shift", -1)),
    "slot_group_shift_2": _case(("slot_group_shift", 2)),
    "accumulate_runs_0": _case(("accumulate_runs", 0)),
    "sample_sort_0": _case(("sample_sort", 0)),
    "camera_far_outside": _case(camera="far"),        # the primaryOutside branch
    "lens": _case(camera="lens"),                     # no constant origin
    "tree_not_nested": _case(tree="poke"),            # a child box sticks out of its parent's: binary records, no cache
}
SCENES = ("duck", "quad")
# (the hand-made tree is the Duck's with one box enlarged: the quad scene's tree is a single leaf)
MATRIX = [(s, c) for s in SCENES for c in CASES if not (s == "quad" and CASES[c].get("tree"))]

_pts = {}


def _pt(scene):
    if scene not in _pts:
        _pts[scene] = rf.PtFormat.from_gltf(os.path.join(GOLDEN, "Duck.glb")) if scene == "duck" else scenes.quad_scene()
    return _pts[scene]


def make_handle(scene, case):
    """The handle of one cell of the matrix, before its first batch (the recorder builds the very same ones)"""
    c = CASES[case]
    pt = _pt(scene)
    a = pt.arrays()
    if c.get("tree") == "poke":
        nodes = a["bvhNodes"].copy()
        nodes[1]["max"] = tuple(np.asarray(nodes[0]["max"]) + np.float32(1.0))
        sc = rf.scene_from_arrays(nodes, a["trianglePositionAttributes"], a["triangleVertexAttributes"], [(px, w, h) for (px, w, h) in a["baseColorTextures"]])
    else:
        sc = pt.scene()
    if c.get("camera") == "far":      # (the camera of test_camera_far_outside_the_scene_keeps_primary_rays_off_the_scalar_path, distance 1000)
        lo, hi = np.array(a["bvhNodes"][0]["min"][:3]), np.array(a["bvhNodes"][0]["max"][:3])
        centre, size, distance = 0.5 * (lo + hi), float(np.max(hi - lo)), 1000.0
        eye = centre + np.array([0.6, 0.4, 0.7]) / np.linalg.norm([0.6, 0.4, 0.7]) * distance * size
        cam = rf.create_camera(eye, centre, 0.0, 1.0, float(2.0 * np.arctan(0.75 / distance)), W / H)
    elif c.get("camera") == "lens":
        cam = rf.fly_camera(W, H, aperture=0.1)
    else:
        cam = rf.fly_camera(W, H)
    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, SPP, BOUNCES, rf.make_sky(), 0.25), sc)
    for name, value in c["options"]:
        r.set_option(name, value)
    if c.get("counting"):
        r.set_counting(True)
    if c.get("aovs"):
        r.set_aovs(True)
    if c.get("moments"):
        r.set_moments(True)
    return r


@pytest.fixture(scope="module")
def recording():
    with open(RECORDING) as f:
        rec = json.load(f)
    fields = rec["batch_fields"] + rec["bounce_fields"]
    # (the distinct rows are stored once: a cell names the rows of its bounces, which do not depend on the sample count, and its batch row per sample count)
    return {f"{cell}/{n}": [dict(zip(fields, rec["batch_rows"][batch] + rec["bounce_rows"][b])) for b in c["bounces"]] for cell, c in rec["cells"].items() for n, batch in c["batch"].items()}


def _check_layout_info(r, plans):
    li = r.layout_info(BOUNCES)
    for b, p in enumerate(plans):
        assert li["closest"][b] == r.LAYOUT_NAMES[p["closest_layout"]] and li["shadow"][b] == r.LAYOUT_NAMES[p["shadow_layout"]], (b, li, p)
        assert li["shadow_cached"][b] == bool(p["shadow_cached"]), (b, li, p)


@pytest.mark.parametrize("scene,case", MATRIX)
def test_the_plan_equals_what_the_parent_launched(recording, scene, case):
    r = make_handle(scene, case)
    wrong = []
    for state in STATES:
        if state == "warm":
            r.render(2)
        for n in SAMPLE_COUNTS:
            plans = [r.launch_plan(b, n) for b in range(1, BOUNCES + 1)]
            want = recording[f"{scene}/{case}/{state}/{n}"]
            assert len(want) == BOUNCES
            for b, (got, ref) in enumerate(zip(plans, want)):
                assert got.keys() == ref.keys()
                wrong += [(state, n, b + 1, k, got[k], ref[k]) for k in got if got[k] != ref[k]]
            _check_layout_info(r, plans)
    r.close()
    assert not wrong, f"(state, samples, bounce, field, plan, parent's launch): {wrong[:12]} ... {len(wrong)} in all"


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("case", ["nothing_set", "shadow_first_look_from_bounce_0", "shadow_first_look_from_bounce_1", "shadow_self_test_0", "occluder_cache_bounces_0", "counting"])
def test_the_counters_of_what_ran_agree_with_the_plan(scene, case):
    """rf_stats' first-look-answered count is non-zero after the second batch exactly when some bounce's plan says firstLook; shadow_rays_self_answered is non-zero
    exactly when some bounce's plan says selfShadow."""
    r = make_handle(scene, case)
    r.render(2)
    r.reset_stats()
    plans = [r.launch_plan(b, 8) for b in range(1, BOUNCES + 1)]      # the second batch, as planned
    r.render(8)
    s = r.stats()
    r.close()
    print(f"{scene}/{case}: first look planned at bounces {[b + 1 for b, p in enumerate(plans) if p['shadow_first_look']]}, answered {s['shadow_rays_hint_answered']}; "
          f"self test planned at bounces {[b + 1 for b, p in enumerate(plans) if p['shadow_self']]}, settled {s['shadow_rays_self_answered']} of {s['shadow_rays']} shadow rays")
    assert (s["shadow_rays_hint_answered"] != 0) == any(p["shadow_first_look"] for p in plans)
    assert (s["shadow_rays_self_answered"] != 0) == any(p["shadow_self"] for p in plans)
