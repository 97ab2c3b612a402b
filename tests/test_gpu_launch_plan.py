"""The launch plan (-m gpu): rf_renderer_launch_plan equals what the parent of the commit that introduced planBatch / planBounce LAUNCHED.

None of the host driver's choices shows in the image (the contract is "same image with any setting"), so the parity tests cannot see a slipped refill threshold,
exit vote, claim size or count word.  tests/golden/launch_plan_parent.json is a recording made at the launch sites of that parent commit (a throw-away patch that
printed one line per launch: profiles/plan/parent_capture.patch, run by profiles/plan/record_parent.py over the matrix below), reworded into the fields of
rf_launch_plan.  A characterisation: the recording is the reference and every field must EQUAL it.  rf_renderer_layout_info must say what the plan says, and two
counters that exist already tie the plan to what ran.

Its CPU twin, tests/test_launch_policy.py, replays the same matrix (tests/launch_plan_cases.py) through the host-only policy unit without a device; this test is what
ties the C ABI, the policy and what actually ran together."""
import json

import pytest

import rayfinder_amd as rf
from launch_plan_cases import BOUNCES, CASES, H, RECORDING, SAMPLE_COUNTS, SCENES, SPP, STATES, W, MATRIX, camera, pt, scene_arrays

pytestmark = pytest.mark.gpu


def make_handle(scene, case):
    """The handle of one cell of the matrix, before its first batch (the recorder builds the very same ones)"""
    c = CASES[case]
    sc = rf.scene_from_arrays(*scene_arrays(scene, c["tree"])) if c.get("tree") else pt(scene).scene()
    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, camera(scene, case), SPP, BOUNCES, rf.make_sky(), 0.25), sc)
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
