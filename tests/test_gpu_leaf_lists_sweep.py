"""Bounce 1's per-pixel leaf lists swept over cameras, scenes, frames and capacities (-m gpu): the cases of tests/leaf_list_cases.py, which the host-side soundness
test (tests/test_leaf_lists_restatement.py) shares.

Per case:  the LISTS THEMSELVES -- the histogram of list lengths, the refusals by reason, pixel count, capacity and batch depth that the renderer reports under
RF_DEBUG_PRIMARY_LISTS -- equal those of the numpy restatement of kPixelLeafLists, as integers; the rays handed on are exactly the samples of the pixels without a list;
the HITS are kTraceWide's: option primary_lists off against on with the AOVs on (kTraceLeafLists) and primary_fused off against on with them off (kPrimaryFused), at
64 samples (every wave one pixel's) and, on handles of its own, at 40 (waves that straddle pixels), bit for bit.  For one camera per scene kind the image is the oracle's.  The
hand-over itself -- kTraceWide working through a list of queue positions, then the listed kShade -- under every record layout the randomized parity test rotates through."""
import os
import re

import numpy as np
import pytest

import leaf_list_cases as cases
import rayfinder_amd as rf
import test_gpu_primary_fused as fused
import test_gpu_primary_lists as lists
from conftest import bits
from oracle import orc

pytestmark = pytest.mark.gpu
LINE = re.compile(r"\[rf-primary-lists\] pixels (\d+), without a list (\d+) \([^)]*\), mean length [0-9.]+, capacity (\d+), samples (\d+) \| length:count((?: \d+:\d+)*) \| "
                  r"no list: signs (\d+), overflow (\d+), big leaf (\d+), stack (\d+)")


def _capacity(case):
    return (("primary_list_capacity", case.capacity),)


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_kernels_lists_are_the_restatements(name, capfd):
    case = cases.BY_NAME[name]
    cam, _ = cases.camera(case)
    expected = cases.restated(name)
    spp = 32
    r = rf.ReferencePathTracer(rf.make_render_parameters(case.w, case.h, cam, 4096, 3, rf.make_sky(), 0.25), cases.scene(case.scene).rf_scene())
    r.set_option("primary_list_capacity", case.capacity)
    capfd.readouterr()
    os.environ["RF_DEBUG_PRIMARY_LISTS"] = "1"
    try:
        r.render(spp)
        _, acc = r.read_accumulation()
    finally:
        os.environ.pop("RF_DEBUG_PRIMARY_LISTS", None)
    s = r.stats()
    r.close()
    err = capfd.readouterr().err
    found = LINE.findall(err)
    print(err.strip())
    assert acc == spp and len(found) == 1, err
    pixels, without, capacity, samples, histogram, signs, overflow, big_leaf, stack = found[0]
    assert (int(pixels), int(capacity), int(samples)) == (case.w * case.h, case.capacity, spp)
    assert {int(l): int(c) for l, c in (pair.split(":") for pair in histogram.split())} == expected.histogram()
    assert dict(zip(("signs", "overflow", "big leaf", "stack"), map(int, (signs, overflow, big_leaf, stack)))) == expected.reasons()
    assert int(without) == expected.without
    assert s["primary_list_rays"] == case.w * case.h * spp
    assert s["primary_fallback_rays"] == spp * expected.without            # (a listed pixel hands no ray on: none is outside class A, none has other signs than its list)


def test_an_eye_with_a_zero_coordinate_keeps_the_old_launches(capfd):
    """The root box of "clutter" is centred on x = z = 0: from its centre the plan does not take the lists (BatchPlan::constOrigin) -- said here by name, so that no case
    of the sweep passes for want of lists"""
    w, h = 32, 24
    cam = cases.root_centre("clutter", w, h)
    assert not cases.eye_keeps_the_lists(rf.camera_to_array(cam))
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, cam, 4096, 3, rf.make_sky(), 0.25), cases.scene("clutter").rf_scene())
    capfd.readouterr()
    os.environ["RF_DEBUG_PRIMARY_LISTS"] = "1"
    try:
        r.render(32)
        _, acc = r.read_accumulation()
    finally:
        os.environ.pop("RF_DEBUG_PRIMARY_LISTS", None)
    s = r.stats()
    r.close()
    assert acc == 32 and s["primary_list_rays"] == 0 and s["primary_fallback_rays"] == 0 and LINE.findall(capfd.readouterr().err) == []


DEPTHS = [64, 40]                        # a batch in which every wave holds one pixel's samples (the scalar-cache path), and one whose waves straddle pixels (per-lane loads)


@pytest.mark.parametrize("spp", DEPTHS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_walker_over_the_lists_finds_kTraceWides_hits(name, spp):
    """the AOVs on: kTraceLeafLists, then kTraceWide over what it hands on"""
    case = cases.BY_NAME[name]
    _, on = lists._off_on(cases.scene(case.scene).rf_scene(), case.w, case.h, cases.camera(case)[0], (spp,), options=_capacity(case))
    assert on["stats"]["primary_list_rays"] == case.w * case.h * spp
    assert on["stats"]["primary_fallback_rays"] == spp * cases.restated(name).without


@pytest.mark.parametrize("spp", DEPTHS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_fused_kernel_finds_kTraceWides_hits(name, spp):
    """the AOVs off: kPrimaryFused, then kTraceWide and the listed kShade over what it hands on"""
    case = cases.BY_NAME[name]
    _, on = fused._off_on(cases.scene(case.scene).rf_scene(), case.w, case.h, cases.camera(case)[0], (spp,), options=_capacity(case))
    assert on["stats"]["primary_fused_rays"] == case.w * case.h * spp
    assert on["stats"]["primary_fallback_rays"] == spp * cases.restated(name).without


ORACLE_CASES = ["octant0_30_duck", "leaf_corner_boxes", "octant2_30_slivers", "octant3_30_duplicates", "octant4_30_clutter", "far_near_camera"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_one_camera_per_scene_kind_is_bit_identical_to_the_oracle(name):
    case = cases.BY_NAME[name]
    w, h, spp, bounces = 24, 16, 32, 2
    cam, cam19 = cases.camera(case, w, h)
    sd = cases.scene(case.scene)
    with np.errstate(all="ignore"):
        ref, st = orc.render(sd.oracle_scene(), orc.make_render_params(w, h, cam19, 4096, bounces, 0.25, rf.aligned_sky_state(rf.make_sky())), 0, spp)
    walker = lists._render(sd.rf_scene(), w, h, cam, (spp,), True, bounces=bounces)
    one_kernel = fused._render(sd.rf_scene(), w, h, cam, (spp,), True, bounces=bounces)
    assert walker["stats"]["primary_list_rays"] == one_kernel["stats"]["primary_fused_rays"] == w * h * spp
    for on in (walker, one_kernel):
        assert on["stats"]["closest_rays"] == st.closestRays
        g = on["img"][..., :3].view(np.float32)
        assert np.array_equal(np.isnan(g), np.isnan(ref[..., :3]))
        assert ((on["img"][..., :3] == bits(ref[..., :3])) | np.isnan(g)).all()


# ---------------------------------------------------------------------------------------------------------------- the hand-over under every record layout
NO_QUAD = (("quad_from_bounce", 0), ("quad_shadow_from_bounce", 0))
LAYOUTS = {
    "quad_off": NO_QUAD,
    "quad_from_3": (("quad_from_bounce", 3),),
    "quad_shadow_from_2": (("quad_from_bounce", 0), ("quad_shadow_from_bounce", 2)),
    "compact": NO_QUAD + (("compact_from_bounce", 1), ("compact_shadow_from_bounce", 1)),
    "hot": NO_QUAD + (("hot_from_bounce", 1), ("hot_shadow_from_bounce", 1)),
    "quad_half_off": (("quad_half_from_bounce", 0), ("quad_half_shadow_from_bounce", 0)),
    "quad_half_1": (("quad_half_from_bounce", 1), ("quad_half_shadow_from_bounce", 1)),
    "quad_half_3": (("quad_half_from_bounce", 3), ("quad_half_shadow_from_bounce", 2)),
    "quad_local_1": (("quad_half_from_bounce", 0), ("quad_half_shadow_from_bounce", 0), ("quad_local_from_bounce", 1), ("quad_local_shadow_from_bounce", 1)),
    "quad_local_behind_half": (("quad_half_from_bounce", 3), ("quad_half_shadow_from_bounce", 0), ("quad_local_from_bounce", 1), ("quad_local_shadow_from_bounce", 2)),
    "shade_sort_0": (("shade_sort_from_bounce", 0),),
    "shade_sort_1": (("shade_sort_from_bounce", 1),),
    "shade_sort_2": (("shade_sort_from_bounce", 2),),
}
DROPS_THE_LISTS = set()                  # (rf_launch_policy.cpp, planBatch: none of these options is among the lists' conditions; every layout's primary launch is kTraceWide)
KEEPS_THREE_LAUNCHES = {"shade_sort_1"}  # (a sorted kShade at bounce 1 is not the shade launch kPrimaryFused stands in for)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", ["axis+x_odd_duck", "capacity2_duck"])
def test_the_hand_over_under_every_record_layout(name, layout):
    """primary_lists off against on under the option set: with the AOVs on (kTraceLeafLists -> kTraceWide through rayList -> kShade) and with them off, where the
    default is the fused kernel (kPrimaryFused -> kTraceWide through rayList -> the listed kShade)"""
    case = cases.BY_NAME[name]
    sc, (cam, _) = cases.scene(case.scene).rf_scene(), cases.camera(case)
    options = LAYOUTS[layout] + _capacity(case)
    steps, rays = (40,), case.w * case.h * 40
    _, on = lists._off_on(sc, case.w, case.h, cam, steps, options=options)
    off = fused._render(sc, case.w, case.h, cam, steps, True, options=options + (("primary_lists", 0),))
    one = fused._render(sc, case.w, case.h, cam, steps, True, options=options + (("primary_lists", 1),))
    print(f"{name} {layout}: fused rays {one['stats']['primary_fused_rays']}, list rays {one['stats']['primary_list_rays']}, handed on {one['stats']['primary_fallback_rays']}")
    assert np.array_equal(off["img"], one["img"]) and off["closest"] == one["closest"] and off["hits"] == one["hits"]
    for k in ("primary_rays", "closest_rays", "shadow_rays", "shadow_rays_self_answered", "abandoned_rays"):
        assert off["stats"][k] == one["stats"][k], k
    assert off["stats"]["primary_list_rays"] == off["stats"]["primary_fused_rays"] == 0
    for s in (on["stats"], one["stats"]):
        if layout in DROPS_THE_LISTS:
            assert s["primary_list_rays"] == 0
        else:
            assert s["primary_list_rays"] == rays and 0 < s["primary_fallback_rays"] < rays
            assert s["primary_fallback_rays"] == 40 * cases.restated(name).without
    assert one["stats"]["primary_fused_rays"] == (0 if layout in DROPS_THE_LISTS | KEEPS_THREE_LAUNCHES else rays)
