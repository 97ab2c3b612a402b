"""Bounce 1's per-pixel leaf lists, on the host (no GPU): is a pixel's list -- as tests/leaf_lists_restatement.py restates kPixelLeafLists, bit for bit -- a superset of
what ANY primary ray of that pixel visits in the reference's walk, in the reference's order, and made for the ray's signs?  That is what the kernel's claim of
bit-identical hits rests on (rf_primary_lists.hip, head comment); a leaf missing from a list is a wrong image, not a crash.  Over the cameras, scenes, frames and
capacities of tests/leaf_list_cases.py.  A set-and-order property: no tolerance anywhere.

Also here: the case table's own conditions (a "covering" case has lists, a "falls_back" case shows the hand-over it was written for), the restated walk against the
oracle's walk, and the restatement's teeth -- a builder that visits the far child first, or drops a leaf, must be caught by the very same check."""
import functools

import numpy as np
import pytest

import leaf_list_cases as cases
import leaf_lists_restatement as restatement
from oracle import orc

SPP = 4096                                                             # samplesPerPixel of the sweep's handles: the blue-noise pair of frame f is that of sample f
FRAMES = 16
FIXED_POINTS = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.0), (0.5, 1.0), (0.0, 0.5), (1.0, 0.5), (0.5, 0.5)]   # corners, edge midpoints, centre


@functools.lru_cache(maxsize=None)
def _blue_noise():
    """[y, x, frame, 2]: orc.animated_blue_noise for every pixel a case's small frame can hold"""
    table = orc.blue_noise_table()
    w, h = max(cases.small_frame(c)[0] for c in cases.CASES), max(cases.small_frame(c)[1] for c in cases.CASES)
    out = np.zeros((h, w, FRAMES, 2), np.float32)
    for y in range(h):
        for x in range(w):
            for f in range(FRAMES):
                out[y, x, f] = orc.animated_blue_noise(x, y, f, SPP, table)
    return out


def soundness_failures(case, check_walk=False, **mutation):
    """Every pixel of the case's small frame that has a list; per pixel the nine fixed sample points and its own blue-noise pairs of frames 0 .. 15; the rays with kRaygen's
    f32 expressions.  -> (failures [(what, x, y, nx, ny)], rays walked, pixels with a list)"""
    sd = cases.scene(case.scene)
    w, h = cases.small_frame(case)
    cam19 = cases.camera(case, w, h)[1]
    lists = restatement.pixel_leaf_lists(sd.nodes, cam19, w, h, case.capacity, **mutation)
    ys, xs = np.nonzero(lists.reason == restatement.HAS_LIST)
    if len(xs) == 0:
        return [], 0, 0
    fixed = np.array(FIXED_POINTS, np.float32)
    noise = _blue_noise()[ys, xs]                                                                    # [pixels, FRAMES, 2]
    points = np.concatenate([np.broadcast_to(fixed, (len(xs),) + fixed.shape), noise], axis=1)       # [pixels, 25, 2]
    _, directions = restatement.ray_directions(cam19, w, h, xs[:, None], ys[:, None], points[..., 0], points[..., 1])
    pixel = np.repeat(np.arange(len(xs)), points.shape[1])
    directions, points = directions.reshape(-1, 3), points.reshape(-1, 2)
    signs = restatement.ray_signs(directions)
    failures = [("signs", int(xs[pixel[r]]), int(ys[pixel[r]]), float(points[r, 0]), float(points[r, 1])) for r in np.flatnonzero(signs != lists.signs[ys, xs][pixel])]
    for s in np.unique(signs):
        rays = np.flatnonzero(signs == s)
        walk = restatement.reference_walk(sd.nodes, sd.positions48, cam19[:3], directions[rays])
        if check_walk:                                                 # the restated walk IS the oracle's: same hit, same t, same number of nodes and triangles on the way
            ref = orc.intersect_bvh_batch(sd.nodes, sd.positions48, np.concatenate([np.broadcast_to(cam19[:3], (len(rays), 3)), directions[rays]], axis=1), float(restatement.T_MAX))
            hit = walk.tri >= 0
            assert np.array_equal(hit, ref["hit"].astype(bool)) and np.array_equal(walk.tri[hit], ref["tri"][hit].astype(np.int64))
            assert np.array_equal(walk.t[hit].view(np.uint32), ref["t"][hit].view(np.uint32))
            assert np.array_equal(walk.nodes_visited, ref["nodesVisited"]) and np.array_equal(walk.triangle_tests, ref["triTests"])
        for k, r in enumerate(rays):
            x, y = int(xs[pixel[r]]), int(ys[pixel[r]])
            if not restatement.is_subsequence(walk.leaves[k], lists.entries(x, y)):
                failures.append(("visits", x, y, float(points[r, 0]), float(points[r, 1])))
    return failures, len(directions), len(xs)


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_list_holds_every_leaf_a_ray_of_its_pixel_reaches_in_the_references_order(name):
    failures, rays, listed = soundness_failures(cases.BY_NAME[name], check_walk=True)
    print(f"{name}: {listed} pixels with a list, {rays} rays")
    assert failures == []


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_case_is_what_its_tag_says(name):
    """conditions on the INPUTS, by the restatement at the case's own frame: a case that misses them is a case to change"""
    case, lists = cases.BY_NAME[name], cases.restated(name)
    listed = lists.pixels - lists.without
    empty = lists.histogram().get(0, 0)
    print(f"{name}: {lists.pixels} pixels, {lists.without} without a list {lists.reasons()}, mean length {lists.mean_length():.2f}, {empty} of {listed} lists empty")
    assert case.w * case.h <= 48 * 40 and cases.eye_keeps_the_lists(cases.camera(case)[1])
    if case.tag == "covering":
        assert 2 * lists.without <= lists.pixels and lists.mean_length() >= 1.0
    else:
        assert case.tag == "falls_back"
        kind, share = case.expect
        if kind == "without":
            assert lists.without >= share * lists.pixels
        else:
            assert kind == "empty" and listed > 0 and empty >= share * listed


def test_the_table_holds_what_it_was_made_for():
    C = cases.CASES
    assert {c.scene for c in C} >= {"duck", "boxes", "slivers", "duplicates", "clutter", "far"}
    assert {(c.w, c.h) for c in C} >= {(1, 1), (1, 40), (40, 1), (33, 40), (48, 40)}
    assert {c.capacity for c in C} == {64, 2, 1}
    # the reasons the table reaches, and lists at their capacity
    total = {k: sum(cases.restated(c.name).reasons()[k] for c in C) for k in ("signs", "overflow", "big leaf")}
    assert all(v > 0 for v in total.values()), total
    assert any(cases.restated(c.name).histogram().get(c.capacity, 0) > 0 for c in C if c.capacity == 64)
    # the sign patterns of the lists: all eight octants
    patterns = set()
    for c in C:
        lists = cases.restated(c.name)
        patterns |= set(np.unique(lists.signs[lists.reason == restatement.HAS_LIST]).tolist())
    assert patterns == set(range(8))


# ---------------------------------------------------------------------------------------------------------------- the teeth
TIE_CASES = [n for n in cases.NAMES if cases.BY_NAME[n].scene in ("tie", "copies") and cases.BY_NAME[n].tag == "covering"]


@pytest.mark.parametrize("name", TIE_CASES)
def test_a_builder_that_visits_the_far_child_first_is_caught(name):
    """On the scenes with coincident triangles whose leaves the lists can hold ("copies", "tie"; the thirty-fold "duplicates" have no list wherever they show).  The
    unmutated builder passes the same check in the test above."""
    failures, rays, _ = soundness_failures(cases.BY_NAME[name], swap_children=True)
    print(f"{name}: {len(failures)} of {rays} rays caught it")
    assert any(what == "visits" for what, *_ in failures)


@pytest.mark.parametrize("name,k", [("root_centre_duck", 0), ("root_centre_duck", 1), ("root_centre_duck", 5), ("root_centre_far", 0), ("root_centre_far", 5),
                                    ("root_centre_slivers", 1), ("tie_from+x", 0), ("tie_from+x", 1), ("leaf_corner_copies", 5)])
def test_a_builder_that_drops_a_leaf_is_caught(name, k):
    """leaf k of every list dropped, on cases in which the rays do reach leaves (from inside the root box every ray reaches one): each case catches it by itself"""
    failures, rays, _ = soundness_failures(cases.BY_NAME[name], drop_emitted=k)
    print(f"{name}: leaf {k} of every list dropped, {len(failures)} of {rays} rays caught it")
    assert any(what == "visits" for what, *_ in failures)
