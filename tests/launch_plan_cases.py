"""The matrix of the launch-plan characterisation, shared by its two tests: tests/test_gpu_launch_plan.py (rf_renderer_launch_plan on a device) and
tests/test_launch_policy.py (the host-only policy unit, rayfinder_amd/csrc/rf_launch_policy.cpp, through tests/launch_policy_main.cpp).  Both compare with
tests/golden/launch_plan_parent.json, cell by cell; the scenes and cameras below are the ones its recorder built."""
import os

import numpy as np

import rayfinder_amd as rf
from rayfinder_amd import scenes

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


def pt(scene):
    if scene not in _pts:
        _pts[scene] = rf.PtFormat.from_gltf(os.path.join(GOLDEN, "Duck.glb")) if scene == "duck" else scenes.quad_scene()
    return _pts[scene]


def scene_arrays(scene, tree=None):
    """-> (nodes, positions, attributes, textures) of a scene; tree="poke": with the first child's box enlarged beyond the root's"""
    a = pt(scene).arrays()
    nodes = a["bvhNodes"]
    if tree == "poke":
        nodes = nodes.copy()
        nodes[1]["max"] = tuple(np.asarray(nodes[0]["max"]) + np.float32(1.0))
    return nodes, a["trianglePositionAttributes"], a["triangleVertexAttributes"], [(px, w, h) for (px, w, h) in a["baseColorTextures"]]


def camera(scene, case):
    c = CASES[case]
    if c.get("camera") == "far":      # (the camera of test_camera_far_outside_the_scene_keeps_primary_rays_off_the_scalar_path, distance 1000)
        root = pt(scene).arrays()["bvhNodes"][0]
        lo, hi = np.array(root["min"][:3]), np.array(root["max"][:3])
        centre, size, distance = 0.5 * (lo + hi), float(np.max(hi - lo)), 1000.0
        eye = centre + np.array([0.6, 0.4, 0.7]) / np.linalg.norm([0.6, 0.4, 0.7]) * distance * size
        return rf.create_camera(eye, centre, 0.0, 1.0, float(2.0 * np.arctan(0.75 / distance)), W / H)
    if c.get("camera") == "lens":
        return rf.fly_camera(W, H, aperture=0.1)
    return rf.fly_camera(W, H)
