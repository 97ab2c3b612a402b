"""The cameras, scenes, frames and capacities at which bounce 1's per-pixel leaf lists are swept -- one table for tests/test_leaf_lists_restatement.py (CPU: is a list a
superset of every ray's visits, in the reference's order?) and tests/test_gpu_leaf_lists_sweep.py (GPU: are the kernel's lists those of the restatement, and the hits
those of kTraceWide?).

A case is a scene, a camera (a function of the frame: the aspect ratio goes into it), a frame, a capacity and a tag:
    covering    the lists carry the frame: by the restatement at most half the pixels are without a list and the mean list length is at least 1;
    falls_back  the case was written for the hand-over: `expect` names what the restatement must show -- ("without", share): at least that share of the pixels without
                a list; ("empty", share): at least that share of the LISTS empty (the pixels look past the scene).
Both are conditions on the inputs (tests/test_leaf_lists_restatement.py asserts them): a case that misses its tag is a case to change.

In the cameras c is the centre of the root box and R its diagonal."""
import collections
import functools

import numpy as np

import rayfinder_amd as rf
import scale_scenes
from conftest import DUCK
from oracle import orc

Case = collections.namedtuple("Case", "name scene camera w h capacity tag expect")
SMALL = (24, 20)                                                       # the CPU soundness test walks rays at no more than this many pixels
FAR_ROW = "unit_at_6e4"


class SceneData:
    """A scene's reference arrays (nodes: NODE_DTYPE records; positions48: [n, 12] f32) and, made on demand, the device's and the oracle's scene over them"""

    def __init__(self, pt, nodes=None):
        self.pt, self.arrays = pt, pt.arrays()
        self.nodes = self.arrays["bvhNodes"] if nodes is None else nodes
        self.positions48 = self.arrays["trianglePositionAttributes"]
        self.own_tree = nodes is not None

    def textures(self):
        return [(px, tw, th) for (px, tw, th) in self.arrays["baseColorTextures"]]

    def rf_scene(self):
        if not self.own_tree:
            return self.pt.scene()
        return rf.scene_from_arrays(self.nodes, self.positions48, self.arrays["triangleVertexAttributes"], self.textures())

    def oracle_scene(self):
        descs, off = [], 0
        for (px, tw, th) in self.textures():
            descs.append((tw, th, off))
            off += px.size
        return orc.OracleScene(self.nodes, self.positions48, self.arrays["triangleVertexAttributes"], np.array(descs, np.uint32), np.concatenate([px for (px, _, _) in self.textures()]))


def _soup(P, colours=(0xFFB4A0C8,), tex_index=None):
    n = P.shape[0]
    N = np.tile(np.array([0, 1, 0], np.float32), (n, 3))
    UV = np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (n, 1))
    return rf.PtFormat.from_triangles(P.reshape(n, 9).astype(np.float32), N, UV, np.zeros(n, np.uint32) if tex_index is None else tex_index,
                                      [(np.array([c], np.uint32), 1, 1) for c in colours])


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> SceneData.  The Duck; the four kinds of tests/test_gpu_parity.py's random scenes at fixed seeds ("duplicates": thirty copies of each triangle, so every leaf
    is an unsplittable one of more than seven and is handed on); "copies": the same recipe with about three copies each, leaves the lists can hold; "tie": two coincident
    triangles in two leaves under a hand-made root, where the visit order decides the winner; one scale_scenes row far from the origin"""
    if name == "duck":
        return SceneData(rf.PtFormat.from_gltf(DUCK))
    if name == "far":
        return SceneData(scale_scenes.soup_pt(scale_scenes.triangles(FAR_ROW)))
    if name == "copies":
        rng = np.random.default_rng(15)
        base = rng.uniform(-2, 2, (150, 1, 3)) + rng.normal(0, 0.5, (150, 3, 3))
        return SceneData(_soup(base[rng.integers(0, 150, 450)]))
    if name == "tie":
        tri = np.array([[-1.0, -0.8, 0.1], [1.0, -0.7, -0.2], [0.1, 0.9, 0.3]])
        pt = _soup(np.stack([tri, tri]), colours=(0xFF2020E0, 0xFF20E020), tex_index=np.array([0, 1], np.uint32))
        lo, hi = tri.min(0).astype(np.float32), tri.max(0).astype(np.float32)
        nodes = np.zeros(3, rf.NODE_DTYPE)
        for i in range(3):
            nodes[i]["min"], nodes[i]["max"] = lo, hi
        nodes[0]["secondChildOffset"], nodes[0]["splitAxis"] = 2, 0
        nodes[1]["trianglesOffset"], nodes[1]["triangleCount"] = 0, 1
        nodes[2]["trianglesOffset"], nodes[2]["triangleCount"] = 1, 1
        return SceneData(pt, nodes)
    import test_gpu_parity
    seed = {"boxes": 11, "slivers": 12, "duplicates": 13, "clutter": 14}[name]
    return SceneData(test_gpu_parity._random_scene(np.random.default_rng(seed), name))


def root(name):
    n = scene(name).nodes[0]
    lo, hi = n["min"].astype(np.float64), n["max"].astype(np.float64)
    return 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))


def _camera(eye, target, focus, vfov_degrees, w, h):
    return rf.create_camera(np.asarray(eye, np.float64), np.asarray(target, np.float64), 0.0, float(focus), float(orc.degrees_to_radians(vfov_degrees)), w / h)


def octant(sx, sy, sz, vfov, focus=None, away=None):
    """from c + (sx, 0.8 sy, 1.2 sz) R at c: at a narrow field of view every pixel direction lies strictly inside one octant.  away: along the same direction, but
    that many R from c"""
    def make(name, w, h):
        c, R = root(name)
        offset = np.array([sx, 0.8 * sy, 1.2 * sz])
        eye = c + offset * R * (1.0 if away is None else away / np.linalg.norm(offset))
        return _camera(eye, c, np.linalg.norm(eye - c) if focus is None else focus, vfov, w, h)
    return make


AXIS_DISTANCE = {"duck": 1.2, "boxes": 0.3, "copies": 1.2, "clutter": 0.4}


def axis(ax, sign, vfov=40.0, distance=1.2):
    """exactly along +-x or +-z: eye - target is exactly (d, 0, 0) or (0, 0, d) (both on the 1/8 grid), so two direction components cross zero in the middle of the
    frame -- on a pixel edge in an even frame, inside a pixel in an odd one.  d = ceil(distance * R)"""
    def make(name, w, h):
        c, R = root(name)
        c = np.round(c * 8) / 8
        c[c == 0.0] = 0.125                                            # (an origin with a zero component keeps the old launches: BatchPlan::constOrigin)
        d = float(np.ceil(distance * R))
        eye = c.copy()
        eye[ax] -= sign * d
        return _camera(eye, c, d, vfov, w, h)
    return make


def telephoto(focus=None):
    """0.6 degrees from 100 R away"""
    def make(name, w, h):
        c, R = root(name)
        eye = c + np.array([1.0, 0.8, 1.2]) / np.linalg.norm([1.0, 0.8, 1.2]) * 100.0 * R
        return _camera(eye, c, np.linalg.norm(eye - c) if focus is None else focus, 0.6, w, h)
    return make


def leaf_corner(name, w, h):
    """the eye exactly on the min corner of a leaf's box, read from the node array (so it is representable): plane - origin is 0 on three axes for that box"""
    nodes = scene(name).nodes
    leaves = np.flatnonzero(nodes["triangleCount"] > 0)
    c, R = root(name)
    leaf = nodes[leaves[len(leaves) // 2]]
    eye = leaf["min"].astype(np.float64)
    assert (eye != 0.0).all()
    return _camera(eye, c + np.array([0.31, 0.17, 0.23]) * R, R, 60.0, w, h)


def root_centre(name, w, h):
    """inside many boxes: every near plane lies behind the eye"""
    c, R = root(name)
    return _camera(c, c + np.array([1.0, 0.8, 1.2]) * R, R, 60.0, w, h)


def on_flat_box(name, w, h):
    """the eye on the plane of a zero-thickness leaf box (axis-aligned geometry), looking along that plane at the box"""
    nodes = scene(name).nodes
    c, R = root(name)
    flat = [(i, a) for i in np.flatnonzero(nodes["triangleCount"] > 0) for a in (0, 2) if nodes[i]["min"][a] == nodes[i]["max"][a]]
    i, a = flat[len(flat) // 2]
    lo, hi = nodes[i]["min"].astype(np.float64), nodes[i]["max"].astype(np.float64)
    target = 0.5 * (lo + hi)
    eye = target + np.array([0.0, 0.03 * R, 0.0])
    eye[2 - a] += 0.08 * R                                             # (a is x or z: step back along the other one, stay ON the plane along a)
    eye[a] = target[a] = lo[a]
    return _camera(eye, target, np.linalg.norm(eye - target), 50.0, w, h)


def tie_view(sign):
    """the tie scene from the side on which the root's first / second child is the near one"""
    def make(name, w, h):
        return _camera((sign * 2.5, 0.3, 2.0), (0.0, 0.05, 0.05), 3.0, 32.0, w, h)
    return make


def _cases():
    C = []

    def add(name, scene_name, camera, w, h, capacity=64, tag="covering", expect=None):
        C.append(Case(name, scene_name, camera, w, h, capacity, tag, expect))

    # octant views at 30 degrees: every direction of the frame in one octant, one view from each of the eight
    octants = [(1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1)]
    narrow = ("duck", "copies", "slivers", "far", "clutter", "duck", "copies", "slivers")
    for k, (sx, sy, sz) in enumerate(octants):
        w, h = ((33, 40), (24, 20), (25, 19), (48, 40))[k % 4]
        add(f"octant{k}_30_{narrow[k]}", narrow[k], octant(sx, sy, sz, 30.0), w, h)
    # ... and at 110 degrees, where the frame reaches into the neighbouring octants and most pixels look past the scene (lists that exist and hold nothing)
    wide = ("boxes", "clutter", "duck", "far", "slivers", "copies")
    for k, (sx, sy, sz) in enumerate(octants[:6]):
        w, h = ((24, 20), (25, 19), (40, 33))[k % 3]
        add(f"octant{k}_110_{wide[k]}", wide[k], octant(sx, sy, sz, 110.0), w, h, tag="falls_back", expect=("empty", 0.5))
    # the unsplittable leaves of "duplicates" (thirty coincident triangles each): whoever sees geometry is handed on for a big leaf
    add("octant3_30_duplicates", "duplicates", octant(1, 1, -1, 30.0), 48, 40, tag="falls_back", expect=("without", 0.25))
    add("octant5_110_duplicates", "duplicates", octant(-1, 1, -1, 110.0), 25, 19, tag="falls_back", expect=("without", 0.25))
    # exactly along an axis, an even and an odd frame each
    for k, (ax, sign, label) in enumerate(((0, 1, "+x"), (0, -1, "-x"), (2, 1, "+z"), (2, -1, "-z"))):
        sc = ("duck", "boxes", "copies", "clutter")[k]
        add(f"axis{label}_even_{sc}", sc, axis(ax, sign, distance=AXIS_DISTANCE[sc]), 24, 20)
        add(f"axis{label}_odd_{sc}", sc, axis(ax, sign, distance=AXIS_DISTANCE[sc]), 25, 19)
    add("axis+z_even_duplicates", "duplicates", axis(2, 1), 24, 20, tag="falls_back", expect=("without", 0.25))
    # very wide: from the octant view's distance and, at 170 degrees, from 0.3 R away the lists that exist are almost all empty; at 150 degrees from 0.3 R the Duck
    # still fills the middle of the frame with long lists under pixels a quarter of the frame wide
    add("octant0_150_duck", "duck", octant(1, 1, 1, 150.0), 32, 24, tag="falls_back", expect=("empty", 0.9))
    add("wide150_duck", "duck", octant(1, 1, 1, 150.0, away=0.3), 32, 24)
    add("wide170_duck", "duck", octant(-1, 1, -1, 170.0, away=0.3), 32, 24, tag="falls_back", expect=("empty", 0.9))
    add("wide170_boxes", "boxes", octant(1, 1, -1, 170.0, away=0.3), 33, 25, tag="falls_back", expect=("empty", 0.9))
    # telephoto
    add("tele_duck", "duck", telephoto(), 32, 24)
    add("tele_focus1_duck", "duck", telephoto(1.0), 32, 24)
    add("tele_slivers", "slivers", telephoto(), 25, 19)
    # focus distances on an octant view: the camera vectors shrink and grow, the directions stay
    add("focus1e-3_duck", "duck", octant(1, 1, 1, 30.0, focus=1e-3), 32, 24)
    add("focus1e4_duck", "duck", octant(1, 1, 1, 30.0, focus=1e4), 32, 24)
    add("focus1e-3_copies", "copies", octant(-1, 1, 1, 30.0, focus=1e-3), 24, 20)
    # eyes in special places
    for sc in ("duck", "boxes", "copies"):
        add(f"leaf_corner_{sc}", sc, leaf_corner, 32, 24)
    add("leaf_corner_duplicates", "duplicates", leaf_corner, 32, 24, tag="falls_back", expect=("without", 0.9))
    for sc in ("duck", "slivers", "far"):                              # (not "clutter": its root box is centred on x = z = 0, and see eye_keeps_the_lists)
        add(f"root_centre_{sc}", sc, root_centre, 32, 24)
    add("on_flat_box_boxes", "boxes", on_flat_box, 32, 24)
    add("on_flat_box_boxes_odd", "boxes", on_flat_box, 33, 25)
    # two coincident triangles in two leaves: the order of the list decides which one a ray keeps
    add("tie_from+x", "tie", tie_view(1.0), 24, 20)
    add("tie_from-x", "tie", tie_view(-1.0), 25, 19)
    # far from the origin: the rounding margin 64 ulp (M / |D| + 1) with M = 6e4; a short focus distance drives it up until hardly a pixel keeps its signs or its room
    add("far_near_camera", "far", octant(1, 1, 1, 40.0), 32, 24)
    add("far_focus1", "far", octant(1, 1, 1, 40.0, focus=1.0), 32, 24, tag="falls_back", expect=("without", 0.9))
    add("far_focus30", "far", octant(-1, 1, 1, 40.0, focus=30.0), 32, 24)
    # frames of one pixel, one row, one column
    add("frame_1x1_duck", "duck", octant(1, 1, 1, 30.0), 1, 1, tag="falls_back", expect=("without", 1.0))
    add("frame_40x1_duck", "duck", octant(1, 1, 1, 30.0), 40, 1, tag="falls_back", expect=("without", 1.0))
    add("frame_1x40_duck", "duck", octant(1, 1, 1, 30.0), 1, 40)
    add("frame_1x40_clutter", "clutter", octant(1, -1, 1, 30.0), 1, 40)
    # capacities: lists that overflow at once
    add("capacity2_duck", "duck", lambda name, w, h: rf.fly_camera(w, h), 40, 33, capacity=2, tag="falls_back", expect=("without", 0.3))
    add("capacity1_duck", "duck", octant(1, 1, 1, 30.0), 33, 40, capacity=1, tag="falls_back", expect=("without", 0.3))
    add("capacity2_copies", "copies", octant(-1, 1, 1, 30.0), 24, 20, capacity=2, tag="falls_back", expect=("without", 0.3))
    add("capacity1_slivers", "slivers", octant(1, 1, -1, 30.0), 25, 19, capacity=1, tag="falls_back", expect=("without", 0.3))
    add("fly_duck", "duck", lambda name, w, h: rf.fly_camera(w, h), 48, 40)
    assert len({c.name for c in C}) == len(C)
    return C


CASES = _cases()
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


def camera(case, w=None, h=None):
    """the case's camera for its own frame (or another one) -> (rf camera, its 19 floats)"""
    cam = case.camera(case.scene, case.w if w is None else w, case.h if h is None else h)
    return cam, rf.camera_to_array(cam)


def eye_keeps_the_lists(cam19):
    """planBatch's condition on the camera (rf_launch_policy.cpp, BatchPlan::constOrigin): a pinhole whose origin has no zero component"""
    return bool(cam19[18] == 0.0 and (cam19[:3] != 0.0).all())


def small_frame(case):
    """the case's frame, or its corner of SMALL where it is larger (the camera follows: its aspect ratio is the frame's)"""
    return (case.w, case.h) if case.w * case.h <= SMALL[0] * SMALL[1] else (min(case.w, SMALL[0]), min(case.h, SMALL[1]))


@functools.lru_cache(maxsize=None)
def restated(name, small=False):
    """the restatement's lists for a case, computed once per process -> PixelLists"""
    import leaf_lists_restatement as restatement
    case = BY_NAME[name]
    w, h = small_frame(case) if small else (case.w, case.h)
    return restatement.pixel_leaf_lists(scene(case.scene).nodes, camera(case, w, h)[1], w, h, case.capacity)
