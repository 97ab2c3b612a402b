"""The scenes of the scene-packing characterisation (tests/test_scene_pack.py; the parent's recording of them: tests/golden/scene_pack_parent.json, made by
profiles/scene_pack/record.py): the smallest scenes that take each branch of packScene (rayfinder_amd/csrc/rf_scene_pack.cpp), and the writer of the raw scene file
tests/scene_pack_main.cpp reads.  Every scene is (nodes[NODE_DTYPE], positions [n, 12] f32, attributes [n, 20] f32, textures [(u32 pixels, w, h)]); every seed
is fixed, so a scene is the same bytes in every process.

BRANCH[name] states what the scene is there to show, as {field of the program's line: value, or a predicate over it}."""
import struct

import numpy as np

import bvh_soups
import rayfinder_amd as rf
import scale_scenes as ss
from conftest import DUCK

EMPTY = 0xCBF29CE484222325                  # FNV-1a of no bytes: an array that is not there
WIDE_NONE = 0xFFFFFFFF


def _absent(v):
    return v == [0, f"{EMPTY:016x}"]


def _present(v):
    return v[0] > 0


def _from_pt(pt):
    a = pt.arrays()
    return a["bvhNodes"], a["trianglePositionAttributes"], a["triangleVertexAttributes"], a["baseColorTextures"]


def _attributes(tris9, texture_indices=None):
    """[n, 9] positions -> the 48-byte position attributes and 80-byte vertex attributes (normal +y, the unit uv triangle)"""
    n = tris9.shape[0]
    pos = np.zeros((n, 12), np.float32)
    pos.reshape(n, 3, 4)[:, :, :3] = tris9.reshape(n, 3, 3)
    att = np.zeros((n, 20), np.float32)
    att.reshape(n, 20)[:, [1, 5, 9]] = 1.0
    att[:, 12:18] = np.array([0, 0, 1, 0, 0, 1], np.float32)
    att.view(np.uint32)[:, 18] = 0 if texture_indices is None else texture_indices
    return pos, att


WHITE = [(np.array([0xFFC8B4A0], np.uint32), 1, 1)]


def _hand_tree(boxes, links):
    """boxes: [(lo, hi)] per node; links: per node ("interior", secondChildOffset, axis) or ("leaf", trianglesOffset, count)"""
    nodes = np.zeros(len(boxes), dtype=rf.NODE_DTYPE)
    for i, ((lo, hi), (kind, a, b)) in enumerate(zip(boxes, links)):
        nodes[i]["min"], nodes[i]["max"] = lo, hi
        if kind == "interior":
            nodes[i]["secondChildOffset"], nodes[i]["splitAxis"] = a, b
        else:
            nodes[i]["trianglesOffset"], nodes[i]["triangleCount"], nodes[i]["splitAxis"] = a, b, 0xFFFFFFFF
    return nodes


def _box_triangles(boxes):
    """one triangle per box, spanning it"""
    return np.array([[lo[0], lo[1], lo[2], hi[0], lo[1], hi[2], lo[0], hi[1], hi[2]] for lo, hi in boxes], np.float32)


def _two_leaves(root, left, right, right_offset=1):
    nodes = _hand_tree([root, left, right], [("interior", 2, 0), ("leaf", 0, 1), ("leaf", right_offset, 1)])
    return nodes, *_attributes(_box_triangles([left, right][:right_offset + 1])), WHITE


def duck():
    return _from_pt(rf.PtFormat.from_gltf(DUCK))


def one_triangle():
    return _from_pt(ss.soup_pt(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)))


def big_leaf():
    return _from_pt(ss.soup_pt(bvh_soups.soup("same_centroid_255_plus_500")[1]))


def shared_first_triangle():
    # both leaves name triangle 0: one slot cannot hold two exact boxes
    return _two_leaves(((-1.5, -0.5, -0.5), (1.5, 0.5, 0.5)), ((-1.5, -0.5, -0.5), (-0.5, 0.5, 0.5)), ((0.5, -0.5, -0.5), (1.5, 0.5, 0.5)), right_offset=0)


def nan_and_inverted_boxes():
    nodes, pos, att, tex = _from_pt(ss.soup_pt(bvh_soups.uniform(np.random.default_rng(41), 40, half=3.0)))
    leaves = np.nonzero(nodes["triangleCount"] > 0)[0]
    nodes[leaves[3]]["max"][1] = np.nan
    lo, hi = nodes[leaves[7]]["min"][0], nodes[leaves[7]]["max"][0]
    nodes[leaves[7]]["min"][0], nodes[leaves[7]]["max"][0] = hi + np.float32(0.5), lo        # inverted on x
    return nodes, pos, att, tex


def parent_box_not_the_union():
    # the root's box is larger than the union of its children (tests/test_host_core.py builds the same tree)
    return _two_leaves(((-5, -5, -5), (5, 5, 5)), ((-1.5, -0.5, -0.5), (-0.5, 0.5, 0.5)), ((0.5, -0.5, -0.5), (1.5, 0.5, 0.5)))


def small_far_from_the_origin():
    return _from_pt(ss.soup_pt(ss.triangles("small_at_6e4")))


def beyond_binary16():
    return _from_pt(ss.soup_pt(ss.triangles("centred_1e6")))


def tiny_triangles():
    # leaves of a few thousandths of a unit in a scene 20 units wide: the occluder cache remembers records above the leaves
    return _from_pt(ss.soup_pt(bvh_soups.uniform(np.random.default_rng(42), 600, half=10.0, edge=0.004)))


def no_texture():
    nodes, pos, att, _ = one_triangle()
    return nodes, pos, att, []


def two_textures():
    rng = np.random.default_rng(43)
    tris = bvh_soups.uniform(rng, 24, half=2.0)
    tex = [(rng.integers(0, 2 ** 32, 6, dtype=np.uint64).astype(np.uint32), 2, 3), (rng.integers(0, 2 ** 32, 5, dtype=np.uint64).astype(np.uint32), 5, 1)]
    n = tris.shape[0]
    pt = rf.PtFormat.from_triangles(tris, np.tile(np.array([0, 1, 0], np.float32), (n, 3)), np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (n, 1)),
                                    (np.arange(n) % 2).astype(np.uint32), tex)
    return _from_pt(pt)


SCENES = {f.__name__: f for f in (duck, one_triangle, big_leaf, shared_first_triangle, nan_and_inverted_boxes, parent_box_not_the_union, small_far_from_the_origin,
                                  beyond_binary16, tiny_triangles, no_texture, two_textures)}

_EVERY_LAYOUT = {k: _present for k in ("wide.nodes", "wide.compact", "wide.hot", "wide.own", "wide.quad", "wide.quadHalf", "wide.quadLocal", "wide.oct")}
BRANCH = {
    "duck": {**_EVERY_LAYOUT, "texels": lambda v: v[0] > 1, "check.flags": 127, "facts.occluderHintLevels": 0, "facts.quadHalfFromBounce": 1},
    "one_triangle": {"wide.rootLeaf": lambda v: v != WIDE_NONE, "wide.quad": _absent, "wide.compact": _absent, "wide.hot": _absent, "check.flags": 1},
    "big_leaf": {"wide.bigLeaves.first.count": lambda v: v >= 8, "facts.maxLeafTriangles": lambda v: v >= 8, "wide.rootLeaf": WIDE_NONE},
    "shared_first_triangle": {"facts.leafBoxesValid": False, "wide.quad": _present, "wide.quadHalf": _absent, "wide.quadLocal": _absent, "wide.oct": _absent,
                              "check.flags": 127,      # (the check builds them; the packing dropped them)
                              "facts.quadHalfFromBounce": 0, "facts.quadHalfShadowFromBounce": 0, "facts.quadLocalFromBounce": 0,
                              "facts.quadLocalShadowFromBounce": 0, "facts.octFromBounce": 0},
    "nan_and_inverted_boxes": {"facts.wideUsable": False, "facts.selfShadowOk": False, "wide.boxesRegular": False},
    "parent_box_not_the_union": {"wide.compact": _absent, "wide.hot": _absent, "wide.own": _absent, "wide.compactUsable": False, "wide.hotUsable": False,
                                 "wide.quad": _present, "facts.wideUsable": True},
    "small_far_from_the_origin": {"wide.quadHalf": _present, "facts.quadHalfFromBounce": 0, "facts.quadLocalFromBounce": 2, "facts.quadLocalShadowFromBounce": 0,
                                  "wide.quadLocal": _present},
    "beyond_binary16": {"wide.quadHalf": _absent, "facts.quadHalfFromBounce": 0, "facts.quadLocalFromBounce": 2, "facts.quadLocalShadowFromBounce": 0,
                        "wide.quadLocal": _present},
    "tiny_triangles": {"facts.occluderHintLevels": lambda v: v > 0},
    "no_texture": {"texels": lambda v: v[0] == 1, "textureDescriptors": lambda v: v[0] == 1, "textureDescriptors.last.offset": 0},
    "two_textures": {"texels": lambda v: v[0] == 11, "textureDescriptors": lambda v: v[0] == 2, "textureDescriptors.last.offset": 6},
}
assert set(BRANCH) == set(SCENES)


def write_scene(path, scene):
    nodes, pos, att, textures = scene
    nodes = np.ascontiguousarray(nodes, rf.NODE_DTYPE)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 12)
    att = np.ascontiguousarray(att, np.float32).reshape(-1, 20)
    assert pos.shape[0] == att.shape[0] and nodes.dtype.itemsize == 48
    with open(path, "wb") as f:
        f.write(b"RFSCENE1" + struct.pack("<QQQ", nodes.shape[0], pos.shape[0], len(textures)))
        f.write(nodes.tobytes() + pos.tobytes() + att.tobytes())
        for px, w, h in textures:
            px = np.ascontiguousarray(px, np.uint32)
            assert px.size == w * h
            f.write(struct.pack("<II", w, h) + px.tobytes())


def write_all(directory):
    """-> the paths, in SCENES' order"""
    paths = []
    for name, make in SCENES.items():
        paths.append(str(directory / f"{name}.scene"))
        write_scene(paths[-1], make())
    return paths
