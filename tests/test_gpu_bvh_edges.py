"""GPU BVH builder (rf_bvh_gpu.hip) at its size thresholds and value edges (-m gpu), on the soups of bvh_soups.py.

Every case: GPU nodes == host nodes == oracle nodes byte for byte, the same triangle permutation, the same depth, a valid
tree by bvh_invariants.check_tree (which knows no builder), and a second GPU build with the same bytes (the mixed-workgroup
global-atomics path of kHistogram is the part that could vary).  test_bvh_invariants.py has already shown, without a GPU,
that host and oracle agree on each of these inputs.

The one documented exception, pinned here instead of merely admitted: where the boxes of a node's triangles hold both -0.0f
and +0.0f at the extreme of a coordinate, the GPU box has -0 for the min and +0 for the max (integer order of the encodings)
and the host keeps the first one its fold met.  zero_sign_differences() allows exactly that and nothing else, computed from the soup, and the
lattice tests show that no ray and no rendered pixel can tell the two trees apart.

Non-finite positions are refused by both builders before the device is touched (profiles/bvh_edges/README.md)."""
import time

import numpy as np
import pytest

import bvh_soups as S
import rayfinder_amd as rf
from bvh_invariants import check_tree, node_ranges
from conftest import bits
from oracle import orc

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
INT_FIELDS = ("trianglesOffset", "secondChildOffset", "triangleCount", "splitAxis")


def zero_sign_differences(tris, host_nodes, gpu_nodes, idx, every_node=False):
    """The strict rule for the sign of zero box coordinates -> number of differing words.
    Equal under float == in every field; integer fields and pads bit-equal; every bit difference at a min / max component in a
    node whose triangles' boxes hold BOTH signs of zero at that extreme (read from the soup), where the GPU has -0 in min, +0 in max.
    every_node: also require the GPU's sign at such places where the host happens to agree."""
    assert len(host_nodes) == len(gpu_nodes)
    for f in host_nodes.dtype.names:
        assert np.array_equal(host_nodes[f], gpu_nodes[f]), f
    for f in INT_FIELDS + ("pad0", "pad1"):
        assert np.array_equal(host_nodes[f].view(np.uint32), gpu_nodes[f].view(np.uint32)), f
    n = len(tris)
    src = np.empty(n, np.int64); src[np.asarray(idx).astype(np.int64)] = np.arange(n)
    ordered = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)[src]                  # leaf order
    # a triangle's own box is the same fold on both sides (v0, v1, v2 in order; a tie, -0 against +0 included, keeps the
    # first): argmin / argmax return the first vertex at the extreme.  The builders differ only in how they fold these boxes.
    tlo = np.take_along_axis(ordered, ordered.argmin(1)[:, None, :], 1)[:, 0, :]
    thi = np.take_along_axis(ordered, ordered.argmax(1)[:, None, :], 1)[:, 0, :]
    first, count, _, _ = node_ranges(gpu_nodes)
    dmin = bits(host_nodes["min"]) != bits(gpu_nodes["min"])
    dmax = bits(host_nodes["max"]) != bits(gpu_nodes["max"])
    look = np.arange(len(gpu_nodes)) if every_node else np.nonzero(dmin.any(1) | dmax.any(1))[0]

    def both_zeros(v):
        z = v[v == 0]
        return len(z) > 0 and np.signbit(z).any() and not np.signbit(z).all()

    for i in look:
        lo, hi = tlo[first[i]:first[i] + count[i]], thi[first[i]:first[i] + count[i]]
        for k in range(3):
            if lo[:, k].min() == 0 and both_zeros(lo[:, k]):
                assert np.signbit(gpu_nodes["min"][i, k]) and gpu_nodes["min"][i, k] == 0, (i, k)
            else:
                assert not dmin[i, k], (i, k, "min differs where the node's triangle boxes do not hold both zeros at the minimum")
            if hi[:, k].max() == 0 and both_zeros(hi[:, k]):
                assert not np.signbit(gpu_nodes["max"][i, k]) and gpu_nodes["max"][i, k] == 0, (i, k)
            else:
                assert not dmax[i, k], (i, k, "max differs where the node's triangle boxes do not hold both zeros at the maximum")
    return int(dmin.sum() + dmax.sum())


def three_way(name, tris, zero_rule=False, oracle=True, allow_nonfinite_area=False):
    t0 = time.perf_counter()
    hn, hi, hd = rf.build_bvh(tris)
    on, oi, od = orc.build_bvh(tris) if oracle else (hn, hi, hd)
    t1 = time.perf_counter()
    gn, gi, gd, ms = rf.build_bvh_gpu(tris)
    gn2, gi2, gd2, ms2 = rf.build_bvh_gpu(tris)
    assert hn.tobytes() == np.ascontiguousarray(on).tobytes() and np.array_equal(hi, oi) and hd == od, name
    differing = 0
    if zero_rule:
        differing = zero_sign_differences(tris, hn, gn, gi)
    else:
        assert len(gn) == len(hn), (name, len(gn), len(hn))
        assert gn.tobytes() == hn.tobytes(), name
    assert np.array_equal(gi, hi), name
    assert gd == hd, (name, gd, hd)
    check_tree(tris, gn, gi, gd, allow_nonfinite_area=allow_nonfinite_area)
    assert gn2.tobytes() == gn.tobytes() and np.array_equal(gi2, gi) and gd2 == gd, (name, "the second GPU build differs")
    print(f"{name}: n {len(tris)}, {len(gn)} nodes, depth {gd}, GPU build {ms:.2f} / {ms2:.2f} ms, references {t1 - t0:.2f} s, "
          f"{differing} zero-sign words")
    return hn, gn, gi, differing


@pytest.mark.parametrize("name", S.names("threshold"))
def test_threshold_sizes(name):
    three_way(*S.soup(name))


@pytest.mark.parametrize("name", S.names("unsplittable"))
def test_unsplittable_boundary(name):
    hn, gn, _, _ = three_way(*S.soup(name))
    k = int(name.split("_")[2 if name.startswith("same") else 1])
    assert int(gn["triangleCount"].max()) == k                      # the k coincident centroids are one leaf, 255 or not


@pytest.mark.parametrize("name", S.names("straddle"))
def test_straddles(name):
    three_way(*S.soup(name))


@pytest.mark.parametrize("name", S.names("partition"))
def test_partition_patterns(name):
    tris = S.soup(name)[1]
    _, gn, gi, _ = three_way(name, tris)
    assert S.partition_ok(len(tris), gn, gi)                        # a stable partition would have given other bytes


@pytest.mark.parametrize("name", S.names("extent_overflow"))
def test_extent_overflow(name):
    three_way(*S.soup(name), allow_nonfinite_area=True)


@pytest.mark.parametrize("name", S.names("other_values"))
def test_other_values(name):
    three_way(*S.soup(name))


@pytest.mark.parametrize("name", S.names("scan_carry"))
def test_scan_carry_sizes(name):
    """More than 1 024 scan blocks: kScanSums' carry loop runs two and three trips.  Against the host builder and check_tree;
    test_bvh_invariants.py compares host and oracle on these two once, on the CPU."""
    three_way(*S.soup(name), oracle=False)


# ---------------------------------------------------------------------------------------------- signed zeros
@pytest.mark.parametrize("name", S.names("signed_zero"))
def test_signed_zeros_follow_the_documented_rule(name):
    tris = S.soup(name)[1]
    hn, gn, gi, differing = three_way(name, tris, zero_rule=True)
    zero_sign_differences(tris, hn, gn, gi, every_node=True)
    if name.endswith("negative"):
        assert differing == 0 and gn.tobytes() == hn.tobytes()      # one sign only: nothing to disagree about


def _lattice_rays(rng, count=20000):
    q = count // 4
    sign = lambda shape: np.where(rng.uniform(size=shape) < 0.5, np.float32(-0.0), np.float32(0.0))
    pick = lambda shape: rng.integers(-7, 8, shape).astype(np.float32) * np.float32(0.5)    # lattice planes and half-way between
    unit = lambda d: d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = []
    # origins with components exactly +-0, on the lattice's zero planes
    o = rng.uniform(-7, 7, (q, 3)).astype(np.float32)
    zero = rng.uniform(size=(q, 3)) < 0.5
    o = np.where(zero, sign((q, 3)), o)
    rays.append(np.concatenate([o, unit(rng.normal(size=(q, 3)))], 1))
    # axis-parallel directions, the other two components +-0, origins on and between the lattice planes
    d = sign((q, 3)); ax = rng.integers(0, 3, q)
    d[np.arange(q), ax] = np.where(rng.uniform(size=q) < 0.5, -1.0, 1.0)
    o = pick((q, 3)); o[np.arange(q), ax] = -9.0 * d[np.arange(q), ax]
    o = np.where(o == 0, sign((q, 3)), o)
    rays.append(np.concatenate([o, d], 1))
    # grazing: inside a zero plane, the direction's component across it +-0
    o = rng.uniform(-7, 7, (q, 3)).astype(np.float32); d = unit(rng.normal(size=(q, 3))).astype(np.float32)
    ax = rng.integers(0, 3, q)
    o[np.arange(q), ax] = sign(q); d[np.arange(q), ax] = sign(q)
    rays.append(np.concatenate([o, unit(d)], 1))
    # and ordinary ones
    o = rng.uniform(-9, 9, (count - 3 * q, 3)); t = rng.uniform(-6, 6, (count - 3 * q, 3))
    rays.append(np.concatenate([o, unit(t - o)], 1))
    return np.concatenate(rays).astype(np.float32)


def test_no_ray_sees_the_zero_sign_difference():
    tris = S.soup("lattice_12x12x4_coin")[1]
    hn, hi, _ = rf.build_bvh(tris)
    gn, gi, _, _ = rf.build_bvh_gpu(tris)
    assert zero_sign_differences(tris, hn, gn, gi) > 0              # the two trees do differ
    ordered = orc.reorder(tris, gi)
    rays = _lattice_rays(np.random.default_rng(41))
    a = orc.intersect_bvh_batch(gn, ordered, rays, 1000.0)
    b = orc.intersect_bvh_batch(hn, ordered, rays, 1000.0)
    assert 0.2 < a["hit"].mean() < 0.95
    for k in ("hit", "tri", "nodesVisited"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("t", "uv"):                                           # uv = (u, v)
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_lattice_bakes_differ_only_in_those_node_bytes_and_render_the_same_image():
    tris = S.soup("lattice_12x12x4_coin")[1]
    n = len(tris)
    rng = np.random.default_rng(42)
    N = np.tile(np.array([0, 0, 1], np.float32), (n, 3))
    T = rng.uniform(0, 1, (n, 6)).astype(np.float32)
    I = rng.integers(0, 2, n).astype(np.uint32)
    textures = [(np.full(16, 0xFF000000 | c, np.uint32), 4, 4) for c in (0xE0C0A0, 0x60A0E0)]
    pt_host = rf.PtFormat.from_triangles(tris, N, T, I, textures)
    rf.set_bake_bvh_builder(0)
    try:
        pt_gpu = rf.PtFormat.from_triangles(tris, N, T, I, textures)
    finally:
        rf.set_bake_bvh_builder(None)
    hn, gn = pt_host.arrays()["bvhNodes"], pt_gpu.arrays()["bvhNodes"]
    assert hn.tobytes() != gn.tobytes()
    sh, sg = pt_host.serialize(), pt_gpu.serialize()
    at = sh.find(hn.tobytes())
    assert at >= 0 and sh.find(hn.tobytes(), at + 1) < 0
    assert sg == sh[:at] + gn.tobytes() + sh[at + len(hn.tobytes()):]      # the node array is the only difference ...
    hi = rf.build_bvh(tris)[1]
    assert zero_sign_differences(tris, hn, gn, hi) > 0                     # ... and there, zero signs by the rule alone
    W, H, spp, bounces = 64, 48, 4, 3
    cam = rf.create_camera((3.0, 4.5, 9.0), (0.0, 0.0, 0.0), 0.0, 1.0, np.radians(60.0), W / H)
    imgs = []
    for pt in (pt_gpu, pt_host):
        r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, spp, bounces, rf.make_sky(), 0.25), pt.scene())
        r.render(spp)
        imgs.append(r.read_accumulation()[0])
        r.close()
    assert np.array_equal(bits(imgs[0]), bits(imgs[1]))
    assert (imgs[0][..., :3] > 0).any() and len(np.unique(bits(imgs[0][..., :3]))) > 100


# ---------------------------------------------------------------------------------------------- non-finite positions
@pytest.mark.parametrize("name", S.names("non_finite"))
def test_gpu_builder_and_gpu_bake_refuse_non_finite_positions(name):
    tris = S.soup(name)[1]
    n = len(tris)
    bad = int(np.nonzero(~np.isfinite(tris).all(axis=1))[0][0])
    with pytest.raises(rf.RayfinderError) as e:
        rf.build_bvh_gpu(tris)
    assert e.value.status == INVALID and f"triangle {bad} " in str(e.value) and "non-finite" in str(e.value)
    rf.set_bake_bvh_builder(0)
    try:
        with pytest.raises(rf.RayfinderError) as e:
            rf.PtFormat.from_triangles(tris, np.zeros((n, 9), np.float32), np.zeros((n, 6), np.float32), np.zeros(n, np.uint32), [])
    finally:
        rf.set_bake_bvh_builder(None)
    assert e.value.status == INVALID and "non-finite" in str(e.value)
    three_way(name + "_finite_rest", tris[np.isfinite(tris).all(axis=1)])      # and the builder is fine afterwards


# ---------------------------------------------------------------------------------------------- seeded soak
FUZZ_SIZES = (1, 2, 3, 5, 17, 63, 64, 65, 129, 255, 256, 257, 1000, 1024, 1025, 5000, 20000, 60000)


def test_forty_seeded_soups_of_random_sizes_and_degeneracies():
    """Random sizes (the thresholds among them), flat / collapsed axes, zero-length edges, duplicates, lattice coordinates:
    GPU == host under the strict zero-sign rule, the same permutation and depth, a valid tree."""
    total = 0
    for seed in range(40):
        rng = np.random.default_rng(7000 + seed)
        n = int(rng.choice(FUZZ_SIZES))
        c = rng.uniform(-10, 10, (n, 1, 3)) * rng.choice([1.0, 0.0, 1e-3], 3)                # flat / collapsed axes now and then
        tris = (c + rng.normal(0, rng.choice([0.0, 1e-4, 0.3]), (n, 3, 3))).astype(np.float32)
        if seed % 3 == 0: tris = tris[rng.integers(0, n, n)]                                   # duplicates
        if seed % 5 == 0: tris = np.round(tris * 4) / 4                                        # lattice coordinates: ties, and both zeros
        tris = np.ascontiguousarray(tris.reshape(-1, 9), np.float32)
        hn, hi, hd = rf.build_bvh(tris)
        gn, gi, gd, _ = rf.build_bvh_gpu(tris)
        total += zero_sign_differences(tris, hn, gn, gi)
        assert np.array_equal(gi, hi) and gd == hd, seed
        check_tree(tris, gn, gi, gd)
    print(f"40 soups: {total} words differing in the sign of a zero, all by the rule")
