"""What a valid tree of the 48-byte node format is, stated with no builder in it (numpy only, vectorised: a few passes over
the node array and the triangle array, no Python loop over nodes or triangles).

check_tree(tris36, nodes, idx, depth) asserts, for nodes in depth-first preorder (contract: src/common/bvh.hpp:23-46):

  permutation   idx (idx[source] = position in leaf order) is a bijection onto 0..n-1
  structure     an interior node's first child is i + 1 and its secondChildOffset is i + 1 + size(first subtree); node 0 covers
                [0, n); the children's ranges are adjacent, non-empty and partition the parent's; the leaves tile [0, n) in preorder
  boxes         a leaf's box is EXACTLY the component-wise f32 min / max of its triangles' vertices, an interior node's the min / max
                of its children's boxes (min / max are exact, so the comparison is `==` on values: -0 == +0, as for a ray)
  fields        pad0 / pad1 are zero bits; a leaf has secondChildOffset 0 and splitAxis 0xFFFFFFFF; an interior node has
                trianglesOffset 0, triangleCount 0 and splitAxis in {0, 1, 2}
  split order   every centroid of the left child is <= every centroid of the right child on the split axis (bucket order implies
                centroid order; the two-triangle median split gives the same)
  depth         the deepest leaf's level, the root at 1
  big leaves    more than 255 triangles in a leaf only if its box has zero area, or its centroids coincide on the widest centroid
                axis, or count * area(box) is not finite in f32 -- the necessary condition of "no finite SAH cost" (every bucket
                cost is at most that product) -- and this last one only with allow_nonfinite_area=True; otherwise it is reported.

Centroids and areas are the builders' own f32 expressions (0.5 * (lo + hi); 2 * ((dx * dy + dx * dz) + dy * dz))."""
import numpy as np

MAX_LEAF = 255
F32 = np.float32


def subtree_ends(nodes):
    """end[i] = one past the last node of i's subtree, by pointer jumping along second children (no recursion).  Asserts
    i + 1 < secondChildOffset < N for interior nodes first, which is what makes the jumps terminate."""
    N = len(nodes)
    ids = np.arange(N, dtype=np.int64)
    leaf = nodes["triangleCount"] > 0
    second = nodes["secondChildOffset"].astype(np.int64)
    inner = ~leaf
    assert np.all((second[inner] > ids[inner] + 1) & (second[inner] < N)), "an interior node's second child is not strictly ahead of its first and inside the array"
    last = np.where(leaf, ids, second)               # -> the rightmost leaf of the subtree
    while True:
        nxt = last[last]
        if np.array_equal(nxt, last):
            break
        last = nxt
    assert np.all(leaf[last])
    return last + 1


def node_ranges(nodes):
    """(first, count, end, level) per node, from the structure alone: triangles in the leaves before / inside the subtree."""
    N = len(nodes)
    end = subtree_ends(nodes)
    cum = np.concatenate([[0], np.cumsum(nodes["triangleCount"].astype(np.int64))])
    first = cum[:-1].copy()
    count = cum[end] - first
    inner = np.nonzero(nodes["triangleCount"] == 0)[0]
    diff = np.bincount(inner + 1, minlength=N + 1) - np.bincount(end[inner], minlength=N + 1)   # +1 over (i, end[i]) per interior i
    level = 1 + np.cumsum(diff[:-1])
    return first, count, end, level


def _area(lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        d = (hi - lo).astype(F32)
        return F32(2.0) * ((d[..., 0] * d[..., 1] + d[..., 0] * d[..., 2]) + d[..., 1] * d[..., 2])


def _max_dimension(lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        d = (hi - lo).astype(F32)
    return np.where((d[..., 0] > d[..., 1]) & (d[..., 0] > d[..., 2]), 0, np.where(d[..., 1] > d[..., 2], 1, 2))


def check_tree(tris36, nodes, idx, depth, allow_nonfinite_area=False):
    tris = np.ascontiguousarray(tris36, F32).reshape(-1, 3, 3)
    n, N = len(tris), len(nodes)
    idx = np.asarray(idx).astype(np.int64)
    ids = np.arange(N, dtype=np.int64)

    # permutation
    assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < n, "triangleIndices out of range"
    seen = np.zeros(n, bool)
    seen[idx] = True
    assert seen.all(), "triangleIndices is not a bijection"

    # fields
    leaf = nodes["triangleCount"] > 0
    inner = ~leaf
    assert not nodes["pad0"].view(np.uint32).any() and not nodes["pad1"].view(np.uint32).any(), "pad0 / pad1 not zero"
    assert np.all(nodes["secondChildOffset"][leaf] == 0), "a leaf with a secondChildOffset"
    assert np.all(nodes["splitAxis"][leaf] == 0xFFFFFFFF), "a leaf whose splitAxis is not 0xFFFFFFFF"
    assert np.all(nodes["trianglesOffset"][inner] == 0), "an interior node with a trianglesOffset"
    assert np.all(nodes["splitAxis"][inner] <= 2), "an interior node whose splitAxis is not 0, 1 or 2"

    # structure
    first, count, end, level = node_ranges(nodes)
    assert end[0] == N, "node 0's subtree is not the whole array"
    assert first[0] == 0 and count[0] == n, "node 0 does not cover [0, n)"
    ii = ids[inner]
    left, right = ii + 1, nodes["secondChildOffset"][ii].astype(np.int64)
    assert np.array_equal(end[left], right), "secondChildOffset is not i + 1 + size(first subtree)"
    assert np.array_equal(end[right], end[ii]), "the second subtree does not end where its parent's does"
    assert np.all((count[left] > 0) & (count[right] > 0)), "an empty child"
    assert np.array_equal(first[left], first[ii]) and np.array_equal(first[right], first[left] + count[left]) and \
        np.array_equal(count[left] + count[right], count[ii]), "the children do not partition the parent's range"
    li = ids[leaf]
    assert np.array_equal(nodes["trianglesOffset"][li].astype(np.int64), first[li]), "the leaves do not tile [0, n) in preorder"
    assert int(level[li].max()) == depth, f"depth {depth} but the deepest leaf is at level {int(level[li].max())}"

    # boxes: leaves from the triangles, interior nodes from their children
    lo_t, hi_t = tris.min(axis=1), tris.max(axis=1)
    with np.errstate(over="ignore"):
        c_t = (F32(0.5) * (lo_t + hi_t)).astype(F32)
    lo_s = np.empty_like(lo_t); hi_s = np.empty_like(hi_t); c_s = np.empty_like(c_t)
    lo_s[idx], hi_s[idx], c_s[idx] = lo_t, hi_t, c_t          # leaf order
    starts = first[li]
    assert np.array_equal(np.minimum.reduceat(lo_s, starts, axis=0), nodes["min"][li]), "a leaf's min is not the min of its triangles"
    assert np.array_equal(np.maximum.reduceat(hi_s, starts, axis=0), nodes["max"][li]), "a leaf's max is not the max of its triangles"
    assert np.array_equal(np.minimum(nodes["min"][left], nodes["min"][right]), nodes["min"][ii]), "an interior min is not the min of its children's"
    assert np.array_equal(np.maximum(nodes["max"][left], nodes["max"][right]), nodes["max"][ii]), "an interior max is not the max of its children's"

    # centroid bounds per node, bottom-up by level (a level's nodes only read deeper ones)
    cmin = np.empty((N, 3), F32); cmax = np.empty((N, 3), F32)
    cmin[li] = np.minimum.reduceat(c_s, starts, axis=0)
    cmax[li] = np.maximum.reduceat(c_s, starts, axis=0)
    order = ii[np.argsort(level[ii], kind="stable")[::-1]]
    bounds = np.nonzero(np.diff(level[order]))[0] + 1
    for group in np.split(order, bounds):
        l, r = group + 1, nodes["secondChildOffset"][group].astype(np.int64)
        cmin[group] = np.minimum(cmin[l], cmin[r])
        cmax[group] = np.maximum(cmax[l], cmax[r])

    # split order
    ax = nodes["splitAxis"][ii].astype(np.int64)
    bad = cmax[left, ax] > cmin[right, ax]
    assert not bad.any(), f"node {ii[bad][:1]}: a left centroid lies beyond a right one on the split axis"

    # big leaves
    big = li[count[li] > MAX_LEAF]
    report = {"big_leaves": len(big), "nonfinite_area_leaves": 0}
    if len(big):
        area = _area(nodes["min"][big], nodes["max"][big])
        axis = _max_dimension(cmin[big], cmax[big])
        k = np.arange(len(big))
        excused = (area == 0) | (cmin[big][k, axis] == cmax[big][k, axis])
        with np.errstate(over="ignore", invalid="ignore"):
            nonfinite = ~np.isfinite(count[big].astype(F32) * area) & ~excused
        report["nonfinite_area_leaves"] = int(nonfinite.sum())
        if allow_nonfinite_area:
            excused |= nonfinite
        assert excused.all(), f"leaf {big[~excused][:1]} holds {count[big[~excused][:1]]} > {MAX_LEAF} triangles and nothing forbids splitting it" + \
            (" (count * area is not finite: pass allow_nonfinite_area=True where that is expected)" if nonfinite.any() else "")
    return report
