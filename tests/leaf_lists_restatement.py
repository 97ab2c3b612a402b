"""Bounce 1's per-pixel leaf lists on the host, bit for bit (numpy), and the reference's closest-hit walk beside them.

pixel_leaf_lists() restates kPixelLeafLists (rayfinder_amd/csrc/rf_primary_lists.hip): the four corner directions of a pixel with kRaygen's f32 expressions in their
order, then everything in f64 -- the direction box and its margins, the interval slab test, the depth-first walk for the pixel's sign pattern, the refusals.  The build
has no contraction and IEEE divide and square root, so every operation is one rounding, here as there: the lists, their signs and the reasons come out EQUAL, not close.
The walk is run for all pixels of one sign pattern at once (they share the visit order); a pixel that is refused leaves the group at the node where the kernel breaks.

reference_walk() restates the reference's walk (wgsl:370-429: the f32 slab test, near child first by dirNeg[splitAxis], Moller-Trumbore, the shrinking rayTMax) for
many rays of ONE sign pattern at once and says, per ray, which leaves it reached, in order -- plus the hit and the visit counts, which the oracle's own walk checks.

Nothing here reads a device or the package: nodes are the reference's 48-byte records (NODE_DTYPE), read the way packScene packs them -- link is trianglesOffset of a
leaf or secondChildOffset of an interior node, leaf-ness is triangleCount > 0, the axis is splitAxis."""
import numpy as np

F = np.float32
T_MAX = F(10000.0)                                                     # wgsl:73
WALK_STACK = 64                                                        # kListWalkStack
INDEX_BITS = 26                                                        # kWideIndexBits
HAS_LIST, SIGNS, OVERFLOW, BIG_LEAF, STACK = 0, 1, 2, 3, 4             # kNoList...
REASONS = {SIGNS: "signs", OVERFLOW: "overflow", BIG_LEAF: "big leaf", STACK: "stack"}
CORNERS = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0))             # (nx, ny) of corner c: c & 1, c & 2


def camera_vectors(cam19):
    """-> origin, lowerLeftCorner, horizontal, vertical (f32 [3] each) of the 19-float camera"""
    c = np.asarray(cam19, np.float32).reshape(19)
    return c[0:3], c[3:6], c[6:9], c[9:12]


def ray_directions(cam19, w, h, x, y, nx, ny):
    """kRaygen under a pinhole camera, in f32: -> (D, normalize(D)) for pixels (x, y) and sample points (nx, ny); all four broadcast against each other"""
    o, ll, hor, ver = camera_vectors(cam19)
    x, y, nx, ny = np.broadcast_arrays(np.asarray(x), np.asarray(y), np.asarray(nx, np.float32), np.asarray(ny, np.float32))
    u = (x.astype(F) + F(0.5)) / F(w)
    v = (y.astype(F) + F(0.5)) / F(h)
    s = (u + nx / F(w))[..., None]
    t = ((F(1.0) - v) + ny / F(h))[..., None]
    D = ((ll + s * hor) + t * ver) - o
    dot = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
    with np.errstate(all="ignore"):
        direction = D * (F(1.0) / np.sqrt(dot))[..., None]
    assert D.dtype == direction.dtype == np.float32
    return D, direction


def ray_signs(direction):
    """dirNeg of the reference (wgsl:437-445: 1 / d < 0, so -0 counts as negative) as bits 0..2"""
    with np.errstate(all="ignore"):
        neg = (F(1.0) / direction) < F(0.0)
    return neg[..., 0].astype(np.uint32) | (neg[..., 1].astype(np.uint32) << 1) | (neg[..., 2].astype(np.uint32) << 2)


class NodeArrays:
    def __init__(self, nodes):
        self.lo32, self.hi32 = np.ascontiguousarray(nodes["min"], np.float32), np.ascontiguousarray(nodes["max"], np.float32)
        self.lo64, self.hi64 = self.lo32.astype(np.float64), self.hi32.astype(np.float64)
        self.count = nodes["triangleCount"].astype(np.int64)
        self.leaf = self.count > 0
        self.link = np.where(self.leaf, nodes["trianglesOffset"], nodes["secondChildOffset"]).astype(np.int64)
        self.axis = (nodes["splitAxis"] & 3).astype(np.int64)


class PixelLists:
    """reason [h, w]: HAS_LIST or why not; signs [h, w]: bits 0..2; length [h, w]; first / count [h, w, capacity]: the entries, in order"""

    def __init__(self, w, h, capacity):
        self.width, self.height, self.capacity = w, h, capacity
        self.reason = np.zeros((h, w), np.int64)
        self.signs = np.zeros((h, w), np.uint32)
        self.length = np.zeros((h, w), np.int64)
        self.first = np.full((h, w, capacity), -1, np.int64)
        self.count = np.zeros((h, w, capacity), np.int64)

    def entries(self, x, y):
        n = int(self.length[y, x])
        return [(int(self.first[y, x, e]), int(self.count[y, x, e])) for e in range(n)]

    @property
    def pixels(self):
        return self.width * self.height

    @property
    def without(self):
        return int((self.reason != HAS_LIST).sum())

    def reasons(self):
        return {name: int((self.reason == code).sum()) for code, name in REASONS.items()}

    def histogram(self):
        """{length: pixels} over the pixels that have a list"""
        lengths, counts = np.unique(self.length[self.reason == HAS_LIST], return_counts=True)
        return {int(l): int(c) for l, c in zip(lengths, counts)}

    def mean_length(self):
        listed = self.reason == HAS_LIST
        return float(self.length[listed].mean()) if listed.any() else 0.0


def pixel_leaf_lists(nodes, cam19, w, h, capacity, swap_children=False, drop_emitted=None):
    """kPixelLeafLists for every pixel of a w x h frame.  The two mutations exist for the tests of this file's teeth: swap_children visits the far child first;
    drop_emitted = k leaves the k-th leaf a pixel would emit off its list."""
    na = NodeArrays(nodes)
    out = PixelLists(w, h, capacity)
    o32, ll, hor, ver = camera_vectors(cam19)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    P = w * h
    # ---- the direction box: corners in f32, the rest in f64
    corner = np.zeros((4, P, 3), np.float64)
    min_len = np.full(P, 1e300)
    for c, (nx, ny) in enumerate(CORNERS):
        D, direction = ray_directions(cam19, w, h, xs.reshape(-1), ys.reshape(-1), F(nx), F(ny))
        D = D.astype(np.float64)
        with np.errstate(all="ignore"):
            length = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
        min_len = np.fmin(min_len, length)
        corner[c] = direction.astype(np.float64)
    lo, hi = np.full((P, 3), 2.0), np.full((P, 3), -2.0)
    for c in range(4):
        lo, hi = np.fmin(lo, corner[c]), np.fmax(hi, corner[c])
    diag2 = np.zeros(P)
    for i in range(4):
        for j in range(i + 1, 4):
            d = corner[i] - corner[j]
            diag2 = np.fmax(diag2, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    big = float(np.fmax.reduce(np.abs(np.concatenate([o32, ll, hor, ver]).astype(np.float64))))
    with np.errstate(all="ignore"):
        rounding = 64.0 * 5.9604644775390625e-08 * (big / min_len + 1.0)
        refused = ~(min_len > 0.0) | (not big < 1e30)
        margin = (0.25 * (hi - lo) + diag2[:, None]) + rounding[:, None]
        lo, hi = lo - margin, hi + margin
        refused |= (~((lo > 0.0) | (hi < 0.0))).any(axis=1)
        neg = hi < 0.0
        inv_lo, inv_hi = 1.0 / hi, 1.0 / lo
    reason = np.where(refused, SIGNS, HAS_LIST).astype(np.int64)
    signs = neg[:, 0].astype(np.uint32) | (neg[:, 1].astype(np.uint32) << 1) | (neg[:, 2].astype(np.uint32) << 2)
    n = np.zeros(P, np.int64)
    seen = np.zeros(P, np.int64)                                       # leaves a pixel has come to emit (== n without drop_emitted)
    first, count = out.first.reshape(P, capacity), out.count.reshape(P, capacity)
    o = o32.astype(np.float64)

    def visit(node, idx, pending, negs):
        idx = idx[reason[idx] == HAS_LIST]
        if idx.size == 0:
            return
        near_lower, far_upper = np.full(idx.size, -1e300), np.full(idx.size, 1e300)
        for a in range(3):
            qn = (na.hi64 if negs[a] else na.lo64)[node, a] - o[a]
            qf = (na.lo64 if negs[a] else na.hi64)[node, a] - o[a]
            tn = np.fmin(qn * inv_lo[idx, a], qn * inv_hi[idx, a])
            tf = np.fmax(qf * inv_lo[idx, a], qf * inv_hi[idx, a])
            tn = tn - (np.abs(tn) * 1e-6 + 1e-30)
            tf = tf + (np.abs(tf) * 1e-6 + 1e-30)
            near_lower, far_upper = np.fmax(near_lower, tn), np.fmin(far_upper, tf)
        acc = idx[(near_lower <= far_upper) & (far_upper > 0.0)]
        if acc.size == 0:
            return
        if na.leaf[node]:
            full = n[acc] == capacity
            if na.count[node] > 7 or na.link[node] >= (1 << INDEX_BITS):
                reason[acc] = np.where(full, OVERFLOW, BIG_LEAF)
                return
            reason[acc[full]] = OVERFLOW
            acc = acc[~full]
            keep = acc if drop_emitted is None else acc[seen[acc] != drop_emitted]
            seen[acc] += 1
            first[keep, n[keep]], count[keep, n[keep]] = na.link[node], na.count[node]
            n[keep] += 1
            return
        if pending == WALK_STACK:
            reason[acc] = STACK
            return
        far_first = bool(negs[na.axis[node]]) != swap_children
        near, far = (na.link[node], node + 1) if far_first else (node + 1, na.link[node])
        visit(int(near), acc, pending + 1, negs)
        visit(int(far), acc, pending, negs)

    with np.errstate(all="ignore"):
        for s in np.unique(signs[reason == HAS_LIST]):
            visit(0, np.flatnonzero((reason == HAS_LIST) & (signs == s)), 0, ((s >> 0) & 1, (s >> 1) & 1, (s >> 2) & 1))
    out.reason[...] = reason.reshape(h, w)
    out.signs[...] = np.where(reason == HAS_LIST, signs, 0).reshape(h, w)
    out.length[...] = np.where(reason == HAS_LIST, n, 0).reshape(h, w)
    return out


# ---------------------------------------------------------------------------------------------------------------- the reference's walk
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0], x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], axis=1)


def _triangle(ro, rd, p0, p1, p2, t_max):
    """wgsl:477-521 for rays [m] against one triangle -> (hit [m], t, u, v)"""
    eps = F(0.00001)
    e1, e2 = (p1 - p0)[None, :], (p2 - p0)[None, :]
    e1, e2 = np.broadcast_to(e1, rd.shape), np.broadcast_to(e2, rd.shape)
    hv = _cross(rd, e2)
    det = _dot(e1, hv)
    ok = ~((det > -eps) & (det < eps))
    inv_det = F(1.0) / det
    s = ro - p0[None, :]
    u = inv_det * _dot(s, hv)
    ok &= ~((u < F(0.0)) | (u > F(1.0)))
    q = _cross(s, e1)
    v = inv_det * _dot(rd, q)
    ok &= ~((v < F(0.0)) | (u + v > F(1.0)))
    t = inv_det * _dot(e2, q)
    ok &= (t > eps) & (t < t_max)
    return ok, t, u, v


class Walks:
    """Per ray: leaves = [(first triangle, count), ...] in the order reached; tri (-1: a miss), t, u, v of the closest hit; nodes visited and triangles tested"""

    def __init__(self, m):
        self.leaves = [[] for _ in range(m)]
        self.tri = np.full(m, -1, np.int64)
        self.t, self.u, self.v = np.full(m, T_MAX, np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32)
        self.nodes_visited, self.triangle_tests = np.zeros(m, np.int64), np.zeros(m, np.int64)


def reference_walk(nodes, positions48, origin, directions, t_max=T_MAX):
    """The reference's closest-hit walk for rays of one origin whose directions [m, 3] f32 share ONE sign pattern (asserted): with the signs fixed, the depth-first
    order is one order for all of them, so the tree is walked once and a node is tested for the rays that reached it -- each against its own rayTMax of that moment."""
    na = NodeArrays(nodes)
    tris = np.asarray(positions48, np.float32).reshape(-1, 12)
    rd = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    m = rd.shape[0]
    ro = np.broadcast_to(np.asarray(origin, np.float32).reshape(1, 3), rd.shape)
    out = Walks(m)
    if m == 0:
        return out
    s = ray_signs(rd)
    assert (s == s[0]).all(), "reference_walk: one sign pattern per call"
    negs = [int(s[0] >> a) & 1 for a in range(3)]
    with np.errstate(all="ignore"):
        inv = F(1.0) / rd
    ray_t = np.full(m, t_max, np.float32)

    def visit(node, idx):
        out.nodes_visited[idx] += 1
        near = [((na.hi32 if negs[a] else na.lo32)[node, a] - ro[idx, a]) * inv[idx, a] for a in range(3)]
        far = [((na.lo32 if negs[a] else na.hi32)[node, a] - ro[idx, a]) * inv[idx, a] for a in range(3)]
        tmin, tmax = near[0], far[0]
        ok = ~((tmin > far[1]) | (near[1] > tmax))
        tmin, tmax = np.where(near[1] < tmin, tmin, near[1]), np.where(tmax < far[1], tmax, far[1])      # glm max(tymin, tmin) / min(tymax, tmax)
        ok &= ~((tmin > far[2]) | (near[2] > tmax))
        tmin, tmax = np.where(near[2] < tmin, tmin, near[2]), np.where(tmax < far[2], tmax, far[2])
        ok &= (tmin < ray_t[idx]) & (tmax > F(0.0))
        acc = idx[ok]
        if acc.size == 0:
            return
        if na.leaf[node]:
            f, c = int(na.link[node]), int(na.count[node])
            for r in acc:
                out.leaves[r].append((f, c))
            for k in range(c):
                p = tris[f + k]
                hit, t, u, v = _triangle(ro[acc], rd[acc], p[0:3], p[4:7], p[8:11], ray_t[acc])
                out.triangle_tests[acc] += 1
                w = acc[hit]
                ray_t[w], out.t[w], out.u[w], out.v[w], out.tri[w] = t[hit], t[hit], u[hit], v[hit], f + k
            return
        far_first = bool(negs[na.axis[node]])
        a, b = (na.link[node], node + 1) if far_first else (node + 1, na.link[node])
        visit(int(a), acc)
        visit(int(b), acc)

    with np.errstate(all="ignore"):
        visit(0, np.arange(m))
    return out


def is_subsequence(walk, entries):
    """are the leaves a ray reached a subsequence of its pixel's list, in order?"""
    it = iter(entries)
    return all(leaf in it for leaf in walk)
