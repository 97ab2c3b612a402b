"""Seeded triangle soups for the BVH builders, shared by the CPU tests (test_bvh_invariants.py: host builder == oracle,
check_tree) and the GPU tests (test_gpu_bvh_edges.py: GPU == host == oracle).  Every generator returns (name, tris36 float32)
and every seed is a fixed integer, so a case is the same bytes in every process.

names(family) lists a family's cases, soup(name) builds one.  The sizes are the GPU builder's thresholds (rf_bvh_gpu.hip):
kSmallMax = 64 triangles per one-wave subtree, kMaxLeaf = 255, 256-lane workgroups, 1 024 triangles per scan block
(kThreads * kScanItems), 1 024 scan blocks per trip of kScanSums' carry loop."""
import numpy as np

F32 = np.float32
_CASES = {}        # name -> (family, thunk)


def _add(family, name, thunk):
    assert name not in _CASES, name
    _CASES[name] = (family, thunk)


def names(family):
    return [k for k, (f, _) in _CASES.items() if f == family]


def soup(name):
    tris = np.ascontiguousarray(_CASES[name][1](), F32).reshape(-1, 9)
    return name, tris


def uniform(rng, n, half=10.0, edge=0.3, centre=(0.0, 0.0, 0.0)):
    c = rng.uniform(-half, half, (n, 1, 3)) + np.asarray(centre, np.float64)
    return (c + rng.normal(0.0, edge, (n, 3, 3))).astype(F32).reshape(-1, 9)


# ------------------------------------------------------------------------------------------------ threshold sizes
THRESHOLD_SIZES = (63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, 4097)
for _n in THRESHOLD_SIZES:
    _add("threshold", f"uniform_{_n}", lambda n=_n: uniform(np.random.default_rng(1000 + n), n))


# ------------------------------------------------------------------------------------------------ unsplittable boundary
def _same_centroid(k, extra):
    """k triangles of different shapes around ONE centroid (count > kMaxLeaf against mustBeLeaf) + `extra` random ones"""
    rng = np.random.default_rng(2000 + k)
    # boxes of half-extent h around (3, -2, 1); h is a multiple of 2^-10, so that centre +- h and their sum are exact in f32 and
    # the centroid 0.5 * (lo + hi) is the centre itself for every triangle
    half = np.round(rng.uniform(0.1, 0.4, (k, 3)) * 1024) / 1024
    lo, hi = np.array([3.0, -2.0, 1.0]) - half, np.array([3.0, -2.0, 1.0]) + half
    tris = np.stack([lo, hi, np.stack([lo[:, 0], hi[:, 1], lo[:, 2]], 1)], 1).reshape(-1, 9)
    return np.concatenate([tris, uniform(rng, extra, half=5.0)]) if extra else tris


for _k in (255, 256, 257):
    _add("unsplittable", f"same_centroid_{_k}_plus_500", lambda k=_k: _same_centroid(k, 500))
for _k in (64, 65, 256):
    _add("unsplittable", f"identical_{_k}", lambda k=_k: np.tile(uniform(np.random.default_rng(2100 + k), 1), (k, 1)))


# ------------------------------------------------------------------------------------------------ straddles
STRADDLES = ((300, 212), (256, 256), (255, 257), (1000, 24, 1000), (64, 65), (1, 1023))


def _clusters(sizes, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([uniform(rng, s, half=0.5, edge=0.05, centre=(-100.0 + 100.0 * i, 0.0, 0.0)) for i, s in enumerate(sizes)])


for _s in STRADDLES:
    _add("straddle", "clusters_" + "_".join(map(str, _s)), lambda s=_s: _clusters(s, 3000 + sum(s) + len(s)))


# ------------------------------------------------------------------------------------------------ partition patterns
PARTITION_PATTERNS = ("alternating", "identity", "reversed", "one_a_at_end", "one_b_at_start", "bernoulli_0.1", "bernoulli_0.9")
PARTITION_SIZES = (8, 33, 64, 65, 300, 1025, 2049, 4100)          # <= 64: the wave path, above: the scan path
# Seed per (pattern, n): the first one, counting up from 0, for which the HOST builder's tree has at least 10 multi-triangle
# leaves (3 for n <= 64) and at least one of them holds its source indices in non-ascending order -- otherwise a STABLE
# partition would pass the case (partition_condition below; test_bvh_invariants.py re-checks every committed seed).
PARTITION_SEEDS = {}


def _pattern_is_a(pattern, n, rng):
    """True where the triangle at that index belongs to cluster A (the first split's left side)"""
    a = np.zeros(n, bool)
    if pattern == "alternating": a[0::2] = True
    elif pattern == "identity": a[:n // 2] = True
    elif pattern == "reversed": a[n - n // 2:] = True
    elif pattern == "one_a_at_end": a[:n // 2 - 1] = True; a[-1] = True                 # A..A B..B A
    elif pattern == "one_b_at_start": a[1:n // 2 + 1] = True                              # B A..A B..B
    else:
        a = rng.uniform(size=n) < float(pattern.split("_")[1])
        if a.sum() < 2: a[rng.permutation(np.nonzero(~a)[0])[:2 - a.sum()]] = True       # both clusters hold a group of two at least
        if (~a).sum() < 2: a[rng.permutation(np.nonzero(a)[0])[:2 - (~a).sum()]] = False
    return a


def _groups(count, rng):
    """sizes in 2..5 that add up to `count` (>= 2)"""
    sizes = []
    while count:
        s = count if count <= 3 else int(rng.integers(2, min(5, count) + 1))
        if count - s == 1: s -= 1                                # never a remainder of one (count >= 4 here, so s was 3 at least)
        sizes.append(s); count -= s
    return sizes


def partition_soup(pattern, n, seed):
    """Two clusters A (x = -50) and B (x = +50); inside each, groups of 2-5 COINCIDENT triangles (multi-triangle leaves whose
    order shows the partition permutation); `pattern` says which index holds an A and which a B, and the copies of each
    cluster's groups are dealt over that cluster's indices in a seeded shuffle."""
    rng = np.random.default_rng([seed, n, PARTITION_PATTERNS.index(pattern)])
    is_a = _pattern_is_a(pattern, n, rng)
    tris = np.empty((n, 9), F32)
    for mask, x in ((is_a, -50.0), (~is_a, 50.0)):
        sizes = _groups(int(mask.sum()), rng)
        base = uniform(rng, len(sizes), half=1.0, edge=0.3, centre=(x, 0.0, 0.0))
        tris[np.nonzero(mask)[0]] = base[rng.permutation(np.repeat(np.arange(len(sizes)), sizes))]
    return tris


def partition_condition(n, nodes, idx):
    """(multi-triangle leaves, those whose source indices are not ascending) of a built tree"""
    src = np.empty(n, np.int64); src[np.asarray(idx).astype(np.int64)] = np.arange(n)     # position -> source
    multi = np.nonzero(nodes["triangleCount"] > 1)[0]
    unordered = 0
    for li in multi:
        o, c = int(nodes["trianglesOffset"][li]), int(nodes["triangleCount"][li])
        unordered += bool(np.any(np.diff(src[o:o + c]) < 0))
    return len(multi), unordered


def partition_ok(n, nodes, idx):
    multi, unordered = partition_condition(n, nodes, idx)
    return multi >= (3 if n <= 64 else 10) and unordered >= 1


def find_partition_seed(pattern, n, build_bvh, limit=4000):
    """How PARTITION_SEEDS was made: build_bvh is the host builder"""
    for seed in range(limit):
        nodes, idx, _ = build_bvh(partition_soup(pattern, n, seed))
        if partition_ok(n, nodes, idx):
            return seed
    raise RuntimeError(f"no seed below {limit} for {pattern} at n = {n}")


PARTITION_SEEDS.update({(p, n): 0 for p in PARTITION_PATTERNS for n in PARTITION_SIZES})    # seed 0 holds the condition everywhere ...
PARTITION_SEEDS["identity", 8] = 1                                                           # ... but here (3 leaves, all ascending)
for _p in PARTITION_PATTERNS:
    for _n in PARTITION_SIZES:
        _add("partition", f"{_p}_{_n}", lambda p=_p, n=_n: partition_soup(p, n, PARTITION_SEEDS[(p, n)]))


# ------------------------------------------------------------------------------------------------ signed zeros
def lattice(dims, shift, zero_signs, seed):
    """One unit right triangle per cell of a dims lattice, translated by -shift so that it straddles the origin.  zero_signs:
    "coin" = every zero coordinate's sign from a seeded coin (both signs on every zero plane, both orders of first appearance),
    "negative" = every zero is -0."""
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 1, 3).astype(F32)
    tris = g + np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32) - np.asarray(shift, F32)
    tris = tris + F32(0.0)                                                   # every zero is +0 now
    zero = tris == 0
    if zero_signs == "coin":
        neg = zero & (np.random.default_rng(seed).uniform(size=tris.shape) < 0.5)
    else:
        neg = zero
    tris[neg] = F32(-0.0)
    return tris.reshape(-1, 9)


_add("signed_zero", "lattice_12x12x4_coin", lambda: lattice((12, 12, 4), (6, 6, 2), "coin", 5001))
_add("signed_zero", "lattice_12x12x4_negative", lambda: lattice((12, 12, 4), (6, 6, 2), "negative", 0))
_add("signed_zero", "lattice_5x4x2_coin", lambda: lattice((5, 4, 2), (2, 2, 1), "coin", 5002))       # 40 triangles: the wave path


# ------------------------------------------------------------------------------------------------ extent overflow
def _wide_x(n, lo, hi, seed):
    """centroids uniform on x in [lo, hi], y / z in [-1e-6, 1e-6]; edges of 1e30 on x (an ulp there is 1e31 at most) and 1e-7
    on y / z, so every vertex stays finite.  y / z are that small so that the AREAS stay finite while the x extent is finite
    (2 * 3.2e38 * 4e-6 times 400 triangles is 1e36): otherwise no SAH cost is finite, the node is one leaf and the buckets
    never matter."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(lo, hi, n), rng.uniform(-1e-6, 1e-6, n), rng.uniform(-1e-6, 1e-6, n)], 1)[:, None, :]
    e = rng.normal(0.0, 1.0, (n, 3, 3)) * np.array([1e30, 1e-7, 1e-7])
    tris = (c + e).astype(F32)
    assert np.isfinite(tris).all()
    return tris.reshape(-1, 9)


# FLT_MAX = 3.4028e38.  A centroid is 0.5 * (lo + hi), so finite centroids lie within +-FLT_MAX / 2 and their extent cannot
# overflow: in the first two sets the extent is finite and the quotient is +inf wherever 12 * (c - min) overflows, that is
# beyond min + FLT_MAX / 12 = min + 2.84e37 (nearly all of set 1, the upper part of set 2).  The extent overflows only through
# lo + hi: beyond +-1.7014e38 the centroid itself is +-inf (sets 3 and 4), and the quotient is NaN -- for every triangle when
# both ends are infinite, at the infinite end and 0 elsewhere when one is.
_add("extent_overflow", "x_pm1.6e38", lambda: _wide_x(400, -1.6e38, 1.6e38, 6001))
_add("extent_overflow", "x_pm4e37", lambda: _wide_x(400, -4e37, 4e37, 6002))
_add("extent_overflow", "x_pm3.2e38", lambda: _wide_x(400, -3.2e38, 3.2e38, 6003))
_add("extent_overflow", "x_0_3.2e38", lambda: _wide_x(400, 0.0, 3.2e38, 6004))


# ------------------------------------------------------------------------------------------------ other values
def _slivers():
    rng = np.random.default_rng(7002)
    reg = uniform(rng, 300, half=4.0).reshape(-1, 3, 3)
    sliver = reg[:150].copy(); sliver[:, 2] = F32(0.5) * (sliver[:, 0] + sliver[:, 1])       # three collinear vertices
    axis = reg[150:250].copy(); axis[:, 1] = axis[:, 0]; axis[:, 2] = axis[:, 0]; axis[:, 1, 0] += 1; axis[:, 2, 0] += 2   # on a line parallel to x
    point = reg[250:].copy(); point[:, 1] = point[:, 0]; point[:, 2] = point[:, 0]           # a point
    tris = np.concatenate([reg, sliver, axis, point]).reshape(-1, 9)
    return tris[rng.permutation(len(tris))]


_add("other_values", "denormal_1e-41", lambda: (np.random.default_rng(7001).uniform(-1, 1, (500, 9)) * 1e-41).astype(F32))
_add("other_values", "slivers_and_points", _slivers)


# ------------------------------------------------------------------------------------------------ non-finite vertices
def _non_finite(n, seed):
    """n regular triangles + one with a NaN vertex, one with +inf, one with -inf.  Both builders and the bake REFUSE these."""
    rng = np.random.default_rng(seed)
    tris = np.concatenate([uniform(rng, n, half=5.0), uniform(rng, 3, half=5.0)])
    at = rng.permutation(n + 3)[:3]
    tris[at[0], 4] = np.nan; tris[at[1], 0] = np.inf; tris[at[2], 8] = -np.inf
    return tris


_add("non_finite", "nan_and_infinities_303", lambda: _non_finite(300, 8001))
_add("non_finite", "nan_and_infinities_40", lambda: _non_finite(37, 8002))
for _i, (_v, _label) in enumerate(((np.nan, "nan"), (np.inf, "plus_inf"), (-np.inf, "minus_inf"))):
    def _one(v=_v, i=_i):
        tris = uniform(np.random.default_rng(8010 + i), 301, half=5.0); tris[150 + i, 3 * i + 1] = v
        return tris
    _add("non_finite", f"only_{_label}_301", _one)


# ------------------------------------------------------------------------------------------------ scan-carry sizes
for _n in (1_048_577, 2_100_000):                # 1 025 and 2 051 scan blocks: two and three trips of kScanSums' carry loop
    _add("scan_carry", f"uniform_{_n}", lambda n=_n: uniform(np.random.default_rng(9000 + n % 1000), n, half=100.0))
