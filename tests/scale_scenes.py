"""One fixed-seed triangle soup, instantiated as base * s + t over a table of scales and placements, and the ray sets that go with it
(shared by tests/test_host_core.py, which runs the host-side checker and the CPU query over the table, and tests/test_gpu_scale.py, which
traces the same scenes and rays on the device).  Everything here is in the SCENE'S OWN UNITS: a row's `unit` is the length that plays the
part "1" plays for a model of ordinary size.

Why no row below s = 1e-2 has rays: the reference's triangle test answers "no hit" for |det| < 1e-5 and for t <= 1e-5, so a soup whose
edges are a few thousandths of a unit is invisible to unit-length rays (oracle hit fraction 0.000 at s = 1e-3) and a lost box could not
change any output.  CHECKER_ONLY_ROWS are covered by the host-side checker alone."""
import numpy as np

import rayfinder_amd as rf

FLT_MAX = float(np.finfo(np.float32).max)
N_TRIANGLES = 1500


def base_soup():
    """1500 triangles, float64, centres uniform in [-3, 3]^3, vertex sigma 0.45.  A sixth of them on the 0.5 lattice (shared planes,
    zero-thickness boxes: lattice-aligned planes are the ones a directed rounding leaves ON its target), a few axis-aligned flat quads,
    and groups of coincident triangles (leaves of several triangles, one of more than seven: the big-leaf table)."""
    rng = np.random.default_rng(20240)
    n = N_TRIANGLES
    tris = rng.uniform(-3, 3, (n, 1, 3)) + rng.normal(0, 0.45, (n, 3, 3))
    k = n // 6
    tris[:k] = np.round(tris[:k] * 2) / 2
    for i in range(k, k + 40):                                # flat, axis-aligned: a zero-thickness box on a lattice plane
        ax = i % 3
        tris[i, :, ax] = np.round(tris[i, 0, ax] * 2) / 2
    tris[k + 40:k + 52] = tris[k + 40]                        # twelve coincident triangles: one leaf of twelve
    for j in range(20):                                       # twenty groups of three
        tris[k + 60 + 3 * j:k + 63 + 3 * j] = tris[k + 60 + 3 * j]
    return tris


# name, s (scalar or per axis), t, unit
def _rows():
    base_r = float(np.abs(base_soup()).max())
    d = np.array([1.0, -1.0, 1.0])
    rows = [("centred_1e-2", 1e-2, 0 * d, 1e-2), ("centred_1", 1.0, 0 * d, 1.0), ("centred_3000", 3000.0, 0 * d, 3000.0),
            ("centred_7000", 7000.0, 0 * d, 7000.0),
            ("centred_binary16_edge", 65000.0 / base_r, 0 * d, 65000.0 / base_r),    # the root's largest coordinate at 65000: the last binary16 binade, spacing 32, 504 below the end
            ("centred_2e4", 2e4, 0 * d, 2e4), ("centred_1e6", 1e6, 0 * d, 1e6), ("centred_1e12", 1e12, 0 * d, 1e12),
            ("unit_at_1e3", 1.0, 1e3 * d, 1.0), ("unit_at_6e4", 1.0, 6e4 * d, 1.0), ("unit_at_1e7", 1.0, 1e7 * d, 1.0),
            ("small_at_1e3", 0.05, 1e3 * d, 0.05), ("small_at_6e4", 0.05, 6e4 * d, 0.05),
            ("unit_at_x_6e4", 1.0, np.array([6e4, 0.0, 0.0]), 1.0), ("unit_at_z_-1e7", 1.0, np.array([0.0, 0.0, -1e7]), 1.0),
            ("extent_1e4_by_1", np.array([1e4, 1.0, 30.0]) / (2 * base_r), 0 * d, 1.0)]     # per-axis local-grid scales
    return rows


ROWS = _rows()
ROW_NAMES = [r[0] for r in ROWS]
CHECKER_ONLY_ROWS = [("centred_1e-6", 1e-6, np.zeros(3), 1e-6), ("centred_1e-3", 1e-3, np.zeros(3), 1e-3)]


def row(name):
    return next(r for r in ROWS + CHECKER_ONLY_ROWS if r[0] == name)


def triangles(name):
    """base * s + t in float64, converted to f32 ONCE: [n, 9] float32."""
    _, s, t, _ = row(name)
    return (base_soup() * np.asarray(s, np.float64) + np.asarray(t, np.float64)).astype(np.float32).reshape(N_TRIANGLES, 9)


def soup_pt(P):
    n = P.shape[0]
    N = np.tile(np.array([0, 1, 0], np.float32), (n, 3))
    UV = np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (n, 1))
    return rf.PtFormat.from_triangles(P, N, UV, np.zeros(n, np.uint32), [(np.array([160 | (180 << 8) | (200 << 16) | (255 << 24)], np.uint32), 1, 1)])


def origin_bound(nodes):
    """4 R + 1 the way buildWide computes it from the root box: in double, then to f32 without rounding up."""
    R = float(max(np.abs(nodes[0]["min"].astype(np.float64)).max(), np.abs(nodes[0]["max"].astype(np.float64)).max()))
    bound = 4.0 * R + 1.0
    b = np.float32(bound)
    if float(b) > bound:
        b = np.nextafter(b, np.float32(0.0))
    return b, R


def root_fits_binary16(nodes):
    """Does every plane of the root box, padded by the builder's margin 2^-21 (originBound + R), stay within +-65504?"""
    b, R = origin_bound(nodes)
    return R + (float(b) + R) * 2.0 ** -21 <= 65504.0


# 1/d components ON each side of the traversal kernel's gate (1e-18 <= |1/d| <= 1e18): the f32 directions around 1e18 and 1e-18
def gate_direction_components():
    out = []
    with np.errstate(all="ignore"):
        for g in (np.float32(1e-18), np.float32(1e18)):
            d0 = np.float32(1.0) / g
            cands = [d0]
            for step in (np.float32(np.inf), np.float32(-np.inf)):
                d = d0
                for _ in range(4):
                    d = np.nextafter(d, step)
                    cands.append(d)
            # (1 / d does not reach every f32: where it skips the gate value itself, the nearest values it does reach on either side stand in)
            ulps = np.array([int(np.float32(np.float32(1.0) / c).view(np.int32)) - int(g.view(np.int32)) for c in cands])
            inside = ulps >= 0 if g < 1 else ulps <= 0
            assert np.abs(ulps[inside]).min() <= 1 and 1 <= np.abs(ulps[~inside]).min() <= 2, ulps
            out += cands
    return np.array(out, np.float32)


def main_rays(rng, n, lo, hi):
    """tests/test_gpu_parity.py's _random_rays with the box given in scene units: origins around the box, a tenth each of axis-parallel,
    non-unit, inside-the-model and zero-component rays."""
    o = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (n, 3))
    target = rng.uniform(lo, hi, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    k = n // 10
    rays[:k, 3:] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], (k, 1)).astype(np.float32)
    rays[k:2 * k, 3:] *= rng.uniform(0.1, 5.0, (k, 1)).astype(np.float32)
    rays[2 * k:3 * k, :3] = rng.uniform(lo, hi, (k, 3)).astype(np.float32)
    rays[3 * k:4 * k, 4] = 0.0
    return rays


N_MAIN = 10000
FRAME = (64, 48)


def scene_rays(nodes, seed=77):
    """-> (rays [m, 6] f32, number of leading "main" rays).  Behind the main set, the hostile families of
    test_render_path_traversal_kernel_on_arbitrary_rays in scene units, and origins / directions that straddle the gate."""
    rng = np.random.default_rng(seed)
    lo, hi = nodes[0]["min"].astype(np.float64), nodes[0]["max"].astype(np.float64)
    ext = np.maximum(hi - lo, 1e-30)
    bound, R = origin_bound(nodes)
    inf32 = np.float32(np.inf)
    fam = []

    def aimed(o, unit=True):
        d = rng.uniform(lo, hi) - np.asarray(o, np.float64)
        nrm = np.linalg.norm(d)
        return d / nrm if (unit and nrm > 0 and np.isfinite(nrm)) else d

    # (1) 0 * inf slabs: a zero direction component with the origin EXACTLY on a plane of a node's box
    for i in range(800):
        nd = nodes[rng.integers(0, len(nodes))]
        ax = int(rng.integers(0, 3))
        o = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext).astype(np.float32)
        o[ax] = nd["min" if i % 2 else "max"][ax]
        d = aimed(o).astype(np.float32)
        d[ax] = np.float32(0.0) if i % 4 < 2 else np.float32(-0.0)
        fam.append(np.concatenate([o, d]))
    # (2) grazing: the origin ON a face of a node's box (exactly, or one ulp to either side), the direction almost inside that face
    for i in range(2000):
        nd = nodes[rng.integers(0, len(nodes))]
        ax = int(rng.integers(0, 3))
        o = rng.uniform(nd["min"].astype(np.float64), nd["max"].astype(np.float64)).astype(np.float32)
        o[ax] = nd["min" if i % 2 else "max"][ax]
        if i % 3:
            o[ax] = np.nextafter(o[ax], inf32 if i % 3 == 1 else -inf32)
        d = rng.normal(size=3).astype(np.float32)
        d[ax] = np.float32(rng.choice([1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3, 1e-12, -1e-12]))
        fam.append(np.concatenate([o, d]))
    # (3) far diagonal origins, R * 10^0.5 ... R * 10^9 (clipped to f32), aimed at the scene: beyond the origin bound
    for i in range(240):
        sgn = np.array([1.0 if (i >> k) & 1 else -1.0 for k in range(3)])
        far = np.clip(sgn * max(R, 1e-30) * 10.0 ** (0.5 * (1 + i % 18)) * rng.uniform(0.8, 1.25, 3), -3e38, 3e38)
        d = rng.uniform(lo, hi) - far
        with np.errstate(all="ignore"):
            d = d / np.linalg.norm(d) if i % 2 else d * 1e-12
        fam.append(np.concatenate([far, d]).astype(np.float32))
    # (4) origins straddling the gate: coordinates AT originBound, one ulp above, one ulp below (either sign; on one axis with the others
    # inside the box, or on all three), aimed at the scene
    steps = (bound, np.nextafter(bound, inf32), np.nextafter(bound, np.float32(0.0)))
    for i in range(540):
        v = steps[i % 3]
        if (i // 3) % 2:
            o = rng.uniform(lo, hi).astype(np.float32)
            o[(i // 6) % 3] = v if (i // 18) % 2 else -v
        else:
            o = np.array([v if (i >> (3 + k)) & 1 else -v for k in range(3)], np.float32)
            if (i // 48) % 2:                                  # two axes at the bound, one anywhere below it
                o[i % 3] = np.float32(rng.uniform(-float(bound), float(bound)))
        fam.append(np.concatenate([o, aimed(o).astype(np.float32)]))
    # (5) 1/d components at 1e-18 and 1e18 and one ulp outside each
    comps = gate_direction_components()
    for i in range(len(comps) * 12):
        c = comps[i % len(comps)]
        o = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext).astype(np.float32)
        d = aimed(o).astype(np.float32)
        ax = (i // len(comps)) % 3
        d[ax] = c if (i // (3 * len(comps))) % 2 else -c
        if c > 1 and i % 2:                                   # a huge component: the others huge as well, so that the ray still points at the scene
            d = (aimed(o) * float(c)).astype(np.float32)
            d[ax] = c if d[ax] >= 0 else -c
        fam.append(np.concatenate([o, d]))
    rays = np.concatenate([main_rays(rng, N_MAIN, lo, hi), np.array(fam, np.float32)])
    # (6) degenerate directions, a denormal component (1/d = inf), NaN origins, huge directions -- over copies of main rays
    extra = rays[:200].copy()
    extra[:50, 3:] = 0.0
    extra[50:100, 3] = np.float32(1e-42)
    extra[100:150, 0] = np.float32(np.nan)
    with np.errstate(all="ignore"):
        extra[150:200, 3:] *= np.float32(1e30)
    return np.concatenate([rays, extra]), N_MAIN


def cameras(nodes, w, h):
    """Two cameras in scene units looking at the middle of the root box, focused on it (the reference's camera places its image plane at
    the focus distance: a plane one unit in front of an eye at 1e7 would collapse every pixel into a handful of directions): one about
    a scene's width away, inside the origin bound; one with a coordinate a quarter beyond originBound, so that the primary launch takes
    `primaryOutside`, its field of view narrowed to the scene.  -> [(label, camera, inside the bound?)]"""
    from oracle import orc
    lo, hi = nodes[0]["min"].astype(np.float64), nodes[0]["max"].astype(np.float64)
    c, ext = 0.5 * (lo + hi), hi - lo
    bound, _ = origin_bound(nodes)
    mid = float(np.sort(ext)[1])                              # (the middle extent: a scene of 1e4 x 1 x 30 is looked at from 50 away, not from 1e4)
    out = []
    near = c + np.array([0.35, 0.3, 0.8]) * 1.7 * mid
    out.append(("near", rf.create_camera(near, c, 0.0, float(np.linalg.norm(near - c)), orc.degrees_to_radians(55.0), w / h), bool(np.abs(near.astype(np.float32)).max() <= bound)))
    ax = int(np.argmax(np.abs(c) + 0.5 * ext))                # away from the origin along the axis on which the scene reaches farthest
    sgn = 1.0 if c[ax] >= 0 else -1.0
    perp = float(np.delete(ext, ax).max())
    far = c + np.array([0.05, 0.04, 0.03]) * perp
    far[ax] = sgn * 1.25 * float(bound)
    dist = float(np.linalg.norm(far - c))
    vfov = 2.0 * np.arctan(0.78 * perp / dist)
    out.append(("far", rf.create_camera(far, c, 0.0, dist, float(vfov), w / h), bool(np.abs(far.astype(np.float32)).max() <= bound)))
    return out
