"""The rays tests/test_gpu_cast_rays.py casts: about 12 000 rays on a scene's box, (N, 6) f32 {origin, direction}, from a fixed seed.  Kinds, in this order:

  random        through the box: from a point on a sphere around it towards a point inside it
  axis          axis-parallel, and with one direction component at +-1e-12 .. +-1e-3, from origins on the box planes and one ulp off them
  far           diagonal origins 1e3 .. 1e20 away, aimed at the box
  special       zero and NaN direction components (and an all-zero direction)
  secondary     rays that start at the OFFSET hit points of the random rays' hits -- what bounce and shadow rays are -- in random directions

`intersect(rays) -> dict(hit, p)` is the oracle's closest-hit query (orc.intersect_bvh_batch over the scene); it is asked once, for the random rays."""
import numpy as np

F = np.float32
KINDS = ("random", "axis", "far", "special", "secondary")


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def generate(lo, hi, intersect, seed=20240611):
    """-> (rays (N, 6) f32, kind index per ray (N,) u8)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    parts = []

    # random through the box
    n = 7000
    inside = (lo + rng.random((n, 3)) * (hi - lo)).astype(F)
    origin = (centre + _unit(rng, n).astype(np.float64) * radius * rng.uniform(1.1, 3.0, (n, 1))).astype(F)
    d = inside - origin
    random = np.concatenate([origin, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)], 1)
    parts.append(random)

    # axis-parallel and nearly so, from the box planes and one ulp off them
    axis = []
    smalls = (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3)
    for a in range(3):
        for sign in (1.0, -1.0):
            for plane in (lo, hi):
                for nudge in (0, 1, -1):
                    for small in smalls:
                        for _ in range(3):
                            o = (lo + rng.random(3) * (hi - lo)).astype(F)
                            b = (a + 1 + int(rng.integers(2))) % 3        # the plane the origin sits on: another axis'
                            o[b] = F(plane[b])
                            if nudge:
                                o[b] = np.nextafter(o[b], F(np.inf if nudge > 0 else -np.inf))
                            o[a] = F(lo[a] - 1.0) if sign > 0 else F(hi[a] + 1.0)
                            dd = np.zeros(3, F)
                            dd[a] = sign
                            dd[(a + 1) % 3] = small
                            axis.append(np.concatenate([o, dd]))
    parts.append(np.array(axis, F))

    # far diagonal origins
    far = []
    for e in range(3, 21):
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    o = (centre + np.array([sx, sy, sz]) * 10.0 ** e).astype(F)
                    for _ in range(3):
                        target = lo + rng.random(3) * (hi - lo)
                        dd = target - o.astype(np.float64)
                        far.append(np.concatenate([o, (dd / np.linalg.norm(dd)).astype(F)]))
    parts.append(np.array(far, F))

    # zero and NaN direction components
    special = []
    for k in range(300):
        r = random[k].copy()
        which = k % 7
        r[3 + which % 3] = 0.0 if which < 3 else np.nan
        if which == 6:
            r[3:] = 0.0
        special.append(r)
    parts.append(np.array(special, F))

    # from the offset hit points of the random rays' hits
    got = intersect(random)
    p = got["p"][got["hit"] != 0][:4000]
    parts.append(np.concatenate([p.astype(F), _unit(rng, p.shape[0])], 1))

    kinds = np.concatenate([np.full(part.shape[0], i, np.uint8) for i, part in enumerate(parts)])
    return np.ascontiguousarray(np.concatenate(parts), F), kinds
