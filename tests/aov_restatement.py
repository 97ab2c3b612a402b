"""Expected first-hit AOVs (rf_renderer_set_aovs), restated from the oracle's own primitives.

Per sample (pixel x, y, frame f): orc.wgsl_camera_ray gives the primary ray the renderer traces, a closest-hit query gives
(hit, t, triangle, u, v), the triangle's packed attributes (rf_oracle.c:1060-1064) give the interpolated shading normal and
uv, orc.texture_lookup gives the albedo.  normalize is rf_math.hpp's v * (1 / sqrt((x*x + y*y) + z*z)), one f32 operation at
a time; a normal without direction (|n|^2 zero or not finite) is (0, 0, 0).  A miss is zeros, coverage included.  Sums are
f32 in frame order, as the renderer keeps them.
"""
import numpy as np

from oracle import orc

F32 = np.float32
T_MAX = 10000.0  # wgsl:73


def oracle_intersect(scene, rays):
    """closest-hit queries through the oracle's BVH walk (the one its renderer uses)."""
    return orc.intersect_bvh_batch(scene.nodes, scene.positions.view(np.float32).reshape(-1, 12), rays, T_MAX)


def _attributes(scene):
    a = np.ascontiguousarray(scene.attrs).view(np.float32).reshape(-1, 20)
    return a, a.view(np.uint32)[:, 18]


def first_hit_attributes(scene, rp, xs, ys, frame, intersect=oracle_intersect):
    """What the first hit of one sample of the pixels (xs[i], ys[i]) at `frame` interpolates, for the m samples that hit: dict of hit (indices into xs),
    tri, tex (the triangle's texture index), uvx, uvy, nrm (m, 3), dd (|nrm|^2) and t, every float in f32."""
    rays = np.stack([orc.wgsl_camera_ray(rp, int(x), int(y), int(frame), scene.blue_noise) for x, y in zip(xs, ys)])
    h = intersect(scene, rays)
    hit = np.nonzero(h["hit"])[0]
    attrs, tex = _attributes(scene)
    tri = h["tri"][hit]
    u, v = h["uv"][hit, 0].astype(F32), h["uv"][hit, 1].astype(F32)
    with np.errstate(all="ignore"):
        b0, b1, b2 = (F32(1.0) - u) - v, u, v                        # wgsl:515
        a = attrs[tri]
        n0, n1, n2 = a[:, 0:3], a[:, 4:7], a[:, 8:11]
        nrm = (b0[:, None] * n0 + b1[:, None] * n1) + b2[:, None] * n2
        uvx = (b0 * a[:, 12] + b1 * a[:, 14]) + b2 * a[:, 16]
        uvy = (b0 * a[:, 13] + b1 * a[:, 15]) + b2 * a[:, 17]
        dd = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
    return dict(n=rays.shape[0], hit=hit, tri=tri, tex=tex[tri], uvx=uvx, uvy=uvy, nrm=nrm, dd=dd, t=h["t"][hit])


def first_hit_samples(scene, rp, xs, ys, frame, intersect=oracle_intersect, attributes=None):
    """AOV values of one sample of the pixels (xs[i], ys[i]) at `frame` -> ({albedo.rgb, coverage}, {normal.xyz, depth}), (n, 4) f32 each.
    `attributes`: first_hit_attributes of the same arguments, where the caller has them already."""
    fa = first_hit_attributes(scene, rp, xs, ys, frame, intersect) if attributes is None else attributes
    n, hit = fa["n"], fa["hit"]
    ac = np.zeros((n, 4), F32)
    nd = np.zeros((n, 4), F32)
    if hit.size == 0:
        return ac, nd
    nrm, dd = fa["nrm"], fa["dd"]
    ok = (dd != 0) & np.isfinite(dd)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        inv = F32(1.0) / np.sqrt(dd)
        unit = np.where(ok[:, None], nrm * inv[:, None], F32(0.0)).astype(F32)
    for j, i in enumerate(hit):
        ac[i, :3] = orc.texture_lookup(scene, int(fa["tex"][j]), fa["uvx"][j], fa["uvy"][j])
    ac[hit, 3] = 1.0
    nd[hit, :3] = unit
    nd[hit, 3] = fa["t"]
    return ac, nd


def aov_sums(scene, rp, frames, x0=0, y0=0, x1=None, y1=None, intersect=oracle_intersect):
    """Sums over `frames` (in that order) for the crop [x0, x1) x [y0, y1) -> ((h, w, 4), (h, w, 4)) f32: {albedo, coverage}, {normal, depth}."""
    x1 = rp.width if x1 is None else x1
    y1 = rp.height if y1 is None else y1
    ys, xs = np.mgrid[y0:y1, x0:x1]
    xs, ys = xs.ravel(), ys.ravel()
    ac_sum = np.zeros((xs.size, 4), F32)
    nd_sum = np.zeros((xs.size, 4), F32)
    for f in frames:
        ac, nd = first_hit_samples(scene, rp, xs, ys, f, intersect)
        ac_sum = ac_sum + ac
        nd_sum = nd_sum + nd
    shape = (y1 - y0, x1 - x0, 4)
    return ac_sum.reshape(shape), nd_sum.reshape(shape)
