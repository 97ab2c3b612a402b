"""The surface attributes rf_renderer_cast_rays gives at a hit, restated in numpy f32 -- one IEEE operation at a time in the order include/rayfinder_amd.h and
rf_shade_device.hpp write them (numpy never contracts a multiply and an add):

    e1 = p1 - p0, e2 = p2 - p0
    geometric_normal = cross(e1, e2) * (1 / sqrt(dot(cross, cross)))        cross(a, b) = (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)
    b0 = (1 - u) - v, b1 = u, b2 = v                                        dot(a, b)   = (a.x b.x + a.y b.y) + a.z b.z
    n = (b0 n0 + b1 n1) + b2 n2
    normal = (0, 0, 0) where dot(n, n) is 0 or not finite, else n * (1 / sqrt(dot(n, n)))
    texcoord = (b0 uv0 + b1 uv1) + b2 uv2, not wrapped
    albedo = the oracle's texture look-up at that texcoord (orc.texture_lookup), texture = the triangle's descriptor index

and on a miss (triangle 0xFFFFFFFF) every float +0 and texture 0xFFFFFFFF.  triangle, t, bary and position are the oracle's own (orc.intersect_bvh_batch)."""
import numpy as np

MISS = np.uint32(0xFFFFFFFF)
F = np.float32
NAMES = ("geometric_normal", "normal", "texcoord", "albedo", "texture")


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], 1)


def _normalize(v):
    return v * (F(1.0) / np.sqrt(_dot(v, v)))[:, None]


def attributes(pos48, attr80, tri, u, v, texture_lookup=None):
    """pos48 (T, 12) f32, attr80 (T, 20) f32 (the scene's PositionAttribute / VertexAttributes), tri (N,) u32, u, v (N,) f32 -> dict of NAMES.
    texture_lookup(descriptor index, uvx, uvy) -> 3 floats (None: no albedo)"""
    pos48, attr80 = np.ascontiguousarray(pos48, F).reshape(-1, 12), np.ascontiguousarray(attr80, F).reshape(-1, 20)
    tri, u, v = np.asarray(tri, np.uint32), np.asarray(u, F), np.asarray(v, F)
    n = tri.shape[0]
    out = dict(geometric_normal=np.zeros((n, 3), F), normal=np.zeros((n, 3), F), texcoord=np.zeros((n, 2), F), texture=np.full(n, MISS, np.uint32))
    if texture_lookup is not None:
        out["albedo"] = np.zeros((n, 3), F)
    hit = np.flatnonzero(tri != MISS)
    if hit.size == 0:
        return out
    with np.errstate(all="ignore"):
        P, A = pos48[tri[hit]], attr80[tri[hit]]
        hu, hv = u[hit], v[hit]
        p0, p1, p2 = P[:, 0:3], P[:, 4:7], P[:, 8:11]
        e1, e2 = p1 - p0, p2 - p0
        out["geometric_normal"][hit] = _normalize(_cross(e1, e2))
        b0, b1, b2 = (F(1.0) - hu) - hv, hu, hv
        n0, n1, n2 = A[:, 0:3], A[:, 4:7], A[:, 8:11]
        nrm = (b0[:, None] * n0 + b1[:, None] * n1) + b2[:, None] * n2
        nn = _dot(nrm, nrm)
        keep = (nn != 0) & np.isfinite(nn)
        unit = np.zeros_like(nrm)
        unit[keep] = _normalize(nrm[keep])
        out["normal"][hit] = unit
        uv0, uv1, uv2 = A[:, 12:14], A[:, 14:16], A[:, 16:18]
        uv = (b0[:, None] * uv0 + b1[:, None] * uv1) + b2[:, None] * uv2
        out["texcoord"][hit] = uv
        tex = np.ascontiguousarray(A[:, 18]).view(np.uint32)
        out["texture"][hit] = tex
        if texture_lookup is not None:
            out["albedo"][hit] = np.stack([texture_lookup(int(tex[k]), uv[k, 0], uv[k, 1]) for k in range(hit.size)]) if hit.size else 0
    return out


def same(got, want):
    """bit for bit, NaNs compared as NaNs (a payload is no value)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got.view(np.uint32) if got.dtype.itemsize == 4 else got, want.view(np.uint32) if want.dtype.itemsize == 4 else want)
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(g) & np.isnan(w)
    return bool(((g.view(np.uint32) == w.view(np.uint32)) | nan).all())


def first_difference(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    for i in range(g.shape[0]):
        if not same(g[i], w[i]):
            return f"row {i}: got {g[i]!r}, want {w[i]!r}"
    return "none"
