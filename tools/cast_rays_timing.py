"""usage: tools/cast_rays_timing.py <package root> [runs] [mode] [sizes, e.g. 1,16]
rf_renderer_cast_rays against the path a caller has without it, on the benchmark's stand-in scene (rayfinder_amd/scenes.py: the atrium).  Prints one JSON line.
Two ray sets of N = 1 M and 16 M rays each: "coherent", the primary rays of a 1920 x 1080 pinhole frame (pixel centres; for 16 M, eight sub-pixel offsets), and
"incoherent", cosine-weighted bounces from those rays' hit points about the geometric normal.  Both are made on the host with numpy from a fixed seed, the hits through
r.intersect_rays, so that every package traces the same rays.
  mode "cast" (this commit's package): wall time and rays/s of cast_rays with outputs triangle + t and with all nine, rays and outputs resident in device tensors;
      each request once before its `runs` timed calls.  Under a kernel trace the dispatches of kCastLoad / kTraceWide / kCastResolve appear in the order of `sequence`.
  mode "host" (any package, the parent commit's too): r.intersect_rays on the same rays from host memory at query_variant 0 and 2, copies included."""
import json
import os
import statistics
import sys
import time

root_dir = os.path.abspath(sys.argv[1])
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
mode = sys.argv[3] if len(sys.argv) > 3 else "cast"
sizes = [int(s) for s in (sys.argv[4] if len(sys.argv) > 4 else "1,16").split(",")]
sys.path.insert(0, root_dir)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402

assert os.path.abspath(rf.__file__).startswith(root_dir), rf.__file__
W, H = 1920, 1080
ALL = ("triangle", "t", "bary", "position", "geometric_normal", "normal", "texcoord", "albedo", "texture")
pt, info = scenes.atrium(1, "plain")
cam = rf.fly_camera(W, H)
r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, 1, 2, rf.make_sky(), 0.25), pt.scene())
pos = pt.arrays()["trianglePositionAttributes"]


def primary(n):
    c = rf.camera_to_array(cam).astype(np.float64)
    origin, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    copies = (n + W * H - 1) // (W * H)
    rng = np.random.default_rng(7)
    out = []
    for k in range(copies):
        dx, dy = (0.5, 0.5) if k == 0 else rng.random(2)
        u = (np.arange(W) + dx) / W
        v = 1.0 - (np.arange(H) + dy) / H
        d = llc[None, None] + u[None, :, None] * hor[None, None] + v[:, None, None] * ver[None, None] - origin[None, None]
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        out.append(np.concatenate([np.broadcast_to(origin, d.shape), d], 2).reshape(-1, 6).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(out)[:n])


def bounces(rays):
    """cosine-weighted directions about the geometric normal at the rays' hits (misses dropped, the set filled up to its size by repetition)"""
    hit = r.intersect_rays(rays, 10000.0)
    found = hit["tri"] != 0xFFFFFFFF
    P = pos[hit["tri"][found]]
    nrm = np.cross(P[:, 4:7] - P[:, 0:3], P[:, 8:11] - P[:, 0:3])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    nrm *= -np.sign(np.sum(nrm * rays[found, 3:], 1, keepdims=True))       # towards the side the ray came from
    rng = np.random.default_rng(11)
    u1, u2 = rng.random(nrm.shape[0]), rng.random(nrm.shape[0])
    a = np.where(np.abs(nrm[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t1 = np.cross(nrm, a)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    rad, phi = np.sqrt(u1), 2 * np.pi * u2
    d = (rad * np.cos(phi))[:, None] * t1 + (rad * np.sin(phi))[:, None] * t2 + np.sqrt(1 - u1)[:, None] * nrm
    out = np.concatenate([hit["p"][found], d], 1).astype(np.float32)
    return np.ascontiguousarray(np.resize(out, (rays.shape[0], 6))), float(found.mean())


def timed(call):
    call()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def summary(ms, n):
    med = statistics.median(ms)
    return dict(median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms), rays=n, rays_per_s=round(n / (med * 1e-3)))


out = dict(mode=mode, runs=runs, package=root_dir, scene=info, sequence=[])
for millions in sizes:
    n = millions << 20
    coherent = primary(n)
    incoherent, hit_fraction = bounces(coherent)
    out[f"{millions}M_primary_hit_fraction"] = round(hit_fraction, 4)
    for name, rays in (("coherent", coherent), ("incoherent", incoherent)):
        key = f"{millions}M_{name}"
        if mode == "host":
            for variant in (0, 2):
                r.set_option("query_variant", variant)
                out[f"{key}_intersect_rays_variant{variant}"] = summary(timed(lambda: r.intersect_rays(rays, 10000.0)), n)
            r.set_option("query_variant", 0)
        else:
            dev = torch.from_numpy(rays).cuda()
            o, d = dev[:, :3], dev[:, 3:]
            for label, names in (("triangle_t", ("triangle", "t")), ("all", ALL)):
                dst = r.cast_rays(o, d, outputs=names)
                out[f"{key}_cast_{label}"] = summary(timed(lambda: r.cast_rays(o, d, outputs=names, out=dst)), n)
                out["sequence"].append(f"{key}_cast_{label}")
                del dst
            vis = r.cast_occlusion(o, d)
            out[f"{key}_cast_occlusion"] = summary(timed(lambda: r.cast_occlusion(o, d, out=vis)), n)
            out["sequence"].append(f"{key}_cast_occlusion")
            del dev, vis
r.close()
print(json.dumps(out))
