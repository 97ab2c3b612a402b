#!/usr/bin/env python3
"""ms of the sum kernels (rf_stats.ms_accumulate: the image, and with them the AOV sums and the moments) and of the frame for the library in RAYFINDER_AMD_LIB:
atrium 1080p, spp per batch from argv (default 320).  --moments / --aovs turn those sums on; --adaptive EVERY renders through render_adaptive at target 0 in steps
of EVERY samples (the tile-list kernels; implies --moments, and keeps the AOVs per tile count)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import rayfinder_amd as rf
from rayfinder_amd import scenes
ap = argparse.ArgumentParser()
ap.add_argument("spp", nargs="?", type=int, default=320)
ap.add_argument("--moments", action="store_true")
ap.add_argument("--aovs", action="store_true")
ap.add_argument("--adaptive", type=int, default=0, metavar="EVERY")
a = ap.parse_args()
spp = a.spp
pt, _ = scenes.atrium()
W, H, b = 1920, 1080, 8
cam = rf.fly_camera(W, H)
r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, spp, b, rf.make_sky(), 0.25), pt.scene())
if a.moments or a.adaptive:
    r.set_moments(True)
if a.aovs:
    r.set_aovs(True, tile_counts=bool(a.adaptive))


def frame():
    if a.adaptive:
        r.render_adaptive(0.0, a.adaptive)
    else:
        r.render(spp)
    r.synchronize()


frame()
best = (1e30, 1e30)
for k in range(3):
    r.set_render_parameters(rf.make_render_parameters(W, H, cam, spp, b, rf.make_sky(), 0.3 + 0.01 * k))
    r.set_timing(True); r.reset_stats()
    t0 = time.perf_counter(); frame(); dt = time.perf_counter() - t0
    s = r.stats()
    best = (min(best[0], s["ms_accumulate"]), min(best[1], dt * 1e3))
img = r.read_accumulation()[0]
what = ("adaptive/%d" % a.adaptive if a.adaptive else "render") + ("+moments" if a.moments and not a.adaptive else "") + ("+aovs" if a.aovs else "")
print(f"{os.path.basename(os.environ.get('RAYFINDER_AMD_LIB', 'default')):34s} {what:24s} accumulate {best[0]:7.3f} ms   frame {best[1]:8.2f} ms   batches {s['batches_traced']:d}   image checksum {int(np.asarray(img).view(np.uint32).astype(np.uint64).sum()):d}")
r.close()
