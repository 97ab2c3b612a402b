#!/usr/bin/env python3
"""Batch-depth sweep for option primary_fused (GPU): the plain atrium at 1920x1080, 8 bounces, on ONE handle -- per samples-per-batch value the option off and on,
two renders each, timing on.  Prints per render: ms_raygen, bounce 1's closest-hit group, the shade group of all bounces, and the whole batch by the host clock
around render + synchronize.  With the option on ms_raygen is 0 and bounce 1's closest-hit group contains generation and shading, so the figure to compare between
the two settings is raygen + bounce-1 closest + shade, or the whole batch.
usage: tools/primary_fused_sweep.py [spp ...]        (default: 16 24 32 64 70 256)"""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import rayfinder_amd as rf
from rayfinder_amd import scenes

depths = [int(a) for a in sys.argv[1:]] or [16, 24, 32, 64, 70, 256]
W, H, B = 1920, 1080, 8
pt, _ = scenes.atrium()
r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, rf.fly_camera(W, H), 1 << 20, B, rf.make_sky(), 0.25), pt.scene())
r.set_timing(True)
r.render(max(depths))          # warm-up: path state of the deepest batch, code objects, the occluder grid
r.synchronize()
for spp in depths:
    row = {}
    for fused in (0, 1):
        r.set_option("primary_fused", fused)
        r.render(spp)          # (untimed: the first batch after a switch)
        r.synchronize()
        runs = []
        for _ in range(2):
            r.reset_stats()
            t0 = time.perf_counter()
            r.render(spp)
            r.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            s, b = r.stats(), r.bounce_stats()
            assert s["batches_traced"] == 1 and s["primary_fused_rays"] == (s["primary_list_rays"] if fused else 0), s
            chain = s["ms_raygen"] + float(b["ms_closest"][0]) + s["ms_shade"]
            runs.append((round(s["ms_raygen"], 3), round(float(b["ms_closest"][0]), 3), round(s["ms_shade"], 3), round(chain, 3), round(ms, 2)))
        row[fused] = runs
    print(f"sweep spp {spp}: (raygen ms, b1 closest ms, shade ms all bounces, their sum, batch ms) off {row[0]} on {row[1]}", flush=True)
r.close()
