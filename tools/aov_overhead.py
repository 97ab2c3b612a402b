#!/usr/bin/env python3
"""What the first-hit AOVs cost: the same frame with the AOVs off and on.

  python tools/aov_overhead.py [--repeat 5] [--out profiles/aov/aov_overhead.json]

Plain atrium stand-in (rayfinder_amd.scenes.atrium()), 1920x1080, 320 spp, 8 bounces, default camera and sky, the whole frame in ONE batch (~100 GB of
path state off, ~120 GB on: one renderer at a time).  Order off, on, off: the two off runs bracket the on run, so drift of the machine shows as their
difference.  Each run: one untimed warm-up frame (it fills the occluder grid), --repeat frames timed by wall clock around render + synchronize with
timing off (the headline), then one more frame with per-stage timing on (raygen / closest / shade / shadow / accumulate).  Images compared bit for bit.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402

W, H, SPP, BOUNCES = 1920, 1080, 320, 8


def run(pt, aov, repeat):
    cam = rf.fly_camera(W, H)
    tiles = ((W + 31) // 32) * ((H + 31) // 32)
    params = [rf.make_render_parameters(W, H, cam, SPP, BOUNCES, rf.make_sky(), e) for e in (0.25, 0.5)]
    r = rf.ReferencePathTracer(params[0], pt.scene(), max_paths_in_flight=SPP * tiles * 1024)
    r.set_aovs(aov)
    r.render(SPP)                                        # warm-up frame
    r.synchronize()
    wall = []
    for i in range(repeat + 1):
        r.set_render_parameters(params[(i + 1) % 2])      # a change: the accumulation (and the AOV sums) restart
        if i == repeat:
            r.reset_stats()
            r.set_timing(True)
        t0 = time.perf_counter()
        r.render(SPP)
        r.synchronize()
        if i < repeat:
            wall.append((time.perf_counter() - t0) * 1e3)
    s = r.stats()
    stages = {k: round(s[k], 3) for k in ("ms_raygen", "ms_closest", "ms_shade", "ms_shadow", "ms_accumulate")}
    stages.update(batches_traced=s["batches_traced"], path_state_bytes=r.memory_info()["path_state_bytes"], aov_samples=r.read_aovs()["samples"])
    img = r.read_accumulation()[0]
    r.close()
    return wall, stages, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "aov", "aov_overhead.json"))
    args = ap.parse_args()
    pt, info = scenes.atrium()
    runs = [run(pt, aov, args.repeat) for aov in (False, True, False)]
    off = statistics.median(runs[0][0] + runs[2][0])
    on = statistics.median(runs[1][0])
    out = dict(workload=f"atrium stand-in ({info['triangles']} triangles), {W}x{H}, {SPP} spp, {BOUNCES} bounces, one batch", repeats=args.repeat,
               wall_ms_off_before=[round(x, 2) for x in runs[0][0]], wall_ms_on=[round(x, 2) for x in runs[1][0]], wall_ms_off_after=[round(x, 2) for x in runs[2][0]],
               median_ms_off=round(off, 2), median_ms_on=round(on, 2), overhead_pct=round(100.0 * (on - off) / off, 2),
               stages_off=runs[0][1], stages_on=runs[1][1],
               image_identical=bool(np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32))))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
