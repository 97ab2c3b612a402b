#!/usr/bin/env python3
"""What the radiance second moments and the noise estimate cost.

  python tools/noise_timing.py [--repeat 3] [--estimates 20] [--out profiles/noise/noise_timing.json]

Plain atrium stand-in (rayfinder_amd.scenes.atrium()), 1920x1080, 320 spp, 8 bounces, default camera and sky, the whole frame in ONE batch.  Order off, on,
off: the two off runs bracket the on run, so drift of the machine shows as their difference.  Each run: one untimed warm-up frame (it fills the occluder
grid), --repeat frames timed by wall clock around render + synchronize with timing off, then one more frame with per-stage timing on (the moments are timed
with the accumulation).  Images compared bit for bit.  The on run then calls noise_estimate --estimates times (wall clock per call: launch, the copies of
the per-tile results and the wait included; no error map).  Per-kernel times come from running this under `rocprofv3 --kernel-trace --stats`
(profiles/noise/README.md).
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


def run(pt, moments, repeat, estimates):
    cam = rf.fly_camera(W, H)
    tiles = ((W + 31) // 32) * ((H + 31) // 32)
    params = [rf.make_render_parameters(W, H, cam, SPP, BOUNCES, rf.make_sky(), e) for e in (0.25, 0.5)]
    r = rf.ReferencePathTracer(params[0], pt.scene(), max_paths_in_flight=SPP * tiles * 1024)
    r.set_moments(moments)
    r.render(SPP)                                        # warm-up frame
    r.synchronize()
    wall = []
    for i in range(repeat + 1):
        r.set_render_parameters(params[(i + 1) % 2])      # a change: the accumulation (and the moments) restart
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
    stages.update(batches_traced=s["batches_traced"], path_state_bytes=r.memory_info()["path_state_bytes"], moment_samples=r.read_moments()[1])
    est_ms, est = [], None
    if moments:
        lib, C = rf._ffi.lib, rf._ffi.C
        e = rf._ffi.NoiseEstimate()
        for _ in range(estimates + 1):                    # (the first call allocates the per-tile buffers)
            t0 = time.perf_counter()
            rf.check(lib.rf_renderer_noise_estimate(r._h, C.byref(e), None, None, None))
            est_ms.append((time.perf_counter() - t0) * 1e3)
        est_ms = sorted(est_ms[1:])
        est = dict(mean_error=e.mean_error, max_error=e.max_error, worst_tile=e.worst_tile, samples=e.samples, pixels=e.pixels, nonfinite_pixels=e.nonfinite_pixels)
    img = r.read_accumulation()[0]
    r.close()
    return wall, stages, img, est_ms, est


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--estimates", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "noise", "noise_timing.json"))
    args = ap.parse_args()
    pt, info = scenes.atrium()
    runs = [run(pt, on, args.repeat, args.estimates) for on in (False, True, False)]
    off = statistics.median(runs[0][0] + runs[2][0])
    on = statistics.median(runs[1][0])
    est_ms = runs[1][3]
    out = dict(workload=f"atrium stand-in ({info['triangles']} triangles), {W}x{H}, {SPP} spp, {BOUNCES} bounces, one batch", repeats=args.repeat,
               wall_ms_off_before=[round(x, 2) for x in runs[0][0]], wall_ms_on=[round(x, 2) for x in runs[1][0]], wall_ms_off_after=[round(x, 2) for x in runs[2][0]],
               median_ms_off=round(off, 2), median_ms_on=round(on, 2), overhead_pct=round(100.0 * (on - off) / off, 2),
               stages_off=runs[0][1], stages_on=runs[1][1],
               image_identical=bool(np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32))),
               estimate_wall_ms_median=round(est_ms[len(est_ms) // 2], 4) if est_ms else None, estimate_wall_ms_min=round(est_ms[0], 4) if est_ms else None,
               estimate=runs[1][4])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
