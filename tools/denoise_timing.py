"""Kernel time of the a-trous denoiser (rf_renderer_denoise) on the 1080p atrium stand-in.

usage: python tools/denoise_timing.py [--width 1920] [--height 1080] [--spp 4] [--iterations 5] [--reps 20] [--out result.json]

Renders `spp` samples with the first-hit AOVs on, then calls denoise `reps` times and reports the wall time per call (denoise + a synchronize:
launch overheads included).  Per-kernel times come from running this under `rocprofv3 --kernel-trace --stats` (profiles/denoise/README.md)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pt, _ = scenes.atrium()
    W, H = a.width, a.height
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), a.spp, a.bounces, rf.make_sky(), 0.25)
    r = rf.ReferencePathTracer(params, pt.scene())
    r.set_aovs(True)
    r.render(a.spp)
    r.synchronize()
    r.denoise(iterations=a.iterations)  # (first call: allocates the work buffers)
    r.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r.denoise(iterations=a.iterations)
        r.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    r.close()
    times.sort()
    res = dict(width=W, height=H, spp=a.spp, iterations=a.iterations, reps=a.reps, wall_ms_median=times[len(times) // 2], wall_ms_min=times[0],
               wall_ms_max=times[-1])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
