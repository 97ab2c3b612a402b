#!/usr/bin/env python3
"""The measurements behind the direct sums under tile-adaptive sampling (profiles/direct_adaptive/README.md).

  python tools/direct_adaptive_measure.py overhead [--out profiles/direct_adaptive/overhead.json]
  python tools/direct_adaptive_measure.py kernels                      (under `rocprofv3 --kernel-trace --stats`: the per-kernel times of the tile-list sum launches)

Both: the bench scene (the atrium stand-in) at 1920x1080, 8 bounces, 64 spp, rf_renderer_render_adaptive with check_every = 16 -- every batch runs under a tile list,
16 samples deep: the LDS-staged sum kernels -- and a target that stops about half of the tiles at the first check (the median of the handle's own tile errors after
16 samples, taken once from a probe frame).
overhead: whole adaptive frames with the direct sums off, on (1 | RF_DIRECT_TILE_COUNTS), off: wall clock of three frames each, then one frame with stage timing on
          (ms_accumulate, launches_accumulate); S compared bit for bit.
kernels:  two adaptive frames with the direct sums on, nothing else: the profiler's kernel statistics carry kSumRuns<RadianceSum, true> (D) next to
          kSumRuns<RadianceMomentSum, true> (S and Q) over the same batches.  RAYFINDER_AMD_LIB picks an experiment build of the library.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402

W, H, SPP, BOUNCES, EVERY = 1920, 1080, 64, 8, 16


def _params(exposure):
    return rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), exposure)


def _target(pt):
    r = rf.ReferencePathTracer(_params(0.25), pt.scene())
    r.set_moments(True)
    r.render(EVERY)
    est = r.noise_estimate()
    r.close()
    tiles_x = (W + 31) // 32
    pixels = np.array([min(32, W - 32 * (t % tiles_x)) * min(32, H - 32 * (t // tiles_x)) for t in range(est["tile_sum"].size)], np.float32)
    return float(np.median(est["tile_sum"].reshape(-1) / pixels))


def _handle(pt, direct):
    r = rf.ReferencePathTracer(_params(0.25), pt.scene())
    r.set_moments(True)
    if direct:
        r.set_direct(True, tile_counts=True)
    return r


def overhead(out):
    pt, _ = scenes.atrium()
    target = _target(pt)
    runs = []
    for on in (False, True, False):
        r = _handle(pt, on)
        res = r.render_adaptive(target, EVERY)                               # warm-up frame
        wall = []
        for i in range(4):
            r.set_render_parameters(_params(0.5 if i % 2 == 0 else 0.25))
            if i == 3:
                r.reset_stats()
                r.set_timing(True)
            t0 = time.perf_counter()
            res = r.render_adaptive(target, EVERY)                           # (waits for the work it enqueues)
            if i < 3:
                wall.append(round((time.perf_counter() - t0) * 1e3, 3))
        s = r.stats()
        runs.append(dict(direct=on, wall_ms=wall, ms_accumulate=round(s["ms_accumulate"], 4), launches_accumulate=s["launches_accumulate"], batches_traced=s["batches_traced"],
                         stopped_tiles=res["stopped_tiles"], tiles=res["tiles"], pixel_samples=res["pixel_samples"], direct_samples=r.read_direct()[1],
                         path_state_bytes=r.memory_info()["path_state_bytes"]))
        runs[-1]["image"] = r.read_accumulation()[0]
        r.close()
    same = bool(np.array_equal(runs[0]["image"].view(np.uint32), runs[1]["image"].view(np.uint32)))
    for run in runs:
        del run["image"]
    off = 0.5 * (runs[0]["ms_accumulate"] + runs[2]["ms_accumulate"])
    res = dict(workload=f"atrium stand-in, {W}x{H}, {SPP} spp, {BOUNCES} bounces, render_adaptive(target {target:.6g}, check_every {EVERY})", runs=runs, image_identical=same,
               added_ms_accumulate_per_frame=round(runs[1]["ms_accumulate"] - off, 4),
               added_ms_accumulate_per_batch=round((runs[1]["ms_accumulate"] - off) / max(runs[1]["batches_traced"], 1), 4))
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def kernels():
    pt, _ = scenes.atrium()
    target = _target(pt)
    r = _handle(pt, True)
    for exposure in (0.25, 0.5):
        r.set_render_parameters(_params(exposure))
        res = r.render_adaptive(target, EVERY)
    print(json.dumps(dict(target=target, stopped_tiles=res["stopped_tiles"], tiles=res["tiles"], batches_traced=r.stats()["batches_traced"])))
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("overhead", "kernels"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    overhead(a.out) if a.what == "overhead" else kernels()


if __name__ == "__main__":
    main()
