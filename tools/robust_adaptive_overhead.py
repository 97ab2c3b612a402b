#!/usr/bin/env python3
"""What the bucket sums cost under tile-adaptive sampling, and what the per-tile combine and robust denoise cost (-> profiles/robust_adaptive/).

  python tools/robust_adaptive_overhead.py [--repeat 3] [--reps 20] [--sections overhead,combine,uniform] [--tree DIR --tag NAME] --out-dir profiles/robust_adaptive

Plain atrium stand-in (rayfinder_amd.scenes.atrium()), 1920x1080, 8 bounces, default camera and sky, 64 spp, check_every 8, min_samples 16 (>= K for both K).
The target is the median of the handle's own per-tile errors after a uniform render(16): about half the tiles stop at the first check.
overhead.json  wall time of ONE rf_renderer_render_adaptive call (a fresh accumulation each time; the call waits for its work) with the buckets off, with
               K = 9 | RF_BUCKETS_TILE_COUNTS, with K = 15 | RF_BUCKETS_TILE_COUNTS and off again: the two off runs bracket the others, so drift of the machine shows as
               their difference.  Each run: one untimed call, then --repeat timed ones.  The schedule (tile counts, pixel-samples) and the image are compared across
               the runs: the buckets must not show in them.
combine.json   in the non-uniform state that call leaves (K = 9, the AOVs with RF_AOV_TILE_COUNTS): wall time per rf_renderer_robust_mean, per
               rf_renderer_denoise_robust (L = 5) and per rf_renderer_denoise call plus a synchronize, --reps calls each after an untimed one.  Each of them first
               waits for the stream and copies the per-tile counts to the device, as every per-tile read does.
uniform_combine[_TAG].json  the UNIFORM state's combine, which this feature re-factored (kRobustMean<K> now calls the body it shares with kRobustMeanTiles<K>, and its
               register allocation moved for K >= 9): wall time per rf_renderer_robust_mean call plus a synchronize after a uniform render(64), K = 9, 11, 13, 15.
               `--sections uniform --tree DIR --tag NAME` runs this one section against the built checkout at DIR (the parent commit's, say), which needs nothing
               newer than rf_renderer_set_buckets(K).
Recorded figures, not pass bars."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

_TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv[:-1] else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(_TREE))
import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402

W, H, SPP, BOUNCES, EVERY, MIN = 1920, 1080, 64, 8, 8, 16


def params(exposure):
    return rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), exposure)


def handle(pt, k, aovs=False):
    r = rf.ReferencePathTracer(params(0.25), pt.scene())
    r.set_moments(True)
    if aovs:
        r.set_aovs(True, tile_counts=True)
    if k:
        r.set_buckets(k, tile_counts=True)
    return r


def adaptive_run(pt, k, target, repeat):
    r = handle(pt, k)
    wall, res = [], None
    for i in range(repeat + 1):
        r.set_render_parameters(params(0.5 if i % 2 == 0 else 0.25))      # a change: the accumulation (and the bucket sums) restart
        r.synchronize()
        t0 = time.perf_counter()
        res = r.render_adaptive(target, EVERY, MIN)
        r.synchronize()
        if i > 0:                                                          # (the first call is the warm-up)
            wall.append((time.perf_counter() - t0) * 1e3)
    counts = r.read_tile_samples().reshape(-1)
    img = r.read_accumulation()[0]
    out = dict(wall_ms=[round(x, 2) for x in wall], median_ms=round(statistics.median(wall), 2), stopped_tiles=res["stopped_tiles"], tiles=res["tiles"],
               pixel_samples=res["pixel_samples"], estimate_passes=res["estimate_passes"], bucket_samples=r.read_buckets()[1])
    r.close()
    return out, counts, img


def timed(r, call, reps):
    """wall time of `call` plus a synchronize, `reps` times after an untimed first call (which allocates the work buffers)"""
    call()
    r.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        r.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return dict(wall_ms_median=round(ms[len(ms) // 2], 4), wall_ms_min=round(ms[0], 4), wall_ms_max=round(ms[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default="")
    ap.add_argument("--sections", default="overhead,combine")
    ap.add_argument("--tree", default="", help="the built checkout whose rayfinder_amd is measured (default: this one)")
    ap.add_argument("--tag", default="", help="suffix of uniform_combine.json")
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    pt, info = scenes.atrium()
    workload = f"atrium stand-in ({info['triangles']} triangles), {W}x{H}, {BOUNCES} bounces, {SPP} spp, check_every {EVERY}, min_samples {MIN}"

    def save(name, result):
        print(name, json.dumps(result), flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, name), "w") as f:
                json.dump(result, f, indent=1)

    if "uniform" in sections:
        result = dict(width=W, height=H, samples=SPP, reps=a.reps, tree=a.tag or "this")
        for k in (9, 11, 13, 15):
            r = rf.ReferencePathTracer(params(0.25), pt.scene())
            r.set_buckets(k)
            r.render(SPP)
            result[f"K{k}"] = timed(r, r.robust_mean, a.reps)
            r.close()
        save("uniform_combine" + ("_" + a.tag if a.tag else "") + ".json", result)
    if not sections & {"overhead", "combine"}:
        return

    r = handle(pt, 0)
    r.render(MIN)
    est = r.noise_estimate()
    r.close()
    tiles_x = (W + 31) // 32
    pixels = np.array([min(32, W - 32 * (t % tiles_x)) * min(32, H - 32 * (t // tiles_x)) for t in range(est["tile_sum"].size)], np.float32)
    target = float(np.float32(np.median(est["tile_sum"].reshape(-1) / pixels)))

    order = (0, 9, 15, 0)
    runs = [adaptive_run(pt, k, target, a.repeat) for k in order]
    off = statistics.median(runs[0][0]["wall_ms"] + runs[3][0]["wall_ms"])
    out = dict(workload=workload, target_tile_error=target, repeats=a.repeat, off_before=runs[0][0], off_after=runs[3][0], median_ms_off=round(off, 2))
    for k, (res, counts, img) in zip(order[1:3], runs[1:3]):
        out[f"K{k}"] = dict(res, overhead_ms=round(res["median_ms"] - off, 2), overhead_pct=round(100.0 * (res["median_ms"] - off) / off, 2),
                            schedule_identical=bool(np.array_equal(counts, runs[0][1])), image_identical=bool(np.array_equal(img.view(np.uint32), runs[0][2].view(np.uint32))),
                            plane_bytes=16 * k * counts.size * 1024)
    save("overhead.json", out)

    r = handle(pt, 9, aovs=True)
    res = r.render_adaptive(target, EVERY, MIN)
    result = dict(width=W, height=H, K=9, iterations=5, reps=a.reps, stopped_tiles=res["stopped_tiles"], tiles=res["tiles"], min_tile_samples=res["min_tile_samples"],
                  max_tile_samples=res["max_tile_samples"])
    for name, call in (("robust_mean", r.robust_mean), ("denoise_robust", r.denoise_robust), ("denoise", r.denoise)):
        result[name] = timed(r, call, a.reps)
    rob = r.read_robust_mean()
    result.update(share_trimmed=float((rob["trim"] > 0).mean()), mean_trim=float(rob["trim"].mean()))
    r.close()
    save("combine.json", result)


if __name__ == "__main__":
    main()
