#!/usr/bin/env python3
"""The measurements behind the direct sums and the split-component denoiser (profiles/split_denoise/README.md).

  python tools/split_denoise_measure.py sweep   [--out profiles/split_denoise/sweep.json]
  python tools/split_denoise_measure.py timing  [--out profiles/split_denoise/filter_timing.json] [--reps 15]
  python tools/split_denoise_measure.py direct  [--out profiles/split_denoise/direct_overhead.json]

sweep:  the two frames of the denoiser's quality test (atrium 480x270 and Duck 160x120, 4 spp against 1024 spp of the same parameters, MSE over covered pixels as
        a ratio to the noisy frame's): L and sigma_color of each component over a grid (sigma_normal / sigma_depth at the one filter's defaults), the one filter's
        default on the same frames next to it, and the pair with the lowest mean ratio among those that beat the one filter on BOTH frames (none: null).
timing: 1080p atrium, 4 spp / 2 bounces: rf_renderer_denoise (L = 5) and rf_renderer_denoise_split (L = 5 for both components, equal and unequal sigma_normal /
        sigma_depth), alternating, wall clock around the call plus a synchronize; medians.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.
direct: 1080p atrium, 64 spp / 8 bounces in one batch, stage timing on: ms_accumulate and launches_accumulate with the direct sums off, on, off; the images compared
        bit for bit.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402

DUCK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "Duck.glb")
# (wide on purpose: the direct component down to no filtering at all, the indirect one out to a colour term that is as good as off -- the best pair sits at those
# ends, profiles/split_denoise/README.md)
L_DIRECT, SC_DIRECT = (0, 1, 2, 3, 5), (0.0625, 0.125, 0.25, 0.5, 1.0)
L_INDIRECT, SC_INDIRECT = (1, 2, 3, 4, 5, 6), (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0)


def _frame(pt, W, H, bounces):
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), 1024, bounces, rf.make_sky(), 0.25)
    ref = rf.ReferencePathTracer(params, pt.scene())
    ref.render(1024)
    truth = ref.read_accumulation()[0][..., :3] / np.float32(1024)
    ref.close()
    r = rf.ReferencePathTracer(params, pt.scene())
    r.set_aovs(True)
    r.set_direct(True)
    r.render(4)
    cov = r.read_aovs()["coverage"] > 0
    mse = lambda img: float(((img.astype(np.float64) - truth)[cov] ** 2).mean())   # noqa: E731
    base = mse(r.read_accumulation()[0][..., :3] / np.float32(4))
    r.denoise()
    one = mse(r.read_denoised()[0]) / base
    grid = {}
    for ld, sd, li, si in itertools.product(L_DIRECT, SC_DIRECT, L_INDIRECT, SC_INDIRECT):
        r.denoise_split(direct=dict(iterations=ld, sigma_color=sd, sigma_normal=0.1, sigma_depth=0.1), indirect=dict(iterations=li, sigma_color=si, sigma_normal=0.1, sigma_depth=0.1))
        grid[(ld, sd, li, si)] = mse(r.read_denoised()[0]) / base
    r.close()
    return one, grid


def sweep(out):
    atrium, _ = scenes.atrium()
    duck = rf.PtFormat.from_gltf(DUCK)
    one_a, grid_a = _frame(atrium, 480, 270, 4)
    one_d, grid_d = _frame(duck, 160, 120, 4)
    rows = sorted(((0.5 * (grid_a[k] + grid_d[k]), k) for k in grid_a))
    beat = [(m, k) for m, k in rows if grid_a[k] < one_a and grid_d[k] < one_d]
    row = lambda k: dict(L_direct=k[0], sigma_color_direct=k[1], L_indirect=k[2], sigma_color_indirect=k[3], atrium=round(grid_a[k], 5), duck=round(grid_d[k], 5),  # noqa: E731
                         mean=round(0.5 * (grid_a[k] + grid_d[k]), 5))
    same = (5, 1.0, 5, 1.0)
    # per component: the best mean ratio reachable at each (L, sigma_color) of that component, over the other component's grid
    marg_d = {f"L{ld} sc{sd}": round(min(0.5 * (grid_a[k] + grid_d[k]) for k in grid_a if k[:2] == (ld, sd)), 5) for ld in L_DIRECT for sd in SC_DIRECT}
    marg_i = {f"L{li} sc{si}": round(min(0.5 * (grid_a[k] + grid_d[k]) for k in grid_a if k[2:] == (li, si)), 5) for li in L_INDIRECT for si in SC_INDIRECT}
    res = dict(metric="MSE over covered pixels of the filtered 4-spp frame against 1024 spp, divided by the noisy 4-spp frame's", sigma_normal=0.1, sigma_depth=0.1,
               one_filter_default=dict(atrium=round(one_a, 5), duck=round(one_d, 5), mean=round(0.5 * (one_a + one_d), 5)),
               split_with_the_one_filters_defaults=row(same), pairs=len(rows), pairs_that_beat_the_one_filter_on_both=len(beat),
               chosen=row(beat[0][1]) if beat else None, best_20_by_mean=[row(k) for _, k in rows[:20]], best_by_direct_setting=marg_d, best_by_indirect_setting=marg_i,
               best_atrium=row(min(grid_a, key=grid_a.get)), best_duck=row(min(grid_d, key=grid_d.get)))
    _write(out, res)


def timing(out, reps):
    pt, _ = scenes.atrium()
    W, H, spp = 1920, 1080, 4
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), spp, 2, rf.make_sky(), 0.25)
    r = rf.ReferencePathTracer(params, pt.scene())
    r.set_aovs(True)
    r.set_direct(True)
    r.render(spp)
    r.synchronize()
    p5 = dict(iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1)
    other = dict(p5, sigma_normal=0.2, sigma_depth=0.05)
    calls = dict(one_filter=lambda: r.denoise(**p5), split_shared_guides=lambda: r.denoise_split(direct=p5, indirect=p5),
                 split_own_guides=lambda: r.denoise_split(direct=p5, indirect=other), split_direct_2_indirect_5=lambda: r.denoise_split(direct=dict(p5, iterations=2), indirect=p5))
    for f in calls.values():                                                 # (first calls: the work buffers)
        f()
    r.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():                                           # alternating
            t0 = time.perf_counter()
            f()
            r.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    r.close()
    res = dict(width=W, height=H, spp=spp, reps=reps, what="wall clock around the call plus a synchronize, ms; launch overheads of prep, the passes and the tonemap included")
    for k, t in times.items():
        res[k] = dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4))
    _write(out, res)


def direct(out):
    pt, _ = scenes.atrium()
    W, H, spp, bounces = 1920, 1080, 64, 8
    tiles = ((W + 31) // 32) * ((H + 31) // 32)
    params = [rf.make_render_parameters(W, H, rf.fly_camera(W, H), spp, bounces, rf.make_sky(), e) for e in (0.25, 0.5)]
    runs = []
    for on in (False, True, False):
        r = rf.ReferencePathTracer(params[0], pt.scene(), max_paths_in_flight=spp * tiles * 1024)
        r.set_direct(on)
        r.render(spp)                                                        # warm-up frame
        r.synchronize()
        wall = []
        for i in range(4):
            r.set_render_parameters(params[(i + 1) % 2])
            if i == 3:
                r.reset_stats()
                r.set_timing(True)
            t0 = time.perf_counter()
            r.render(spp)
            r.synchronize()
            if i < 3:
                wall.append(round((time.perf_counter() - t0) * 1e3, 3))
        s = r.stats()
        runs.append(dict(direct=on, wall_ms=wall, ms_accumulate=round(s["ms_accumulate"], 4), launches_accumulate=s["launches_accumulate"], batches_traced=s["batches_traced"],
                         path_state_bytes=r.memory_info()["path_state_bytes"], direct_samples=r.read_direct()[1]))
        runs[-1]["image"] = r.read_accumulation()[0]
        r.close()
    same = bool(np.array_equal(runs[0]["image"].view(np.uint32), runs[1]["image"].view(np.uint32)))
    for run in runs:
        del run["image"]
    res = dict(workload=f"atrium stand-in, {W}x{H}, {spp} spp, {bounces} bounces, one batch", runs=runs, image_identical=same,
               added_ms_accumulate_per_batch=round(runs[1]["ms_accumulate"] - 0.5 * (runs[0]["ms_accumulate"] + runs[2]["ms_accumulate"]), 4))
    _write(out, res)


def _write(out, res):
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("sweep", "timing", "direct"))
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if a.what == "sweep":
        sweep(a.out)
    elif a.what == "timing":
        timing(a.out, a.reps)
    else:
        direct(a.out)


if __name__ == "__main__":
    main()
