#!/usr/bin/env python3
"""Tile-adaptive sampling: what it saves at equal quality and what it costs when nothing stops (-> profiles/adaptive/).

  python tools/adaptive_gain.py [--detail plain|clutter] [--width 1920 --height 1080 --bounces 8 --spp 256 --every 8] --out gain.json

Gain: for a target T, rf_renderer_render_adaptive's pixel-samples and wall time against the UNIFORM run to the same criterion -- the smallest multiple of
`every` at which every tile's mean error is <= T, found by stepping a uniform handle and estimating at each step.  Three targets: the uniform run's per-tile
median at 16, 64 and 256 spp.  By construction the adaptive run never traces more (asserted).
Overhead: target 0 (no tile ever stops) against render() in the same steps of `every` with the moments on and with them off.
Wall times are medians of --repeat runs after one untimed warm-up run of each kind; every run ends with a synchronize."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detail", default="plain", choices=("plain", "clutter"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H, spp, every = a.width, a.height, a.spp, a.every
    pt, _ = scenes.atrium(1, a.detail)
    cam, sky = rf.fly_camera(W, H), rf.make_sky()
    expo = [0.25]

    def fresh(r):
        expo[0] = 0.75 - expo[0]                                            # a changed parameter restarts the accumulation (and clears the tile counts)
        r.set_render_parameters(rf.make_render_parameters(W, H, cam, spp, a.bounces, sky, expo[0]))

    def timed(r, work):
        fresh(r)
        r.synchronize()
        t0 = time.perf_counter()
        out = work()
        r.synchronize()
        return time.perf_counter() - t0, out

    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, spp, a.bounces, sky, 0.25), pt.scene())
    r.set_moments(True)
    tiles = r.read_tile_samples().size

    # the uniform run, stepped: per-tile errors after every step
    fresh(r)
    pixels = None
    errors = {}
    for n in range(every, spp + 1, every):
        r.render(every)
        e = r.noise_estimate()
        if pixels is None:                                                  # in-frame pixels per tile: from a map of ones
            ones = np.ones((H, W), np.float32)
            pixels = np.array([ones[ty * 32:(ty + 1) * 32, tx * 32:(tx + 1) * 32].sum() for ty in range((H + 31) // 32) for tx in range((W + 31) // 32)], np.float32)
        errors[n] = (e["tile_sum"] / pixels).astype(np.float32)
    targets = {n: float(np.float32(np.median(errors[n]))) for n in (16, 64, 256) if n in errors}

    def uniform_to(n):
        def work():
            for _ in range(n // every):
                r.render(every)
                r.noise_estimate()
        return work

    out = dict(scene=f"atrium ({a.detail})", width=W, height=H, bounces=a.bounces, spp=spp, check_every=every, tiles=int(tiles), repeat=a.repeat, gain=[], overhead={})
    for at, target in targets.items():
        need = next((n for n in sorted(errors) if (errors[n] <= np.float32(target)).all()), None)
        if need is None:
            need = spp                                                      # not reached within spp: the uniform run spends them all
        timed(r, lambda: r.render_adaptive(target, every, every))           # warm-up
        runs = [timed(r, lambda: r.render_adaptive(target, every, every)) for _ in range(a.repeat)]
        res = runs[0][1]
        t_adaptive = statistics.median(t for t, _ in runs)
        t_uniform = statistics.median(timed(r, uniform_to(need))[0] for _ in range(a.repeat))
        uniform_samples = W * H * need
        assert res["pixel_samples"] <= uniform_samples, (res["pixel_samples"], uniform_samples)
        out["gain"].append(dict(target_from_spp=at, target=target, uniform_spp=need, uniform_pixel_samples=uniform_samples, uniform_s=t_uniform,
                                adaptive_pixel_samples=res["pixel_samples"], adaptive_s=t_adaptive, stopped_tiles=res["stopped_tiles"],
                                min_tile_samples=res["min_tile_samples"], max_tile_samples=res["max_tile_samples"], estimate_passes=res["estimate_passes"],
                                sample_ratio=res["pixel_samples"] / uniform_samples, time_ratio=t_adaptive / t_uniform))
        print(json.dumps(out["gain"][-1]), flush=True)

    # overhead when nothing stops
    def plain():
        for _ in range(spp // every):
            r.render(every)

    timed(r, lambda: r.render_adaptive(0.0, every, every))
    t_zero = [timed(r, lambda: r.render_adaptive(0.0, every, every))[0] for _ in range(a.repeat)]
    t_on = [timed(r, plain)[0] for _ in range(a.repeat)]
    r.set_moments(False)
    timed(r, plain)
    t_off = [timed(r, plain)[0] for _ in range(a.repeat)]
    out["overhead"] = dict(adaptive_target_0_s=t_zero, render_moments_on_s=t_on, render_moments_off_s=t_off,
                           ratio_to_moments_off=statistics.median(t_zero) / statistics.median(t_off),
                           spread_moments_off=(max(t_off) - min(t_off)) / statistics.median(t_off))
    r.close()
    print(json.dumps(out["overhead"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
