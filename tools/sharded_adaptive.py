#!/usr/bin/env python3
"""Tile-adaptive sampling across ranks: what the slot addressing costs and what a static deal leaves (-> profiles/sharded_adaptive/).

  python tools/sharded_adaptive.py [--detail plain|clutter] [--width 1920 --height 1080 --bounces 8 --spp 256 --every 8] --out-dir DIR

The configuration is tools/adaptive_gain.py's.  The target is the uniform run's per-tile median error at 64 spp.
overhead.json: rf_comm_render_adaptive on a world-size-1 communicator (slot addressing: ShardList sum kernels, kNoiseEstimateSlots, four all-reduces) against
  rf_renderer_render_adaptive on the same handle and frame, for that target and for target 0 (only tiles without any variance stop); --repeat timed runs each, alternating, after one
  untimed run of each; every run ends with a synchronize.  Both leave the same tile counts (asserted).
balance.json: the per-tile sample map of one un-sharded adaptive run, dealt by tiles_for_rank for worlds 2, 4 and 8: pixel-samples per rank and mean / max -- the
  efficiency a static deal leaves under adaptive sampling.  Host arithmetic over one run's map."""
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
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    W, H, spp, every = a.width, a.height, a.spp, a.every
    pt, _ = scenes.atrium(1, a.detail)
    cam, sky = rf.fly_camera(W, H), rf.make_sky()
    expo = [0.25]

    def fresh(r):
        expo[0] = 0.75 - expo[0]                                            # a changed parameter restarts the accumulation (and clears the tile counts)
        r.set_render_parameters(rf.make_render_parameters(W, H, cam, spp, a.bounces, sky, expo[0]))

    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, spp, a.bounces, sky, 0.25), pt.scene())
    r.set_moments(True)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    tx, ty = (W + 31) // 32, (H + 31) // 32
    pixels = np.array([min(32, W - x * 32) * min(32, H - y * 32) for y in range(ty) for x in range(tx)], np.int64)

    r.render(64)
    target = float(np.float32(np.median(r.noise_estimate()["tile_sum"] / pixels.astype(np.float32))))

    def timed(work):
        fresh(r)
        r.synchronize()
        t0 = time.perf_counter()
        res = work()
        r.synchronize()
        return time.perf_counter() - t0, res, r.read_tile_samples().reshape(-1).astype(np.int64)

    out = dict(scene=f"atrium ({a.detail})", width=W, height=H, bounces=a.bounces, spp=spp, check_every=every, tiles=int(tx * ty), repeat=a.repeat,
               transport="local" if comm.local_transport() else "rccl", cases=[])
    counts_at_target = None
    for name, t in (("median tile error at 64 spp", target), ("target 0: only tiles without any variance stop", 0.0)):
        kinds = dict(renderer=lambda: r.render_adaptive(t, every, every), comm=lambda: comm.render_adaptive(r, t, every, every)["rank"])
        for work in kinds.values():
            timed(work)                                                      # untimed: one run of each kind first
        seconds, counts, results = {k: [] for k in kinds}, {}, {}
        for _ in range(a.repeat):
            for k, work in kinds.items():                                    # alternating
                s, results[k], counts[k] = timed(work)
                seconds[k].append(s)
        assert np.array_equal(counts["renderer"], counts["comm"]) and results["renderer"]["pixel_samples"] == results["comm"]["pixel_samples"]
        if t != 0.0:
            counts_at_target = counts["renderer"]
        med = {k: statistics.median(v) for k, v in seconds.items()}
        out["cases"].append(dict(case=name, target_tile_error=t, pixel_samples=int(results["comm"]["pixel_samples"]), of=W * H * spp,
                                 estimate_passes=int(results["comm"]["estimate_passes"]), seconds=seconds, median_seconds=med,
                                 comm_over_renderer=med["comm"] / med["renderer"]))
        print(json.dumps(out["cases"][-1]), flush=True)

    balance = dict(scene=out["scene"], width=W, height=H, bounces=a.bounces, spp=spp, check_every=every, target_tile_error=target,
                   tile_samples_min=int(counts_at_target.min()), tile_samples_max=int(counts_at_target.max()), pixel_samples=int((pixels * counts_at_target).sum()), worlds={})
    for world in (2, 4, 8):
        per_rank = [int((pixels[t] * counts_at_target[t]).sum()) for t in (rf.tiles_for_rank(W, H, k, world) for k in range(world))]
        balance["worlds"][str(world)] = dict(pixel_samples_per_rank=per_rank, mean_over_max=statistics.mean(per_rank) / max(per_rank))
    print(json.dumps(balance["worlds"]), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        json.dump(out, open(os.path.join(a.out_dir, "overhead.json"), "w"), indent=1)
        json.dump(balance, open(os.path.join(a.out_dir, "balance.json"), "w"), indent=1)
    comm.close()
    r.close()


if __name__ == "__main__":
    main()
