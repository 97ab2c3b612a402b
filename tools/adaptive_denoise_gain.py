#!/usr/bin/env python3
"""Denoising adaptively sampled frames: what keeping the AOVs per tile count costs, what the denoiser costs on such a frame, and what the combination buys
(-> profiles/adaptive_denoise/).

  python tools/adaptive_denoise_gain.py [--width 1920 --height 1080 --bounces 8 --spp 256 --every 8 --reference-spp 1024] --out-dir profiles/adaptive_denoise

overhead.json   three kinds of run, --repeat timed runs each, alternating, after one untimed run of each: render() in steps of `every` with set_aovs(True) and the
                moments on (the path that was there before); render_adaptive with target 0 and RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS (a tile whose mean error is
                exactly 0 stops all the same: the books of every run are recorded); and render_adaptive with min_samples = spp, in which no tile can stop
                (asserted: no stopped tile, the uniform run's pixel-samples and primary rays).  The differences of the medians next to the uniform runs' spread.
crosscheck.json 16 spp in two steps on fresh handles: every array (S, Q and the four AOV sums) of the adaptive runs against a uniform handle at each tile's own
                count, element by element, with a second uniform handle as the control (asserted: no element differs).
--sections trace_render_aovs_moments | trace_adaptive_target_0 | trace_adaptive_no_tile_can_stop: three passes of one kind, for a rocprofv3 --kernel-trace --stats
                run of its own.
denoise_timing_nonuniform.json   wall time per rf_renderer_denoise call (+ a synchronize) in the non-uniform state, L = 5, as tools/denoise_timing.py measures it
                in the uniform state.
gain.json       for two targets (the uniform run's per-tile median error at 16 and 64 spp): the RMSE against a uniform --reference-spp render of the same view
                (other samples: the frame counter runs on) of the adaptive frame, plain and denoised, and of a uniform frame of the same number of pixel-samples
                (rounded to whole samples per pixel), plain and denoised.  Recorded figures, not a pass bar.
Every timed run ends with a synchronize."""
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
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--denoise-reps", type=int, default=20)
    ap.add_argument("--sections", default="overhead,crosscheck,denoise,gain")
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    W, H, spp, every = a.width, a.height, a.spp, a.every
    sections = set(a.sections.split(","))
    pt, _ = scenes.atrium(1, a.detail)
    cam, sky = rf.fly_camera(W, H), rf.make_sky()
    expo = [0.25]
    common = dict(scene=f"atrium ({a.detail})", width=W, height=H, bounces=a.bounces, spp=spp, check_every=every)

    def save(name, result):
        print(name, json.dumps(result), flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, name), "w") as f:
                json.dump(result, f, indent=1)

    def fresh(r, n=None):
        expo[0] = 0.75 - expo[0]                                            # a changed parameter restarts the accumulation (and clears the tile counts)
        r.set_render_parameters(rf.make_render_parameters(W, H, cam, n or spp, a.bounces, sky, expo[0]))

    def sums(r):
        s = r.read_aovs()
        return [np.ascontiguousarray(x, np.float32).view(np.uint32) for x in (r.read_accumulation()[0], r.read_moments()[0], s["albedo"], s["coverage"], s["normal"], s["depth"])]

    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, spp, a.bounces, sky, 0.25), pt.scene())
    r.set_moments(True)

    def plain():
        for _ in range(spp // every):
            r.render(every)

    def one_count(res, rays):
        """The books of an adaptive run in which no tile may have stopped"""
        return dict(stopped_tiles=res["stopped_tiles"], pixel_samples=res["pixel_samples"], estimate_passes=res["estimate_passes"], primary_rays=rays)

    # The three kinds of run that are compared.  A target of 0 does NOT keep every tile going: a tile whose mean error is exactly 0 (every pixel without variance so
    # far: black, constant or non-finite) is <= 0 and stops at the first check.  min_samples = spp moves the first (and only) check to the cap: no tile can stop.
    kinds = {"render_aovs_moments": (False, plain),
             "adaptive_target_0": (True, lambda: r.render_adaptive(0.0, every, every)),
             "adaptive_no_tile_can_stop": (True, lambda: r.render_adaptive(0.0, every, spp))}

    def run(kind):
        bit, work = kinds[kind]
        r.set_aovs(True, tile_counts=bit)
        fresh(r)
        r.reset_stats()
        r.synchronize()
        t0 = time.perf_counter()
        res = work()
        r.synchronize()
        t = time.perf_counter() - t0
        rays = r.stats()["primary_rays"]
        return t, (one_count(res, rays) if res is not None else dict(primary_rays=rays))

    for k in kinds:                                                         # under rocprofv3 --kernel-trace --stats: one kind per process, three passes
        if "trace_" + k in sections:
            for _ in range(3):
                print(k, run(k), flush=True)

    if "overhead" in sections:
        times, books = {k: [] for k in kinds}, {k: [] for k in kinds}
        for rep in range(a.repeat + 1):                                     # (run 0 of each kind: untimed warm-up)
            for k in kinds:
                t, b = run(k)
                if rep:
                    times[k].append(t)
                    books[k].append(b)
        med = {k: statistics.median(v) for k, v in times.items()}
        u = times["render_aovs_moments"]
        out = dict(common, repeat=a.repeat, full_pixel_samples=W * H * spp, seconds=times, books=books, uniform_spread_s=max(u) - min(u))
        for k in ("adaptive_target_0", "adaptive_no_tile_can_stop"):
            out[k + "_minus_uniform_s"] = med[k] - med["render_aovs_moments"]
            out[k + "_ratio"] = med[k] / med["render_aovs_moments"]
        save("overhead.json", out)
        for b in books["adaptive_no_tile_can_stop"]:
            assert b["stopped_tiles"] == 0 and b["pixel_samples"] == W * H * spp == b["primary_rays"], b
        for b in books["render_aovs_moments"]:
            assert b["primary_rays"] == W * H * spp, b

    if "crosscheck" in sections:
        # the defining property at this size, 16 spp in two steps of 8, fresh handles (same frame numbers): per array and per tile, with a uniform-against-uniform control
        names = ("S", "Q", "albedo", "coverage", "normal", "depth")

        def handle(kind):
            h = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, 16, a.bounces, sky, 0.25), pt.scene())
            h.set_moments(True)
            h.set_aovs(True, tile_counts=kind != "uniform")
            snaps, res = {}, None
            if kind == "uniform":
                for n in (8, 16):
                    h.render(8)
                    snaps[n] = sums(h)
            else:
                res = h.render_adaptive(0.0, 8, 8 if kind == "target_0" else 16)
                snaps[16] = sums(h)
            counts = h.read_tile_samples()
            rays = h.stats()["primary_rays"]
            h.close()
            return snaps, counts, res, rays

        u1, _, _, rays_u = handle("uniform")
        u2, _, _, _ = handle("uniform")
        per_pixel = lambda counts: np.repeat(np.repeat(counts, 32, 0), 32, 1)[:H, :W]  # noqa: E731
        result = dict(common, spp=16, check_every=8, uniform_primary_rays=rays_u,
                      uniform_vs_uniform={n: int((x != y).sum()) for n, x, y in zip(names, u1[16], u2[16])})
        for kind in ("target_0", "no_tile_can_stop"):
            got, counts, res, rays = handle(kind)
            n_px = per_pixel(counts)
            diff = {}
            for name, x, w8, w16 in zip(names, got[16], u1[8], u1[16]):
                sel = (n_px == 8) if x.ndim == 2 else (n_px == 8)[..., None]
                diff[name] = int((x != np.where(sel, w8, w16)).sum())      # every tile against the uniform handle AT THE TILE'S OWN COUNT
            result[kind] = dict(one_count(res, rays), tile_counts={int(c): int((counts == c).sum()) for c in np.unique(counts)},
                                differing_elements_against_uniform_at_each_tiles_count=diff)
        save("crosscheck.json", result)
        assert not any(result["uniform_vs_uniform"].values()), result["uniform_vs_uniform"]
        for kind in ("target_0", "no_tile_can_stop"):
            assert not any(result[kind]["differing_elements_against_uniform_at_each_tiles_count"].values()), result[kind]
        assert result["no_tile_can_stop"]["stopped_tiles"] == 0 and result["no_tile_can_stop"]["primary_rays"] == rays_u

    r.set_aovs(True, tile_counts=True)
    # per-tile errors of the uniform run at 16 and 64 spp: the two targets
    targets = {}
    if sections & {"denoise", "gain"}:
        fresh(r)
        pixels = np.array([min(32, H - ty * 32) * min(32, W - tx * 32) for ty in range((H + 31) // 32) for tx in range((W + 31) // 32)], np.float32)
        done = 0
        for n in (16, 64):
            r.render(n - done)
            done = n
            targets[n] = float(np.float32(np.median((r.noise_estimate()["tile_sum"] / pixels).astype(np.float32))))

    if "denoise" in sections:
        fresh(r)
        res = r.render_adaptive(targets[16], every, every)
        r.denoise(iterations=5)                                             # (first call: allocates the work buffers)
        r.synchronize()
        ms = []
        for _ in range(a.denoise_reps):
            t0 = time.perf_counter()
            r.denoise(iterations=5)
            r.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        save("denoise_timing_nonuniform.json", dict(width=W, height=H, iterations=5, reps=a.denoise_reps, stopped_tiles=res["stopped_tiles"], tiles=res["tiles"],
                                                    min_tile_samples=res["min_tile_samples"], max_tile_samples=res["max_tile_samples"], wall_ms_median=ms[len(ms) // 2],
                                                    wall_ms_min=ms[0], wall_ms_max=ms[-1]))

    if "gain" in sections:
        fresh(r, a.reference_spp)
        r.render(a.reference_spp)
        ref = r.read_mean()[..., :3].astype(np.float64)

        def rmse(img, clamp=None):
            x, y = img[..., :3].astype(np.float64), ref
            if clamp is not None:
                x, y = np.minimum(x, clamp), np.minimum(y, clamp)
            return float(np.sqrt(np.mean((x - y) ** 2)))

        def figures(plain_mean):
            r.denoise()
            den = r.read_denoised()[0]
            return dict(rmse=rmse(plain_mean), rmse_denoised=rmse(den), rmse_clamped_4=rmse(plain_mean, 4.0), rmse_denoised_clamped_4=rmse(den, 4.0))

        rows = []
        for at, target in targets.items():
            fresh(r)
            res = r.render_adaptive(target, every, every)
            adaptive = figures(r.read_mean())
            equal_spp = max(1, int(round(res["pixel_samples"] / (W * H))))
            fresh(r)
            r.render(equal_spp)
            uniform = figures(r.read_mean())
            rows.append(dict(target_from_spp=at, target=target, adaptive_pixel_samples=res["pixel_samples"], stopped_tiles=res["stopped_tiles"],
                             min_tile_samples=res["min_tile_samples"], max_tile_samples=res["max_tile_samples"], adaptive=adaptive, uniform_spp=equal_spp,
                             uniform_pixel_samples=W * H * equal_spp, uniform=uniform))
            print(json.dumps(rows[-1]), flush=True)
        save("gain.json", dict(common, reference_spp=a.reference_spp, tiles=int(r.read_tile_samples().size), rows=rows))
    r.close()


if __name__ == "__main__":
    main()
