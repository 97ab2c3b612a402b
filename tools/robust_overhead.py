#!/usr/bin/env python3
"""What the bucket sums cost, what the robust mean costs, and what it buys (-> profiles/robust/).

  python tools/robust_overhead.py [--repeat 3] [--sections overhead,combine,gain] --out-dir profiles/robust

Plain atrium stand-in (rayfinder_amd.scenes.atrium()), 1920x1080, 8 bounces, default camera and sky.
overhead.json        ms per 320-spp batch (the whole frame in ONE batch, ~100 GB of path state: one renderer at a time) with the buckets off, K = 9, K = 15 and off
                     again: the two off runs bracket the others, so drift of the machine shows as their difference.  Each run: one untimed warm-up frame, --repeat
                     frames timed by wall clock around render + synchronize with timing off, then one more frame with per-stage timing on.  rf_stats times the
                     batch's sums as ONE stage (ms_accumulate: the image kernel, and the bucket kernel behind it while the buckets are on), so the bucket kernel's own
                     time is ms_accumulate with the buckets on minus ms_accumulate with them off.  Beside it the bytes the bucket kernel must move -- one read of the
                     radiance stream (16 B per path slot) plus a read and a write of K planes (32 B per pixel and plane) -- and the rate that time amounts to.
                     The image is compared bit for bit across the runs.
combine_timing.json  wall time per rf_renderer_robust_mean and per rf_renderer_denoise_robust call (+ a synchronize) at 1080p, K = 9, L = 5.
gain.json            the protocol of profiles/adaptive_denoise/gain.json for the robust mean: RMSE (rgb, linear; raw and with both images clamped at 4.0) against a
                     uniform --reference-spp render of the same view made from other samples (the frame counter runs on), of the plain mean, the robust mean, the
                     denoised and the robust-denoised frame at 16 and 64 spp, K = 9, with the mean trim count and the share of pixels with trim > 0.  Recorded
                     figures, not a pass bar.
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

W, H, SPP, BOUNCES = 1920, 1080, 320, 8
TILES = ((W + 31) // 32) * ((H + 31) // 32)


def batch_run(pt, k, repeat):
    cam = rf.fly_camera(W, H)
    params = [rf.make_render_parameters(W, H, cam, SPP, BOUNCES, rf.make_sky(), e) for e in (0.25, 0.5)]
    r = rf.ReferencePathTracer(params[0], pt.scene(), max_paths_in_flight=SPP * TILES * 1024)
    r.set_buckets(k)
    r.render(SPP)                                        # warm-up frame
    r.synchronize()
    wall = []
    for i in range(repeat + 1):
        r.set_render_parameters(params[(i + 1) % 2])      # a change: the accumulation (and the bucket sums) restart
        if i == repeat:
            r.reset_stats()
            r.set_timing(True)
        t0 = time.perf_counter()
        r.render(SPP)
        r.synchronize()
        if i < repeat:
            wall.append((time.perf_counter() - t0) * 1e3)
    s = r.stats()
    stages = {name: round(s[name], 3) for name in ("ms_raygen", "ms_closest", "ms_shade", "ms_shadow", "ms_accumulate")}
    stages.update(batches_traced=s["batches_traced"], launches_accumulate=s["launches_accumulate"], path_state_bytes=r.memory_info()["path_state_bytes"],
                  bucket_samples=r.read_buckets()[1])
    img = r.read_accumulation()[0]
    r.close()
    return wall, stages, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--combine-reps", type=int, default=20)
    ap.add_argument("--sections", default="overhead,combine,gain")
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    pt, info = scenes.atrium()
    workload = f"atrium stand-in ({info['triangles']} triangles), {W}x{H}, {BOUNCES} bounces"

    def save(name, result):
        print(name, json.dumps(result), flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, name), "w") as f:
                json.dump(result, f, indent=1)

    if "overhead" in sections:
        order = (0, 9, 15, 0)
        runs = [batch_run(pt, k, a.repeat) for k in order]
        off = statistics.median(runs[0][0] + runs[3][0])
        acc_off = statistics.mean((runs[0][1]["ms_accumulate"], runs[3][1]["ms_accumulate"]))
        out = dict(workload=workload + f", {SPP} spp in one batch", repeats=a.repeat, wall_ms_off_before=[round(x, 2) for x in runs[0][0]],
                   wall_ms_off_after=[round(x, 2) for x in runs[3][0]], median_ms_off=round(off, 2), stages_off_before=runs[0][1], stages_off_after=runs[3][1],
                   ms_accumulate_off=round(acc_off, 3))
        for k, (wall, stages, img) in zip(order[1:3], runs[1:3]):
            on = statistics.median(wall)
            kernel_ms = stages["ms_accumulate"] - acc_off
            bytes_moved = 16 * SPP * TILES * 1024 + 2 * 16 * k * W * H
            out[f"K{k}"] = dict(wall_ms=[round(x, 2) for x in wall], median_ms=round(on, 2), overhead_ms=round(on - off, 2), overhead_pct=round(100.0 * (on - off) / off, 2),
                                stages=stages, bucket_kernel_ms=round(kernel_ms, 3), bucket_kernel_bytes=bytes_moved,
                                bucket_kernel_gb_per_s=round(bytes_moved / (kernel_ms * 1e-3) / 1e9, 1) if kernel_ms > 0 else None,
                                plane_bytes=16 * k * TILES * 1024,
                                image_identical=bool(np.array_equal(runs[0][2].view(np.uint32), img.view(np.uint32))))
        save("overhead.json", out)

    if not sections & {"combine", "gain"}:
        return
    cam, sky = rf.fly_camera(W, H), rf.make_sky()
    expo = [0.25]
    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, 64, BOUNCES, sky, 0.25), pt.scene())
    r.set_aovs(True)
    r.set_buckets(9)

    def fresh(n):
        expo[0] = 0.75 - expo[0]                                            # a changed parameter restarts the accumulation (and clears the bucket sums)
        r.set_render_parameters(rf.make_render_parameters(W, H, cam, n, BOUNCES, sky, expo[0]))

    if "combine" in sections:
        fresh(64)
        r.render(64)
        result = dict(width=W, height=H, K=9, samples=64, iterations=5, reps=a.combine_reps)
        for name, call in (("robust_mean", r.robust_mean), ("denoise_robust", r.denoise_robust), ("denoise", r.denoise)):
            call()                                                          # (first call: allocates the work buffers)
            r.synchronize()
            ms = []
            for _ in range(a.combine_reps):
                t0 = time.perf_counter()
                call()
                r.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            ms.sort()
            result[name] = dict(wall_ms_median=ms[len(ms) // 2], wall_ms_min=ms[0], wall_ms_max=ms[-1])
        save("combine_timing.json", result)

    if "gain" in sections:
        rows = []
        frames = {}
        for n in (16, 64):
            fresh(n)
            r.render(n)
            plain = r.read_mean()[..., :3]
            r.robust_mean()
            rob = r.read_robust_mean()
            r.denoise()
            den = r.read_denoised()[0]
            r.denoise_robust()
            rden = r.read_denoised()[0]
            frames[n] = dict(plain=plain, robust=rob["mean"], denoised=den, robust_denoised=rden, trim=rob["trim"])
        r.set_buckets(0)
        fresh(a.reference_spp)
        r.render(a.reference_spp)
        ref = r.read_mean()[..., :3].astype(np.float64)

        def rmse(img, clamp=None):
            x, y = img.astype(np.float64), ref
            if clamp is not None:
                x, y = np.minimum(x, clamp), np.minimum(y, clamp)
            return float(np.sqrt(np.mean((x - y) ** 2)))

        for n, f in frames.items():
            row = dict(spp=n, K=9, mean_trim=float(f["trim"].mean()), share_trimmed=float((f["trim"] > 0).mean()),
                       trim_histogram={int(c): int((f["trim"] == c).sum()) for c in np.unique(f["trim"])},
                       mean_level_plain=float(f["plain"].astype(np.float64).mean()), mean_level_robust=float(f["robust"].astype(np.float64).mean()),
                       mean_level_reference=float(ref.mean()))
            for name in ("plain", "robust", "denoised", "robust_denoised"):
                row["rmse_" + name] = rmse(f[name])
                row["rmse_" + name + "_clamped_4"] = rmse(f[name], 4.0)
            rows.append(row)
            print(json.dumps(row), flush=True)
        save("gain.json", dict(scene="atrium (plain)", width=W, height=H, bounces=BOUNCES, reference_spp=a.reference_spp, rows=rows))
    r.close()


if __name__ == "__main__":
    main()
