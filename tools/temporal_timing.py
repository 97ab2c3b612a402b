"""usage: tools/temporal_timing.py run [out.json]            the timing run (plain, or under `rocprofv3 --kernel-trace -- python tools/temporal_timing.py run`)
       tools/temporal_timing.py kernels <kernel_trace.csv> <run.json>     the kernel times of a traced run, next to the run's wall times
The temporal history at full size: the Duck at 1920 x 1080, 2 bounces, the AOVs on, 4 samples per view.  View A is accumulated and committed; in view B
rf_renderer_temporal_accumulate (one kTemporalReproject<true> launch over the handle's tile-major sums and A's planes) is called RUNS times after two warm-up calls, each
followed by a stream wait, under a host clock; then rf_renderer_denoise with ONE iteration (kDenoisePrep, one kDenoiseAtrous pass, kTonemap) the same number of times,
for scale: the a-trous pass reads 25 taps of three planes where the reprojection reads 4 taps of two.  Bytes per pixel of the reprojection, counting every plane once:
3 x 16 (S, AC, ND) + 2 x 16 (T', G': each texel is a tap of about four pixels, fetched once) + 16 + 16 + 4 written = 116.  Prints JSON."""
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
W, H, SPP, BOUNCES, RUNS = 1920, 1080, 4, 2, 20
BYTES_PER_PIXEL = 3 * 16 + 2 * 16 + 16 + 16 + 4
VIEWS = (dict(position=(0.75, 1.0, -0.75), yaw_degrees=129.64, pitch_degrees=-13.73), dict(position=(0.62, 1.02, -0.86), yaw_degrees=123.0, pitch_degrees=-13.0))


def run(out_path):
    import rayfinder_amd as rf
    pt = rf.PtFormat.from_gltf(os.path.join(ROOT, "tests", "golden", "Duck.glb"))
    params = [rf.make_render_parameters(W, H, rf.fly_camera(W, H, **v), 64, BOUNCES, rf.make_sky(), 0.25) for v in VIEWS]
    r = rf.ReferencePathTracer(params[0], pt.scene())
    r.set_aovs(True)
    r.render(SPP)
    r.temporal_accumulate()
    r.temporal_commit()
    r.set_render_parameters(params[1])
    r.render(SPP)
    r.synchronize()

    def timed(call):
        ms = []
        for i in range(RUNS + 2):
            t = time.perf_counter()
            call()
            r.synchronize()
            if i >= 2:
                ms.append((time.perf_counter() - t) * 1e3)
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    out = dict(frame=[W, H], samples=SPP, runs=RUNS, bytes_per_pixel=BYTES_PER_PIXEL, bytes=BYTES_PER_PIXEL * W * H,
               temporal_accumulate=timed(r.temporal_accumulate), denoise_one_iteration=timed(lambda: r.denoise(iterations=1)))
    got = r.read_temporal()
    took = got["color"][..., 3] > SPP
    out["pixels_that_took_history"] = int(took.sum())
    out["memory"] = r.memory_info()
    r.close()
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


def kernels(trace, run_json):
    timing = json.load(open(run_json))
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for name, keep in (("kTemporalReproject", timing["runs"]), ("kDenoiseAtrous", timing["runs"]), ("kDenoisePrep", timing["runs"])):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name + "<" in r["Kernel_Name"] or name + "(" in r["Kernel_Name"]][-keep:]
        assert len(us) == keep, (name, len(us))
        out[name] = dict(dispatches=len(us), kernel_us_median=round(statistics.median(us), 2), kernel_us_min=round(min(us), 2), kernel_us_max=round(max(us), 2))
    med = out["kTemporalReproject"]["kernel_us_median"]
    out["kTemporalReproject"].update(bytes=timing["bytes"], bytes_per_s=round(timing["bytes"] / (med * 1e-6)), fraction_of_copy_rate=round(timing["bytes"] / (med * 1e-6) / 6.29e12, 4))
    out["reprojection_over_one_atrous_pass"] = round(med / out["kDenoiseAtrous"]["kernel_us_median"], 3)
    out["call_wall_ms"] = dict(temporal_accumulate=timing["temporal_accumulate"], denoise_one_iteration=timing["denoise_one_iteration"])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) == 4 and sys.argv[1] == "kernels":
        kernels(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
