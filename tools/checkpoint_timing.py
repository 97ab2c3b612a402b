"""The state digest, save and load at 1920x1080 on the benchmark's scene (the synthetic atrium, 8 bounces, default camera and sky), S only (1 plane) and with every
channel on (AOVs, moments, direct, K = 9: 14 planes):
  * kDigestTiles' own time per call (rf_state_digest.kernel_ms: two hipEvents around the launch on the handle's stream) and its GB/s over the planes it reads;
  * in the same run, a device-to-device copy of one plane (33.4 MB; torch's copy_ of a contiguous tensor, which is a hipMemcpyAsync), between two events;
  * wall time of state_digest(), save_checkpoint() and load_checkpoint() next to one render(1), synchronized.
usage: python tools/checkpoint_timing.py OUT.json [repeats]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rayfinder_amd as rf  # noqa: E402
from rayfinder_amd import scenes  # noqa: E402

W, H, BOUNCES = 1920, 1080, 8
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
PLANE_BYTES = 2040 * 1024 * 16


def spread(values):
    return dict(values=[round(v, 4) for v in values], min=round(min(values), 4), median=round(float(np.median(values)), 4), max=round(max(values), 4))


def wall(call, repeats):
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        call()
        out.append((time.perf_counter() - t) * 1e3)
    return spread(out)


def switches(r, everything):
    if everything:
        r.set_aovs(True), r.set_moments(True), r.set_direct(True), r.set_buckets(9)


def main():
    pt, info = scenes.atrium(1, "plain")
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), 64, BOUNCES, rf.make_sky(), 0.25)
    result = dict(scene=info.get("name"), width=W, height=H, bounces=BOUNCES, plane_mb=round(PLANE_BYTES / 1e6, 2), repeats=REPEATS)
    plane = torch.rand(PLANE_BYTES // 4, dtype=torch.float32, device="cuda")
    copy = torch.empty_like(plane)

    def d2d_ms():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        copy.copy_(plane)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    for name, everything, planes in (("one_plane", False, 1), ("all_14_planes", True, 14)):
        r = rf.ReferencePathTracer(params, pt.scene())
        switches(r, everything)
        r.render(2)
        r.synchronize()
        kernel, copies = [], []
        for _ in range(REPEATS + 1):  # (interleaved: the kernel, then the copy; the first pair is a warm-up)
            kernel.append(r.state_digest(timing=True)["kernel_ms"])
            copies.append(d2d_ms())
        kernel, copies = kernel[1:], copies[1:]
        entry = dict(kernel_ms=spread(kernel), d2d_copy_one_plane_ms=spread(copies))
        entry["kernel_gb_per_s_read"] = round(planes * PLANE_BYTES / 1e9 / (float(np.median(kernel)) * 1e-3), 1)
        entry["copy_gb_per_s_read_plus_written"] = round(2 * PLANE_BYTES / 1e9 / (float(np.median(copies)) * 1e-3), 1)
        entry["kernel_bytes_per_s_over_copy_bytes_per_s"] = round(entry["kernel_gb_per_s_read"] / entry["copy_gb_per_s_read_plus_written"], 3)

        def one_sample():
            r.render(1)
            r.synchronize()

        entry["render_1_ms"] = wall(one_sample, 5)
        entry["state_digest_wall_ms"] = wall(r.state_digest, 5)
        blob = [None]

        def save():
            blob[0] = r.save_checkpoint()

        entry["save_ms"] = wall(save, 4)
        entry["blob_mb"] = round(len(blob[0]) / 1e6, 1)
        other = rf.ReferencePathTracer(params, pt.scene())
        switches(other, everything)
        entry["load_ms"] = wall(lambda: other.load_checkpoint(blob[0]), 4)
        entry["same_digest"] = other.state_digest() == r.state_digest()
        result[name] = entry
        r.close(), other.close()
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
