"""usage: tools/features_timing.py <package root> [runs] [mode]
The feature export at 1920x1080 on one GPU, Duck, every sum family on.  Prints one JSON line.
  mode "export" (this commit's package): the wall time of rf_renderer_export_features per request -- the call enqueues one kernel and waits for it, so the wall time is
      the kernel plus a launch and a wait -- from the handle in the uniform state (8 samples) and in the non-uniform state (render_adaptive to the median tile error
      of the first check), and of rf_comm_export_features over the row-major planes of a world-size-1 gather; the bytes each request moves (planes read x 16 B +
      C x element size, per pixel) and the rate that wall time gives.  Every request is called once before its `runs` timed calls.  The kernel's own time comes
      from a kernel trace around this script: the dispatches appear in the order of `sequence`, 1 + runs per entry.
  mode "host" (any package, the parent commit's too): the path a caller has without the export -- read_accumulation + read_aovs, the means in numpy,
      torch.from_numpy(...).cuda() -- for color + albedo + normal + depth as a (10, H, W) f32 tensor; wall time per call."""
import json
import os
import statistics
import sys
import time

root_dir = os.path.abspath(sys.argv[1])
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 20
mode = sys.argv[3] if len(sys.argv) > 3 else "export"
sys.path.insert(0, root_dir)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rayfinder_amd as rf  # noqa: E402

assert os.path.abspath(rf.__file__).startswith(root_dir), rf.__file__
W, H, B, CAP, EVERY = 1920, 1080, 2, 24, 8
COPY_RATE = 6.29e12  # bytes/s, the measured device copy rate the project's figures are set against
pt = rf.PtFormat.from_gltf(os.path.join(root_dir, "tests", "golden", "Duck.glb"))
GUIDES = ("color", "albedo", "normal", "depth")
ALL = ("color", "albedo", "normal", "depth", "coverage", "direct", "indirect", "variance", "error", "samples")
REQUESTS = (("guides_f32_chw", GUIDES, "chw", "f32"), ("guides_f16_chw", GUIDES, "chw", "f16"), ("all_f32_hwc", ALL, "hwc", "f32"))


def handle(tile_counts=False):
    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, rf.fly_camera(W, H), CAP, B, rf.make_sky(), 0.25), pt.scene())
    r.set_aovs(True, tile_counts=tile_counts)
    r.set_moments(True)
    r.set_direct(True, tile_counts=tile_counts)
    return r


def timed(call):
    call()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def summary(ms, nbytes=None):
    out = dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms))
    if nbytes:
        rate = nbytes / (out["median_ms"] * 1e-3)
        out.update(bytes=nbytes, bytes_per_s_from_wall=round(rate), fraction_of_copy_rate_from_wall=round(rate / COPY_RATE, 4))
    return out


def request_bytes(channels, dtype):
    planes = sum(1 for need in (("color", "indirect", "variance", "error"), ("variance", "error"), ("albedo", "normal", "depth", "coverage"),
                                ("albedo", "normal", "depth", "coverage"), ("direct", "indirect")) if any(c in channels for c in need))
    return W * H * (planes * 16 + rf.feature_channels(channels)[1] * (2 if dtype == "f16" else 4))


out = dict(mode=mode, width=W, height=H, runs=runs, package=root_dir)
if mode == "host":
    r = handle()
    r.render(EVERY)

    def host_path():
        S, n = r.read_accumulation()
        a = r.aov_means()
        chw = np.concatenate([(S[..., :3] / np.float32(n)).transpose(2, 0, 1), a["albedo"].transpose(2, 0, 1), a["normal"].transpose(2, 0, 1), a["depth"][None]], 0)
        t = torch.from_numpy(np.ascontiguousarray(chw, np.float32)).cuda()
        torch.cuda.synchronize()
        return t

    assert tuple(host_path().shape) == (10, H, W)
    out["host_path_guides_f32_chw"] = summary(timed(host_path))
    r.close()
else:
    sequence = []
    for state in ("uniform", "nonuniform"):
        if state == "uniform":
            r = handle()
            r.render(EVERY)
        else:
            probe = handle(True)
            probe.render(EVERY)
            est = probe.noise_estimate()
            probe.close()
            tiles = est["tile_sum"].reshape(-1)
            ty, tx = (H + 31) // 32, (W + 31) // 32
            pixels = np.array([min(32, W - 32 * x) * min(32, H - 32 * y) for y in range(ty) for x in range(tx)], np.float32)
            r = handle(True)
            res = r.render_adaptive(float(np.median(tiles / pixels)), EVERY)
            assert res["min_tile_samples"] < res["max_tile_samples"], res
            out["nonuniform_tiles"] = dict(min=res["min_tile_samples"], max=res["max_tile_samples"], stopped=res["stopped_tiles"], tiles=res["tiles"])
        for name, channels, layout, dtype in REQUESTS:
            dst = r.export_features(channels, layout=layout, dtype=dtype)
            ms = timed(lambda: r.export_features(channels, layout=layout, dtype=dtype, out=dst))
            out[f"{state}_{name}"] = summary(ms, request_bytes(channels, dtype))
            sequence.append(f"{state}_{name}")
            del dst
        if state == "uniform":
            # the row-major source: the planes of a world-size-1 gather, on the same device
            comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
            assert r.gather_frame(comm, root=0, aovs=True, moments=True, direct=True)
            r.synchronize()
            for name, channels, layout, dtype in (REQUESTS[0], REQUESTS[2]):
                dst = comm.export_features(r, channels, layout=layout, dtype=dtype)
                ms = timed(lambda: comm.export_features(r, channels, layout=layout, dtype=dtype, out=dst))
                out[f"root_{name}"] = summary(ms, request_bytes(channels, dtype))
                sequence.append(f"root_{name}")
                del dst
            comm.close()
        r.close()
    out["sequence"] = sequence
print(json.dumps(out))
