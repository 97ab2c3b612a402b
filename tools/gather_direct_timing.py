"""usage: tools/gather_direct_timing.py <package root> [runs]
World 4 through the local transport on one GPU, 1920x1080 Duck, 2 samples: the root's rf_comm_last_exchange_ms of `runs` gathers (after one warm-up) with the AOVs
alone and, where the package has the flag, with the AOVs and the direct sums; the wall time of rf_comm_denoise_split on the root and of rf_renderer_denoise_split on a
whole-frame handle (L = 5 for both components, the stream drained before and after; the parent commit's package has the second only); and rf_comm_read_split's wall
time, which is mostly its two copies to the host (its kernel's time comes from a kernel trace around this script).  Prints one JSON line."""
import json, os, statistics, sys, threading, time
root_dir = sys.argv[1]
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 10
sys.path.insert(0, root_dir)
os.environ["RF_COMM_TRANSPORT"] = "local"
os.environ["RF_COMM_TIMEOUT_S"] = "120"
import numpy as np
import rayfinder_amd as rf
assert os.path.abspath(rf.__file__).startswith(os.path.abspath(root_dir)), rf.__file__
W, H, SPP, B, WORLD = 1920, 1080, 2, 2, 4
L5 = dict(iterations=5)
has_direct = hasattr(rf, "RF_GATHER_DIRECT")
pt = rf.PtFormat.from_gltf(os.path.join(root_dir, "tests", "golden", "Duck.glb"))
uid = rf.comm_unique_id()
out, errors = {}, []


def handle():
    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, B, rf.make_sky(), 0.25), pt.scene())
    r.set_aovs(True); r.set_direct(True)
    return r


def timed(call, sync):
    ms = []
    for i in range(runs + 1):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        if i:
            ms.append(round((time.perf_counter() - t0) * 1e3, 4))
    return ms


def rank_main(rank):
    try:
        r = handle()
        r.set_tile_shard(rank, WORLD)
        comm = rf.TileComm(uid, rank, WORLD, 0)
        r.render(SPP)
        modes = [("aovs", dict(aovs=True))] + ([("aovs_direct", dict(aovs=True, direct=True))] if has_direct else [])
        for name, flags in modes:
            ms = []
            for i in range(runs + 1):
                r.synchronize()
                comm.all_reduce_max(0.0, r)                  # every rank's stream has drained: the window holds the exchange alone
                r.gather_frame(comm, root=0, **flags)
                r.synchronize()
                if rank == 0 and i:
                    ms.append(round(comm.last_exchange_ms(), 4))
            if rank == 0:
                out["exchange_ms_" + name] = ms
        if rank == 0 and has_direct:                         # (the other ranks wait at the barrier below: the device is the root's)
            out["comm_denoise_split_ms"] = timed(lambda: comm.denoise_split(r, L5, L5), r.synchronize)
            out["comm_read_split_wall_ms"] = timed(lambda: comm.read_split(r), r.synchronize)
            rgb, bgra, _ = comm.read_denoised(r)
            out["check_comm"] = [int(bgra.sum() & 0xFFFFFFFF), float(rgb.sum(dtype=np.float64))]
        comm.all_reduce_max(0.0, r)
        comm.close(); r.close()
    except BaseException as e:  # noqa: BLE001
        errors.append((rank, repr(e)))


threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(WORLD)]
for t in threads: t.start()
for t in threads: t.join(400)
assert not errors and not any(t.is_alive() for t in threads), errors
# the whole-frame handle's own call, alone on the device
os.environ.pop("RF_COMM_TRANSPORT")
r = handle()
r.render(SPP)
out["renderer_denoise_split_ms"] = timed(lambda: r.denoise_split(L5, L5), r.synchronize)
rgb, bgra, _ = r.read_denoised()
out["check_renderer"] = [int(bgra.sum() & 0xFFFFFFFF), float(rgb.sum(dtype=np.float64))]
r.close()
med = {k + "_median": round(statistics.median(v), 4) for k, v in out.items() if k.endswith("_ms")}
print(json.dumps(dict(tree=os.path.basename(os.path.abspath(root_dir)), frame=[W, H], world=WORLD, runs=runs, **out, **med)), flush=True)
