"""usage: tools/gather_robust_tiles_timing.py [runs]
What RF_BUCKETS_SHARD_TILE_COUNTS costs where it runs (-> profiles/gather_robust_tiles/): world 4 through the local transport on one GPU, 1920x1080 Duck, 2 bounces,
32 spp, check_every 4, min_samples 12, the target the median tile error of a whole-frame handle at 12 samples.
Every rank holds two tile-sharded handles, one with the buckets off and one with K = 9 | RF_BUCKETS_TILE_COUNTS | RF_BUCKETS_SHARD_TILE_COUNTS; `runs` times, after one
untimed round, alternating and taking turns at going first: a fresh accumulation on the handle, every stream drained and a barrier, then the host clock around rf_comm_render_adaptive and a
synchronize; the slowest rank's time is the round's (an all-reduce).  Both handles trace the same samples in round i (the same schedule, asserted: the same counts).
For the handle with the buckets the gather with RF_GATHER_ROBUST_MEAN | RF_GATHER_TILE_COUNTS | AOVs | moments is timed the same way behind it (exchange_ms: the root's
rf_comm_last_exchange_ms; wall_ms also holds the ranks' own combine, kRobustMeanShardTiles), and for the other one the same gather without the robust mean."""
import json, os, sys, threading, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["RF_COMM_TRANSPORT"] = "local"
os.environ["RF_COMM_TIMEOUT_S"] = "120"
import numpy as np
import rayfinder_amd as rf
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
W, H, SPP, B, WORLD, K, EVERY, MIN = 1920, 1080, 32, 2, 4, 9, 4, 12
pt = rf.PtFormat.from_gltf(os.path.join(os.path.dirname(os.path.abspath(rf.__file__)), "..", "tests", "golden", "Duck.glb"))
cam, sky = rf.fly_camera(W, H), rf.make_sky()


def handle(buckets):
    r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, cam, SPP, B, sky, 0.25), pt.scene())
    r.set_aovs(True, tile_counts=True)
    r.set_moments(True)
    if buckets:
        r.set_buckets(K, tile_counts=True, shard=True)
    return r


tx, ty = (W + 31) // 32, (H + 31) // 32
pixels = np.array([min(32, W - x * 32) * min(32, H - y * 32) for y in range(ty) for x in range(tx)], np.float32)
probe = handle(False)
probe.render(MIN)
target = float(np.float32(np.median(probe.noise_estimate()["tile_sum"].reshape(-1) / pixels)))
probe.close()
uid = rf.comm_unique_id()
out = {name: dict(adaptive_ms=[], gather_wall_ms=[], exchange_ms=[], counts=[]) for name in ("off", "on")}
errors = []


def rank_main(rank):
    try:
        handles = dict(off=handle(False), on=handle(True))
        for r in handles.values():
            r.set_tile_shard(rank, WORLD)
        comm = rf.TileComm(uid, rank, WORLD, 0)
        exposure = 0.25
        for i in range(runs + 1):
            exposure = 0.75 - exposure
            for name, r in (list(handles.items())[::-1] if i % 2 else handles.items()):    # (whoever goes second finds the scene in the caches: take turns)
                r.set_render_parameters(rf.make_render_parameters(W, H, cam, SPP, B, sky, exposure))   # a fresh accumulation
                r.synchronize()
                comm.all_reduce_max(0.0, r)
                t0 = time.perf_counter()
                res = comm.render_adaptive(r, target, EVERY, MIN)
                r.synchronize()
                adaptive = comm.all_reduce_max((time.perf_counter() - t0) * 1e3, r)
                t0 = time.perf_counter()
                r.gather_frame(comm, root=0, aovs=True, moments=True, tile_counts=True, robust_mean=name == "on")
                r.synchronize()
                gather = comm.all_reduce_max((time.perf_counter() - t0) * 1e3, r)
                if rank == 0 and i > 0:
                    o = out[name]
                    o["adaptive_ms"].append(round(adaptive, 3)), o["gather_wall_ms"].append(round(gather, 3)), o["exchange_ms"].append(round(comm.last_exchange_ms(), 4))
                    counts = comm.read_tile_samples().reshape(-1)
                    o["counts"].append([int(counts.min()), int(counts.max()), int(counts.sum()), res["frame_leading_samples"], res["frame_min_tile_samples"]])
                    if name == "on":
                        got = comm.read_robust_mean(r)
                        o["check"] = [int(got["trim"].sum()), got["samples"], got["K"]]
        comm.all_reduce_max(0.0, handles["on"])
        comm.close()
        for r in handles.values():
            r.close()
    except BaseException as e:  # noqa: BLE001
        errors.append((rank, repr(e)))


threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(WORLD)]
for t in threads: t.start()
for t in threads: t.join(500)
assert not errors and not any(t.is_alive() for t in threads), errors
assert out["off"]["counts"] == out["on"]["counts"], "the two handles did not follow the same schedule"
print(json.dumps(dict(frame=[W, H], world=WORLD, K=K, spp=SPP, bounces=B, check_every=EVERY, min_samples=MIN, target_tile_error=target, runs=runs, **out)), flush=True)
