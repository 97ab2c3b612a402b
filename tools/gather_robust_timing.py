"""usage: tools/gather_robust_timing.py <package root> <plain|planes4|planes5|post_host|post_root> [runs]
World 4 through the local transport on one GPU, 1920x1080 Duck, K = 9 bucket sums, 9 samples.
  plain / planes4 / planes5   the root's rf_comm_last_exchange_ms of `runs` gathers after one warm-up: the image alone, image + AOVs + moments, and those with the
                              robust mean as plane 4.  wall_ms: the host clock from the barrier to the drained stream, which for planes5 also holds the rank's own
                              combine (kRobustMeanShard is enqueued in front of the exchange's first event)
  post_root                   wall time on the root from the end of rendering (all ranks drained, barrier) to M and trim in host memory: gather with the robust mean,
                              rf_comm_read_robust_mean
  post_host                   the same window by the only route without the flag: every rank's read_buckets, the planes summed on the host, rf_robust_mean_images
`plain`, `planes4` and `post_host` run on a tree without RF_GATHER_ROBUST_MEAN too (the modes ask for nothing newer)."""
import json, os, sys, threading, time
root_dir, mode = sys.argv[1], sys.argv[2]
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
sys.path.insert(0, root_dir)
os.environ["RF_COMM_TRANSPORT"] = "local"
os.environ["RF_COMM_TIMEOUT_S"] = "120"
import numpy as np
import rayfinder_amd as rf
assert os.path.abspath(rf.__file__).startswith(os.path.abspath(root_dir)), rf.__file__
W, H, SPP, B, WORLD, K = 1920, 1080, 9, 2, 4, 9
pt = rf.PtFormat.from_gltf(os.path.join(root_dir, "tests", "golden", "Duck.glb"))
uid = rf.comm_unique_id()
flags = dict(plain={}, planes4=dict(aovs=True, moments=True), planes5=dict(aovs=True, moments=True, robust_mean=True), post_root=dict(robust_mean=True), post_host={})[mode]
out, errors = {"ms": [], "wall_ms": []}, []
shared = {}

def rank_main(rank):
    try:
        r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, B, rf.make_sky(), 0.25), pt.scene())
        if mode != "plain":
            r.set_aovs(True); r.set_moments(True); r.set_buckets(K)
        r.set_tile_shard(rank, WORLD)
        comm = rf.TileComm(uid, rank, WORLD, 0)
        r.render(SPP)
        for i in range(runs + 1):
            r.synchronize()
            comm.all_reduce_max(0.0, r)                      # every rank's frame has drained: the window holds the exchange and what follows it, not a peer's render
            t0 = time.perf_counter()
            if mode == "post_host":
                shared[rank] = r.read_buckets()[0]
                comm.all_reduce_max(0.0, r)
                if rank == 0:
                    got = rf.robust_mean_images(sum(shared[k] for k in range(WORLD)), SPP, exposure=0.25)      # (disjoint tiles, zeros elsewhere)
            elif mode == "post_root":
                r.gather_frame(comm, root=0, **flags)
                if rank == 0:
                    got = comm.read_robust_mean(r)
            else:
                r.gather_frame(comm, root=0, **flags)
                r.synchronize()
            if rank == 0 and i > 0:
                out["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
                if mode != "post_host":
                    out["ms"].append(round(comm.last_exchange_ms(), 4))
                if mode.startswith("post"):
                    out["check"] = [int(got["trim"].sum()), int(got["bgra8"].sum() & 0xFFFFFFFF), float(got["mean"].astype(np.float64).sum())]
        comm.all_reduce_max(0.0, r)
        comm.close(); r.close()
    except BaseException as e:  # noqa: BLE001
        errors.append((rank, repr(e)))

threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(WORLD)]
for t in threads: t.start()
for t in threads: t.join(400)
assert not errors and not any(t.is_alive() for t in threads), errors
print(json.dumps(dict(tree=os.path.basename(os.path.abspath(root_dir)), mode=mode, frame=[W, H], world=WORLD, K=K, samples=SPP, exchange_ms=out["ms"], wall_ms=out["wall_ms"],
                      check=out.get("check"))), flush=True)
