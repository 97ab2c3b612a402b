"""usage: tools/gather_sums_timing.py <package root> <plain|planes|post_host|post_root> [runs]
World 4 through the local transport on one GPU, 1920x1080 Duck: the root's rf_comm_last_exchange_ms of `runs` gathers (after one warm-up), or the wall time from the
end of rendering (all ranks synchronised, barrier) to the denoised + estimated frame on the host side of the root."""
import json, os, sys, threading, time
root_dir, mode = sys.argv[1], sys.argv[2]
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
sys.path.insert(0, root_dir)
os.environ["RF_COMM_TRANSPORT"] = "local"
os.environ["RF_COMM_TIMEOUT_S"] = "120"
import numpy as np
import rayfinder_amd as rf
assert os.path.abspath(rf.__file__).startswith(os.path.abspath(root_dir)), rf.__file__
W, H, SPP, B, WORLD = 1920, 1080, 2, 2, 4
pt = rf.PtFormat.from_gltf(os.path.join(root_dir, "tests", "golden", "Duck.glb"))
uid = rf.comm_unique_id()
sums = mode != "plain"
out, errors = {"ms": [], "wall_ms": []}, []
shared = {}

def rank_main(rank):
    try:
        r = rf.ReferencePathTracer(rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, B, rf.make_sky(), 0.25), pt.scene())
        if sums:
            r.set_aovs(True); r.set_moments(True)
        r.set_tile_shard(rank, WORLD)
        comm = rf.TileComm(uid, rank, WORLD, 0)
        r.render(SPP)
        for i in range(runs + 1):
            r.synchronize()
            comm.all_reduce_max(0.0, r)                      # every rank's frame has drained: the window holds the exchange and what follows it, not a peer's render
            t0 = time.perf_counter()
            if mode == "post_host":                          # the parent's path: plain gather, every rank's AOV and moment reads, host-assembled frames, upload again
                r.gather_frame(comm, root=0)
                a = r.read_aovs(); q, _ = r.read_moments()
                shared[rank] = (np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), q)
                comm.all_reduce_max(0.0, r)
                if rank == 0:
                    S = comm.read_frame(r, W, H)
                    AC, ND, Q = (sum(shared[k][j] for k in range(WORLD)) for j in range(3))     # (disjoint tiles, zeros elsewhere)
                    rgb, bgra = rf.denoise_images(S, AC, ND, SPP, exposure=0.25)
                    est = rf.noise_estimate_images(S, Q, SPP)
            elif mode == "post_root":
                r.gather_frame(comm, root=0, aovs=True, moments=True)
                if rank == 0:
                    comm.denoise(r)
                    rgb, bgra, _ = comm.read_denoised(r)
                    est = comm.noise_estimate(r)
            else:
                r.gather_frame(comm, root=0, **(dict(aovs=True, moments=True) if sums else {}))
                r.synchronize()
            if rank == 0 and i > 0:
                out["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
                out["ms"].append(round(comm.last_exchange_ms(), 4))
                if mode.startswith("post"):
                    out["check"] = [float(est["mean_error"]), int(bgra.sum() & 0xFFFFFFFF)]
        comm.all_reduce_max(0.0, r)
        comm.close(); r.close()
    except BaseException as e:  # noqa: BLE001
        errors.append((rank, repr(e)))

threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(WORLD)]
for t in threads: t.start()
for t in threads: t.join(400)
assert not errors and not any(t.is_alive() for t in threads), errors
print(json.dumps(dict(tree=os.path.basename(os.path.abspath(root_dir)), mode=mode, frame=[W, H], world=WORLD, exchange_ms=out["ms"], wall_ms=out["wall_ms"], check=out.get("check"))), flush=True)
