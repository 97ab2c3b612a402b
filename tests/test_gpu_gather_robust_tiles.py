"""The robust mean of an adaptively sampled frame across ranks (-m gpu): RF_BUCKETS_SHARD_TILE_COUNTS.  With K | RF_BUCKETS_TILE_COUNTS | RF_BUCKETS_SHARD_TILE_COUNTS
rf_comm_render_adaptive runs with the buckets on -- the bucket kernels address every plane through the shard's slot list (kBucketSumRuns / kBucketSumPixels over
ShardList) --, and a gather with RF_GATHER_ROBUST_MEAN | RF_GATHER_TILE_COUNTS combines every slot of the shard with its own count (kRobustMeanShardTiles<K>) before
plane 4 travels.  N tile-sharded handles and N communicators of the local test transport in one process, one host thread per rank, in the form of
tests/test_gpu_gather_robust.py.  The defining properties (include/rayfinder_amd.h): the K planes of every tile are bit for bit the whole-frame handle's after the same
rf_renderer_render_adaptive calls, and M, the texels, the trim image, the counts and the robust-denoised frame on the root are that handle's.  Every comparison is exact.
The main shape is tests/test_gpu_robust_adaptive.py's frame A (Duck, 150 x 90, 32 spp, K = 9, tiles at 12 and at 32 samples); the target, the expected counts, planes
and combine come from the restatement there, never from the code under test."""
import functools
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import play, tile_slices
from conftest import bits
from robust_tiles_restatement import robust_mean_tiles
from test_gpu_adaptive import BOUNCES, EXPOSURE, H, SPP, W
from test_gpu_robust_adaptive import COUNTS_A, EVERY, K, MIN, _samples, _target, _tile_planes, _want

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
MAIN = (W, H, SPP)                  # 150 x 90: 5 x 3 tiles, ragged right and bottom
SMALL = (72, 40, 32)                # 6 tiles: a world of 8 leaves ranks 6 and 7 without a tile
ONE_CALL = ((EVERY, MIN, 0),)
TWO_CALLS = ((EVERY, MIN, 20), (EVERY, MIN, 0))
FIVES = ((5, MIN, 0),)
SCALARS = ("mean_error", "max_error", "worst_tile", "samples", "pixels", "nonfinite_pixels")

_PT = {}


@pytest.fixture(autouse=True)
def _scene(duck_pt):
    _PT["duck"] = duck_pt


def _handle(pt, frame, k=K, shard=True, opts=()):
    """Moments and AOVs per tile count, and the buckets as K | RF_BUCKETS_TILE_COUNTS (| RF_BUCKETS_SHARD_TILE_COUNTS); k = 0: the buckets off"""
    w, h, spp = frame
    r = rf.ReferencePathTracer(rf.make_render_parameters(w, h, rf.fly_camera(w, h), spp, BOUNCES, rf.make_sky(), EXPOSURE), pt.scene())
    for name, value in dict(opts).items():
        r.set_option(name, value)
    r.set_aovs(True, tile_counts=True)
    r.set_moments(True)
    if k:
        r.set_buckets(k, tile_counts=True, shard=shard)
    return r


def _sums(r):
    """[S, AC, ND, Q] as the gather numbers the planes"""
    S, _ = r.read_accumulation()
    a = r.read_aovs()
    Q, _ = r.read_moments()
    return [S, np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), Q]


@functools.lru_cache(maxsize=None)
def _whole(frame, k, target, calls, opts=()):
    """The equal-bits partner: ONE handle without a tile shard and without the new bit after the same rf_renderer_render_adaptive calls -- its counts, sums, bucket
    planes, robust mean, both denoisers' frames and its estimate.  Computed once per case; read-only."""
    r = _handle(_PT["duck"], frame, k, shard=False, opts=opts)
    for every, lo, hi in calls:
        r.render_adaptive(target, every, lo, hi)
    out = dict(counts=r.read_tile_samples().reshape(-1), planes=_sums(r), B=r.read_buckets()[0])
    r.robust_mean()
    out["robust"] = r.read_robust_mean()
    r.denoise_robust()
    out["denoised_robust"] = r.read_denoised()
    r.denoise()
    out["denoised"] = r.read_denoised()
    out["estimate"] = r.noise_estimate()
    r.close()
    for a in out["planes"] + [out["B"], out["counts"], out["robust"]["mean"], out["robust"]["bgra8"], out["robust"]["trim"]]:
        a.setflags(write=False)
    return out


def _local(monkeypatch):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "60")


def _local_world(world, make, script):
    """tests/test_gpu_gather_robust.py::_local_world: every rank makes its handle (make()), shard and communicator and runs script(rank, r, comm, out), which the ranks
    walk in step; all_reduce_max is the barrier before tear-down."""
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = make()
            r.set_tile_shard(rank, world)
            comm = rf.TileComm(uid, rank, world, 0)
            assert comm.local_transport() and comm.info()["rccl_ranks"] == world
            script(rank, r, comm, out)
            out[("max", rank)] = comm.all_reduce_max(float(rank), r)
            comm.close()
            r.close()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(i,)) for i in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(300)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads), "a rank hangs in the exchange"
    assert all(out[("max", i)] == float(world - 1) for i in range(world))
    return out


def _refused(match, call, *args, **kw):
    with pytest.raises(rf.RayfinderError, match=match) as e:
        call(*args, **kw)
    assert e.value.status == INVALID
    return str(e.value)


def _tiles(frame, rank, world):
    return [int(t) for t in rf.tiles_for_rank(frame[0], frame[1], rank, world)]


def _deal(frame, counts, world):
    """The counts of every rank's tiles, in slot order"""
    return [[int(counts[t]) for t in _tiles(frame, rank, world)] for rank in range(world)]


def _assert_the_deal(world):
    """What the issue's table says about frame A's deal, from tilesForRank's rule and COUNTS_A alone"""
    deal = _deal(MAIN, COUNTS_A, world)
    assert sorted(t for rank in range(world) for t in _tiles(MAIN, rank, world)) == list(range(15))
    if world == 2:
        assert all(set(c) == {12, 32} for c in deal), deal                   # every rank holds tiles at both counts
    elif world == 4:
        assert deal[2] == [12, 12, 12] and all(set(deal[k]) == {12, 32} for k in (0, 1, 3)), deal   # rank 2: uniform in a non-uniform frame
    elif world == 6:
        assert _tiles(MAIN, 0, 6) == [0, 13] and deal[0] == [12, 12], deal   # rank 0: uniform at 12 as well, and it holds tile 13 (see the gather test)
    else:
        assert deal[0] == [12] and deal[5] == [12, 12] and deal[3] == [32, 32], deal   # one tile only, at 12; only at 12; only at 32
        assert all(sorted(deal[k]) == [12, 32] for k in (1, 2, 4, 6, 7)), deal          # mixed
        assert any(_tiles(MAIN, k, 8)[slot] != slot for k in range(8) for slot in range(len(deal[k])))   # a slot that differs from the tile id
    return deal


def _untiled(frame, world, per_rank):
    """The frame put together from every rank's read (its own tiles' pixels; zeros elsewhere, asserted)"""
    w, h, _ = frame
    slices = tile_slices(w, h)
    whole = np.zeros_like(per_rank[0])
    for rank in range(world):
        mine = np.zeros((h, w), bool)
        for t in _tiles(frame, rank, world):
            rows, cols = slices[t]
            mine[rows, cols] = True
            whole[..., rows, cols, :] = per_rank[rank][..., rows, cols, :]
        assert not bits(per_rank[rank])[..., ~mine, :].any(), rank
    return whole


def _same_robust(got, want, what):
    assert got["mean"].shape == want["mean"].shape, what
    assert np.array_equal(bits(got["mean"]), bits(want["mean"])), (what, "mean")
    assert np.array_equal(got["bgra8"], want["bgra8"]), (what, "texels")
    assert got["trim"].dtype == np.uint8 and np.array_equal(got["trim"], want["trim"]), (what, "trim")


def _same_denoised(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2], what


def _same_estimate(got, want, what):
    assert all(got[key] == want[key] for key in SCALARS), what
    assert all(np.array_equal(bits(got[key]), bits(want[key])) for key in ("error_map", "tile_sum", "tile_max")), what


def _state(r):
    S, n = r.read_accumulation()
    B, nb = r.read_buckets()
    Q, nq = r.read_moments()
    a = r.read_aovs()
    return (bits(S).tobytes(), n, bits(B).tobytes(), nb, bits(Q).tobytes(), nq, bits(a["albedo"]).tobytes(), a["samples"], r.read_tile_samples().tobytes())


# ---- 1. the planes
@pytest.mark.parametrize("name,calls,opts", [
    ("the default options", ONE_CALL, ()),
    ("the staged kernels off", ONE_CALL, (("accumulate_runs", 0),)),
    ("continued over two calls", TWO_CALLS, ()),
    ("steps of five samples", FIVES, ()),
])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_every_tiles_planes_are_the_whole_frame_handle_s(duck_pt, monkeypatch, world, name, calls, opts):
    """On every rank the K planes of its tiles (read_buckets on the owner) are the restatement's bucket sums of each tile's first samples and the whole-frame handle's
    planes; S, Q, the AOV sums, the counts, the result structs and the ray counts are those of a run with the buckets off (a second handle per rank on the same
    communicator, in step).
    Which kernel runs: a batch of up to 4 samples takes the one-lane-per-pixel kernels whatever the options say, so with check_every = 4 every batch of the first three
    cases runs kBucketSumPixels over the slot list.  The fourth case is here for kBucketSumRuns: check_every = 5 gives batches of 5 samples through the staged kernel,
    whose phase 5 j mod 9 wraps, and a last batch of 2 (30 -> 32) through the other one, in one accumulation."""
    _assert_the_deal(world)
    samples, S, Q = _samples()
    target = _target()
    played = None
    for every, lo, hi in calls:                                               # the restatement's schedule, call after call
        played = play(S, Q, W, H, target, every, min_samples=lo, max_samples=hi, counts=None if played is None else played["counts"])
        if calls is TWO_CALLS and hi:                                         # the first call stops at 20: some tiles at 12, the rest go on in the second
            assert sorted(set(played["counts"].tolist())) == [12, 20]
    low = 15 if calls is FIVES else 12                                        # (steps of five: the first check at or above min_samples = 12 is at 15)
    counts = played["counts"].tolist()
    assert counts == [low if c == 12 else 32 for c in COUNTS_A], counts       # the deal's shape is frame A's in every case
    deal = _deal(MAIN, counts, world)
    want_B = _want()["B"] if counts == COUNTS_A else _tile_planes(samples, played["counts"], K, W, H)
    whole = _whole(MAIN, K, target, calls, opts)
    assert whole["counts"].tolist() == counts and np.array_equal(bits(whole["B"]), bits(want_B))
    _local(monkeypatch)

    def script(rank, r, comm, out):
        off = _handle(duck_pt, MAIN, 0, opts=opts)
        off.set_tile_shard(rank, world)
        res, res_off = [], []
        for every, lo, hi in calls:
            res.append(comm.render_adaptive(r, target, every, lo, hi))
            res_off.append(comm.render_adaptive(off, target, every, lo, hi))
        assert res == res_off, (rank, res, res_off)
        st, st_off = r.stats(), off.stats()
        assert all(st[key] == st_off[key] for key in ("primary_rays", "closest_rays", "shadow_rays")), rank
        for a, b in zip(_sums(r), _sums(off)):
            assert np.array_equal(bits(a), bits(b)), rank
        assert np.array_equal(r.read_tile_samples(), off.read_tile_samples()) and r.read_accumulation()[1] == off.read_accumulation()[1]
        off.close()
        B, n = r.read_buckets()
        assert B.shape == (K, H, W, 4) and n == (max(deal[rank]) if deal[rank] else 0), (rank, n)   # the bucket sample count is the rank's own leading count
        out[("B", rank)], out[("S", rank)], out[("res", rank)] = B, r.read_accumulation()[0], res[-1]
        out[("counts", rank)] = [int(c) for c in r.read_tile_samples().reshape(-1)[_tiles(MAIN, rank, world)]]

    out = _local_world(world, lambda: _handle(duck_pt, MAIN, opts=opts), script)
    assert [out[("counts", k)] for k in range(world)] == deal
    assert all(out[("res", k)]["frame_leading_samples"] == 32 and out[("res", k)]["frame_min_tile_samples"] == low for k in range(world))
    B = _untiled(MAIN, world, [out[("B", k)] for k in range(world)])
    assert np.array_equal(bits(B), bits(want_B)), name
    assert np.array_equal(bits(B), bits(whole["B"])), name
    frame_S = _untiled(MAIN, world, [out[("S", k)] for k in range(world)])
    assert np.array_equal(bits(frame_S), bits(whole["planes"][0])) and np.array_equal(bits(frame_S)[..., :3], bits(played["S"])[..., :3])


# ---- 2. the gather
@pytest.mark.parametrize("world", [2, 4, 6, 8])
def test_the_gathered_robust_mean_takes_every_tiles_own_count(duck_pt, monkeypatch, world):
    """Three gathers on every rank: with the flag (root 0, the root's shard read in place), without it, and with the flag under loop-back (root N - 1).  On the root M,
    the texels, the trim image, K and the count (32, the largest) are the restatement's and the whole-frame handle's, rf_comm_denoise_robust is that handle's
    denoise_robust, and planes 0 .. 3, the counts, rf_comm_denoise and rf_comm_noise_estimate are what they are without the flag.
    World 6 is here for its rank 0: in the restatement every trimmed pixel of a tile at 12 samples lies in tile 13, which at world 4 belongs to a mixed rank (the
    tiles of world 4's uniform rank hold no trimmed pixel); at world 6 the rank that is uniform at 12 holds it."""
    deal = _assert_the_deal(world)
    want = _want()
    slices = tile_slices(W, H)
    trimmed = [int((want["trim"][slices[t]] > 0).sum()) for t in range(15)]
    assert [t for t in range(15) if COUNTS_A[t] == 12 and trimmed[t]] == [13] and 0 < trimmed[13] < want["trim"][slices[13]].size
    if world == 6:                                                            # a rank that is uniform at 12 in a non-uniform frame, with trimmed and untrimmed pixels
        assert deal[0] == [12, 12] and 13 in _tiles(MAIN, 0, 6)
    target = _target()
    whole = _whole(MAIN, K, target, ONE_CALL)
    assert np.array_equal(bits(whole["robust"]["mean"]), bits(want["M"])) and np.array_equal(whole["robust"]["trim"], want["trim"]) and whole["robust"]["samples"] == SPP
    _local(monkeypatch)

    def root_reads(r, comm, what, robust):
        g = comm.gathered_planes()
        assert g["aovs"] and g["moments"] and g["tile_counts"] and g["robust_mean"] == robust and g["samples"] == SPP, (what, g)
        assert comm.read_tile_samples().reshape(-1).tolist() == COUNTS_A, what
        for plane in range(4):
            assert np.array_equal(bits(comm.read_plane(r, plane)), bits(whole["planes"][plane])), (what, plane)
        comm.denoise(r)
        _same_denoised(comm.read_denoised(r), whole["denoised"], (what, "denoise"))
        _same_estimate(comm.noise_estimate(r), whole["estimate"], what)
        if not robust:
            _refused("did not carry the robust mean", comm.read_robust_mean, r)
            return
        got = comm.read_robust_mean(r)
        _same_robust(got, whole["robust"], what)
        assert np.array_equal(bits(got["mean"]), bits(want["M"])) and np.array_equal(got["trim"], want["trim"]), what
        assert got["K"] == K and got["samples"] == SPP, (what, got["K"], got["samples"])
        comm.denoise_robust(r)
        _same_denoised(comm.read_denoised(r), whole["denoised_robust"], (what, "denoise_robust"))

    def script(rank, r, comm, out):
        comm.render_adaptive(r, target, EVERY, MIN)
        before = _state(r)
        for step, (root, loopback, robust) in enumerate(((0, False, True), (0, False, False), (world - 1, True, True))):
            ptr = r.gather_frame(comm, root=root, loopback=loopback, aovs=True, moments=True, tile_counts=True, robust_mean=robust)
            assert bool(ptr) == (rank == root)
            if rank == root:
                root_reads(r, comm, (world, root, loopback, robust), robust)
                out[("checked", step)] = rank
        assert _state(r) == before, rank                                      # the gather reads the sums and writes the handle's plane-4 buffer alone

    out = _local_world(world, lambda: _handle(duck_pt, MAIN), script)
    assert [out[("checked", step)] for step in range(3)] == [0, 0, world - 1]


# ---- 3. a rank without a tile
def test_ranks_without_a_tile_take_part_and_a_root_without_a_tile_un_tiles(duck_pt, monkeypatch):
    """72 x 40 (6 tiles) at world 8: ranks 6 and 7 own no tile.  The partner is one whole-frame handle after the same call; the target is the median of a whole-frame
    handle's tile errors at min_samples, so that half the tiles stop there."""
    w, h, _ = SMALL
    assert [len(_tiles(SMALL, k, 8)) for k in range(8)] == [1, 1, 1, 1, 1, 1, 0, 0]
    probe = _handle(duck_pt, SMALL, 0)
    probe.render(MIN)
    est = probe.noise_estimate()
    probe.close()
    pixels = np.array([(rows.stop - rows.start) * (cols.stop - cols.start) for rows, cols in tile_slices(w, h)], np.float32)
    target = float(np.float32(np.median(est["tile_sum"].reshape(-1) / pixels)))
    whole = _whole(SMALL, K, target, ONE_CALL)
    counts = whole["counts"]
    print("72 x 40 counts:", counts.tolist())
    assert K <= counts.min() < counts.max()
    _local(monkeypatch)

    def script(rank, r, comm, out):
        res = comm.render_adaptive(r, target, EVERY, MIN)
        assert res["frame_leading_samples"] == counts.max() and res["frame_min_tile_samples"] == counts.min()
        out[("B", rank)] = r.read_buckets()[0]
        for root in (0, 7):
            ptr = r.gather_frame(comm, root=root, aovs=True, moments=True, tile_counts=True, robust_mean=True)
            assert bool(ptr) == (rank == root)
            if rank != root:
                continue
            got = comm.read_robust_mean(r)
            _same_robust(got, whole["robust"], root)
            assert got["K"] == K and got["samples"] == counts.max()
            assert comm.read_tile_samples().reshape(-1).tolist() == counts.tolist()
            for plane in range(4):
                assert np.array_equal(bits(comm.read_plane(r, plane)), bits(whole["planes"][plane])), (root, plane)
            comm.denoise_robust(r)
            _same_denoised(comm.read_denoised(r), whole["denoised_robust"], root)
            out[("checked", root)] = rank

    out = _local_world(8, lambda: _handle(duck_pt, SMALL), script)
    assert out[("checked", 0)] == 0 and out[("checked", 7)] == 7
    assert np.array_equal(bits(_untiled(SMALL, 8, [out[("B", k)] for k in range(8)])), bits(whole["B"]))


# ---- 4. K at the ends
@pytest.mark.parametrize("k", [3, 15])
def test_the_smallest_and_the_largest_k(duck_pt, monkeypatch, k):
    """min_samples = 15: the first check is at 16 samples, so every tile holds at least K = 15.  Against the restatement and the whole-frame handle, at world 2."""
    lo = 15
    samples, S, Q = _samples()
    target = _target()
    played = play(S, Q, W, H, target, EVERY, min_samples=lo)
    counts = played["counts"]
    assert 16 == counts.min() < counts.max() == SPP, counts.tolist()
    assert all(len(set(c)) > 1 for c in _deal(MAIN, counts, 2))              # both ranks hold tiles at different counts
    B = _tile_planes(samples, counts, k, W, H)
    M, trim = robust_mean_tiles(B, counts, W, H)
    assert 0 < int((trim > 0).sum()) < W * H and int(trim.max()) <= (k - 1) // 2
    calls = ((EVERY, lo, 0),)
    whole = _whole(MAIN, k, target, calls)
    assert whole["counts"].tolist() == counts.tolist()
    _local(monkeypatch)
    root = 1

    def script(rank, r, comm, out):
        comm.render_adaptive(r, target, EVERY, lo)
        out[("B", rank)] = r.read_buckets()[0]
        r.gather_frame(comm, root=root, aovs=True, tile_counts=True, robust_mean=True)
        if rank != root:
            return
        got = comm.read_robust_mean(r)
        _same_robust(got, whole["robust"], k)
        assert np.array_equal(bits(got["mean"]), bits(M)) and np.array_equal(got["trim"], trim)
        assert got["K"] == k and got["samples"] == SPP
        comm.denoise_robust(r)
        _same_denoised(comm.read_denoised(r), whole["denoised_robust"], k)
        out["root finished"] = rank

    out = _local_world(2, lambda: _handle(duck_pt, MAIN, k), script)
    assert out["root finished"] == root
    assert np.array_equal(bits(_untiled(MAIN, 2, [out[("B", rank)] for rank in range(2)])), bits(B))


# ---- 5. refusals
def test_refusals_keep_the_state_on_every_rank(duck_pt, monkeypatch):
    """Both ranks walk the same script, so what is refused on one is refused on the other and nobody waits: after every refusal the handle reads as before and the
    communicator serves an all_reduce_max."""
    _local(monkeypatch)
    world, root, k = 2, 0, 15
    target = _target()
    assert min(COUNTS_A) == 12 < k

    def script(rank, r, comm, out):
        def refused(match, call, *args, **kw):
            before = _state(r)
            msg = _refused(match, call, *args, **kw)
            assert _state(r) == before, match
            assert comm.all_reduce_max(float(rank), r) == float(world - 1)
            return msg

        # without the new bit rf_comm_render_adaptive is refused as ever, in both older forms
        r.set_buckets(k, tile_counts=True)
        refused("RF_BUCKETS_TILE_COUNTS covers rf_renderer_render_adaptive only", comm.render_adaptive, r, target, EVERY, MIN)
        r.set_buckets(k)
        refused("they keep ONE sample count for the frame", comm.render_adaptive, r, target, EVERY, MIN)
        # with the bit the call runs; K = 15 and min_samples = 12: tiles below K
        r.set_buckets(k, tile_counts=True, shard=True)
        res = comm.render_adaptive(r, target, EVERY, MIN)
        assert (res["frame_leading_samples"], res["frame_min_tile_samples"]) == (32, 12)
        # ... so the gather is refused on all ranks alike; the message names K and the smallest count
        for flags in (dict(), dict(aovs=True, moments=True), dict(loopback=True)):
            msg = refused(f"every one of the {k} buckets of every tile needs a sample, and the smallest tile count is 12", r.gather_frame, comm, root=root, robust_mean=True,
                          tile_counts=True, **flags)
            assert "RF_GATHER_ROBUST_MEAN" in msg
        # without the counts flag the non-uniform state's older refusal comes first
        msg = refused("rf_renderer_gather_frame: the tiles hold different sample counts", r.gather_frame, comm, root=root, robust_mean=True)
        assert "RF_GATHER_ROBUST_MEAN" not in msg
        _refused("no gather has been made", comm.gathered_planes)
        # the same frame without the flag travels, and the switch cannot change in this state
        assert bool(r.gather_frame(comm, root=root, tile_counts=True, moments=True)) == (rank == root)
        if rank == root:
            assert comm.read_tile_samples().reshape(-1).tolist() == COUNTS_A and comm.gathered_planes()["robust_mean"] is False
        refused("different sample counts", r.set_buckets, 9, tile_counts=True, shard=True)
        # buckets turned on partway: a new accumulation with the buckets off, then on with both bits
        r.set_buckets(0)
        r.set_render_parameters(rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
        r.render(4)
        r.set_buckets(k, tile_counts=True, shard=True)
        refused("the bucket sample count does not cover the accumulation", comm.render_adaptive, r, target, EVERY, MIN)
        refused(r"the bucket sample count \(0\) differs from the accumulated sample count \(4\)", r.gather_frame, comm, root=root, robust_mean=True, tile_counts=True)
        out[("finished", rank)] = True

    out = _local_world(world, lambda: _handle(duck_pt, MAIN, 0), script)
    assert out[("finished", 0)] and out[("finished", 1)]


# ---- 6. RCCL at world size 1
def test_rccl_world_size_one_carries_the_per_tile_robust_mean(duck_pt, monkeypatch):
    """A whole-frame handle with both bits after rf_renderer_render_adaptive (the handle's own tiles at different counts, no frame figures: the smallest count is the
    smallest of its own tiles): the gather carries plane 4 through ncclSend / ncclRecv (loop-back) and in place, and the root's reads equal the handle's own robust_mean
    and denoise_robust, which are what they are with RF_BUCKETS_TILE_COUNTS alone (the restatement's).  Without the new bit the gather is refused as ever."""
    monkeypatch.delenv("RF_COMM_TRANSPORT", raising=False)
    want = _want()
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert not comm.local_transport()
    r = _handle(duck_pt, MAIN, K, shard=False)
    r.render_adaptive(_target(), EVERY, MIN)
    before = _state(r)
    msg = _refused("RF_GATHER_ROBUST_MEAN: the tiles hold different sample counts", r.gather_frame, comm, root=0, robust_mean=True, tile_counts=True)
    assert "ONE count" in msg and _state(r) == before
    r.close()

    r = _handle(duck_pt, MAIN, K)
    res = r.render_adaptive(_target(), EVERY, MIN)
    counts = r.read_tile_samples().reshape(-1)
    assert counts.tolist() == COUNTS_A and res["stopped_tiles"] > 0
    assert np.array_equal(bits(r.read_buckets()[0]), bits(want["B"]))
    sums = _sums(r)
    r.robust_mean()
    own = r.read_robust_mean()
    assert np.array_equal(bits(own["mean"]), bits(want["M"])) and np.array_equal(own["trim"], want["trim"]) and own["samples"] == SPP
    r.denoise_robust()
    own_denoised = r.read_denoised()
    _refused("rf_renderer_gather_frame: the tiles hold different sample counts", r.gather_frame, comm, root=0, robust_mean=True)   # without the counts: the older refusal
    for loopback in (True, False):
        assert r.gather_frame(comm, root=0, loopback=loopback, aovs=True, moments=True, tile_counts=True, robust_mean=True)
        g = comm.gathered_planes()
        assert g["robust_mean"] and g["tile_counts"] and g["aovs"] and g["moments"] and g["samples"] == SPP
        got = comm.read_robust_mean(r)
        _same_robust(got, own, loopback)
        assert got["K"] == K and got["samples"] == SPP
        assert np.array_equal(comm.read_tile_samples().reshape(-1), counts)
        for plane in range(4):
            assert np.array_equal(bits(comm.read_plane(r, plane)), bits(sums[plane])), (loopback, plane)
        comm.denoise_robust(r)
        _same_denoised(comm.read_denoised(r), own_denoised, loopback)
    assert comm.all_reduce_max(3.5, r) == 3.5
    # a change of the bit alone clears the bucket sums (the switch is refused in the non-uniform state, so: a new accumulation first)
    r.set_render_parameters(rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
    r.render(K)
    assert r.read_buckets()[1] == K
    r.set_buckets(K, tile_counts=True, shard=True)                            # the same word: nothing changes
    assert r.read_buckets()[1] == K
    r.set_buckets(K, tile_counts=True)
    assert r.read_buckets()[1] == 0 and r.read_accumulation()[1] == K
    comm.close()
    r.close()
