"""The robust mean across ranks (-m gpu): rf_renderer_gather_frame with RF_GATHER_ROBUST_MEAN, rf_comm_read_robust_mean and rf_comm_denoise_robust.  Every rank
combines its own shard-compact bucket planes before the exchange (kRobustMeanShard) and ONE plane {M.rgb, float(c)} travels as plane 4; the root's un-tile
(kUntileRobust) splits it into M and the trim image.  N tile-sharded handles and N communicators of the local test transport in one process, one host thread per rank,
in the form of tests/test_gpu_gather_sums.py.  The defining property (include/rayfinder_amd.h): mean, texels, trim and count on the root are bit for bit
rf_renderer_read_robust_mean of ONE handle without a tile shard, and rf_comm_denoise_robust is that handle's rf_renderer_denoise_robust.  Every comparison is exact.
The main shape is tests/test_gpu_robust.py's: Duck, 72 x 40 (3 x 2 tiles, both edges ragged: the shards hold padding pixels), 3 bounces, 70 samples, K = 9."""
import functools
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import bits
from robust_restatement import robust_mean

pytestmark = pytest.mark.gpu

MAIN = (72, 40)             # 6 tiles: a world of 8 leaves ranks 6 and 7 without a tile
SECOND = (96, 64)           # the second frame size of one communicator: 3 x 2 whole tiles
BOUNCES, EXPOSURE, SPP, K = 3, 0.25, 70, 9
CAP = SPP + 2               # the parameters' samples per pixel: render() stops there, and one test renders past the 70 samples it gathers
CUSTOM = dict(iterations=3, sigma_color=0.7, sigma_normal=0.2, sigma_depth=0.05)
SCALARS = ("mean_error", "max_error", "worst_tile", "samples", "pixels", "nonfinite_pixels")

_PT = {}


@pytest.fixture(autouse=True)
def _scene(duck_pt):
    _PT["duck"] = duck_pt


def _params(frame, exposure=EXPOSURE):
    return rf.make_render_parameters(frame[0], frame[1], rf.fly_camera(*frame), CAP, BOUNCES, rf.make_sky(), exposure)


def _handle(pt, frame, k):
    r = rf.ReferencePathTracer(_params(frame), pt.scene())
    r.set_aovs(True)
    r.set_moments(True)
    if k:
        r.set_buckets(k)
    return r


def _sums(r):
    """The four per-pixel sums of a handle as the gather numbers them: [S, AC, ND, Q]"""
    S, n = r.read_accumulation()
    a = r.read_aovs()
    Q, nq = r.read_moments()
    assert a["samples"] == n and nq == n
    return [S, np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), Q], n


@functools.lru_cache(maxsize=None)
def _whole(frame, k, n):
    """ONE handle without a tile shard over `frame` with K = k after n samples: its sums, bucket planes, robust mean, both denoisers' frames and its estimate.
    Computed once per shape; read-only."""
    r = _handle(_PT["duck"], frame, k)
    r.render(n)
    planes, count = _sums(r)
    assert count == n
    out = dict(planes=planes, buckets=r.read_buckets()[0], denoised={}, denoised_robust={})
    r.robust_mean()
    out["robust"] = r.read_robust_mean()
    assert out["robust"]["samples"] == n
    for name, params in (("default", {}), ("custom", CUSTOM), ("none", dict(iterations=0))):
        r.denoise_robust(**params)
        out["denoised_robust"][name] = r.read_denoised()
    r.denoise()
    out["denoised"] = r.read_denoised()
    out["estimate"] = r.noise_estimate()
    r.close()
    for a in planes + [out["buckets"], out["robust"]["mean"], out["robust"]["bgra8"], out["robust"]["trim"]]:
        a.setflags(write=False)
    return out


def _local_world(pt, frame, world, script, k=K):
    """tests/test_gpu_gather_sums.py::_local_world with the buckets on: every rank makes its handle, shard and communicator and runs script(rank, r, comm, out), which the
    ranks walk in step; all_reduce_max is the barrier before tear-down."""
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _handle(pt, frame, k)
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


def _local(monkeypatch):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "60")


def _refused(match, call, *args, **kw):
    with pytest.raises(rf.RayfinderError, match=match) as e:
        call(*args, **kw)
    assert e.value.status == rf._ffi.RF_ERROR_INVALID_ARGUMENT


def _owns_tiles(frame, rank, world):
    return len(rf.tiles_for_rank(frame[0], frame[1], rank, world)) > 0


def _same_robust(got, want, what):
    """mean, texels and trim of two read_robust_mean dicts, as bits"""
    assert got["mean"].shape == want["mean"].shape, what
    assert np.array_equal(bits(got["mean"]), bits(want["mean"])), (what, "mean")
    assert np.array_equal(got["bgra8"], want["bgra8"]), (what, "texels")
    assert got["trim"].dtype == np.uint8 and np.array_equal(got["trim"], want["trim"]), (what, "trim")


def _same_denoised(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2], what


def _check_estimate(got, want, what):
    assert all(got[key] == want[key] for key in SCALARS), what
    assert all(np.array_equal(bits(got[key]), bits(want[key])) for key in ("error_map", "tile_sum", "tile_max")), what


def test_the_whole_frame_reference_trims_some_pixels_and_not_others():
    """Both c = 0 and c > 0 occur at the main shape, so plane 4's .w carries both on its way to the root."""
    trim = _whole(MAIN, K, SPP)["robust"]["trim"]
    assert 0 < (trim > 0).sum() < MAIN[0] * MAIN[1]


@pytest.mark.parametrize("world", [2, 3, 8])
def test_the_gathered_robust_mean_equals_the_whole_frame_handle_s(duck_pt, monkeypatch, world):
    """Roots 0 and N - 1 (at world 8 the last rank owns no tile: it un-tiles from the staging area alone), with and without the tile counts in the same group; the
    other planes, the denoiser and the estimate of the same gather are what they are without the flag."""
    _local(monkeypatch)
    want = _whole(MAIN, K, SPP)
    assert 0 < (want["robust"]["trim"] > 0).sum() < MAIN[0] * MAIN[1]

    for root in sorted({0, world - 1}):
        owns = _owns_tiles(MAIN, root, world)
        assert owns == (world != 8 or root == 0)

        def script(rank, r, comm, out, root=root, owns=owns):
            r.render(SPP)
            for tile_counts in (False, True):
                what = (world, root, tile_counts)
                ptr = r.gather_frame(comm, root=root, aovs=True, moments=True, tile_counts=tile_counts, robust_mean=True)
                assert bool(ptr) == (rank == root)
                if rank != root:
                    _refused("was not the root of the last gather", comm.read_robust_mean, r)
                    continue
                n = SPP if owns or tile_counts else 0          # the root handle's accumulated count (0 without a tile), or the largest gathered tile count
                g = comm.gathered_planes()
                assert g["robust_mean"] is True and g["aovs"] and g["moments"] and g["tile_counts"] == tile_counts, (what, g)
                assert (g["width"], g["height"], g["samples"]) == (MAIN[0], MAIN[1], n), (what, g)
                got = comm.read_robust_mean(r)
                _same_robust(got, want["robust"], what)
                assert got["K"] == K and got["samples"] == n, (what, got["K"], got["samples"])
                # planes 0 .. 3, the plain denoiser and the estimate of the same gather
                for plane in range(4):
                    assert np.array_equal(bits(comm.read_plane(r, plane)), bits(want["planes"][plane])), (what, plane)
                _refused("plane out of range", comm.read_plane, r, 4)
                if n == 0:
                    _refused("hold no sample", comm.denoise, r)
                    _refused("hold no sample", comm.denoise_robust, r)
                    _refused("at least 2 accumulated samples", comm.noise_estimate, r)
                else:
                    comm.denoise(r)
                    _same_denoised(comm.read_denoised(r), want["denoised"], (what, "denoise"))
                    _check_estimate(comm.noise_estimate(r), want["estimate"], what)
                    comm.denoise_robust(r)
                    _same_denoised(comm.read_denoised(r), want["denoised_robust"]["default"], (what, "denoise_robust"))
                out[("checked", tile_counts)] = rank

        out = _local_world(duck_pt, MAIN, world, script)
        assert out[("checked", False)] == out[("checked", True)] == root


def test_denoise_robust_on_the_root_equals_the_whole_frame_handle_s(duck_pt, monkeypatch):
    _local(monkeypatch)
    want = _whole(MAIN, K, SPP)
    world, root = 3, 2

    def script(rank, r, comm, out):
        r.render(SPP)
        r.gather_frame(comm, root=root, aovs=True, robust_mean=True)
        if rank != root:
            _refused("was not the root of the last gather", comm.denoise_robust, r)
            return
        _refused("no denoised image", comm.read_denoised, r)
        for name, params in (("default", None), ("custom", CUSTOM), ("none", dict(iterations=0))):
            comm.denoise_robust(r, params)
            _same_denoised(comm.read_denoised(r), want["denoised_robust"][name], name)
        # iterations = 0 returns M, and its texels are the robust mean's
        rgb, bgra, n = comm.read_denoised(r)
        robust = comm.read_robust_mean(r)
        assert np.array_equal(bits(rgb), bits(robust["mean"])) and np.array_equal(bgra, robust["bgra8"]) and n == robust["samples"] == SPP
        _refused("iterations", comm.denoise_robust, r, dict(iterations=9))
        _refused("sigma", comm.denoise_robust, r, dict(sigma_depth=float("nan")))
        out["root finished"] = rank

    assert _local_world(duck_pt, MAIN, world, script)["root finished"] == root


@pytest.mark.parametrize("k,n,loopback", [(3, 5, False), (15, 17, True)])
def test_unequal_bucket_sizes_at_the_smallest_and_the_largest_k(duck_pt, monkeypatch, k, n, loopback):
    """N mod K = 2: buckets 0 and 1 hold one sample more than the rest.  Against the un-sharded handle and against the restatement over its bucket reads; K = 15
    with the root's own shard through the exchange as well (loop-back: every tile is un-tiled from the staging area)."""
    _local(monkeypatch)
    want = _whole(MAIN, k, n)
    M, trim = robust_mean(want["buckets"], n)
    assert np.array_equal(bits(want["robust"]["mean"]), bits(M)) and np.array_equal(want["robust"]["trim"], trim)
    world, root = 3, 1

    def script(rank, r, comm, out):
        if loopback:
            r.set_buckets(k, tile_counts=True)      # RF_BUCKETS_TILE_COUNTS makes no difference under a shard (the reference handle is without it)
        r.render(n)
        r.gather_frame(comm, root=root, loopback=loopback, robust_mean=True)
        if rank != root:
            return
        got = comm.read_robust_mean(r)
        _same_robust(got, want["robust"], (k, n))
        assert np.array_equal(bits(got["mean"]), bits(M)) and np.array_equal(got["trim"], trim)
        assert got["K"] == k and got["samples"] == n and int(got["trim"].max()) <= (k - 1) // 2
        g = comm.gathered_planes()
        assert g["robust_mean"] and not g["aovs"] and not g["moments"] and not g["tile_counts"]
        assert np.array_equal(bits(comm.read_plane(r, 0)), bits(want["planes"][0]))
        _refused("did not carry the first-hit AOVs", comm.denoise_robust, r)
        out["root finished"] = rank

    assert _local_world(duck_pt, MAIN, world, script, k=k)["root finished"] == root


def test_the_snapshot_is_the_gather_s_and_follows_the_frame_size(duck_pt, monkeypatch):
    """What the root reads is the state at the gather, whatever the root renders afterwards; a second frame size on the same communicator; a later gather drops the
    denoise snapshot, and a plain one the robust mean."""
    _local(monkeypatch)
    first, second = _whole(MAIN, K, SPP), _whole(SECOND, K, K)
    world, root = 2, 0

    def script(rank, r, comm, out):
        r.set_render_parameters(_params(MAIN))                        # (the handles are made at the larger of the two frame sizes)
        r.render(SPP)
        r.gather_frame(comm, root=root, aovs=True, robust_mean=True)
        if rank == root:
            r.render(1)                                               # the root's bucket planes move on; nothing is gathered
            got = comm.read_robust_mean(r)
            _same_robust(got, first["robust"], "after render(1)")
            assert got["samples"] == SPP and r.read_accumulation()[1] == SPP + 1
        # (a handle's frame counter outlives its accumulations and sample j of an accumulation is frame j mod CAP's: every rank completes the cycle of CAP frames, so
        # that the next accumulation starts where the reference handle's does)
        r.render(CAP - r.read_accumulation()[1])
        r.set_render_parameters(_params(SECOND))                      # another frame size on the same handle and communicator (restarts every sum)
        r.render(K)
        r.gather_frame(comm, root=root, aovs=True, robust_mean=True)
        if rank == root:
            got = comm.read_robust_mean(r)
            _same_robust(got, second["robust"], "second frame size")
            assert got["K"] == K and got["samples"] == K
            comm.denoise_robust(r)
            _same_denoised(comm.read_denoised(r), second["denoised_robust"]["default"], "second frame size")
        r.gather_frame(comm, root=root, aovs=True, robust_mean=True)  # the same gather again: the denoise snapshot is dropped
        if rank == root:
            _refused("no denoised image", comm.read_denoised, r)
            _same_robust(comm.read_robust_mean(r), second["robust"], "gathered again")
        r.gather_frame(comm, root=root)                               # a plain gather: the robust mean is gone, its image is right
        if rank == root:
            _refused("did not carry the robust mean", comm.read_robust_mean, r)
            _refused("did not carry", comm.denoise_robust, r)
            _refused("did not carry", comm.read_denoised, r)
            assert comm.gathered_planes()["robust_mean"] is False
            assert comm.gathered_planes() == dict(aovs=False, moments=False, width=SECOND[0], height=SECOND[1], samples=K)
            assert np.array_equal(bits(comm.read_plane(r, 0)), bits(second["planes"][0]))
            out["root finished"] = rank

    assert _local_world(duck_pt, SECOND, world, script)["root finished"] == root


def test_refusals_keep_the_state_on_every_rank(duck_pt, monkeypatch):
    """Both ranks own tiles of the 72 x 40 frame and walk the same script, so a gather refused on one is refused on the other and nobody waits: after every refusal
    the handle's sums and counts read as before and the communicator serves an all_reduce_max."""
    _local(monkeypatch)
    world, root = 2, 1
    want = _whole(MAIN, K, K)

    def state(r):
        S, n = r.read_accumulation()
        B, nb = r.read_buckets()
        Q, nq = r.read_moments()
        a = r.read_aovs()
        return (bits(S).tobytes(), n, bits(B).tobytes(), nb, bits(Q).tobytes(), nq, bits(a["albedo"]).tobytes(), a["samples"])

    def gathered(comm):
        try:
            return dict(comm.gathered_planes())
        except rf.RayfinderError as e:
            return str(e)

    def script(rank, r, comm, out):
        def gather_refused(match, **flags):
            before, left = state(r), gathered(comm)
            _refused(match, r.gather_frame, comm, root=root, robust_mean=True, **flags)
            assert state(r) == before, match
            assert gathered(comm) == left, match                                             # (a refused gather is no gather: what the last one left stays)
            assert comm.all_reduce_max(float(rank), r) == float(world - 1)

        # a call before any gather
        _refused("no gather has been made", comm.read_robust_mean, r)
        _refused("no gather has been made", comm.denoise_robust, r)
        # the handle's own call under a shard
        _refused("shard", r.robust_mean)
        # nothing accumulated
        gather_refused("RF_GATHER_ROBUST_MEAN: no sample has been accumulated")
        _refused("no gather has been made", comm.gathered_planes)
        # N = K - 1: a bucket without a sample; the message names K and N
        r.render(K - 1)
        gather_refused(f"every one of the {K} buckets needs a sample, and only {K - 1} are accumulated")
        gather_refused(f"every one of the {K} buckets needs a sample, and only {K - 1} are accumulated", loopback=True, aovs=True, moments=True, tile_counts=True)
        _refused("shard", r.robust_mean)
        _refused("no gather has been made", comm.gathered_planes)
        # the state was kept: one more sample and the gather goes through
        r.render(1)
        r.gather_frame(comm, root=root, robust_mean=True)
        if rank != root:
            _refused("was not the root of the last gather", comm.read_robust_mean, r)
            _refused("was not the root of the last gather", comm.denoise_robust, r)
        else:
            got = comm.read_robust_mean(r)
            _same_robust(got, want["robust"], "N = K")
            assert got["samples"] == K and got["K"] == K
            _refused("did not carry the first-hit AOVs", comm.denoise_robust, r)           # a gather without RF_GATHER_AOVS
        # a gather without the flag
        r.gather_frame(comm, root=root, aovs=True)
        if rank == root:
            assert comm.gathered_planes()["robust_mean"] is False
            _refused("did not carry the robust mean", comm.read_robust_mean, r)
            _refused("did not carry the robust mean", comm.denoise_robust, r)
            comm.denoise(r)
            _same_denoised(comm.read_denoised(r), want["denoised"], "plain denoise")
        _refused("shard", r.robust_mean)
        # the buckets off
        r.set_buckets(0)
        r.set_render_parameters(_params(MAIN, exposure=0.5))                                 # (restarts the accumulation)
        r.render(10)
        gather_refused("RF_GATHER_ROBUST_MEAN needs the bucket sums", aovs=True)
        # turned on after 10 samples: the message holds both counts
        r.set_buckets(K)
        gather_refused(r"the bucket sample count \(0\) differs from the accumulated sample count \(10\)")
        r.render(2)
        gather_refused(r"the bucket sample count \(2\) differs from the accumulated sample count \(12\)", moments=True, tile_counts=True)
        if rank == root:
            _refused("did not carry the robust mean", comm.read_robust_mean, r)             # still the aovs-only gather's record
        out[("finished", rank)] = True

    out = _local_world(duck_pt, MAIN, world, script)
    assert out[("finished", 0)] and out[("finished", 1)]


def test_the_non_uniform_state_is_refused_whatever_the_other_flags(duck_pt, monkeypatch):
    """RCCL at world size 1 with a whole-frame handle, the one setup in which the bucket planes can follow per-tile counts (RF_BUCKETS_TILE_COUNTS, then
    rf_renderer_render_adaptive: tests/test_gpu_robust_adaptive.py's frame A, where tiles stop at 12 and at 32 samples).  Plane 4 is combined with ONE count, so the
    flag is refused there also with RF_GATHER_TILE_COUNTS, which lifts the refusal for every other plane; the state is kept and the handle's own per-tile combine runs."""
    from test_gpu_robust_adaptive import EVERY, MIN, _bucket_renderer, _target
    monkeypatch.delenv("RF_COMM_TRANSPORT", raising=False)
    r = _bucket_renderer(duck_pt, aovs=True)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert not comm.local_transport()
    res = r.render_adaptive(_target(), EVERY, MIN)
    counts = r.read_tile_samples()
    assert res["stopped_tiles"] > 0 and counts.min() < counts.max()
    before = (bits(r.read_accumulation()[0]).tobytes(), bits(r.read_buckets()[0]).tobytes(), r.read_buckets()[1], counts.tobytes())
    for flags in (dict(tile_counts=True), dict(tile_counts=True, aovs=True, moments=True), dict(tile_counts=True, loopback=True)):
        with pytest.raises(rf.RayfinderError, match="RF_GATHER_ROBUST_MEAN: the tiles hold different sample counts") as e:
            r.gather_frame(comm, root=0, robust_mean=True, **flags)
        assert e.value.status == rf._ffi.RF_ERROR_INVALID_ARGUMENT and "ONE count" in str(e.value)
        _refused("no gather has been made", comm.gathered_planes)
    _refused("rf_renderer_gather_frame: the tiles hold different sample counts", r.gather_frame, comm, root=0, robust_mean=True)   # without the counts: the older refusal, first
    assert before == (bits(r.read_accumulation()[0]).tobytes(), bits(r.read_buckets()[0]).tobytes(), r.read_buckets()[1], r.read_tile_samples().tobytes())
    assert r.gather_frame(comm, root=0, tile_counts=True, aovs=True, moments=True)          # the same frame without the flag travels
    assert comm.gathered_planes()["robust_mean"] is False and np.array_equal(comm.read_tile_samples(), counts)
    _refused("did not carry the robust mean", comm.read_robust_mean, r)
    r.robust_mean()                                                                          # the handle's own combine, per tile count
    assert r.read_robust_mean()["samples"] == counts.max()
    assert comm.all_reduce_max(2.5, r) == 2.5
    comm.close()
    r.close()


def test_rccl_world_size_one_carries_the_robust_mean(duck_pt, monkeypatch):
    """RCCL itself: a world-size-1 communicator, plane 4 sent to itself through ncclSend / ncclRecv in the one group behind planes 0 .. 3 (loop-back), then read in
    place; the robust mean, the robust denoise and the other planes equal the handle's own."""
    monkeypatch.delenv("RF_COMM_TRANSPORT", raising=False)
    r = _handle(duck_pt, MAIN, K)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert not comm.local_transport()
    r.render(SPP)
    want, n = _sums(r)
    r.robust_mean()
    own = r.read_robust_mean()
    r.denoise_robust()
    own_denoised = r.read_denoised()
    for loopback in (True, False):
        assert r.gather_frame(comm, root=0, loopback=loopback, aovs=True, moments=True, robust_mean=True)
        g = comm.gathered_planes()
        assert g["robust_mean"] and g["aovs"] and g["moments"] and g["samples"] == n == SPP
        got = comm.read_robust_mean(r)
        _same_robust(got, own, loopback)
        assert got["K"] == K and got["samples"] == n
        for plane in range(4):
            assert np.array_equal(bits(comm.read_plane(r, plane)), bits(want[plane])), (loopback, plane)
        comm.denoise_robust(r)
        _same_denoised(comm.read_denoised(r), own_denoised, loopback)
    assert comm.all_reduce_max(3.5, r) == 3.5
    comm.close()
    r.close()
