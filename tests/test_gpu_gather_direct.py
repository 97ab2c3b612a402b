"""The direct sums across ranks (-m gpu): rf_renderer_gather_frame with RF_GATHER_DIRECT, rf_comm_read_plane(5), rf_comm_denoise_split and rf_comm_read_split.
D travels as plane 5, a sum plane behind plane 4, and is un-tiled by the sum planes' one kUntilePlanes launch; the root filters the two components where the gathered
sums lie and forms them as means with one kernel (kSplitMeanRows).  N tile-sharded handles and N communicators of the local test transport in one process, one host
thread per rank, in the form of tests/test_gpu_gather_robust.py.  The defining property (include/rayfinder_amd.h): plane 5, the split-denoised frame and the two
components on the root are bit for bit those of ONE handle without a tile shard.  Every comparison is exact.
Shape: Duck, 72 x 40 (3 x 2 tiles, both edges ragged: the shards hold padding pixels), 3 bounces, 6 samples; a second frame of 96 x 64 on the same communicator."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import bits
from split_mean_restatement import read_split

pytestmark = pytest.mark.gpu

MAIN = (72, 40)             # 6 tiles: a world of 8 leaves ranks 6 and 7 without a tile
SECOND = (96, 64)           # the second frame size of one communicator: 3 x 2 whole tiles, larger images on the root
BOUNCES, EXPOSURE, SPP, K = 3, 0.25, 6, 3
CAP = 24                    # the parameters' samples per pixel: the adaptive frame's leading tiles stop there
EVERY = 8                   # render_adaptive's check_every, as in tests/test_gpu_direct_adaptive.py
CUSTOM = (dict(iterations=2, sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05), dict(iterations=3, sigma_color=4.0, sigma_normal=0.15, sigma_depth=0.2))
PAIRS = (("default", (None, None)), ("custom", CUSTOM), ("none", (dict(iterations=0), dict(iterations=0))))

_PT = {}


@pytest.fixture(autouse=True)
def _scene(duck_pt):
    _PT["duck"] = duck_pt


def _params(frame, exposure=EXPOSURE):
    return rf.make_render_parameters(frame[0], frame[1], rf.fly_camera(*frame), CAP, BOUNCES, rf.make_sky(), exposure)


def _handle(pt, frame, adaptive=False, direct=True):
    """Every sum the gather can carry, on from the first sample; adaptive: D and the AOVs kept per tile count (and no buckets: they would need their own bits)"""
    r = rf.ReferencePathTracer(_params(frame), pt.scene())
    r.set_aovs(True, tile_counts=adaptive)
    r.set_moments(True)
    if not adaptive:
        r.set_buckets(K)
    if direct:
        r.set_direct(True, tile_counts=adaptive)
    return r


def _sums(r):
    """The four per-pixel sums of a handle as the gather numbers them: [S, AC, ND, Q]"""
    S, n = r.read_accumulation()
    a = r.read_aovs()
    Q, nq = r.read_moments()
    assert a["samples"] == n and nq == n
    return [S, np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), Q], n


def _components(S, D, counts):
    """D / n and (S - D) / n formed from a handle's reads, f32: what a caller of rf_renderer_read_direct forms on the host"""
    h, w = S.shape[:2]
    n = np.asarray(counts, np.float32)
    if n.ndim:
        n = np.repeat(np.repeat(n, 32, 0), 32, 1)[:h, :w, None]
    direct, indirect = np.ones_like(S), np.ones_like(S)
    direct[..., :3] = D[..., :3] / n
    indirect[..., :3] = (S[..., :3] - D[..., :3]) / n
    return direct, indirect


def _finish_reference(r, out, counts):
    """What every reference shares: D, the split-denoised frames, the two components; made read-only"""
    out["D"], nd = r.read_direct()
    assert nd == out["n"]
    out["denoised_split"] = {}
    for name, (pd, pi) in PAIRS:
        r.denoise_split(direct=pd, indirect=pi)
        out["denoised_split"][name] = r.read_denoised()
    r.denoise()
    out["denoised"] = r.read_denoised()
    out["split"] = _components(out["planes"][0], out["D"], counts)
    for a in out["planes"] + [out["D"]] + list(out["split"]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _whole(frame, n=SPP):
    """ONE handle without a tile shard over `frame` after n samples.  Computed once per shape; read-only."""
    r = _handle(_PT["duck"], frame)
    r.render(n)
    planes, count = _sums(r)
    assert count == n
    out = dict(planes=planes, n=n)
    r.robust_mean()
    out["robust"] = r.read_robust_mean()
    _finish_reference(r, out, n)
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def _whole_adaptive():
    """ONE handle without a tile shard after render_adaptive, in the non-uniform state.  The target is the median of the tile errors at the first check (L = EVERY),
    as tests/test_gpu_direct_adaptive.py chooses it -- here from a handle's own estimate after EVERY samples: the tiles at or below it stop there, the rest go on."""
    probe = _handle(_PT["duck"], MAIN, adaptive=True)
    probe.render(EVERY)
    est = probe.noise_estimate()
    probe.close()
    pixels = np.array([min(32, MAIN[0] - 32 * x) * min(32, MAIN[1] - 32 * y) for y in range(2) for x in range(3)], np.float32)
    errors = (est["tile_sum"].reshape(-1) / pixels).astype(np.float32)
    target = float(np.float32(np.median(errors)))
    r = _handle(_PT["duck"], MAIN, adaptive=True)
    res = r.render_adaptive(target, EVERY)
    counts = r.read_tile_samples()
    assert res["stopped_tiles"] > 0 and not r.tile_samples_uniform()
    planes, n = _sums(r)
    out = dict(planes=planes, n=n, counts=counts, target=target)
    _finish_reference(r, out, counts)
    r.close()
    counts.setflags(write=False)
    return out


def _local_world(pt, frame, world, script, **handle):
    """tests/test_gpu_gather_robust.py::_local_world: every rank makes its handle, shard and communicator and runs script(rank, r, comm, out), which the ranks walk in
    step; all_reduce_max is the barrier before tear-down."""
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _handle(pt, frame, **handle)
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


def _same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def _same_denoised(got, want, what):
    assert _same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], what


def _check_split_reads(comm, r, want, counts, what):
    """Plane 5 and the two components on the root against the whole-frame handle's and against the restatement over the gathered planes themselves"""
    D = comm.read_plane(r, 5)
    assert _same(D, want["D"]), (what, "plane 5")
    direct, indirect = comm.read_split(r)
    assert _same(direct, want["split"][0]) and _same(indirect, want["split"][1]), (what, "read_split against the whole-frame handle's reads")
    re_direct, re_indirect = read_split(comm.read_plane(r, 0), D, counts)
    assert _same(direct, re_direct) and _same(indirect, re_indirect), (what, "read_split against the restatement")


def _check_denoise_split(comm, r, want, what):
    for name, (pd, pi) in PAIRS:
        comm.denoise_split(r, direct=pd, indirect=pi)
        _same_denoised(comm.read_denoised(r), want["denoised_split"][name], (what, name))


def test_the_whole_frame_reference_has_direct_and_indirect_light():
    """Against a vacuous comparison: D is non-zero somewhere, S - D is non-zero somewhere and D differs from S somewhere -- in the adaptive frame too"""
    for want in (_whole(MAIN), _whole(SECOND), _whole_adaptive()):
        S, D = want["planes"][0], want["D"]
        assert D[..., :3].any() and (S[..., :3] - D[..., :3]).any() and not np.array_equal(bits(D), bits(S))
        assert want["split"][0][..., :3].any() and want["split"][1][..., :3].any()
    a = _whole_adaptive()
    assert len(set(a["counts"].reshape(-1).tolist())) >= 2, a["counts"]
    # per tile count is not one count: the filter with the leading count alone gives another frame
    S, AC, ND, _ = a["planes"]
    uniform, _ = rf.denoise_split_images(S, a["D"], AC, ND, a["n"], exposure=EXPOSURE)
    assert not _same(uniform, a["denoised_split"]["default"][0])


# direct=True alone, and with every other flag added: one at a time, then all of them
FLAGS = (dict(), dict(aovs=True), dict(moments=True), dict(robust_mean=True), dict(tile_counts=True), dict(aovs=True, moments=True, robust_mean=True, tile_counts=True))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_the_gathered_direct_sums_equal_the_whole_frame_handle_s(duck_pt, monkeypatch, world):
    """Roots 0 and N - 1 (at world 8 the last rank owns no tile: it un-tiles from the staging area alone), the root's shard read in place and through the exchange
    (loop-back); the other planes and the robust mean of the same gather are what they are without the flag."""
    _local(monkeypatch)
    want = _whole(MAIN)

    def script(rank, r, comm, out):
        r.render(SPP)
        for root, loopback, flags in ((a, b, c) for a in sorted({0, world - 1}) for b in (False, True) for c in FLAGS):
            what = (world, root, loopback, tuple(flags))
            owns = _owns_tiles(MAIN, root, world)
            assert owns == (world != 8 or root == 0)
            ptr = r.gather_frame(comm, root=root, loopback=loopback, direct=True, **flags)
            assert bool(ptr) == (rank == root)
            if rank != root:
                continue
            counted = flags.get("tile_counts", False)
            n = SPP if owns or counted else 0          # the root handle's accumulated count (0 without a tile), or the largest gathered tile count
            g = comm.gathered_planes()
            assert g["direct"] is True and g.get("direct") is True, (what, g)
            assert (g["aovs"], g["moments"], g["robust_mean"], g["tile_counts"]) == tuple(flags.get(k, False) for k in ("aovs", "moments", "robust_mean", "tile_counts")), (what, g)
            assert (g["width"], g["height"], g["samples"]) == (MAIN[0], MAIN[1], n), (what, g)
            # planes 0 .. 3 and the robust mean of the same gather
            carried = [0] + ([1, 2] if flags.get("aovs") else []) + ([3] if flags.get("moments") else [])
            for plane in carried:
                assert _same(comm.read_plane(r, plane), want["planes"][plane]), (what, plane)
            if flags.get("robust_mean"):
                got = comm.read_robust_mean(r)
                assert _same(got["mean"], want["robust"]["mean"]) and np.array_equal(got["bgra8"], want["robust"]["bgra8"]) and np.array_equal(got["trim"], want["robust"]["trim"]), what
                assert got["K"] == K and got["samples"] == n, what
            assert _same(comm.read_plane(r, 5), want["D"]), (what, "plane 5")
            if n == 0:
                _refused("hold no sample", comm.read_split, r)
                _refused("hold no sample" if flags.get("aovs") else "did not carry the first-hit AOVs", comm.denoise_split, r)
            else:
                _check_split_reads(comm, r, want, np.full((2, 3), SPP, np.uint32) if counted else SPP, what)
                if flags.get("aovs"):
                    _check_denoise_split(comm, r, want, what)
                    comm.denoise(r)
                    _same_denoised(comm.read_denoised(r), want["denoised"], (what, "the one filter of the same gather"))
                else:
                    _refused("did not carry the first-hit AOVs", comm.denoise_split, r)
            out[("checked", root, loopback, tuple(flags))] = rank

    out = _local_world(duck_pt, MAIN, world, script)
    assert sum(1 for k in out if k[0] == "checked") == len(sorted({0, world - 1})) * 2 * len(FLAGS)


@pytest.mark.parametrize("world", [1, 3])
def test_an_adaptively_sampled_frame_is_gathered_and_split_per_tile_count(duck_pt, monkeypatch, world):
    """After rf_comm_render_adaptive the tiles hold different counts: D follows them (RF_DIRECT_TILE_COUNTS), the gather carries it with the counts, and plane 5, the
    split-denoised frame and the two components are the whole-frame handle's after rf_renderer_render_adaptive, each tile with its own count."""
    _local(monkeypatch)
    want = _whole_adaptive()
    root = world - 1

    def script(rank, r, comm, out):
        res = comm.render_adaptive(r, want["target"], EVERY)
        assert (res["frame_leading_samples"], res["frame_min_tile_samples"]) == (int(want["counts"].max()), int(want["counts"].min()))
        # the non-uniform state: without the counts the older refusal, word for word; plain 1 cannot be reached (the adaptive call refuses it, and so does the switch here)
        _refused("rf_renderer_gather_frame: the tiles hold different sample counts", r.gather_frame, comm, root=root, aovs=True, direct=True)
        _refused("ONE sample count", r.set_direct, True)
        for loopback in (False, True):
            ptr = r.gather_frame(comm, root=root, loopback=loopback, aovs=True, direct=True, tile_counts=True)
            assert bool(ptr) == (rank == root)
            if rank != root:
                continue
            counts = comm.read_tile_samples()
            assert len(set(counts.reshape(-1).tolist())) >= 2, counts                              # the frame is non-uniform, or this test shows nothing
            assert np.array_equal(counts, want["counts"])
            g = comm.gathered_planes()
            assert g["direct"] and g["aovs"] and g["tile_counts"] and g["samples"] == int(counts.max()) == want["n"]
            for plane in range(3):
                assert _same(comm.read_plane(r, plane), want["planes"][plane]), (loopback, plane)
            _check_split_reads(comm, r, want, counts, (world, loopback))
            _check_denoise_split(comm, r, want, (world, loopback))
            out[("checked", loopback)] = rank

    out = _local_world(duck_pt, MAIN, world, script, adaptive=True)
    assert out[("checked", False)] == out[("checked", True)] == root


def test_refusals_keep_the_state_on_every_rank(duck_pt, monkeypatch):
    """Both ranks own tiles of the 72 x 40 frame and walk the same script, so a gather refused on one is refused on the other and nobody waits: after every refusal
    the handle's sums and counts read as before, the communicator's record is what it was, and a plain gather goes through."""
    _local(monkeypatch)
    world, root = 2, 1
    want = _whole(MAIN)

    def state(r):
        S, n = r.read_accumulation()
        D, nd = r.read_direct()
        a = r.read_aovs()
        return (bits(S).tobytes(), n, bits(D).tobytes(), nd, bits(a["albedo"]).tobytes(), a["samples"])

    def gathered(comm):
        try:
            return dict(comm.gathered_planes())
        except rf.RayfinderError as e:
            return str(e)

    def script(rank, r, comm, out):
        def gather_refused(match, **flags):
            before, left = state(r), gathered(comm)
            _refused(match, r.gather_frame, comm, root=root, direct=True, **flags)
            assert state(r) == before, match
            assert gathered(comm) == left, match                                                 # (a refused gather is no gather: what the last one left stays)
            assert comm.all_reduce_max(float(rank), r) == float(world - 1)

        r.set_render_parameters(_params(MAIN))                                                    # (the handles are made at the larger of the two frame sizes)
        # before any gather
        for call in (comm.denoise_split, comm.read_split):
            _refused("no gather has been made", call, r)
        _refused("no gather has been made", comm.read_plane, r, 5)
        # the direct sums off
        r.render(2)
        gather_refused("RF_GATHER_DIRECT needs the direct sums")
        gather_refused("RF_GATHER_DIRECT needs the direct sums", loopback=True, aovs=True, moments=True, tile_counts=True)
        # turned on after the first sample: the message holds both counts
        r.set_direct(True)
        gather_refused(r"RF_GATHER_DIRECT: the direct sample count \(0\) differs from the accumulated sample count \(2\).*turn the direct sums on before the first sample")
        r.render(1)
        gather_refused(r"the direct sample count \(1\) differs from the accumulated sample count \(3\)", aovs=True, tile_counts=True)
        _refused("no gather has been made", comm.gathered_planes)
        # the state was kept: a gather without the flag goes through, and leaves no plane 5
        assert bool(r.gather_frame(comm, root=root, aovs=True)) == (rank == root)
        if rank == root:
            assert comm.gathered_planes()["direct"] is False and "direct" not in comm.gathered_planes()
            assert comm.gathered_planes() == dict(aovs=True, moments=False, width=MAIN[0], height=MAIN[1], samples=3)
            _refused("did not carry the direct sums.*RF_GATHER_DIRECT", comm.read_plane, r, 5)
            _refused("did not carry the direct sums.*RF_GATHER_DIRECT", comm.denoise_split, r)
            _refused("did not carry the direct sums.*RF_GATHER_DIRECT", comm.read_split, r)
            comm.denoise(r)                                                                       # the gathered frame itself is served as ever
        else:
            for call in (comm.denoise_split, comm.read_split):
                _refused("was not the root of the last gather", call, r)
            _refused("was not the root of the last gather", comm.read_plane, r, 5)
        # nothing accumulated (every rank completes the cycle of CAP frames first, so that the next accumulation starts where the reference handle's does)
        r.render(CAP - r.read_accumulation()[1])
        r.set_render_parameters(_params(SECOND))                                                  # (another frame size and back: the accumulation restarts)
        r.set_render_parameters(_params(MAIN))
        assert r.read_accumulation()[1] == 0 and r.read_direct()[1] == 0
        gather_refused("RF_GATHER_DIRECT: no sample has been accumulated")
        gather_refused("RF_GATHER_DIRECT: no sample has been accumulated", tile_counts=True, loopback=True)
        # on from the first sample: the gather goes through; without the AOVs the filter is refused, the reads are served
        r.render(SPP)
        assert bool(r.gather_frame(comm, root=root, direct=True)) == (rank == root)
        if rank == root:
            assert comm.gathered_planes() == dict(aovs=False, moments=False, width=MAIN[0], height=MAIN[1], samples=SPP, direct=True)
            _check_split_reads(comm, r, want, SPP, "without the AOVs")
            _refused("did not carry the first-hit AOVs", comm.denoise_split, r)
            _refused("no denoised image|did not carry", comm.read_denoised, r)
            _refused("plane out of range", comm.read_plane, r, 4)                                 # plane 4 is no sum plane, gathered or not
            _refused("plane out of range", comm.read_plane, r, 6)
            _refused("plane out of range", comm.read_plane, r, 0xFFFFFFFF)
        else:
            _refused("was not the root of the last gather", comm.read_split, r)
            _refused("was not the root of the last gather", comm.denoise_split, r)
            _refused("was not the root of the last gather", comm.read_plane, r, 5)
        # bad parameters, refused as everywhere else
        r.gather_frame(comm, root=root, aovs=True, direct=True)
        if rank == root:
            _refused("iterations", comm.denoise_split, r, dict(iterations=9))
            _refused("sigma", comm.denoise_split, r, None, dict(sigma_depth=float("nan")))
            with pytest.raises(TypeError):
                comm.denoise_split(r, dict(sigma=1.0))
            _refused("no denoised image", comm.read_denoised, r)
            _check_denoise_split(comm, r, want, "after the refusals")
        out[("finished", rank)] = True

    out = _local_world(duck_pt, SECOND, world, script, direct=False)
    assert out[("finished", 0)] and out[("finished", 1)]


def test_the_snapshot_s_sequencing_and_a_second_frame_size(duck_pt, monkeypatch):
    """The last of rf_comm_denoise, rf_comm_denoise_robust and rf_comm_denoise_split wins the one snapshot; a gather without the flag makes plane 5 unavailable again;
    a larger frame on the same communicator regrows the root's images and the two components' buffer."""
    _local(monkeypatch)
    first, second = _whole(MAIN), _whole(SECOND)
    world, root = 2, 0

    def script(rank, r, comm, out):
        r.set_render_parameters(_params(MAIN))                        # (the handles are made at the larger of the two frame sizes)
        r.render(SPP)
        r.gather_frame(comm, root=root, aovs=True, direct=True, robust_mean=True)
        if rank == root:
            _refused("no denoised image", comm.read_denoised, r)
            comm.denoise(r)
            _same_denoised(comm.read_denoised(r), first["denoised"], "denoise")
            comm.denoise_split(r)
            _same_denoised(comm.read_denoised(r), first["denoised_split"]["default"], "denoise, then denoise_split")
            assert not _same(first["denoised"][0], first["denoised_split"]["default"][0])
            comm.denoise(r)
            _same_denoised(comm.read_denoised(r), first["denoised"], "denoise again")
            comm.denoise_split(r, *CUSTOM)
            comm.denoise_robust(r)
            comm.denoise_split(r, *CUSTOM)
            _same_denoised(comm.read_denoised(r), first["denoised_split"]["custom"], "the last of the three")
            r.render(1)                                               # the root's sums move on; what was gathered stays
            _check_split_reads(comm, r, first, SPP, "after render(1)")
        # (every rank completes the cycle of CAP frames, so that the next accumulation starts where the reference handle's does)
        r.render(CAP - r.read_accumulation()[1])
        r.set_render_parameters(_params(SECOND))
        r.render(SPP)
        for flags in (dict(aovs=True, moments=True), dict(aovs=True, tile_counts=True, loopback=True)):
            r.gather_frame(comm, root=root, direct=True, **flags)
            if rank == root:
                _refused("no denoised image", comm.read_denoised, r)  # dropped by the gather
                g = comm.gathered_planes()
                assert (g["width"], g["height"], g["samples"], g["direct"]) == (SECOND[0], SECOND[1], SPP, True)
                _check_split_reads(comm, r, second, np.full((2, 3), SPP, np.uint32) if flags.get("tile_counts") else SPP, ("second frame size", tuple(flags)))
                _check_denoise_split(comm, r, second, ("second frame size", tuple(flags)))
        r.gather_frame(comm, root=root, aovs=True)                    # a gather without the flag: plane 5 is gone, the rest is right
        if rank == root:
            assert comm.gathered_planes() == dict(aovs=True, moments=False, width=SECOND[0], height=SECOND[1], samples=SPP)
            _refused("did not carry the direct sums", comm.read_plane, r, 5)
            _refused("did not carry the direct sums", comm.read_split, r)
            _refused("did not carry the direct sums", comm.denoise_split, r)
            assert _same(comm.read_plane(r, 0), second["planes"][0])
            comm.denoise(r)
            _same_denoised(comm.read_denoised(r), second["denoised"], "a gather without the flag")
        r.gather_frame(comm, root=root, direct=True)                  # ... and with it again
        if rank == root:
            assert _same(comm.read_plane(r, 5), second["D"])
            out["root finished"] = rank

    assert _local_world(duck_pt, SECOND, world, script)["root finished"] == root


def test_rccl_world_size_one_carries_the_direct_sums(duck_pt, monkeypatch):
    """RCCL itself: a world-size-1 communicator, plane 5 sent to itself through ncclSend / ncclRecv in the one group behind planes 0 .. 4 (loop-back), then read in
    place; plane 5, the split-denoised frame and the two components equal the handle's own."""
    monkeypatch.delenv("RF_COMM_TRANSPORT", raising=False)
    want = _whole(MAIN)
    r = _handle(duck_pt, MAIN)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert not comm.local_transport()
    r.render(SPP)
    for loopback in (True, False):
        assert r.gather_frame(comm, root=0, loopback=loopback, aovs=True, moments=True, robust_mean=True, direct=True)
        g = comm.gathered_planes()
        assert g["direct"] and g["robust_mean"] and g["aovs"] and g["moments"] and g["samples"] == SPP
        for plane in range(4):
            assert _same(comm.read_plane(r, plane), want["planes"][plane]), (loopback, plane)
        assert _same(comm.read_robust_mean(r)["mean"], want["robust"]["mean"]), loopback
        # the planes' device images: D has its own, plane 4 is served by neither call
        device = []
        for plane in (0, 1, 2, 3, 5):
            p = C.c_void_p()
            rf.check(rf._ffi.lib.rf_comm_plane_device(comm._h, plane, C.byref(p)))
            device.append(p.value)
        assert all(device) and len(set(device)) == 5, device
        for plane in (4, 6):
            p = C.c_void_p(7)
            assert rf._ffi.lib.rf_comm_plane_device(comm._h, plane, C.byref(p)) == rf._ffi.RF_ERROR_INVALID_ARGUMENT and p.value == 7
            assert "plane out of range" in rf._ffi.lib.rf_last_error_message().decode()
        _check_split_reads(comm, r, want, SPP, loopback)
        _check_denoise_split(comm, r, want, loopback)
    assert comm.all_reduce_max(3.5, r) == 3.5
    comm.close()
    r.close()
