"""Tile-adaptive sampling across ranks (-m gpu): rf_comm_render_adaptive on N tile-sharded handles, the frame gather carrying the per-tile counts
(RF_GATHER_TILE_COUNTS) and the root's reads, denoiser and estimate over them.  N handles and N communicators of the local test transport live in this one process,
one host thread per rank, in the shape of tests/test_gpu_gather_sums.py.  The defining property (include/rayfinder_amd.h): after the same calls, every tile's count
and sums are bit for bit what ONE handle without a tile shard holds after rf_renderer_render_adaptive.  Targets and expected counts come from the numpy restatement
(tests/adaptive_restatement.py) played over the oracle's samples, never from the code under test."""
import functools
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import play, prefix_sums, tile_errors
from conftest import DUCK, bits, oracle_scene_from_pt
from noise_restatement import estimate, oracle_samples
from oracle import orc

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
BOUNCES, EXPOSURE = 3, 0.25
FRAME = (150, 90, 32)               # 5 x 3 tiles, ragged right and bottom
CUSTOM = dict(iterations=3, sigma_color=0.7, sigma_normal=0.2, sigma_depth=0.05)
WHY = "different sample counts"


def _params(frame, exposure=EXPOSURE):
    w, h, spp = frame
    return rf.make_render_parameters(w, h, rf.fly_camera(w, h), spp, BOUNCES, rf.make_sky(), exposure)


def _handle(pt, frame, aovs=True, exposure=EXPOSURE):
    r = rf.ReferencePathTracer(_params(frame, exposure), pt.scene())
    if aovs:
        r.set_aovs(True, tile_counts=True)
    r.set_moments(True)
    return r


@functools.lru_cache(maxsize=None)
def _oracle(frame):
    """The oracle's per-sample radiance of Duck over `frame` as prefix sums (computed once; read-only)"""
    w, h, spp = frame
    sc, _ = oracle_scene_from_pt(rf.PtFormat.from_gltf(DUCK))
    rp = orc.make_render_params(w, h, rf.camera_to_array(rf.fly_camera(w, h)), spp, BOUNCES, EXPOSURE, rf.aligned_sky_state(rf.make_sky()))
    S, Q = prefix_sums(list(oracle_samples(orc, sc, rp, range(spp))))
    for a in S + Q:
        a.setflags(write=False)
    return S, Q


def _errors_at(frame, n):
    S, Q = _oracle(frame)
    return tile_errors(estimate(S[n], Q[n], n))


def _median_target(frame, n):
    return float(np.float32(np.median(_errors_at(frame, n))))


def _played(frame, calls):
    """The restatement's state after a sequence of calls (target, check_every, min_samples, max_samples)"""
    S, Q = _oracle(frame)
    want = None
    for target, every, lo, hi in calls:
        want = play(S, Q, frame[0], frame[1], target, every, min_samples=lo, max_samples=hi, counts=None if want is None else want["counts"])
    return want


def _sums(r):
    """[S, AC, ND, Q] as the gather numbers the planes"""
    S, _ = r.read_accumulation()
    a = r.read_aovs()
    Q, _ = r.read_moments()
    return [S, np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), Q]


_PT = {}


@pytest.fixture(autouse=True)
def _scene(duck_pt):
    _PT["duck"] = duck_pt


@functools.lru_cache(maxsize=None)
def _whole(frame, calls, aovs=True, denoised=False):
    """The equal-bits partner: ONE handle without a tile shard after the same rf_renderer_render_adaptive calls.  Computed once per case; read-only."""
    r = _handle(_PT["duck"], frame, aovs)
    for target, every, lo, hi in calls:
        r.render_adaptive(target, every, lo, hi)
    out = dict(counts=r.read_tile_samples(), mean=r.read_mean(), planes=_sums(r) if aovs else [r.read_accumulation()[0], None, None, r.read_moments()[0]])
    if denoised:
        out["denoised"] = {}
        for name, params in (("default", {}), ("custom", CUSTOM)):
            r.denoise(**params)
            out["denoised"][name] = r.read_denoised()
        out["estimate"] = r.noise_estimate()
    r.close()
    return out


def _local(monkeypatch):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "120")


def _local_world(pt, frame, world, script, aovs=True):
    """N renderers + N communicators of the LOCAL test transport in this one process, one host thread per rank; every rank runs script(rank, r, comm, out), and the
    ranks walk it in step (every exchange is collective).  all_reduce_max is the barrier before tear-down."""
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _handle(pt, frame, aovs)
            r.set_tile_shard(rank, world)
            comm = rf.TileComm(uid, rank, world, 0)
            assert comm.local_transport()
            script(rank, r, comm, out)
            comm.all_reduce_max(0.0, r)
            comm.close()
            r.close()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(300)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads), "a rank hangs in an exchange"
    return out


def _refused(match, call, *args, **kw):
    with pytest.raises(rf.RayfinderError, match=match) as e:
        call(*args, **kw)
    assert e.value.status == INVALID


def _shard_counts(frame, counts, rank, world):
    return [int(counts[t]) for t in rf.tiles_for_rank(frame[0], frame[1], rank, world)]


def _pixels(frame, tiles):
    w, h, _ = frame
    tx = (w + 31) // 32
    return [min(32, w - (t % tx) * 32) * min(32, h - (t // tx) * 32) for t in tiles]


def _check_root(comm, r, frame, want_counts, whole, aovs, what):
    """Root, after a gather with every plane and the counts: the reads equal the un-sharded handle's as bits."""
    g = comm.gathered_planes()
    assert g.get("tile_counts") and g["aovs"] == aovs and g["moments"] and g["samples"] == int(max(want_counts)), (what, g)
    got = comm.read_tile_samples()
    assert got.reshape(-1).tolist() == list(want_counts) == whole["counts"].reshape(-1).tolist(), (what, got.reshape(-1).tolist())
    for plane in range(4):
        if whole["planes"][plane] is not None:
            assert np.array_equal(bits(comm.read_plane(r, plane)), bits(whole["planes"][plane])), (what, plane)
    assert np.array_equal(bits(comm.read_mean(r)), bits(whole["mean"])), what


def _check_ranks(out, frame, world, want, what):
    """The result structs of one call on a fresh accumulation: the ranks' figures add up to the restatement's, the frame figures are the same on every rank."""
    figures = [out[("res", k)]["rank"]["pixel_samples"] for k in range(world)]
    assert sum(figures) == want["pixel_samples"], (what, figures)
    for k in range(world):
        res, mine = out[("res", k)], _shard_counts(frame, want["counts"], k, world)
        assert out[("rays", k)] == figures[k] == sum(p * c for p, c in zip(_pixels(frame, rf.tiles_for_rank(frame[0], frame[1], k, world)), mine)), (what, k)
        assert res["frame_leading_samples"] == want["max_tile_samples"] and res["frame_min_tile_samples"] == want["min_tile_samples"], (what, k, res)
        assert res["max_rank_pixel_samples"] == max(figures), (what, k)
        assert res["rank"]["tiles"] == len(mine) and res["rank"]["stopped_tiles"] == sum(c < want["max_tile_samples"] for c in mine), (what, k, res)
        assert out[("counts", k)] == mine, (what, k)


def _adaptive_and_gather(frame, world, root, calls, aovs=True, check=None):
    """The script of most tests: the calls, then a gather with everything; the root checks its reads against the un-sharded handle's."""
    want, whole = _played(frame, calls), _whole(frame, calls, aovs)

    def script(rank, r, comm, out):
        for target, every, lo, hi in calls:
            out[("res", rank)] = comm.render_adaptive(r, target, every, lo, hi)
        out[("rays", rank)] = r.stats()["primary_rays"]
        mine = rf.tiles_for_rank(frame[0], frame[1], rank, world)
        out[("counts", rank)] = [int(c) for c in r.read_tile_samples().reshape(-1)[mine]]
        ptr = r.gather_frame(comm, root=root, aovs=aovs, moments=True, tile_counts=True)
        assert bool(ptr) == (rank == root)
        if rank == root:
            _check_root(comm, r, frame, want["counts"].tolist(), whole, aovs, (frame, world, root))
            # ... and the restatement's own sums
            assert np.array_equal(bits(comm.read_plane(r, 0))[..., :3], bits(want["S"])[..., :3]) and np.array_equal(bits(comm.read_plane(r, 3)), bits(want["Q"]))
            if check:
                check(r, comm, whole)
            out["root finished"] = rank

    out = _local_world(_PT["duck"], frame, world, script, aovs)
    assert out["root finished"] == root
    return out, want


@pytest.mark.parametrize("world", [2, 3, 8])
def test_one_call_leaves_every_tile_what_the_unsharded_handle_holds(duck_pt, monkeypatch, world):
    target = _median_target(FRAME, 4)
    calls = ((target, 4, 4, 0),)
    want = _played(FRAME, calls)
    # before the GPU is touched: the schedule and the deal are the ones this test is about
    assert want["counts"].tolist() == [4, 32, 32, 4, 4, 4, 32, 32, 28, 4, 4, 32, 32, 4, 4]
    if world == 8:
        assert _shard_counts(FRAME, want["counts"], 5, 8) == [4, 4]          # every tile below L, one shared count
        assert _shard_counts(FRAME, want["counts"], 7, 8) == [28, 4]         # every tile below L, two counts
        assert _shard_counts(FRAME, want["counts"], 3, 8) == [32, 32]        # every tile at L
        assert any(len(set(_shard_counts(FRAME, want["counts"], k, 8))) == 2 and 32 in _shard_counts(FRAME, want["counts"], k, 8) for k in range(8))   # mixed ranks
    _local(monkeypatch)
    for root in sorted({0, world - 1}):
        out, _ = _adaptive_and_gather(FRAME, world, root, calls)
        _check_ranks(out, FRAME, world, want, (world, root))
        assert all(out[("res", k)]["frame_leading_samples"] == 32 and out[("res", k)]["frame_min_tile_samples"] == 4 for k in range(world))


def test_the_root_denoises_and_estimates_with_the_gathered_counts(duck_pt, monkeypatch):
    calls = ((_median_target(FRAME, 4), 4, 4, 0),)
    whole = _whole(FRAME, calls, True, True)
    _local(monkeypatch)

    def check(r, comm, _):
        for name, params in (("default", None), ("custom", CUSTOM)):
            comm.denoise(r, params)
            rgb, bgra, n = comm.read_denoised(r)
            w_rgb, w_bgra, w_n = whole["denoised"][name]
            assert np.array_equal(bits(rgb), bits(w_rgb)) and np.array_equal(bgra, w_bgra), name
            assert n == w_n == 32                                            # the largest count
        got, own = comm.noise_estimate(r), whole["estimate"]
        for key in ("mean_error", "max_error", "worst_tile", "samples", "pixels", "nonfinite_pixels"):
            assert got[key] == own[key], (key, got[key], own[key])
        assert got["samples"] == 32
        for key in ("error_map", "tile_sum", "tile_max"):
            assert np.array_equal(bits(got[key]), bits(own[key])), key

    _adaptive_and_gather(FRAME, 3, 1, calls, check=check)


def test_a_second_call_never_revives_a_tile_below_the_frame_s_leading_count(duck_pt, monkeypatch):
    first = (_median_target(FRAME, 4), 4, 4, 16)
    lower = (float(np.float32(np.sort(_errors_at(FRAME, 4))[3])), 4, 4, 0)
    after_first, want = _played(FRAME, (first,)), _played(FRAME, (first, lower))
    assert after_first["counts"].tolist() == [4, 16, 16, 4, 4, 4, 16, 16, 16, 4, 4, 16, 16, 4, 4]
    assert want["counts"].tolist() == [4, 32, 32, 4, 4, 4, 32, 32, 32, 4, 4, 32, 32, 4, 4]
    # rank 5 of 8 holds [4, 4] after the first call: its own leading count is 4, the frame's is 16.  Taking the rank's own would revive both tiles
    assert _shard_counts(FRAME, after_first["counts"], 5, 8) == [4, 4] == _shard_counts(FRAME, want["counts"], 5, 8)
    _local(monkeypatch)
    out, _ = _adaptive_and_gather(FRAME, 8, 0, (first, lower))
    for k in range(8):
        assert out[("counts", k)] == _shard_counts(FRAME, want["counts"], k, 8), k
        assert out[("res", k)]["frame_leading_samples"] == 32 and out[("res", k)]["frame_min_tile_samples"] == 4
    assert sum(out[("res", k)]["rank"]["pixel_samples"] for k in range(8)) == want["pixel_samples"]
    assert max(out[("res", k)]["max_rank_pixel_samples"] for k in range(8)) > 0 and out[("res", 5)]["rank"]["estimate_passes"] == 0


@pytest.mark.parametrize("frame,every,world,counts,empty_ranks", [
    ((150, 90, 32), 3, 3, [3, 32, 32, 3, 3, 3, 32, 32, 27, 3, 3, 32, 32, 3, 3], 0),   # steps of <= 4 samples: kSumPixels
    ((64, 64, 48), 40, 8, [48, 40, 40, 48], 4),                                       # a 40-sample step, then 8: kSumRuns past one 32-sample chunk
    ((70, 45, 16), 4, 8, [8, 12, 4, 4, 8, 4], 2),
])
def test_both_sum_kernels_and_ragged_worlds(duck_pt, monkeypatch, frame, every, world, counts, empty_ranks):
    calls = ((_median_target(frame, max(every, 2)), every, 0, 0),)
    want = _played(frame, calls)
    assert want["counts"].tolist() == counts
    assert sum(len(rf.tiles_for_rank(frame[0], frame[1], k, world)) == 0 for k in range(world)) == empty_ranks
    _local(monkeypatch)
    out, _ = _adaptive_and_gather(frame, world, world - 1, calls, aovs=frame[2] != 48)       # (once without the AOVs: the sums of S and Q alone)
    _check_ranks(out, frame, world, want, frame)


def test_states_and_refusals(duck_pt, monkeypatch):
    """Every rank makes the same calls, so a refusal on one is a refusal on all and nobody waits."""
    world, root, frame = 8, 3, FRAME
    target = _median_target(frame, 4)
    calls = ((target, 4, 4, 0),)
    want, whole = _played(frame, calls), _whole(frame, calls)
    assert _shard_counts(frame, want["counts"], 5, 8) == [4, 4]
    # the partner of the ordinary state: the un-sharded handle after the same calls -- 8 samples in every tile under another exposure, traced behind the 32 frames
    # of the first accumulation (the frame counter of every rank, rank 5's included, stands at 32 by then)
    u = _handle(duck_pt, frame)
    u.render_adaptive(target, 4, 4)
    u.set_render_parameters(_params(frame, 0.5))
    u.render_adaptive(target, 4, 8, 8)
    assert u.read_tile_samples().reshape(-1).tolist() == [8] * 15
    uniform = dict(planes=_sums(u), estimate=u.noise_estimate())
    u.denoise()
    uniform["denoised"] = u.read_denoised()
    u.close()
    _local(monkeypatch)

    def script(rank, r, comm, out):
        # bad arguments and preconditions: refused on every rank before any exchange; the state is kept
        r.set_moments(False)
        _refused("moments", comm.render_adaptive, r, target, 4, 4)
        r.set_moments(True)
        r.set_aovs(True)
        _refused("RF_AOV_TILE_COUNTS", comm.render_adaptive, r, target, 4, 4)
        r.set_aovs(True, tile_counts=True)
        _refused("check_every", comm.render_adaptive, r, target, 0, 4)
        _refused("target_tile_error", comm.render_adaptive, r, float("nan"), 4, 4)
        r.set_tile_shard((rank + 1) % world, world)
        _refused("differs from the communicator", comm.render_adaptive, r, target, 4, 4)
        r.set_tile_shard(rank, world)
        _refused("shard", r.render_adaptive, target, 4, 4)                     # the un-sharded call stays refused under a shard
        # the valid call succeeds
        res = comm.render_adaptive(r, target, 4, 4)
        assert (res["frame_leading_samples"], res["frame_min_tile_samples"]) == (32, 4)
        mine = rf.tiles_for_rank(frame[0], frame[1], rank, world)
        assert [int(c) for c in r.read_tile_samples().reshape(-1)[mine]] == _shard_counts(frame, want["counts"], rank, world)
        # the non-uniform FRAME state, on rank 5 (own tiles [4, 4]) as on every other
        _refused(WHY, r.render, 1)
        _refused(WHY, r.render_until, 0.1, 4)
        _refused(WHY, r.gather_frame, comm, root=root)
        _refused(WHY, r.gather_frame, comm, root=root, aovs=True, moments=True)
        _refused(WHY, r.set_tile_shard, rank, world)
        ptr = r.gather_frame(comm, root=root, aovs=True, moments=True, tile_counts=True)
        assert bool(ptr) == (rank == root)
        if rank == root:
            _check_root(comm, r, frame, want["counts"].tolist(), whole, True, "non-uniform")
        # a restart clears it all; with min_samples = the cap no tile can stop: the ordinary state, where nothing refuses
        r.set_render_parameters(_params(frame, 0.5))
        res = comm.render_adaptive(r, target, 4, 8, 8)
        assert (res["frame_leading_samples"], res["frame_min_tile_samples"]) == (8, 8) and res["rank"]["stopped_tiles"] == 0
        r.render(0)
        ptr = r.gather_frame(comm, root=root, aovs=True, moments=True, tile_counts=True)
        if rank == root:
            assert comm.read_tile_samples().reshape(-1).tolist() == [8] * 15 and comm.gathered_planes()["samples"] == 8
            for plane in range(4):
                assert np.array_equal(bits(comm.read_plane(r, plane)), bits(uniform["planes"][plane])), plane
            comm.denoise(r)
            rgb, bgra, n = comm.read_denoised(r)
            assert np.array_equal(bits(rgb), bits(uniform["denoised"][0])) and np.array_equal(bgra, uniform["denoised"][1]) and n == 8
        # a gather without the counts: the root-side calls are what they were
        r.gather_frame(comm, root=root, aovs=True, moments=True)
        if rank == root:
            assert comm.gathered_planes() == dict(aovs=True, moments=True, width=frame[0], height=frame[1], samples=8)
            _refused("did not carry the per-tile sample counts", comm.read_tile_samples)
            _refused("did not carry the per-tile sample counts", comm.read_mean, r)
            comm.denoise(r)
            rgb, bgra, n = comm.read_denoised(r)
            assert np.array_equal(bits(rgb), bits(uniform["denoised"][0])) and np.array_equal(bgra, uniform["denoised"][1]) and n == 8
            got = comm.noise_estimate(r)
            assert all(got[k] == uniform["estimate"][k] for k in ("mean_error", "max_error", "worst_tile", "samples", "pixels", "nonfinite_pixels"))
            assert all(np.array_equal(bits(got[k]), bits(uniform["estimate"][k])) for k in ("error_map", "tile_sum", "tile_max"))
        out[("finished", rank)] = True

    out = _local_world(duck_pt, frame, world, script)
    assert all(out[("finished", k)] for k in range(world))


def test_rccl_world_size_one_carries_the_counts(duck_pt, monkeypatch):
    """RCCL itself: a world-size-1 communicator; the counts go to the rank itself through ncclSend / ncclRecv in the one group (loop-back)."""
    monkeypatch.delenv("RF_COMM_TRANSPORT", raising=False)
    calls = ((_median_target(FRAME, 4), 4, 4, 0),)
    want, whole = _played(FRAME, calls), _whole(FRAME, calls)
    r = _handle(duck_pt, FRAME)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert not comm.local_transport()
    res = comm.render_adaptive(r, *calls[0])
    assert res["rank"]["pixel_samples"] == res["max_rank_pixel_samples"] == want["pixel_samples"] and res["frame_leading_samples"] == 32
    for loopback in (True, False):
        assert r.gather_frame(comm, root=0, loopback=loopback, aovs=True, moments=True, tile_counts=True)
        _check_root(comm, r, FRAME, want["counts"].tolist(), whole, True, ("rccl", loopback))
    comm.close()
    r.close()
