"""The frame gather carrying the AOV and moment sums, and the denoiser / noise estimate on the root (rf_renderer_gather_frame with RF_GATHER_AOVS / RF_GATHER_MOMENTS,
rf_comm_read_plane / _denoise / _read_denoised / _noise_estimate): N tile-sharded handles and N communicators of the local test transport in one process, one host
thread per rank.  The defining property (include/rayfinder_amd.h): the gathered planes, the denoised frame and the estimate on the root are bit for bit what ONE
handle without a tile shard gives after the same samples."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

BIG = (200, 150, 3, 2)      # 35 tiles, ragged on both edges; wide enough that the step-16 a-trous taps cross several owners' tiles
SMALL = (70, 45, 2, 2)      # 6 tiles: fewer tiles than ranks at world 8
SECOND = (96, 64, 2, 2)     # the second frame size of one communicator
CUSTOM = dict(iterations=3, sigma_color=0.7, sigma_normal=0.2, sigma_depth=0.05)


def _params(W, H, spp, bounces, exposure=0.25):
    return rf.make_render_parameters(W, H, rf.fly_camera(W, H), spp, bounces, rf.make_sky(), exposure)


def _handle(pt, frame, aovs=True, moments=True):
    r = rf.ReferencePathTracer(_params(*frame), pt.scene())
    if aovs:
        r.set_aovs(True)
    if moments:
        r.set_moments(True)
    return r


def _sums(r):
    """The four per-pixel sums of a handle as the gather numbers them: [S, AC, ND, Q]"""
    S, n = r.read_accumulation()
    a = r.read_aovs()
    Q, nq = r.read_moments()
    assert a["samples"] == n and nq == n
    return [S, np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), Q], n


_PT = {}


@functools.lru_cache(maxsize=None)
def _whole(frame):
    """ONE handle without a tile shard over `frame`: its sums, its denoised frame for both parameter sets and its estimate.  Computed once; read-only."""
    r = _handle(_PT["duck"], frame)
    r.render(frame[2])
    planes, n = _sums(r)
    out = dict(planes=planes, samples=n, denoised={})
    for name, params in (("default", {}), ("custom", CUSTOM)):
        r.denoise(**params)
        out["denoised"][name] = r.read_denoised()
    out["estimate"] = r.noise_estimate() if n >= 2 else None
    r.close()
    for p in planes:
        p.setflags(write=False)
    return out


@pytest.fixture(autouse=True)
def _scene(duck_pt):
    _PT["duck"] = duck_pt


def _local_world(pt, frame, world, script, aovs=True, moments=True):
    """N renderers + N communicators of the LOCAL test transport in this one process, one host thread per rank (ctypes releases the GIL), in the shape of
    tests/test_gpu_parity.py's _local_world_gather: every rank makes its handle, shard and communicator and runs script(rank, r, comm, out), which the ranks must
    walk in step (every gather is collective); all_reduce_max is the barrier before tear-down."""
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _handle(pt, frame, aovs, moments)
            r.set_tile_shard(rank, world)
            comm = rf.TileComm(uid, rank, world, 0)
            assert comm.local_transport() and comm.info()["rccl_ranks"] == world
            script(rank, r, comm, out)
            out[("max", rank)] = comm.all_reduce_max(float(rank), r)   # (also a barrier: nobody tears its buffers down while a peer still copies from them)
            comm.close()
            r.close()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(300)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads), "a rank hangs in the exchange"
    assert all(out[("max", k)] == float(world - 1) for k in range(world))
    return out


def _local(monkeypatch):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "120")


def _refused(match, call, *args, **kw):
    with pytest.raises(rf.RayfinderError, match=match) as e:
        call(*args, **kw)
    assert e.value.status == rf._ffi.RF_ERROR_INVALID_ARGUMENT


def _owns_tiles(frame, rank, world):
    return len(rf.tiles_for_rank(frame[0], frame[1], rank, world)) > 0


def _check_planes(comm, r, frame, world, root, aovs, moments, what):
    """Root: gathered_planes() reports the gather, the carried planes equal the whole-frame handle's reads as bits, the others are refused."""
    want = _whole(frame)
    g = comm.gathered_planes()
    assert (g["aovs"], g["moments"], g["width"], g["height"]) == (aovs, moments, frame[0], frame[1]), (what, g)
    assert g["samples"] == (frame[2] if _owns_tiles(frame, root, world) else 0), (what, g)      # the root handle's accumulated count
    carried = [True, aovs, aovs, moments]
    for plane in range(4):
        if carried[plane]:
            assert np.array_equal(bits(comm.read_plane(r, plane)), bits(want["planes"][plane])), (what, plane)
        else:
            _refused("did not carry", comm.read_plane, r, plane)
    _refused("plane out of range", comm.read_plane, r, 4)
    assert np.array_equal(bits(comm.read_frame(r, frame[0], frame[1])), bits(want["planes"][0])), what        # (the plain read still reads plane 0)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_gathered_planes_equal_the_whole_frame_handle_s_reads(duck_pt, monkeypatch, world):
    """Every combination of carried planes, loop-back on top, a second and a third frame size on the same communicator (the small one has fewer tiles than a world
    of 8 has ranks), and a plain gather afterwards, for roots 0 and N - 1: kUntilePlanes assembles each plane from the root's own shard (in place) and the N - 1
    staged ones."""
    _local(monkeypatch)
    for root in sorted({0, world - 1}):
        def script(rank, r, comm, out, root=root):
            is_root = rank == root
            r.render(BIG[2])
            for aovs, moments, loopback in ((True, True, False), (True, False, False), (False, True, False), (True, True, True)):
                ptr = r.gather_frame(comm, root=root, loopback=loopback, aovs=aovs, moments=moments)
                assert bool(ptr) == is_root
                if is_root:
                    _check_planes(comm, r, BIG, world, root, aovs, moments, (world, root, aovs, moments, loopback))
                assert comm.last_exchange_ms() >= 0.0
            for frame in (SECOND, SMALL):                    # another frame size on the same handle and communicator: the layout, staging areas and images follow
                r.set_render_parameters(_params(*frame))
                r.render(frame[2])
                r.gather_frame(comm, root=root, aovs=True, moments=True)
                if is_root:
                    _check_planes(comm, r, frame, world, root, True, True, (world, root, frame))
            r.gather_frame(comm, root=root)                  # a plain gather: the extra planes are gone, its image is right
            if is_root:
                _check_planes(comm, r, SMALL, world, root, False, False, (world, root, "plain"))
                out["root finished"] = rank

        assert _local_world(duck_pt, BIG, world, script)["root finished"] == root


@pytest.mark.parametrize("world", [2, 3])
def test_denoise_on_the_root_equals_the_whole_frame_handle_s(duck_pt, monkeypatch, world):
    _local(monkeypatch)
    want = _whole(BIG)
    root = world - 1

    def script(rank, r, comm, out):
        r.render(BIG[2])
        r.gather_frame(comm, root=root, aovs=True)
        if rank != root:
            return
        _refused("no denoised image", comm.read_denoised, r)
        for name, params in (("default", None), ("custom", CUSTOM)):
            comm.denoise(r, params)
            rgb, bgra, n = comm.read_denoised(r)
            w_rgb, w_bgra, w_n = want["denoised"][name]
            assert np.array_equal(bits(rgb), bits(w_rgb)), (world, name)
            assert np.array_equal(bgra, w_bgra), (world, name)
            assert n == w_n == BIG[2]
        _refused("iterations", comm.denoise, r, dict(iterations=9))
        _refused("sigma", comm.denoise, r, dict(sigma_depth=float("nan")))
        out["root finished"] = rank

    assert _local_world(duck_pt, BIG, world, script, moments=False)["root finished"] == root


def test_noise_estimate_on_the_root_equals_the_whole_frame_handle_s(duck_pt, monkeypatch):
    _local(monkeypatch)
    want = _whole(BIG)["estimate"]
    world, root = 3, 0

    def script(rank, r, comm, out):
        r.render(BIG[2])
        r.gather_frame(comm, root=root, moments=True)
        if rank != root:
            return
        got = comm.noise_estimate(r)
        for key in ("mean_error", "max_error", "worst_tile", "samples", "pixels", "nonfinite_pixels"):
            assert got[key] == want[key], (key, got[key], want[key])
        assert got["samples"] == BIG[2] == 3
        for key in ("error_map", "tile_sum", "tile_max"):
            assert np.array_equal(bits(got[key]), bits(want[key])), key
        scalars = comm.noise_estimate(r, maps=False)
        assert scalars["error_map"] is None and scalars["mean_error"] == want["mean_error"] and scalars["max_error"] == want["max_error"]
        out["root finished"] = rank

    assert _local_world(duck_pt, BIG, world, script, aovs=False)["root finished"] == root


RAGGED = (72, 40, 3, 4)     # 3 x 2 tiles, ragged on both edges: a world of 8 leaves ranks 6 and 7 without a tile


@functools.lru_cache(maxsize=None)
def _whole_with_counts():
    """ONE handle without a tile shard over RAGGED, the AOVs kept with tile counts: its four sums and its per-tile counts.  Computed once; read-only."""
    r = _handle(_PT["duck"], RAGGED, aovs=False)
    r.set_aovs(True, tile_counts=True)
    r.render(RAGGED[2])
    planes, n = _sums(r)
    counts = r.read_tile_samples()
    r.close()
    for a in planes + [counts]:
        a.setflags(write=False)
    return dict(planes=planes, samples=n, counts=counts)


@pytest.mark.parametrize("world,root", [(3, 2), (8, 7)])
def test_one_gather_carries_every_plane_and_the_tile_counts(duck_pt, monkeypatch, world, root):
    """ONE gather with the AOVs, the moments and the per-tile counts in its group, to a root that is not rank 0 and, at world 8, owns no tile (it passes no buffer of
    its own and un-tiles from the staging areas alone): the four planes and the counts on the root equal the whole-frame handle's reads bit for bit."""
    _local(monkeypatch)
    want = _whole_with_counts()
    assert _owns_tiles(RAGGED, root, world) == (world == 3)

    def script(rank, r, comm, out):
        r.set_aovs(True, tile_counts=True)
        r.render(RAGGED[2])
        ptr = r.gather_frame(comm, root=root, aovs=True, moments=True, tile_counts=True)
        assert bool(ptr) == (rank == root)
        if rank != root:
            return
        g = comm.gathered_planes()
        assert g.get("tile_counts") and g["aovs"] and g["moments"] and (g["width"], g["height"], g["samples"]) == (RAGGED[0], RAGGED[1], want["samples"]), g
        for plane in range(4):
            assert np.array_equal(bits(comm.read_plane(r, plane)), bits(want["planes"][plane])), plane
        got = comm.read_tile_samples()
        assert got.dtype == want["counts"].dtype and np.array_equal(got, want["counts"]), got
        out["root finished"] = rank

    assert _local_world(duck_pt, RAGGED, world, script, aovs=False)["root finished"] == root


def test_refusals_keep_the_state(duck_pt, monkeypatch):
    """Every refusal is an RF_ERROR_INVALID_ARGUMENT that leaves the handle and the communicator as they were: the valid call that follows succeeds.  Both ranks walk
    the same script (each owns tiles of the 70 x 45 frame), so a gather refused on one is refused on the other and nobody waits."""
    _local(monkeypatch)
    frame, world, root = SMALL, 2, 1
    want = _whole(frame)

    def root_side(comm, r, match):
        _refused(match, comm.gathered_planes)
        _refused(match, comm.read_plane, r, 0)
        _refused(match, comm.denoise, r)
        _refused(match, comm.read_denoised, r)
        _refused(match, comm.noise_estimate, r)

    def script(rank, r, comm, out):
        is_root = rank == root
        # before any sample, before any gather
        _refused("RF_GATHER_AOVS: no sample has been accumulated", r.gather_frame, comm, root=root, aovs=True)
        _refused("RF_GATHER_MOMENTS: no sample has been accumulated", r.gather_frame, comm, root=root, moments=True)
        root_side(comm, r, "no gather has been made")
        # the switches off
        r.set_aovs(False)
        r.set_moments(False)
        r.render(1)
        _refused("RF_GATHER_AOVS needs the first-hit AOVs", r.gather_frame, comm, root=root, aovs=True)
        _refused("RF_GATHER_MOMENTS needs the radiance second moments", r.gather_frame, comm, root=root, moments=True)
        # turned on after the first sample
        r.set_aovs(True)
        r.set_moments(True)
        r.render(1)
        _refused(r"the AOV sample count \(1\) differs from the accumulated sample count \(2\)", r.gather_frame, comm, root=root, aovs=True, moments=False)
        _refused(r"the moment sample count \(1\) differs from the accumulated sample count \(2\)", r.gather_frame, comm, root=root, moments=True)
        root_side(comm, r, "no gather has been made")                       # (a refused gather is no gather)
        # the state was kept: the plain gather of the two samples succeeds and is right
        ptr = r.gather_frame(comm, root=root)
        assert bool(ptr) == is_root and r.read_accumulation()[1] == 2
        if not is_root:
            root_side(comm, r, "was not the root of the last gather")
        else:
            assert comm.gathered_planes() == dict(aovs=False, moments=False, width=frame[0], height=frame[1], samples=2)
            assert np.array_equal(bits(comm.read_plane(r, 0)), bits(want["planes"][0]))
            _refused("did not carry the first-hit AOVs", comm.denoise, r)
            _refused("did not carry the first-hit AOVs", comm.read_denoised, r)
            _refused("did not carry the radiance second moments", comm.noise_estimate, r)
            _refused("did not carry the first-hit AOVs", comm.read_plane, r, 1)
            _refused("did not carry the radiance second moments", comm.read_plane, r, 3)
        # one sample with everything on from the start: the planes travel, the denoiser runs, the estimate needs two
        r.set_render_parameters(_params(*frame, exposure=0.5))                 # (restarts the accumulation)
        r.render(1)
        r.gather_frame(comm, root=root, aovs=True, moments=True)
        if is_root:
            assert comm.gathered_planes()["samples"] == 1
            _refused("at least 2 accumulated samples", comm.noise_estimate, r)
            comm.denoise(r)
            assert comm.read_denoised(r)[2] == 1
        r.render(1)
        r.gather_frame(comm, root=root, aovs=True, moments=True)
        if is_root:
            _refused("no denoised image", comm.read_denoised, r)             # the snapshot was dropped by the gather
            got = comm.noise_estimate(r, maps=False)
            assert got["samples"] == 2 and got["mean_error"] == want["estimate"]["mean_error"]
            for plane in range(4):
                assert np.array_equal(bits(comm.read_plane(r, plane)), bits(want["planes"][plane])), plane
        out[("finished", rank)] = True

    out = _local_world(duck_pt, frame, world, script)
    assert out[("finished", 0)] and out[("finished", 1)]


def test_rccl_world_size_one_carries_every_plane(duck_pt, monkeypatch):
    """RCCL itself: a world-size-1 communicator, every plane sent to itself through ncclSend / ncclRecv in the one group (loop-back), un-tiled by kUntilePlanes; the
    planes, the denoised frame and the estimate equal the handle's own."""
    monkeypatch.delenv("RF_COMM_TRANSPORT", raising=False)
    frame = BIG
    r = _handle(duck_pt, frame)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert not comm.local_transport()
    r.render(frame[2])
    want, n = _sums(r)
    for loopback in (True, False):
        ptr = r.gather_frame(comm, root=0, loopback=loopback, aovs=True, moments=True)
        assert ptr
        assert comm.gathered_planes() == dict(aovs=True, moments=True, width=frame[0], height=frame[1], samples=n)
        # the planes' device images: plane 0 is the image the gather returned, and each has its own
        device = []
        for plane in range(4):
            p = C.c_void_p()
            rf.check(rf._ffi.lib.rf_comm_plane_device(comm._h, plane, C.byref(p)))
            device.append(p.value)
        assert device[0] == ptr and len(set(device)) == 4 and all(device)
        assert np.array_equal(r.tonemap_device_image(device[0], frame[0], frame[1], n), r.read_tonemapped())
        for plane in range(4):
            assert np.array_equal(bits(comm.read_plane(r, plane)), bits(want[plane])), (loopback, plane)
        comm.denoise(r)
        rgb, bgra, dn = comm.read_denoised(r)
        r.denoise()
        w_rgb, w_bgra, w_n = r.read_denoised()
        assert np.array_equal(bits(rgb), bits(w_rgb)) and np.array_equal(bgra, w_bgra) and dn == w_n == n
        got, own = comm.noise_estimate(r), r.noise_estimate()
        assert all(got[k] == own[k] for k in ("mean_error", "max_error", "worst_tile", "samples", "pixels", "nonfinite_pixels"))
        assert all(np.array_equal(bits(got[k]), bits(own[k])) for k in ("error_map", "tile_sum", "tile_max"))
    assert comm.all_reduce_max(3.5, r) == 3.5
    comm.close()
    r.close()


def test_rf_render_writes_the_same_files_on_three_ranks(duck_pt, tmp_path):
    """rf-render --gpus 3 takes every output from the planes gathered on rank 0 (rf_comm_denoise, rf_comm_noise_estimate, rf_comm_read_plane): each file is
    byte-identical to the --gpus 1 run's, which takes them from the handle."""
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    W, H, spp, bounces = 200, 150, 3, 2
    names = ("out.png", "i.pfm", "d.png", "d.pfm", "m.pfm", "a.pfm", "n.pfm", "z.pfm")
    files, lines = {}, {}
    env = dict(os.environ, RF_COMM_TRANSPORT="local", RF_COMM_TIMEOUT_S="120")
    for gpus in (1, 3):
        d = tmp_path / f"g{gpus}"
        d.mkdir()
        txt = subprocess.check_output([exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces), "--out", str(d / "out.png"),
                                       "--pfm", str(d / "i.pfm"), "--denoise", str(d / "d.png"), "--denoise-pfm", str(d / "d.pfm"), "--noise-map", str(d / "m.pfm"),
                                       "--aov-albedo", str(d / "a.pfm"), "--aov-normal", str(d / "n.pfm"), "--aov-depth", str(d / "z.pfm"), "--gpus", str(gpus)],
                                      env=env, timeout=300).decode()
        assert f"on {gpus} GPU(s)" in txt
        lines[gpus] = [line for line in txt.splitlines() if line.startswith("noise at")]
        files[gpus] = {name: open(d / name, "rb").read() for name in names}
    for name in names:
        assert len(files[1][name]) > 100 and files[3][name] == files[1][name], name
    assert lines[1] == lines[3] and len(lines[1]) == 1
