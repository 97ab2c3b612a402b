"""Checkpoint, resume and re-shard on the GPU, and the device state digest against its restatement (tests/digest_restatement.py).
Frames are 70 x 45 (3 x 2 tiles, ragged right and bottom), Duck, 3 bounces, at most 16 spp.  Corrupt inputs only change float payload bits or stored digests: every
length and count of a blob is checked on the host before any copy."""
import numpy as np
import pytest

import rayfinder_amd as rf
import digest_restatement as dr
from conftest import bits
from noise_restatement import estimate
from adaptive_restatement import tile_errors

pytestmark = pytest.mark.gpu
INVALID, CORRUPT = rf._ffi.RF_ERROR_INVALID_ARGUMENT, rf._ffi.RF_ERROR_CORRUPT
W, H, SPP, BOUNCES, EXPOSURE = 70, 45, 16, 3, 0.25
MASK = (1 << 64) - 1


def _camera(w=W, h=H, second=False):
    return rf.fly_camera(w, h, position=(1.0, 1.4, -1.4), yaw_degrees=125.0) if second else rf.fly_camera(w, h)


def _params(w=W, h=H, spp=SPP, bounces=BOUNCES, second=False):
    return rf.make_render_parameters(w, h, _camera(w, h, second), spp, bounces, rf.make_sky(), EXPOSURE)


def _handle(pt, everything=True, adaptive=False, params=None, **kw):
    """everything: AOVs, moments, direct, buckets K = 3 (adaptive: each with its per-tile-count bit)"""
    r = rf.ReferencePathTracer(params or _params(), pt.scene(), **kw)
    r.set_moments(True)
    if everything:
        r.set_aovs(True, tile_counts=adaptive)
        r.set_direct(True, tile_counts=adaptive)
        r.set_buckets(3, tile_counts=adaptive)
    return r


def _planes(r):
    """The handle's sums as the digest sees them: name -> (H, W, 4) image, None while off"""
    a = r.read_aovs()
    k, _ = r.read_buckets()
    d = r.state_digest()
    return dict(accumulation=r.read_accumulation()[0],
                albedo_coverage=np.concatenate([a["albedo"], a["coverage"][..., None]], -1) if d["family_on"][1] else None,
                normal_depth=np.concatenate([a["normal"], a["depth"][..., None]], -1) if d["family_on"][1] else None,
                moments=r.read_moments()[0] if d["family_on"][2] else None, direct=r.read_direct()[0] if d["family_on"][3] else None, buckets=k if len(k) else None)


def _reads(r, whole=True):
    """Everything the handle reports, as bit patterns / integers"""
    img, acc = r.read_accumulation()
    a = r.read_aovs()
    q, nq = r.read_moments()
    d, nd = r.read_direct()
    b, nb = r.read_buckets()
    out = dict(S=bits(img), acc=acc, albedo=bits(a["albedo"]), normal=bits(a["normal"]), depth=bits(a["depth"]), coverage=bits(a["coverage"]), na=a["samples"], Q=bits(q), nq=nq,
               D=bits(d), nd=nd, B=bits(b), nb=nb, counts=r.read_tile_samples().reshape(-1).astype(np.int64), mean=bits(r.read_mean()), bgra=r.read_tonemapped())
    return out


def _differ(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def _restated(r):
    return dr.handle_digest(_planes(r), r.read_tile_samples().reshape(-1), r.shard_tiles())


def _check_digest(r):
    d, want = r.state_digest(), _restated(r)
    for k, v in want.items():
        assert d[k] == v, (k, d[k], v)
    return d


def _refused(call, status, *words):
    with pytest.raises(rf.RayfinderError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ------------------------------------------------------------------------------------------------ 1
def test_resume_with_everything_on_equals_the_uninterrupted_render(duck_pt):
    def start():
        r = _handle(duck_pt)
        r.render(3)
        r.set_render_parameters(_params(second=True))  # a restart: the accumulation now begins at frame counter 3
        return r

    a = start()
    a.render(8)
    blob = a.save_checkpoint()
    info = rf.checkpoint_info(blob)
    assert (info["frame_count"], info["accumulated"], info["num_tiles"], info["stored_planes"]) == (11, 8, 6, 8)
    b = _handle(duck_pt, params=_params(second=True))
    b.load_checkpoint(blob)
    assert b.state_digest() == a.state_digest()
    assert not _differ(_reads(a), _reads(b))
    a.render(8), b.render(8)
    c = start()
    c.render(16)
    want = _reads(c)
    assert want["acc"] == 16 and not _differ(want, _reads(a)) and not _differ(want, _reads(b))
    assert b.state_digest() == c.state_digest() and c.state_digest()["frame_count"] == 19
    # (a loader that ignored the saved frame counter would have traced frames 0 .. 7 again)
    fresh = _handle(duck_pt, params=_params(second=True))
    fresh.render(16)
    assert _differ(want, _reads(fresh))
    for r in (a, b, c, fresh):
        r.close()


def test_resume_sets_the_switches_from_the_file(duck_pt, tmp_path):
    a = _handle(duck_pt)
    a.render(5)
    path = tmp_path / "duck.ckpt"
    assert a.save_checkpoint(path) == path.read_bytes() and not list(tmp_path.glob("*.tmp*"))
    b = rf.ReferencePathTracer(_params(), duck_pt.scene())
    info = b.resume(path)
    assert (info["aov_flags"], info["moments_on"], info["direct_word"], info["buckets_word"]) == (1, 1, 1, 3)
    assert b.state_digest() == a.state_digest() and not _differ(_reads(a), _reads(b))
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------ 2
def test_the_non_uniform_state_survives_a_checkpoint(duck_pt):
    probe = _handle(duck_pt, everything=False)
    probe.render(4)
    target = float(np.float32(np.median(tile_errors(estimate(probe.read_accumulation()[0], probe.read_moments()[0], 4)))))
    probe.close()
    a, c = _handle(duck_pt, adaptive=True), _handle(duck_pt, adaptive=True)
    for r in (a, c):
        r.render_adaptive(target, 4, 4)
    counts = a.read_tile_samples().reshape(-1)
    assert len(set(counts.tolist())) >= 2, counts
    _check_digest(a)
    b = _handle(duck_pt, adaptive=True)
    b.load_checkpoint(a.save_checkpoint())
    assert b.state_digest() == a.state_digest() and not _differ(_reads(a), _reads(b))
    assert not b.tile_samples_uniform()
    for r in (b, c):
        r.render_adaptive(target / 2, 4, 4)
    want = _reads(c)
    assert not _differ(want, _reads(b)) and b.state_digest() == c.state_digest()
    for r in (b, c):
        r.denoise()
    assert np.array_equal(bits(b.read_denoised()[0]), bits(c.read_denoised()[0]))
    for r in (b, c):
        r.denoise_split()
    assert np.array_equal(bits(b.read_denoised()[0]), bits(c.read_denoised()[0]))
    for r in (a, b, c):
        r.close()


# ------------------------------------------------------------------------------------------------ 3
def test_reshard_one_to_three_and_three_to_one(duck_pt):
    whole = _handle(duck_pt)
    whole.render(6)
    blob = whole.save_checkpoint()
    ranks = []
    for k in range(3):
        r = _handle(duck_pt)
        r.set_tile_shard(k, 3)
        r.load_checkpoint(blob)  # the tiles of the other two ranks are ignored
        ranks.append(r)
    whole.render(4)
    for r in ranks:
        r.render(4)
    want = _reads(whole)
    for key, read in (("S", lambda r: r.read_accumulation()[0]), ("Q", lambda r: r.read_moments()[0]), ("D", lambda r: r.read_direct()[0]), ("B", lambda r: r.read_buckets()[0]),
                      ("albedo", lambda r: r.read_aovs()["albedo"]), ("normal", lambda r: r.read_aovs()["normal"]), ("depth", lambda r: r.read_aovs()["depth"]),
                      ("coverage", lambda r: r.read_aovs()["coverage"])):
        # (every pixel belongs to one rank and the others read it as +0.0, all bits clear: the assembly is the OR of the bit patterns)
        assert np.array_equal(bits(read(ranks[0])) | bits(read(ranks[1])) | bits(read(ranks[2])), want[key]), key
    digests = [_check_digest(r) for r in ranks]
    total = _check_digest(whole)
    for key in ("accumulation", "albedo_coverage", "normal_depth", "moments", "direct", "counts"):
        assert sum(d[key] for d in digests) & MASK == total[key], key
    assert [sum(d["bucket"][b] for d in digests) & MASK for b in range(15)] == total["bucket"]
    # 3 -> 1
    blobs = [r.save_checkpoint() for r in ranks]
    one = _handle(duck_pt)
    before = one.state_digest()
    _refused(lambda: one.load_checkpoint(blobs[:2]), INVALID, "missing")
    _refused(lambda: one.load_checkpoint(blobs + blobs[1:2]), INVALID, "twice")
    assert one.state_digest() == before
    one.load_checkpoint(blobs)
    assert one.state_digest() == total and not _differ(want, _reads(one))
    for r in ranks + [whole, one]:
        r.close()


# ------------------------------------------------------------------------------------------------ 4
def test_the_digest_equals_its_restatement(duck_pt):
    r = _handle(duck_pt)
    restarted = _check_digest(r)  # nothing rendered: the zeros of its frame
    assert restarted["accumulation"] == dr.plane_digest(0, np.zeros((H, W, 4), np.float32)) != 0 and restarted["accumulated"] == 0
    r.render(5)
    d5 = _check_digest(r)
    assert d5["family_on"] == [1] * 5 and d5["family_samples"] == [5] * 5 and (d5["frame_count"], d5["num_tiles"]) == (5, 6)
    r.render(1)
    d6 = _check_digest(r)
    assert all(d6[k] != d5[k] for k in ("accumulation", "moments", "direct", "counts")) and d6["bucket"][2] != d5["bucket"][2]
    r.close()
    # scheduling is invisible; off families digest 0
    for opts, kw in (({"traversal_variant": 0}, {}), ({"traversal_variant": 1}, {}), ({}, {"max_paths_in_flight": 3 * 6 * 1024})):
        v = _handle(duck_pt, **kw)
        for name, value in opts.items():
            v.set_option(name, value)
        v.render(6)
        assert v.state_digest() == d6, (opts, kw)
        v.close()
    plain = _handle(duck_pt, everything=False)
    plain.render(6)
    d = _check_digest(plain)
    assert d["accumulation"] == d6["accumulation"] and d["moments"] == d6["moments"]
    assert d["albedo_coverage"] == d["normal_depth"] == d["direct"] == 0 and d["bucket"] == [0] * 15 and d["family_on"] == [1, 0, 1, 0, 0]
    plain.close()
    # one row of pixels over two tiles, the second a single column
    thin = _handle(duck_pt, params=_params(33, 1))
    thin.render(3)
    assert _check_digest(thin)["num_tiles"] == 2
    thin.close()
    # every rank of world 3: restarted (the zeros of its own shard, which add up to the zeros of the frame), then after samples
    ranks = []
    for k in range(3):
        s = _handle(duck_pt)
        s.set_tile_shard(k, 3)
        ranks.append((s, _check_digest(s)))
    assert all(d["accumulated"] == 0 and d["family_samples"] == [0] * 5 and d["num_tiles"] == 2 for _, d in ranks)
    for key in ("accumulation", "albedo_coverage", "normal_depth", "moments", "direct", "counts"):
        assert sum(d[key] for _, d in ranks) & MASK == restarted[key], key
        assert len({d[key] for _, d in ranks}) == 3, key  # (the same zeros at other frame indices: another digest)
    for s, _ in ranks:
        s.render(6)
    after = [_check_digest(s) for s, _ in ranks]
    for key in ("accumulation", "albedo_coverage", "normal_depth", "moments", "direct", "counts"):
        assert sum(d[key] for d in after) & MASK == d6[key], key
    for s, _ in ranks:
        s.close()


def test_the_digest_on_a_bound_accumulation_buffer(duck_pt):
    import torch
    r = _handle(duck_pt, everything=False)
    _, nbytes = r.accumulation_device_buffer()
    own = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    r.bind_accumulation_buffer(own.data_ptr(), nbytes)
    r.render(4)
    d = _check_digest(r)
    blob = r.save_checkpoint()
    other = _handle(duck_pt, everything=False)
    mine = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    other.bind_accumulation_buffer(mine.data_ptr(), nbytes)
    other.load_checkpoint(blob)
    other.synchronize()
    assert other.state_digest() == d and torch.equal(own, mine)
    r.close(), other.close()


# ------------------------------------------------------------------------------------------------ 5
def test_refusals_change_nothing(duck_pt):
    a = _handle(duck_pt)
    a.render(6)
    blob = a.save_checkpoint()
    a.close()

    def refused(handle, *words, what=blob):
        handle.render(2)
        before, reads = handle.state_digest(), _reads(handle)
        _refused(lambda: handle.load_checkpoint(what), INVALID, *words)
        assert handle.state_digest() == before and not _differ(reads, _reads(handle))
        handle.close()

    refused(_handle(duck_pt, params=_params(64, 45)), "size")
    refused(_handle(duck_pt, params=_params(second=True)), "camera")
    refused(_handle(duck_pt, params=_params(bounces=2)), "numBounces")
    refused(_handle(duck_pt, params=_params(spp=4)), "numSamplesPerPixel")
    other = _handle(duck_pt)
    other.set_buckets(5)
    refused(other, "switch")
    import analytic_scene as an
    from test_oracle_pins import corner_rects
    P, N, T, I, tex = an.scene_arrays(corner_rects())
    refused(_handle(rf.PtFormat.from_triangles(P, N, T, I, tex)), "scene")


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("where", ["payload", "digest"])
def test_a_flipped_bit_is_corrupt_and_the_handle_stays_usable(duck_pt, where):
    a = _handle(duck_pt)
    a.render(6)
    blob = bytearray(a.save_checkpoint())
    a.close()
    n, planes = 6, 8
    at = 288 + 8 * n + 8 * planes * n  # the first plane's first texel
    if where == "payload":
        blob[at + 16 * 1024 * 4 + 16 * 5 + 1] ^= 0x10  # a mantissa bit of an in-frame texel of tile 4 of S
    else:
        blob[288 + 8 * n + 8 * (2 * n + 3)] ^= 0x01    # the stored digest of plane ND, tile 3
    b = _handle(duck_pt)
    b.render(3)
    _refused(lambda: b.load_checkpoint(bytes(blob)), CORRUPT, "corrupt")
    d = _check_digest(b)
    assert (d["frame_count"], d["accumulated"]) == (3, 0) and d["family_samples"] == [0] * 5
    assert not b.read_accumulation()[0].any() and b.read_accumulation()[1] == 0
    b.render(4)
    fresh = _handle(duck_pt)
    fresh.render(3)
    fresh.set_render_parameters(_params(second=True)), fresh.set_render_parameters(_params())  # restarted at frame counter 3
    fresh.render(4)
    assert not _differ(_reads(fresh), _reads(b)) and b.state_digest() == fresh.state_digest()
    b.close(), fresh.close()


# ------------------------------------------------------------------------------------------------ 7
def _local_world(pt, world, script):
    """`world` handles and communicators of the local test transport in this one process, one host thread per rank; every rank runs script(rank, r, comm, out) and the
    ranks walk it in step.  all_reduce_max is the barrier before tear-down."""
    import threading
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _sharded_handle(pt)
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
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads), "a rank hangs in an exchange"
    return out


def _sharded_handle(pt):
    """moments, AOVs and direct sums, each kept per tile count"""
    r = rf.ReferencePathTracer(_params(), pt.scene())
    r.set_moments(True)
    r.set_aovs(True, tile_counts=True)
    r.set_direct(True, tile_counts=True)
    return r


def _frame_reads(r):
    a = r.read_aovs()
    return dict(counts=r.read_tile_samples().reshape(-1).astype(np.int64), S=bits(r.read_accumulation()[0]), Q=bits(r.read_moments()[0]), D=bits(r.read_direct()[0]),
                AC=bits(np.concatenate([a["albedo"], a["coverage"][..., None]], -1)), ND=bits(np.concatenate([a["normal"], a["depth"][..., None]], -1)), mean=bits(r.read_mean()))


def test_across_ranks_through_the_local_transport(duck_pt, monkeypatch):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "60")
    probe = _handle(duck_pt, everything=False)
    probe.render(4)
    target = float(np.float32(np.median(tile_errors(estimate(probe.read_accumulation()[0], probe.read_moments()[0], 4)))))
    probe.close()
    one = _sharded_handle(duck_pt)
    one.render_adaptive(target, 4, 4)
    first, first_digest = _frame_reads(one), one.state_digest()
    assert len(set(first["counts"].tolist())) >= 2, first["counts"]
    one.render_adaptive(target / 2, 4, 4)
    second = _frame_reads(one)
    assert _differ(first, second)
    one.close()

    # every rank of world 2 samples adaptively and saves; the two blobs load into a whole-frame handle
    def save(rank, r, comm, out):
        res = comm.render_adaptive(r, target, 4, 4)
        out[("blob", rank)], out[("digest", rank)], out[("res", rank)] = r.save_checkpoint(), r.state_digest(), res

    out = _local_world(duck_pt, 2, save)
    infos = [rf.checkpoint_info(out[("blob", k)]) for k in range(2)]
    assert all(i["frame_leading_samples"] == int(first["counts"].max()) and i["frame_min_tile_samples"] == int(first["counts"].min()) for i in infos), infos
    whole = _sharded_handle(duck_pt)
    whole.load_checkpoint([out[("blob", k)] for k in range(2)])
    assert not _differ(first, _frame_reads(whole))
    got = whole.state_digest()
    assert got == first_digest
    for key in ("accumulation", "albedo_coverage", "normal_depth", "moments", "direct", "counts"):
        assert sum(out[("digest", k)][key] for k in range(2)) & MASK == got[key], key
    blob = whole.save_checkpoint()
    whole.close()

    # ... whose blob loads into world 2; a second call there, and the gathered frame is the one-GPU handle's after ITS second call
    def resume(rank, r, comm, out):
        r.load_checkpoint(blob)
        # the FRAME is non-uniform on every rank, whatever its own tiles hold (one tile, or none): a plain render is refused as after rf_comm_render_adaptive
        _refused(lambda: r.render(1), INVALID, "different sample counts")
        comm.render_adaptive(r, target / 2, 4, 4)
        ptr = r.gather_frame(comm, root=0, aovs=True, moments=True, tile_counts=True, direct=True)
        if rank == 0:
            assert ptr
            assert comm.read_tile_samples().reshape(-1).tolist() == second["counts"].tolist()
            for plane, key in ((0, "S"), (1, "AC"), (2, "ND"), (3, "Q"), (5, "D")):
                assert np.array_equal(bits(comm.read_plane(r, plane)), second[key]), key
            assert np.array_equal(bits(comm.read_mean(r)), second["mean"])
            out["root finished"] = True

    assert _local_world(duck_pt, 2, resume)["root finished"]
    # ... and into world 8, where ranks 6 and 7 hold no tile: they load with no sample of their own and follow the frame through the second call all the same
    assert len(rf.tiles_for_rank(W, H, 7, 8)) == 0
    assert _local_world(duck_pt, 8, resume)["root finished"]


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_walk_survives_two_checkpoint_cycles(seed):
    """tests/handle_walk.py's seeded call sequences against the model (tests/checkpoint_model.py); at two random points the handle is saved, closed, created again
    and loaded.  After every call, and after each cycle, the handle's observables equal the model's."""
    import handle_walk as hw
    import test_gpu_handle_walk as g
    from checkpoint_model import CheckpointedModel
    calls, scheduling = hw.walk(seed)
    scene, camera, sky = hw.frame()
    model = CheckpointedModel(scene, hw.W, hw.H, hw.SPP, hw.BOUNCES, hw.EXPOSURE, camera, sky)
    rng = np.random.default_rng(7000 + seed)
    cycles = set(int(c) for c in rng.choice(np.arange(2, len(calls)), 2, replace=False))
    r, keep = g.new_handle(scheduling), []
    try:
        for i, call in enumerate(calls):
            if i in cycles:
                blob = r.save_checkpoint()
                r.close()
                r, keep = g.new_handle(scheduling), []
                r.set_render_parameters(g._params(model.exposure))
                if model.world != 1:
                    r.set_tile_shard(model.rank, model.world)
                info = rf.checkpoint_info(blob)
                rf.check(rf.lib.rf_renderer_set_aovs(r._h, info["aov_flags"]))
                r.set_moments(info["moments_on"])
                rf.check(rf.lib.rf_renderer_set_buckets(r._h, info["buckets_word"]))
                r.load_checkpoint(blob)
                model.checkpoint_cycle()
                assert g.against_model(g.observe_gpu(r), model) == [], (seed, i, "after the cycle")
            want, got = hw.apply(model, call), g.apply_gpu(r, call, keep)
            assert got[0] == want[0], (seed, i, call, got, want)
            assert g.against_model(g.observe_gpu(r), model) == [], (seed, i, call)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 9
def test_rf_render_resumes_to_the_bytes_of_an_uninterrupted_run(duck_pt, tmp_path):
    import os
    import subprocess

    from conftest import ROOT
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    base = [exe, str(scene), "--width", str(W), "--height", str(H), "--bounces", str(BOUNCES)]

    def run(*args):
        return subprocess.run(base + [str(a) for a in args], capture_output=True, timeout=120)

    def files(name):
        return (tmp_path / f"{name}.png").read_bytes(), (tmp_path / f"{name}.pfm").read_bytes()

    ck = tmp_path / "duck.ckpt"
    assert run("--spp", 16, "--out", tmp_path / "plain.png", "--pfm", tmp_path / "plain.pfm").returncode == 0
    first = run("--spp", 8, "--checkpoint", ck, "--checkpoint-every", 3, "--out", tmp_path / "half.png")
    assert first.returncode == 0, first.stderr
    info = rf.checkpoint_info(ck)
    assert (info["accumulated"], info["frame_count"], info["width"], info["height"]) == (8, 8, W, H) and not list(tmp_path.glob("*.tmp"))
    second = run("--resume", ck, "--spp", 16, "--out", tmp_path / "resumed.png", "--pfm", tmp_path / "resumed.pfm")
    assert second.returncode == 0, second.stderr
    assert files("resumed") == files("plain")
    assert (tmp_path / "half.png").read_bytes() != (tmp_path / "plain.png").read_bytes()
    # refusals: several ranks, and a file that is not a checkpoint
    for option in (("--checkpoint", ck), ("--resume", ck)):
        bad = run("--spp", 16, "--gpus", 2, *option)
        assert bad.returncode != 0 and b"--checkpoint / --resume need --gpus 1" in bad.stderr, bad.stderr
    bad = run("--resume", scene, "--spp", 16)
    assert bad.returncode != 0 and b"magic" in bad.stderr, bad.stderr
