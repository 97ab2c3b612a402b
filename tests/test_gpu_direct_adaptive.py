"""The direct sums under tile-adaptive sampling and the split-component denoiser with one count per tile, on the GPU (-m gpu): with 1 | RF_DIRECT_TILE_COUNTS
rf_renderer_render_adaptive and rf_comm_render_adaptive keep their schedule and their other sums, D of every tile is bit for bit the oracle's 1-bounce accumulation of
that tile's own count (and a plain 1-bounce handle's) whichever list-addressed radiance-sum kernel ran, and rf_renderer_denoise_split / rf_denoise_split_tiles equal
tests/split_tiles_restatement.py.  Every comparison is exact.  Targets and expected schedules come from the restatements over the oracle's samples, never from the
code under test; the conditions a schedule is chosen for are asserted from the restatement before the GPU is looked at."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import rayfinder_amd as rf
from adaptive_restatement import play, tile_errors, tile_slices
from conftest import DUCK, ROOT, bits, oracle_scene_from_pt
from noise_restatement import estimate
from oracle import orc
from split_tiles_restatement import denoise_split_tiles
from test_gpu_adaptive import BOUNCES, EXPOSURE, _oracle, _renderer
from test_gpu_split import _decode_png, _read_pfm, _synthetic

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
W, H, SPP, TILES = 150, 90, 48, 15                                            # 5 x 3 tiles, ragged right (22 columns) and bottom (26 rows)
WHY = "different sample counts"
CUSTOM = (dict(iterations=2, sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05), dict(iterations=3, sigma_color=4.0, sigma_normal=0.15, sigma_depth=0.2))


def _refused(call, *words):
    with pytest.raises(rf.RayfinderError) as e:
        call()
    assert e.value.status == INVALID, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def _target(first):
    """The median of the oracle's tile errors at the first check, L = first: about half the tiles stop there"""
    S, Q, _ = _oracle(W, H, SPP)
    return float(np.float32(np.median(tile_errors(estimate(S[first], Q[first], first)))))


def _played(calls):
    """The restatement's state after a sequence of calls (target, check_every, min_samples, max_samples) over the oracle's samples"""
    S, Q, _ = _oracle(W, H, SPP)
    want = None
    for target, every, lo, hi in calls:
        want = play(S, Q, W, H, target, every, min_samples=lo, max_samples=hi, counts=None if want is None else want["counts"])
    return want


@functools.lru_cache(maxsize=None)
def _oracle_direct(tile, count):
    """The oracle's 1-bounce accumulation of the first `count` samples over one tile's in-frame pixels (computed once per (tile, count); read-only)"""
    sc, _ = oracle_scene_from_pt(rf.PtFormat.from_gltf(DUCK))
    rp = orc.make_render_params(W, H, rf.camera_to_array(rf.fly_camera(W, H)), SPP, 1, EXPOSURE, rf.aligned_sky_state(rf.make_sky()))
    rows, cols = tile_slices(W, H)[tile]
    ref, _ = orc.render(sc, rp, 0, count, cols.start, rows.start, cols.stop, rows.stop)
    out = ref[rows, cols].copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _one_bounce_handle(count):
    """read_accumulation of a plain handle with num_bounces = 1 after `count` samples (computed once per count; read-only)"""
    params = rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, 1, rf.make_sky(), EXPOSURE)
    pt = rf.PtFormat.from_gltf(DUCK)
    r = rf.ReferencePathTracer(params, pt.scene())
    r.render(count)
    img, n = r.read_accumulation()
    r.close()
    assert n == count
    img.setflags(write=False)
    return img


def _check_direct_per_tile(D, counts, what):
    """The defining property: D of tile t is the 1-bounce accumulation of the tile's own first counts[t] samples -- the oracle's, and a plain GPU handle's"""
    assert D[..., :3].any()
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        n = int(counts[t])
        assert np.array_equal(bits(D[rows, cols, :3]), bits(_oracle_direct(t, n)[..., :3])), (what, "oracle", t, n)
        assert np.array_equal(bits(D[rows, cols]), bits(_one_bounce_handle(n)[rows, cols])), (what, "1-bounce handle", t, n)


def _handle(pt, direct="tiles", aovs=True, opts=(), **kw):
    """direct: None (never touched), False (set off), True (plain 1), "tiles" (1 | RF_DIRECT_TILE_COUNTS)"""
    r = _renderer(pt, w=W, h=H, spp=SPP, opts=opts, **kw)
    if aovs:
        r.set_aovs(True, tile_counts=True)
    if direct is not None:
        r.set_direct(bool(direct), tile_counts=direct == "tiles")
    return r


def _sums(r):
    S, n = r.read_accumulation()
    a = r.read_aovs()
    return S, np.concatenate([a["albedo"], a["coverage"][..., None]], -1), np.concatenate([a["normal"], a["depth"][..., None]], -1), r.read_moments()[0], n


def _rays(r):
    s = r.stats()
    return {k: v for k, v in s.items() if k.endswith("_rays")}


# ---- 1. D per tile against the oracle, through every kernel form
@pytest.mark.parametrize("name,every,opts,max_paths,runs,counts", [
    ("one lane per pixel: steps of 3", 3, {}, 0, 0, [3, 48, 48, 3, 3, 3, 48, 48, 27, 3, 3, 48, 48, 3, 3]),
    ("staged: a full chunk and a ragged one, 37 = 32 + 5, then 11", 37, {}, 0, 1, [37, 48, 48, 37, 37, 37, 48, 48, 48, 37, 37, 48, 48, 37, 37]),
    ("staged, no sample permutation", 37, dict(sample_sort=0), 0, 1, None),
    ("one lane per pixel over deep batches: slot groups of 8 pixels, permuted samples", 37, dict(slot_group_shift=3), 0, 0, None),
    # room for 5 samples of the 15 tiles: the first step is 4 + 4 + 4 + 4 (one lane per pixel), the steps of the 7 tiles left 8 + 8 (staged)
    ("batches split mid-step", 16, {}, 5 * TILES * 1024, None, [16, 48, 48, 16, 16, 16, 48, 48, 48, 16, 16, 48, 48, 16, 16]),
])
def test_every_tiles_direct_sums_are_the_one_bounce_accumulation_of_its_own_count(duck_pt, name, every, opts, max_paths, runs, counts):
    target = _target(every)
    want = _played(((target, every, 0, 0),))
    # before the GPU is looked at: the restatement alone yields stopped and running tiles for this target
    assert len(set(want["counts"].tolist())) >= 2 and (want["counts"] == every).any() and (want["counts"] == SPP).any(), want["counts"].tolist()
    if counts is not None:
        assert want["counts"].tolist() == counts
    r = _handle(duck_pt, opts=opts, max_paths_in_flight=max_paths)
    r.set_timing(True)
    plan, split = r.launch_plan(1, every), (r.launch_plan(1, 4)["runs"], r.launch_plan(1, 8)["runs"])
    res = r.render_adaptive(target, every)
    D, n = r.read_direct()
    S, _, _, Q, acc = _sums(r)
    got = r.read_tile_samples().reshape(-1)
    stats = r.stats()
    r.close()
    print(name, "counts:", got.tolist(), "batches:", stats["batches_traced"], "accumulate launches:", stats["launches_accumulate"])
    assert got.tolist() == want["counts"].tolist() and n == acc == SPP          # the direct sample count advances with L
    assert res["stopped_tiles"] == want["stopped_tiles"] > 0
    # which kernel form ran: the plan of a batch of `every` samples (the adaptive loop adds its tile list to it), and how many batches the steps took
    assert plan["sample_perm"] == (0 if opts.get("sample_sort") == 0 else 1)
    steps = -(-SPP // every)
    if runs is None:
        assert stats["batches_traced"] == 4 + 2 + 2 and split == (0, 1)
    else:
        assert plan["runs"] == runs and stats["batches_traced"] == steps
    assert np.array_equal(bits(S)[..., :3], bits(want["S"])[..., :3]) and np.array_equal(bits(Q), bits(want["Q"]))
    _check_direct_per_tile(D, got, name)


# ---- 2. non-invasive; the bit shows nowhere before the first adaptive call; a second call continues
def test_direct_with_the_bit_is_non_invasive_under_render_adaptive(duck_pt):
    target = _target(8)

    def run(direct):
        r = _handle(duck_pt, direct=direct)
        r.set_timing(True)
        plans = [r.launch_plan(b, 8) for b in (1, 2, 3)]
        res = r.render_adaptive(target, 8)
        s = r.stats()
        out = dict(sums=[bits(a) for a in _sums(r)[:4]], counts=r.read_tile_samples().tolist(), rays=_rays(r), plans=plans, res=res,
                   launches=s["launches_accumulate"], batches=s["batches_traced"])
        r.close()
        return out

    never, off, on = run(None), run(False), run("tiles")
    assert len(set(np.array(never["counts"]).reshape(-1).tolist())) >= 2
    for other in (off, on):
        assert all(np.array_equal(a, b) for a, b in zip(never["sums"], other["sums"]))
        for k in ("counts", "rays", "plans", "res", "batches"):
            assert never[k] == other[k], k
    assert off["launches"] == never["launches"] and on["launches"] == never["launches"] + on["batches"]


def test_before_the_first_adaptive_call_the_bit_changes_nothing(duck_pt):
    def run(direct):
        r = _handle(duck_pt, direct=direct)
        r.set_timing(True)
        plans = [r.launch_plan(b, n) for b in (1, 2, 3) for n in (3, 11)]
        mem = r.memory_info()
        r.render(5)
        r.render(11)
        s = r.stats()
        out = [bits(a) for a in _sums(r)[:4]] + [bits(r.read_direct()[0])], r.read_direct()[1], plans, mem, r.memory_info(), r.read_tonemapped(), \
            {k: v for k, v in s.items() if k.startswith("launches_") or k.endswith("_rays") or k == "batches_traced"}
        r.close()
        return out

    plain, bit = run(True), run("tiles")
    assert all(np.array_equal(a, b) for a, b in zip(plain[0], bit[0])) and plain[1] == bit[1] == 16
    assert plain[2:5] == bit[2:5] and np.array_equal(plain[5], bit[5]) and plain[6] == bit[6]
    assert np.array_equal(bit[0][4], bits(_one_bounce_handle(16)))


def test_a_second_call_continues_from_the_non_uniform_state(duck_pt):
    S, Q, _ = _oracle(W, H, SPP)
    first = (_target(8), 8, 0, 24)
    lower = (float(np.sort(tile_errors(estimate(S[8], Q[8], 8)))[3]), 8, 0, 0)
    after_first, want = _played((first,)), _played((first, lower))
    assert after_first["counts"].tolist() == [8, 24, 24, 8, 8, 8, 24, 24, 24, 8, 8, 24, 24, 8, 8]
    assert want["counts"].tolist() == [8, 48, 48, 8, 8, 8, 48, 48, 48, 8, 8, 48, 48, 8, 8]
    r = _handle(duck_pt)
    r.render_adaptive(*first)
    D, n = r.read_direct()
    assert n == 24 and r.read_tile_samples().reshape(-1).tolist() == after_first["counts"].tolist()
    _check_direct_per_tile(D, after_first["counts"], "first call")
    r.render_adaptive(*lower)
    D, n = r.read_direct()
    assert n == 48 and r.read_tile_samples().reshape(-1).tolist() == want["counts"].tolist()
    _check_direct_per_tile(D, want["counts"], "second call")
    r.close()


# ---- 3. bookkeeping
def test_the_flag_word_and_its_bookkeeping(duck_pt):
    lib = rf._ffi.lib
    target = _target(8)
    r = _handle(duck_pt, direct=True)
    r.render(4)
    r.denoise_split()
    assert r.read_denoised()[2] == 4
    before = r.read_direct()
    assert before[1] == 4 and before[0].any()
    for word in (0x100, 0x102, 0x200, 0x301, 0x501, 2, 3, -1):                  # the bit alone, unknown bits: refused, the state kept
        assert lib.rf_renderer_set_direct(r._h, word) == INVALID, hex(word)
        after = r.read_direct()
        assert after[1] == 4 and np.array_equal(bits(after[0]), bits(before[0])) and r.read_denoised()[2] == 4
    r.set_direct(True)                                                          # the same value: nothing is cleared
    assert r.read_direct()[1] == 4 and r.read_denoised()[2] == 4
    r.set_direct(True, tile_counts=True)                                        # 1 -> 1 | bit: D is cleared and the snapshot dropped
    assert r.read_direct()[1] == 0 and not r.read_direct()[0].any()
    _refused(r.read_denoised, "no denoised image")
    _refused(lambda: r.render_adaptive(target, 8), "direct", "restart")         # D on partway: it does not cover the 4 accumulated samples
    r.set_render_parameters(rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), 0.5))
    r.render(4)
    r.denoise_split()
    r.set_direct(True)                                                          # 1 | bit -> 1: cleared again
    assert r.read_direct()[1] == 0
    _refused(r.read_denoised, "no denoised image")
    r.set_render_parameters(rf.make_render_parameters(W, H, rf.fly_camera(W, H), SPP, BOUNCES, rf.make_sky(), EXPOSURE))
    _refused(lambda: r.render_adaptive(target, 8), "direct sums are on", "turn them off")   # plain 1: the old refusal
    assert r.tile_samples_uniform() and r.read_accumulation()[1] == 0
    # the non-uniform state: turning D on is refused in either form
    r.set_direct(False)
    r.render_adaptive(target, 8)
    assert not r.tile_samples_uniform()
    _refused(lambda: r.set_direct(True), WHY)
    _refused(lambda: r.set_direct(True, tile_counts=True), WHY)
    assert lib.rf_renderer_set_direct(r._h, 0x100) == INVALID
    r.close()


# ---- 4. the filter on synthetic inputs
def test_denoise_split_tiles_bit_identical_to_the_restatement_on_synthetic_inputs():
    Hs, Ws = 45, 70                                                             # 3 x 2 tiles, ragged both ways
    S, D, AC, ND = _synthetic(Hs, Ws, 6, 4570)
    assert (AC[..., 3] == 0).any() and (AC[..., 3] > 0).any()
    counts = np.array([2, 5, 32, 32, 2, 5], np.uint32)
    one = dict(iterations=5, sigma_color=1.0, sigma_normal=0.1, sigma_depth=0.1)
    cases = [(None, None), (one, one), CUSTOM, (dict(iterations=0), None), (None, dict(iterations=0)), (dict(iterations=0), dict(iterations=0)),
             (dict(CUSTOM[0], iterations=0), dict(CUSTOM[1], iterations=4)), (dict(CUSTOM[0], iterations=4), dict(CUSTOM[1], iterations=0))]
    for pd, pi in cases:
        rgb, bgra = rf.denoise_split_tiles(S, D, AC, ND, counts, exposure=0.25, direct=pd, indirect=pi)
        assert np.array_equal(bits(rgb), bits(denoise_split_tiles(S, D, AC, ND, counts, pd, pi))), (pd, pi)
        same, same_bgra = rf.denoise_split_tiles(S, D, AC, ND, np.full(6, 5, np.uint32), exposure=0.25, direct=pd, indirect=pi)
        uniform, uniform_bgra = rf.denoise_split_images(S, D, AC, ND, 5, exposure=0.25, direct=pd, indirect=pi)
        assert np.array_equal(bits(same), bits(uniform)) and np.array_equal(same_bgra, uniform_bgra), (pd, pi)
        assert not np.array_equal(bits(rgb), bits(uniform))                   # (the counts do show)


# ---- 5. the filter on rendered frames
@pytest.fixture(scope="module")
def frame(duck_pt):
    """One adaptively sampled frame with D and the AOVs kept per tile count, in the non-uniform state; read-only for the tests that share it"""
    target = _target(8)
    want = _played(((target, 8, 0, 0),))
    assert want["counts"].tolist() == [8, 48, 48, 8, 8, 8, 48, 48, 48, 8, 8, 48, 48, 8, 8]
    r = _handle(duck_pt)
    r.render_adaptive(target, 8)
    S, AC, ND, _, n = _sums(r)
    D, nd = r.read_direct()
    counts = r.read_tile_samples()
    assert counts.reshape(-1).tolist() == want["counts"].tolist() and n == nd == SPP
    out = {}
    for name, (pd, pi) in (("default", (None, None)), ("custom", CUSTOM)):
        r.denoise_split(direct=pd, indirect=pi)
        out[name] = r.read_denoised()
    yield dict(r=r, target=target, S=S, D=D, AC=AC, ND=ND, counts=counts, denoised=out)
    r.close()


def test_denoise_split_in_the_non_uniform_state_equals_the_restatement_and_the_tiles_call(frame):
    S, D, AC, ND, counts = (frame[k] for k in ("S", "D", "AC", "ND", "counts"))
    _check_direct_per_tile(D, counts.reshape(-1), "the shared frame")
    for name, (pd, pi) in (("default", (None, None)), ("custom", CUSTOM)):
        rgb, bgra, n = frame["denoised"][name]
        assert n == SPP                                                         # the snapshot's count is the leading count
        assert np.array_equal(bits(rgb), bits(denoise_split_tiles(S, D, AC, ND, counts, pd, pi))), name
        t_rgb, t_bgra = rf.denoise_split_tiles(S, D, AC, ND, counts, exposure=EXPOSURE, direct=pd, indirect=pi)
        assert np.array_equal(bits(rgb), bits(t_rgb)) and np.array_equal(bgra, t_bgra), name
    uniform, _ = rf.denoise_split_images(S, D, AC, ND, SPP, exposure=EXPOSURE)
    assert not np.array_equal(bits(uniform), bits(frame["denoised"]["default"][0]))


def test_denoise_split_is_refused_in_the_non_uniform_state_when_either_bit_is_missing(duck_pt, frame):
    for aovs_bit, direct in ((False, "tiles"), (True, False), (True, None)):
        r = _handle(duck_pt, direct=direct, aovs=aovs_bit)                      # (AOVs with plain RF_AOV_FIRST_HIT would refuse render_adaptive itself: off)
        r.render_adaptive(frame["target"], 8)
        assert not r.tile_samples_uniform()
        _refused(r.denoise_split, WHY)
        _refused(r.read_denoised, "no denoised image")
        r.close()


# ---- 6. across ranks, the local transport
@pytest.mark.parametrize("world", [2, 3])
def test_the_ranks_direct_reads_sum_to_the_whole_frames_and_denoise_on_the_host(duck_pt, monkeypatch, frame, world):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "120")
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _handle(duck_pt)
            r.set_tile_shard(rank, world)
            comm = rf.TileComm(uid, rank, world, 0)
            assert comm.local_transport()
            res = comm.render_adaptive(r, frame["target"], 8)
            assert (res["frame_leading_samples"], res["frame_min_tile_samples"]) == (48, 8)
            out[("D", rank)] = r.read_direct()
            ptr = r.gather_frame(comm, root=0, aovs=True, moments=True, tile_counts=True)
            if rank == 0:
                assert ptr
                out["planes"] = [comm.read_plane(r, k) for k in range(3)]
                out["counts"] = comm.read_tile_samples()
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
    parts = [out[("D", k)][0] for k in range(world)]
    for a in range(world):
        for b in range(a + 1, world):
            assert not (parts[a].any(-1) & parts[b].any(-1)).any()            # disjoint pixels
    D = functools.reduce(np.add, parts)
    assert np.array_equal(bits(D), bits(frame["D"]))
    assert out["counts"].reshape(-1).tolist() == frame["counts"].reshape(-1).tolist()
    S, AC, ND = out["planes"]
    for name, (pd, pi) in (("default", (None, None)), ("custom", CUSTOM)):
        rgb, bgra = rf.denoise_split_tiles(S, D, AC, ND, out["counts"], exposure=EXPOSURE, direct=pd, indirect=pi)
        w_rgb, w_bgra, _ = frame["denoised"][name]
        assert np.array_equal(bits(rgb), bits(w_rgb)) and np.array_equal(bgra, w_bgra), name


# ---- 7. the command-line tool
def test_rf_render_adaptive_with_direct_indirect_and_denoise_split_matches_python(duck_pt, tmp_path, frame):
    scene = tmp_path / "Duck.pt"
    duck_pt.save(scene)
    exe = os.path.join(ROOT, "rayfinder_amd", "bin", "rf-render")
    args = [exe, str(scene), "--width", str(W), "--height", str(H), "--spp", str(SPP), "--bounces", str(BOUNCES), "--out", str(tmp_path / "o.png"),
            "--adaptive", repr(frame["target"]), "--adaptive-every", "8", "--sample-map", str(tmp_path / "n.pfm"),
            "--direct", str(tmp_path / "d.pfm"), "--indirect", str(tmp_path / "i.pfm"), "--denoise-split", str(tmp_path / "s.png")]
    subprocess.check_output(args, timeout=300)
    S, D, counts = frame["S"], frame["D"], frame["counts"]
    nf = np.zeros((H, W, 1), np.float32)
    for t, (rows, cols) in enumerate(tile_slices(W, H)):
        nf[rows, cols] = np.float32(counts.reshape(-1)[t])
    assert len(np.unique(nf)) == 2
    assert np.array_equal(bits(_read_pfm(tmp_path / "d.pfm", W, H)), bits(D[..., :3] / nf))
    assert np.array_equal(bits(_read_pfm(tmp_path / "i.pfm", W, H)), bits((S[..., :3] - D[..., :3]) / nf))
    bgra = frame["denoised"]["default"][1]
    png = _decode_png(open(tmp_path / "s.png", "rb").read(), W, H)
    assert np.array_equal(png[..., :3], np.stack([(bgra >> 16) & 255, (bgra >> 8) & 255, bgra & 255], -1).astype(np.uint8))
    env = dict(os.environ, RF_COMM_TRANSPORT="local", RF_COMM_TIMEOUT_S="120")
    res = subprocess.run(args[:12] + ["--gpus", "2", "--direct", str(tmp_path / "d2.pfm")], env=env, capture_output=True, timeout=300)
    assert res.returncode != 0 and b"--gpus 1" in res.stderr and not os.path.exists(tmp_path / "d2.pfm")
