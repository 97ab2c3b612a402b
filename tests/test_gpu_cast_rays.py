"""rf_renderer_cast_rays on the GPU (-m gpu): rays from torch tensors through the production traversal, hits and surface attributes into torch tensors (kCastLoad,
kTraceWide, kCastResolve; rf_ray_query.hip).  Every comparison is exact -- bit for bit against the oracle's host queries (orc.intersect_bvh_batch, orc.shadow_batch),
tests/cast_rays_restatement.py and the handle's own first-hit AOVs, NaNs compared as NaNs -- and every output is written into the middle of a marked, larger tensor
whose ends are checked afterwards (the canary of tests/test_gpu_features.py).  The scene is the Duck; the rays are tests/cast_rays_inputs.py's (about 12 700)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cast_rays_inputs as ci
import cast_rays_restatement as cr
import rayfinder_amd as rf
from conftest import oracle_scene_from_pt
from oracle import orc

pytestmark = pytest.mark.gpu

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
T_MAX = np.float32(10000.0)
CANARY = 64           # elements in front of and behind every output
MARK_F, MARK_I = -1234.5, -77
CLOSEST = tuple(o[0] for o in rf._ffi.RAY_OUTPUTS if o[1] == 0)
WIDTH = {o[0]: o[2] for o in rf._ffi.RAY_OUTPUTS}
IS_WORD = {o[0]: o[3] == "u" for o in rf._ffi.RAY_OUTPUTS}

_PT = {}


@pytest.fixture(autouse=True)
def _scene(duck_pt):
    _PT["duck"] = duck_pt


def _handle(frame=(64, 48), spp=1, bounces=1, scene=None):
    params = rf.make_render_parameters(frame[0], frame[1], rf.fly_camera(*frame), spp, bounces, rf.make_sky(), 0.25)
    return rf.ReferencePathTracer(params, scene if scene is not None else _PT["duck"].scene())


@functools.lru_cache(maxsize=None)
def _reference():
    """Computed once, read-only: the oracle's scene, the rays, the oracle's answers to them and the restated attributes at its hits; and one handle for the tests that
    only cast."""
    sc, a = oracle_scene_from_pt(_PT["duck"])
    nodes, pos, att = a["bvhNodes"], a["trianglePositionAttributes"], a["triangleVertexAttributes"]
    corners = pos.reshape(-1, 3, 4)[:, :, :3].reshape(-1, 3)
    rays, kinds = ci.generate(corners.min(0), corners.max(0), lambda r: orc.intersect_bvh_batch(nodes, pos, r, T_MAX))
    want = _oracle_closest(nodes, pos, att, sc, rays)
    for v in (rays, kinds, *want.values()):
        v.setflags(write=False)
    return dict(sc=sc, nodes=nodes, pos=pos, att=att, rays=rays, kinds=kinds, want=want, handle=_handle())


def _oracle_closest(nodes, pos, att, sc, rays, t_max=T_MAX, albedo=True):
    o = orc.intersect_bvh_batch(nodes, pos, rays, t_max)
    hit = o["hit"] != 0
    want = dict(triangle=np.where(hit, o["tri"], 0xFFFFFFFF).astype(np.uint32), t=np.where(hit, o["t"], 0).astype(np.float32),
                bary=np.where(hit[:, None], o["uv"], 0).astype(np.float32), position=np.where(hit[:, None], o["p"], 0).astype(np.float32))
    want.update(cr.attributes(pos, att, want["triangle"], want["bary"][:, 0], want["bary"][:, 1], (lambda i, u, v: orc.texture_lookup(sc, i, u, v)) if albedo else None))
    return want


def _rays_on_device(rays):
    t = torch.from_numpy(np.array(rays, np.float32)).cuda()       # (a copy: the reference's arrays are read-only)
    return t[:, :3], t[:, 3:]          # the two halves of an (N, 6) tensor: row stride 6


def _marked(name, n, offset=0):
    """-> (the whole marked buffer, the output tensor in its middle, `offset` elements off the allocation's start)"""
    word = IS_WORD[name]
    numel = n * WIDTH[name]
    whole = torch.full((CANARY + offset + numel + CANARY,), MARK_I if word else MARK_F, dtype=torch.int32 if word else torch.float32, device="cuda")
    out = whole[CANARY + offset:CANARY + offset + numel]
    out = out if WIDTH[name] == 1 else out.view(n, WIDTH[name])
    assert out.storage_offset() == CANARY + offset and out.is_contiguous()
    return whole, out


def _unmarked(name, whole, n, offset=0):
    host = whole.cpu().numpy()
    mark, lo, hi = (MARK_I if IS_WORD[name] else MARK_F), CANARY + offset, CANARY + offset + n * WIDTH[name]
    assert (host[:lo] == mark).all() and (host[hi:] == mark).all(), f"{name}: the call wrote outside its output"
    got = host[lo:hi].copy()
    got = got.view(np.uint32) if IS_WORD[name] else got
    return got if WIDTH[name] == 1 else got.reshape(n, WIDTH[name])


def _cast(r, rays, names, t_max=T_MAX, offset=0, inputs=None):
    """cast_rays into marked buffers -> dict of numpy arrays, once every buffer's ends are seen intact"""
    o, d = inputs if inputs is not None else _rays_on_device(rays)
    n = int(o.shape[0])
    buffers = {name: _marked(name, n, offset) for name in names}
    got = r.cast_rays(o, d, t_max=float(t_max), outputs=names, out={name: b[1] for name, b in buffers.items()})
    assert set(got) == set(names) and all(got[name] is buffers[name][1] for name in names)
    return {name: _unmarked(name, buffers[name][0], n, offset) for name in names}


def _occlusion(r, rays, t_max, offset=0, inputs=None):
    o, d = inputs if inputs is not None else _rays_on_device(rays)
    n = int(o.shape[0])
    whole, out = _marked("visibility", n, offset)
    assert r.cast_occlusion(o, d, t_max=float(t_max), out=out) is out
    return _unmarked("visibility", whole, n, offset)


def _assert_same(got, want, what):
    assert cr.same(got, want), (what, cr.first_difference(got, want))


# ---------------------------------------------------------------------------------------- values
def test_the_rays_are_not_vacuous():
    ref = _reference()
    rays, kinds, want = ref["rays"], ref["kinds"], ref["want"]
    assert 11000 <= rays.shape[0] <= 14000 and set(np.unique(kinds)) == set(range(len(ci.KINDS)))
    hit = want["triangle"] != 0xFFFFFFFF
    assert 0.3 < hit.mean() < 0.9 and hit[kinds == 4].any() and not hit[kinds == 4].all()
    assert np.isnan(rays).any() and (rays[:, 3:] == 0).any() and np.abs(rays[:, :3]).max() >= 1e20
    for name in ("geometric_normal", "normal", "texcoord", "albedo"):
        assert want[name][hit].any(), name
    assert len(np.unique(want["albedo"][hit], axis=0)) >= 10           # more than a handful of texels: a constant albedo would not pass


def test_closest_hit_is_the_host_query_bit_for_bit():
    ref = _reference()
    # the Duck's rays take kTraceWide: what the policy picks for the closest-hit and the any-hit launch of bounce 2 (the launch a query is planned as) is a wide layout
    # (the mirror of test_unusable_wide_records_take_the_scalar_traversal, where both are "scalar")
    info = ref["handle"].layout_info(2)
    assert info["closest"][1] not in ("scalar", "packet") and info["shadow"][1] not in ("scalar", "packet"), info
    got = _cast(ref["handle"], ref["rays"], ("triangle", "t", "bary", "position"))
    for name in got:
        _assert_same(got[name], ref["want"][name], name)


@pytest.mark.parametrize("t_max", [10000.0, 1.0])
def test_any_hit_is_shadow_ray_bit_for_bit(t_max):
    ref = _reference()
    want = orc.shadow_batch(ref["nodes"], ref["pos"], ref["rays"], np.float32(t_max))
    if t_max == 1.0:
        full = orc.shadow_batch(ref["nodes"], ref["pos"], ref["rays"], T_MAX)
        assert (want != full).sum() > 100          # this t_max cuts hits off
    assert 0.1 < want.mean() < 0.9
    _assert_same(_occlusion(ref["handle"], ref["rays"], t_max), want, f"visibility at t_max {t_max}")


def test_attributes_are_the_restatement_alone_and_together():
    ref = _reference()
    r, rays, want = ref["handle"], ref["rays"], ref["want"]
    together = _cast(r, rays, CLOSEST)
    for name in CLOSEST:
        _assert_same(together[name], want[name], ("all together", name))
    for name in CLOSEST:
        _assert_same(_cast(r, rays, (name,))[name], want[name], ("alone", name))
    # the default request and tensors of the library's own making
    o, d = _rays_on_device(rays)
    made = r.cast_rays(o, d)
    assert tuple(made) == ("triangle", "t", "position", "normal", "albedo")
    for name, t in made.items():
        assert t.device.type == "cuda" and t.dtype == (torch.int32 if IS_WORD[name] else torch.float32)
        got = t.cpu().numpy()
        _assert_same(got.view(np.uint32) if IS_WORD[name] else got, want[name], ("default", name))
    assert r.cast_rays(o[:0], d[:0])["t"].shape == (0,) and r.cast_occlusion(o[:0], d[:0]).shape == (0,)


def test_primary_rays_give_the_first_hit_aovs():
    """Frame 0 of a 64 x 48, 1-sample, 1-bounce render: albedo, normal, t and the hit mask of its primary rays are the handle's AOV sums after that one sample.
    The AOVs are SUMS: after one sample each holds +0 + value, which is the value bit for bit except that a -0 component becomes +0 -- so the call's values go through
    the same one addition before they are compared."""
    W, H = 64, 48
    r = _handle((W, H), spp=1, bounces=1)
    r.set_aovs(True)
    r.render(1)
    aov = r.read_aovs()
    assert aov["samples"] == 1
    rp = orc.make_render_params(W, H, rf.camera_to_array(rf.fly_camera(W, H)), 1, 1, 0.25, rf.aligned_sky_state(rf.make_sky()))
    rays = np.array([orc.wgsl_camera_ray(rp, x, y, 0) for y in range(H) for x in range(W)], np.float32)
    got = _cast(r, rays, ("triangle", "t", "normal", "albedo"))
    hit = (got["triangle"] != 0xFFFFFFFF).reshape(H, W)
    assert hit.any() and not hit.all()
    _assert_same(hit.astype(np.float32), aov["coverage"], "hit mask")
    zero = np.float32(0.0)
    _assert_same(zero + got["t"].reshape(H, W), aov["depth"], "t")
    _assert_same(zero + got["normal"].reshape(H, W, 3), aov["normal"], "normal")
    _assert_same(zero + got["albedo"].reshape(H, W, 3), aov["albedo"], "albedo")
    r.close()


# ---------------------------------------------------------------------------------------- sizes, chunks, layouts
def _subset(n):
    """n rays across the kinds"""
    rays = _reference()["rays"]
    idx = (np.arange(n, dtype=np.int64) * 7919) % rays.shape[0]
    return idx


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_small_sizes(n):
    ref = _reference()
    idx = _subset(n)
    got = _cast(ref["handle"], ref["rays"][idx], CLOSEST)
    for name in CLOSEST:
        _assert_same(got[name], ref["want"][name][idx], (n, name))
    _assert_same(_occlusion(ref["handle"], ref["rays"][idx], T_MAX), orc.shadow_batch(ref["nodes"], ref["pos"], ref["rays"][idx], T_MAX), (n, "visibility"))


@pytest.mark.parametrize("chunk", [1000, 4096])
def test_chunked_calls_match_the_single_chunk(chunk):
    ref = _reference()
    r = _handle()
    single = {name: ref["want"][name] for name in CLOSEST}
    shadow = orc.shadow_batch(ref["nodes"], ref["pos"], ref["rays"], T_MAX)
    r.set_option("cast_chunk", chunk)
    for n in (chunk - 1, chunk, chunk + 1, 3 * chunk + 77):
        assert n <= ref["rays"].shape[0]
        got = _cast(r, ref["rays"][:n], CLOSEST)
        for name in CLOSEST:
            _assert_same(got[name], single[name][:n], (chunk, n, name))
        _assert_same(_occlusion(r, ref["rays"][:n], T_MAX), shadow[:n], (chunk, n, "visibility"))
    # ... and the unchunked call on the same handle
    r.set_option("cast_chunk", 0)
    got = _cast(r, ref["rays"], ("triangle", "albedo"))
    _assert_same(got["triangle"], single["triangle"], "unchunked")
    _assert_same(got["albedo"], single["albedo"], "unchunked")
    r.close()


def test_strides_and_storage_offsets():
    ref = _reference()
    r, n = ref["handle"], 1500
    rays = ref["rays"][:n]
    names = ("triangle", "t", "bary", "normal", "albedo", "texture")
    # stride 8 with padding that holds NaNs, origins and directions in tensors of their own
    pad_o = torch.full((n, 8), float("nan"), device="cuda")
    pad_d = torch.full((n, 8), float("nan"), device="cuda")
    pad_o[:, :3], pad_d[:, :3] = torch.from_numpy(rays[:, :3].copy()).cuda(), torch.from_numpy(rays[:, 3:].copy()).cuda()
    # every tensor one element off its allocation: inputs in a flat buffer from element 1 on, outputs at offset 1 behind the canary
    flat = torch.zeros(1 + n * 6, device="cuda")
    flat[1:] = torch.from_numpy(rays.reshape(-1).copy()).cuda()
    shifted = flat[1:].view(n, 6)
    assert shifted.storage_offset() == 1
    for what, inputs, offset in (("stride 8", (pad_o[:, :3], pad_d[:, :3]), 0), ("offset 1", (shifted[:, :3], shifted[:, 3:]), 1), ("contiguous", (shifted[:, :3].contiguous(), shifted[:, 3:].contiguous()), 3)):
        got = _cast(r, None, names, inputs=inputs, offset=offset)
        for name in names:
            _assert_same(got[name], ref["want"][name][:n], (what, name))
        _assert_same(_occlusion(r, None, 1.0, inputs=inputs, offset=offset), orc.shadow_batch(ref["nodes"], ref["pos"], rays, np.float32(1.0)), (what, "visibility"))


# ---------------------------------------------------------------------------------------- read-only
def _state(r):
    s = r.stats()
    b = r.bounce_stats()
    return r.state_digest(), {k: v for k, v in s.items() if not k.startswith("ms_")}, {k: v.tolist() for k, v in b.items() if not k.startswith("ms_")}


@pytest.mark.parametrize("shard", [None, (1, 3)])
def test_a_query_leaves_the_handle_as_it_was(shard):
    """No field of rf_stats or rf_renderer_get_bounce_stats is excepted: the query's rays count into a counter block of their own (the ms_* fields are times, not
    counts: they are 0 here, timing is off)"""
    ref = _reference()
    frame = (96, 80)
    r, twin = _handle(frame, spp=16, bounces=3), _handle(frame, spp=16, bounces=3)
    for h in (r, twin):
        h.set_aovs(True)
        if shard:
            h.set_tile_shard(*shard)
    r.render(3)
    before = _state(r)
    got = _cast(r, ref["rays"], ("triangle", "albedo"))
    _assert_same(got["triangle"], ref["want"]["triangle"], "triangle")
    _assert_same(_occlusion(r, ref["rays"], T_MAX), orc.shadow_batch(ref["nodes"], ref["pos"], ref["rays"], T_MAX), "visibility")
    assert _state(r) == before
    assert all(v == 0 for k, v in r.stats().items() if k.startswith("ms_"))
    r.render(3)
    twin.render(6)
    a, b = r.read_accumulation(), twin.read_accumulation()
    assert a[1] == b[1] == 6 and cr.same(a[0], b[0]) and a[0].any()
    assert r.state_digest() == twin.state_digest()
    sa, sb = r.read_aovs(), twin.read_aovs()
    assert all(cr.same(sa[k], sb[k]) for k in ("albedo", "normal", "depth", "coverage"))
    r.close(), twin.close()


# ---------------------------------------------------------------------------------------- a scene the wide records cannot serve
def test_unusable_wide_records_take_the_scalar_traversal():
    """Duck's arrays with one leaf's min.x and max.x exchanged, given as raw arrays: the wide records are refused, the call runs the reference-order traversal and
    gives the oracle's values over the same nodes"""
    ref = _reference()
    a = _PT["duck"].arrays()
    nodes = a["bvhNodes"].copy()
    leaves = np.flatnonzero(nodes["triangleCount"] > 0)
    leaf = leaves[len(leaves) // 2]
    lo, hi = nodes[leaf]["min"][0], nodes[leaf]["max"][0]
    assert lo < hi
    nodes[leaf]["min"][0], nodes[leaf]["max"][0] = hi, lo
    scene = rf.scene_from_arrays(nodes, ref["pos"], ref["att"], a["baseColorTextures"])
    r = _handle(scene=scene)
    assert r.layout_info(2)["closest"][0] == "scalar"
    rays = ref["rays"]
    want = _oracle_closest(nodes, ref["pos"], ref["att"], ref["sc"], rays)
    assert not np.array_equal(want["triangle"], ref["want"]["triangle"])       # the inverted box hides its leaf from some rays
    r.set_option("cast_chunk", 5000)
    got = _cast(r, rays, CLOSEST)
    for name in CLOSEST:
        _assert_same(got[name], want[name], name)
    _assert_same(_occlusion(r, rays, 1.0), orc.shadow_batch(nodes, ref["pos"], rays, np.float32(1.0)), "visibility")
    r.close()


# ---------------------------------------------------------------------------------------- refusals
def _raw(r, n=256, kind=0, stride=(3, 3), t_max=1.0, reserved=(0, 0), **pointers):
    batch = rf._ffi.RayBatch()
    batch.origin_stride, batch.direction_stride, batch.num_rays, batch.t_max, batch.kind = stride[0], stride[1], n, t_max, kind
    batch.reserved[0], batch.reserved[1] = reserved
    for name, p in pointers.items():
        setattr(batch, name, p)
    return rf._ffi.lib.rf_renderer_cast_rays(r._h, C.byref(batch))


def test_refusals_keep_the_state():
    r = _handle()
    r.render(1)
    digest = r.state_digest()
    n = 256
    message = lambda: rf._ffi.lib.rf_last_error_message().decode()    # noqa: E731
    dev = {name: torch.full((n * 3,), MARK_F, device="cuda") for name in ("origins", "directions", "t", "position", "albedo", "visibility")}
    dev["triangle"] = torch.full((n,), MARK_I, dtype=torch.int32, device="cuda")
    ptr = {name: t.data_ptr() for name, t in dev.items()}
    host = np.zeros(n * 3, np.float32)
    pinned = torch.zeros(n * 3).pin_memory()
    good = dict(origins=ptr["origins"], directions=ptr["directions"], triangle=ptr["triangle"], position=ptr["position"])
    assert _raw(r, **good) == 0                                          # the call these are variations of
    dev["triangle"].fill_(MARK_I), dev["position"].fill_(MARK_F)

    def refused(word, **kw):
        args = dict(good)
        args.update(kw)
        assert _raw(r, **args) == INVALID and word in message(), (kw, message())
        assert r.state_digest() == digest
        assert (dev["triangle"] == MARK_I).all() and (dev["position"] == MARK_F).all(), "a refused call wrote to an output"

    # a host pointer, then pinned host memory, for each buffer in turn
    for name in ("origins", "directions") + CLOSEST:
        refused("not device memory", **{name: host.ctypes.data})
        refused("not device memory", **{name: pinned.data_ptr()})
    assert _raw(r, kind=1, origins=ptr["origins"], directions=ptr["directions"], visibility=host.ctypes.data) == INVALID and "not device memory" in message()
    # (a range that leaves its allocation is refused where the runtime can tell the allocation; torch's caching allocator hands out parts of larger ones, so no
    # tensor here can show it)
    # overlaps: two outputs, an output and the origins, an output and the directions
    refused("overlaps", t=ptr["triangle"])
    refused("overlaps", t=ptr["position"] + 4 * (3 * n - 1))
    refused("overlaps origins", position=ptr["origins"])
    refused("overlaps directions", triangle=ptr["directions"] + 4 * (3 * n - 1))
    # wrong kind / output pairs
    refused("visibility", visibility=ptr["visibility"])
    refused("RF_RAYS_ANY", kind=1, visibility=ptr["visibility"])                       # (the closest-hit outputs of `good` are still given)
    refused("RF_RAYS_ANY", kind=1, triangle=None, visibility=ptr["visibility"])
    # the rest of the header's list
    refused("origins", origins=None)
    refused("origins and directions", directions=None)
    refused("stride", stride=(2, 3))
    refused("stride", stride=(3, 0))
    refused("kind", kind=2, triangle=None, position=None, visibility=ptr["visibility"])
    refused("reserved", reserved=(0, 1))
    refused("no output", triangle=None, position=None)
    refused("NaN", t_max=float("nan"))
    # num_rays == 0 returns 0 and touches nothing; so does a valid any-hit call
    assert _raw(r, n=0) == 0 and _raw(r, n=0, **good) == 0
    assert _raw(r, kind=1, origins=ptr["origins"], directions=ptr["directions"], visibility=ptr["visibility"]) == 0
    assert r.state_digest() == digest
    with pytest.raises(rf.RayfinderError) as e:                                        # through the wrapper: an output that is the origins' own memory
        o = dev["origins"].view(n, 3)
        r.cast_rays(o, dev["directions"].view(n, 3), outputs=("position",), out={"position": o})
    assert e.value.status == INVALID and r.state_digest() == digest
    r.close()
