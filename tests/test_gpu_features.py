"""The feature export on the GPU (-m gpu): rf_renderer_export_features, rf_comm_export_features and rf_export_features_images (kExportFeatures, rf_features.hip).
Every comparison is exact -- bit for bit against tests/features_restatement.py (NaNs compared as NaNs: a payload is no value) -- and every call into caller-owned
device memory is made into the middle of a larger buffer whose ends are checked for overruns afterwards (the canary).
Frames are tiny: the Duck at 64 x 48 (whole tiles, both 16-byte store paths), the shapes at which the store paths and the partial tiles differ, 96 x 80 after
render_adaptive (3 x 3 tiles, a ragged last row), 72 x 40 across ranks."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

import features_restatement as fr
import rayfinder_amd as rf
from conftest import bits

pytestmark = pytest.mark.gpu

INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
ALL = tuple(g for g, _, _ in fr.GROUPS)
SPARSE = (("depth", "samples"), ("normal", "indirect", "error"), ("color", "albedo", "normal", "depth"))
FORMS = tuple((layout, dtype) for layout in ("chw", "hwc") for dtype in ("f32", "f16"))
BOUNCES, EXPOSURE = 3, 0.25
CANARY = 64          # elements in front of and behind every destination
MARK = -1234.5       # exact in f32 and in f16

_PT = {}


@pytest.fixture(autouse=True)
def _scene(duck_pt):
    _PT["duck"] = duck_pt


def _handle(frame, spp_cap=64, aovs=True, moments=True, direct=True, tile_counts=False, bounces=BOUNCES):
    params = rf.make_render_parameters(frame[0], frame[1], rf.fly_camera(*frame), spp_cap, bounces, rf.make_sky(), EXPOSURE)
    r = rf.ReferencePathTracer(params, _PT["duck"].scene())
    if aovs:
        r.set_aovs(True, tile_counts=tile_counts)
    if moments:
        r.set_moments(True)
    if direct:
        r.set_direct(True, tile_counts=tile_counts)
    return r


def _sums(r):
    """The handle's sums through its host reads, as the restatement takes them: dict(S, Q, AC, ND, D) of (H, W, 4) f32 (None: the family is off) and the count"""
    S, n = r.read_accumulation()
    out = dict(S=S, Q=None, AC=None, ND=None, D=None)
    a = r.read_aovs()
    if a["samples"]:
        out["AC"] = np.concatenate([a["albedo"], a["coverage"][..., None]], -1)
        out["ND"] = np.concatenate([a["normal"], a["depth"][..., None]], -1)
    Q, nq = r.read_moments()
    if nq:
        out["Q"] = Q
    D, nd = r.read_direct()
    if nd:
        out["D"] = D
    return out, n


def _shape(frame, count, layout):
    return (count, frame[1], frame[0]) if layout == "chw" else (frame[1], frame[0], count)


def _guarded(call, frame, channels, layout, dtype, offset=0):
    """call(out=...) into the middle of a marked buffer, `offset` elements off the allocation's alignment; -> the result as numpy, once both ends are seen intact"""
    count = rf.feature_channels(channels)[1]
    shape = _shape(frame, count, layout)
    numel = int(np.prod(shape))
    whole = torch.full((CANARY + offset + numel + CANARY,), MARK, dtype=torch.float16 if dtype == "f16" else torch.float32, device="cuda")
    out = whole[CANARY + offset:CANARY + offset + numel].view(shape)
    assert out.storage_offset() == CANARY + offset and out.is_contiguous()
    got = call(channels=channels, layout=layout, dtype=dtype, out=out)
    assert got is out
    host = whole.cpu().numpy()
    assert (host[:CANARY + offset] == MARK).all() and (host[CANARY + offset + numel:] == MARK).all(), "the export wrote outside its destination"
    return host[CANARY + offset:CANARY + offset + numel].reshape(shape).copy()


def _want(channels, frame, sums, samples=0, tile_samples=None, layout="chw", dtype="f32"):
    return fr.features(fr.mask_of(channels), frame[0], frame[1], sums["S"], sums["Q"], sums["AC"], sums["ND"], sums["D"], samples, tile_samples, layout, dtype)


def _images(channels, sums, samples=0, tile_samples=None, layout="chw", dtype="f32"):
    return rf.export_features_images(sums["S"], sums["Q"], sums["AC"], sums["ND"], sums["D"], samples=samples, tile_samples=tile_samples, channels=channels, layout=layout,
                                     dtype=dtype)


def _assert_same(got, want, what):
    assert fr.same(got, want), (what, fr.first_difference(got, want))


def _refused(match, call, *args, **kw):
    with pytest.raises(rf.RayfinderError, match=match) as e:
        call(*args, **kw)
    assert e.value.status == INVALID


# ---------------------------------------------------------------------------------------- 1. the handle: tile-major source
MAIN = (64, 48)
SPP = 16


@functools.lru_cache(maxsize=None)
def _main():
    """The Duck at 64 x 48 after 16 samples with every family on: the handle (kept for the tests that export from it) and its sums.  Computed once; read-only."""
    r = _handle(MAIN)
    r.render(SPP)
    sums, n = _sums(r)
    assert n == SPP and all(v is not None for v in sums.values())
    for v in sums.values():
        v.setflags(write=False)
    return r, sums


def test_the_reference_frame_is_not_vacuous():
    _, sums = _main()
    want = _want(ALL, MAIN, sums, SPP, layout="hwc")
    names = rf.feature_channels(ALL)[0]
    assert want.shape == (48, 64, 22) and len(names) == 22
    for c, name in enumerate(names):
        assert want[..., c].any(), name                       # every channel holds something
    depth, normal = want[..., names.index("depth")], want[..., names.index("normal.x"):names.index("normal.z") + 1]
    assert (depth == 0).any() and (depth > 0).any()           # the frame has background and surface
    assert not normal[depth == 0].any()
    assert not np.array_equal(want[..., 0:3], want[..., names.index("direct.r"):names.index("direct.b") + 1])


@pytest.mark.parametrize("layout,dtype", FORMS)
def test_the_handle_exports_what_the_restatement_gives(layout, dtype):
    r, sums = _main()
    for channels in (ALL,) + SPARSE:
        got = _guarded(r.export_features, MAIN, channels, layout, dtype)
        _assert_same(got, _want(channels, MAIN, sums, SPP, None, layout, dtype), (channels, layout, dtype))
    # the default request and a tensor of the library's own making
    t = r.export_features(layout=layout, dtype=dtype)
    assert t.device.type == "cuda" and t.dtype == (torch.float16 if dtype == "f16" else torch.float32) and tuple(t.shape) == _shape(MAIN, 10, layout)
    _assert_same(t.cpu().numpy(), _want(SPARSE[2], MAIN, sums, SPP, None, layout, dtype), ("default", layout, dtype))


def test_the_sample_count_is_reported():
    r, _ = _main()
    out = torch.empty((1, 48, 64), device="cuda")
    n = C.c_uint32(0)
    req = rf._ffi.FeatureRequest(0x200, 0, 0, 0)
    rf.check(rf._ffi.lib.rf_renderer_export_features(r._h, C.byref(req), C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(n)))
    assert n.value == SPP and (out == float(SPP)).all()


# ---------------------------------------------------------------------------------------- 2. store paths and partial tiles
# (width, height): one pixel; narrower than a vector; one pixel short of / past a tile in either direction; a width that is a multiple of 4 and not of 8 (f32 takes
# the 16-byte path, f16 does not) over ragged tiles; more tiles than rows.  72 x 40 is this file's own: a multiple of 8 with ragged tiles both ways (both 16-byte paths).
SHAPES = ((1, 1), (3, 5), (31, 33), (33, 31), (100, 36), (130, 2), (72, 40))


@pytest.mark.parametrize("frame", SHAPES)
def test_frame_shapes_through_the_handle_and_through_the_images_call(frame):
    r = _handle(frame, bounces=2)
    r.render(4)
    sums, n = _sums(r)
    assert n == 4
    for layout, dtype in FORMS:
        want = _want(ALL, frame, sums, 4, None, layout, dtype)
        rows = _images(ALL, sums, 4, None, layout, dtype)                       # the row-major source
        _assert_same(rows, want, (frame, layout, dtype, "images"))
        for offset in (0, 1):
            tiles = _guarded(r.export_features, frame, ALL, layout, dtype, offset)   # the tile-major source; offset 1: never 16-byte aligned
            assert tiles.shape == rows.shape and fr.same(tiles, rows), (frame, layout, dtype, offset, fr.first_difference(tiles, rows))
    r.close()


# ---------------------------------------------------------------------------------------- 3. the non-uniform state
ADAPTIVE = (96, 80)
CAP, EVERY = 24, 8


@functools.lru_cache(maxsize=None)
def _adaptive():
    """The Duck at 96 x 80 after render_adaptive with every family kept per tile count; the target is the median tile error at the first check, so that about half
    of the nine tiles stop there.  -> the handle, its sums, the counts."""
    probe = _handle(ADAPTIVE, CAP, tile_counts=True)
    probe.render(EVERY)
    est = probe.noise_estimate()
    probe.close()
    pixels = np.array([min(32, ADAPTIVE[0] - 32 * x) * min(32, ADAPTIVE[1] - 32 * y) for y in range(3) for x in range(3)], np.float32)
    target = float(np.float32(np.median((est["tile_sum"].reshape(-1) / pixels).astype(np.float32))))
    r = _handle(ADAPTIVE, CAP, tile_counts=True)
    res = r.render_adaptive(target, EVERY)
    assert res["min_tile_samples"] < res["max_tile_samples"], res             # or this state is the uniform one
    counts = r.read_tile_samples()
    sums, n = _sums(r)
    assert n == res["max_tile_samples"] and not r.tile_samples_uniform()
    for v in list(sums.values()) + [counts]:
        v.setflags(write=False)
    return r, sums, counts, target


@pytest.mark.parametrize("layout,dtype", FORMS)
def test_every_pixel_takes_its_tiles_count(layout, dtype):
    r, sums, counts, _ = _adaptive()
    assert counts.shape == (3, 3) and counts.min() < counts.max() and counts.min() >= 2
    got = _guarded(r.export_features, ADAPTIVE, ALL, layout, dtype)
    _assert_same(got, _want(ALL, ADAPTIVE, sums, 0, counts, layout, dtype), (layout, dtype))
    _assert_same(_images(ALL, sums, 0, counts, layout, dtype), got, (layout, dtype, "images with tile_samples"))
    # SAMPLES is read_tile_samples spread over the pixels
    samples = got[-1] if layout == "chw" else got[..., -1]
    assert np.array_equal(samples.astype(np.float32), np.repeat(np.repeat(counts, 32, 0), 32, 1)[:80, :96].astype(np.float32))
    # with the leading count for every pixel the frame differs: the counts matter
    assert not fr.same(got, _want(ALL, ADAPTIVE, sums, int(counts.max()), None, layout, dtype))


def test_equal_tile_counts_give_the_one_count_result():
    _, sums = _main()
    for layout, dtype in FORMS:
        one = _images(ALL, sums, SPP, None, layout, dtype)
        per_tile = _images(ALL, sums, 0, np.full(4, SPP, np.uint32), layout, dtype)
        assert fr.same(per_tile, one), (layout, dtype)


# ---------------------------------------------------------------------------------------- 4. crafted sums (the row-major path)
CRAFT = (40, 33)            # 2 x 2 tiles, both edges ragged; width a multiple of 8


def _crafted():
    """Five planes of plausible sums with every special value planted in every plane, and the cases the definition names"""
    rng = np.random.default_rng(20240611)
    w, h = CRAFT
    sums = {k: rng.uniform(0.05, 6.0, (h, w, 4)).astype(np.float32) for k in ("S", "Q", "AC", "ND", "D")}
    sums["Q"] += np.float32(8.0)
    specials = np.float32([np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-40, 1.1754942e-38, 3.4028235e38, 0.0, 65504.0, 65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24])
    for p, key in enumerate(("S", "Q", "AC", "ND", "D")):
        for i, v in enumerate(specials):
            for c in range(4):
                # one special value per (plane, component, value), every one at its own pixel, spread over the four tiles
                x, y = (7 * i + 3 * c + p) % w, (5 * i + 11 * c + 2 * p) % h
                sums[key][y, x, c] = v
    AC, ND, S, Q = sums["AC"], sums["ND"], sums["S"], sums["Q"]
    AC[1, 1, 3] = 0.0                                   # background: no coverage
    AC[1, 2, 3], ND[1, 2, 3] = 2.0, 0.0                 # z = 0
    AC[1, 3, 3], ND[1, 3, 3] = 2.0, -3.0                # z < 0
    AC[1, 4, 3], ND[1, 4, 3] = 2.0, np.nan              # z NaN
    AC[1, 5, 3], ND[1, 5, 3] = -2.0, -3.0               # z > 0 from two negative sums: a surface
    AC[2, 1, 3], ND[2, 1] = 2.0, (0.0, 0.0, 0.0, 3.0)   # dot(m, m) = 0
    AC[2, 2, 3], ND[2, 2] = 2.0, (3e19, 3e19, 3e19, 3.0)  # dot(m, m) overflows
    AC[2, 3, 3], ND[2, 3] = 2.0, (2e-22, 0.0, 1e-22, 3.0)  # dot(m, m) subnormal
    AC[2, 4, 3], ND[2, 4] = 2.0, (np.inf, 0.0, 0.0, 3.0)   # dot(m, m) = inf
    S[3, 1, :3], Q[3, 1, :3] = (4.0, 8.0, 2.0), (1.0, 1.0, 0.5)  # Q < S mu: v clamped
    S[3, 2, :3], Q[3, 2, :3] = (-1.0, -1.0, -1.0), (9.0, 9.0, 9.0)  # negative luminance: e < 0 or huge
    S[3, 3, :3], Q[3, 3, :3] = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    S[3, 4, :3], Q[3, 4, :3] = (-0.00390625 * 2, 0.0, 0.0), (1.0, 1.0, 1.0)  # l + eps = 0 with two samples: e = inf -> 0
    return sums


@pytest.mark.parametrize("layout,dtype", FORMS)
def test_crafted_special_values(layout, dtype):
    sums = _crafted()
    for samples, tile_samples in ((2, None), (3, None), (7, None), (2 ** 24 + 1, None), (0, [2, 3, 7, 2 ** 24 + 1]), (0, [2 ** 24 + 1, 7, 3, 2])):
        got = _images(ALL, sums, samples, tile_samples, layout, dtype)
        want = _want(ALL, CRAFT, sums, samples, tile_samples, layout, dtype)
        _assert_same(got, want, (samples, tile_samples, layout, dtype))
    # the same values through the element-wise store path: 37 pixels wide is a multiple of neither vector length
    narrow = {k: np.ascontiguousarray(v[:, :37]) for k, v in sums.items()}
    for samples, tile_samples in ((3, None), (0, [2, 3, 7, 2 ** 24 + 1])):
        got = _images(ALL, narrow, samples, tile_samples, layout, dtype)
        _assert_same(got, _want(ALL, (37, CRAFT[1]), narrow, samples, tile_samples, layout, dtype), ("narrow", samples, tile_samples, layout, dtype))
    hwc = _images(ALL, sums, 2, None, "hwc", "f32")
    names = rf.feature_channels(ALL)[0]
    n0, dz, er, var = names.index("normal.x"), names.index("depth"), names.index("error"), names.index("variance.r")
    for x in (1, 2, 3, 4):
        assert not hwc[1, x, n0:n0 + 3].any() and hwc[1, x, dz] == 0, x          # the four backgrounds
    assert hwc[1, 5, dz] == 1.5 and hwc[1, 5, n0:n0 + 3].any()
    assert not hwc[2, 1, n0:n0 + 3].any() and not hwc[2, 2, n0:n0 + 3].any() and not hwc[2, 4, n0:n0 + 3].any() and hwc[2, 1, dz] == 1.5
    assert np.isfinite(hwc[2, 3, n0:n0 + 3]).all() and hwc[2, 3, n0] > 0.5       # a subnormal dot(m, m) still normalises
    assert not hwc[3, 1, var:var + 3].any() and hwc[3, 1, er] == 0                # the clamped variance
    assert hwc[3, 4, er] == 0 and np.isfinite(hwc[..., er]).all()                 # e = inf, and every other non-finite e: 0
    assert (hwc[..., names.index("samples")] == 2).all()
    big = _images(("samples",), sums, 2 ** 24 + 1, None, "chw", "f32")
    assert (big == np.float32(2 ** 24)).all()                                     # float(2^24 + 1): one round-to-nearest-even conversion


def test_the_f16_conversion_is_one_round_to_nearest_even():
    """COLOR with one sample is S itself: the values at which a half conversion can go wrong, against numpy's float32 -> float16 and against the bits written out"""
    cases = [(65504.0, 0x7BFF), (65519.99, 0x7BFF), (65520.0, 0x7C00), (-65520.0, 0xFC00), (1e9, 0x7C00), (np.inf, 0x7C00), (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000),
             (-2.0 ** -25, 0x8000), (np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 0x0001), (1.5 * 2.0 ** -24, 0x0002), (2.5 * 2.0 ** -24, 0x0002), (2.0 ** -14, 0x0400),
             (2.0 ** -14 - 2.0 ** -25, 0x0400), (2.0 ** -15, 0x0200), (1023.5 * 2.0 ** -24, 0x0400), (1e-45, 0x0000), (-1e-45, 0x8000), (-0.0, 0x8000), (0.0, 0x0000),
             (1.0 + 2.0 ** -11, 0x3C00), (1.0 + 3 * 2.0 ** -11, 0x3C02), (1.0 + 2.0 ** -11 + 2.0 ** -20, 0x3C01), (1.0 - 2.0 ** -12, 0x3C00), (2049.0, 0x6800), (2051.0, 0x6802),
             (2048.0, 0x6800), (2050.0, 0x6801), (2049.001, 0x6801), (0.1, 0x2E66), (-3.14159, 0xC248)]
    w = 40
    S = np.zeros((1, w, 4), np.float32)
    values = np.float32([v for v, _ in cases] + [np.nan])
    S[0, :len(values), 0] = values
    S[0, :len(values), 1] = -values
    for layout in ("chw", "hwc"):
        got = rf.export_features_images(S, samples=1, channels=("color",), layout=layout, dtype="f16")
        red = got[0, 0] if layout == "chw" else got[0, :, 0]
        green = got[1, 0] if layout == "chw" else got[0, :, 1]
        with np.errstate(all="ignore"):
            assert fr.same(red[:len(values)], values.astype(np.float16)) and fr.same(green[:len(values)], (-values).astype(np.float16)), layout
        assert red[:len(cases)].view(np.uint16).tolist() == [b for _, b in cases], layout
        assert np.isnan(red[len(cases)]) and np.isnan(green[len(cases)])
    # the element-wise store path converts alike: 3 pixels wide is never vectorised
    narrow = rf.export_features_images(S[:, 6:9].copy(), samples=1, channels=("color",), dtype="f16")
    assert narrow[0, 0].view(np.uint16).tolist() == [b for _, b in cases[6:9]]


def test_a_tile_without_a_sample():
    """The definition gives +0 in every channel of a pixel whose count is 0, and the kernel implements it; rf_export_features_images, the one way crafted counts reach
    the kernel, refuses a tile count of 0 before any device call (rf_denoise_tiles' rule), so what is checked here is that refusal.  On the root a gathered tile
    without a sample is the case the rule serves."""
    sums = _crafted()
    _refused("every tile", _images, ("color", "samples"), sums, 0, [2, 0, 3, 3])


# ---------------------------------------------------------------------------------------- 5. read-only
def _state(r):
    s = r.stats()
    return r.state_digest(), bits(r.read_accumulation()[0]).copy(), {k: v for k, v in s.items() if k.endswith("_rays") or k == "paths"}


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_the_export_changes_nothing():
    for r, frame in ((_main()[0], MAIN), (_adaptive()[0], ADAPTIVE)):
        before = _state(r)
        for layout, dtype in FORMS:
            _guarded(r.export_features, frame, ALL, layout, dtype)
        assert _same_state(_state(r), before)
    # and the handle goes on as one that never exported: the same sums as a fresh handle's after the same samples
    r = _handle(MAIN)
    r.render(8)
    r.export_features(ALL)
    r.render(8)
    assert np.array_equal(bits(r.read_accumulation()[0]), bits(_main()[1]["S"]))
    r.close()


# ---------------------------------------------------------------------------------------- 6. refusals on a handle
def _raw_export(r, request, ptr, nbytes):
    return rf._ffi.lib.rf_renderer_export_features(r._h, C.byref(rf._ffi.FeatureRequest(*request)), C.c_void_p(ptr), nbytes, None)


def test_refusals_keep_the_state_and_write_nothing():
    r, _ = _main()
    before = _state(r)
    numel = 22 * 48 * 64
    dst = torch.full((numel + 8,), MARK, device="cuda")
    message = lambda: rf._ffi.lib.rf_last_error_message().decode()  # noqa: E731
    # the request
    for request in ((0, 0, 0, 0), (0x400, 0, 0, 0), (1, 2, 0, 0), (1, 0, 2, 0), (1, 0, 0, 1)):
        assert _raw_export(r, request, dst.data_ptr(), numel * 4) == INVALID, request
    # the destination: too small by one byte, host memory (pageable and pinned), NULL
    assert _raw_export(r, (0x3FF, 0, 0, 0), dst.data_ptr(), numel * 4 - 1) == INVALID and "bytes" in message()
    assert _raw_export(r, (0x3FF, 0, 1, 0), dst.data_ptr(), numel * 2 - 1) == INVALID
    host = np.full(numel, MARK, np.float32)
    assert _raw_export(r, (0x3FF, 0, 0, 0), host.ctypes.data, numel * 4) == INVALID and "not device memory" in message()
    pinned = torch.full((numel,), MARK).pin_memory()
    assert _raw_export(r, (0x3FF, 0, 0, 0), pinned.data_ptr(), numel * 4) == INVALID and "not device memory" in message()
    assert (host == MARK).all() and (pinned == MARK).all()
    assert _raw_export(r, (1, 0, 0, 0), 0, numel * 4) == INVALID
    # the Python wrapper's own checks of `out`
    for bad in (torch.empty((22, 48, 64)), torch.empty((22, 48, 64), device="cuda", dtype=torch.float16), torch.empty((22, 48, 65), device="cuda"),
                torch.empty((22, 64, 48), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError):
            r.export_features(ALL, out=bad)
    assert _same_state(_state(r), before)
    # the handle's state: a family that is off
    bare = _handle(MAIN, aovs=False, moments=False, direct=False)
    _refused("no sample", bare.export_features, ("color",))
    bare.render(1)
    for channels, word in ((("albedo",), "AOVs"), (("normal",), "AOVs"), (("depth",), "AOVs"), (("coverage",), "AOVs"), (("direct",), "direct"), (("indirect",), "direct"),
                           (("variance",), "moments"), (("error",), "moments")):
        _refused(word, bare.export_features, channels)
    got = _guarded(bare.export_features, MAIN, ("color", "samples"), "chw", "f32")     # COLOR and SAMPLES need nothing but samples
    assert (got[3] == 1).all() and got[:3].any()
    # a family turned on after the first sample does not cover the accumulation
    bare.set_aovs(True); bare.set_moments(True); bare.set_direct(True)
    bare.render(1)
    state = _state(bare)
    for channels in (("albedo",), ("direct",), ("variance",)):
        _refused("differs from the accumulated", bare.export_features, channels)
    assert _same_state(_state(bare), state)
    bare.close()
    # VARIANCE / ERROR with one sample; a tile shard
    one = _handle(MAIN)
    one.render(1)
    _refused("at least 2", one.export_features, ("variance",))
    _refused("at least 2", one.export_features, ("error",))
    one.export_features(("color", "albedo", "direct"))
    one.set_tile_shard(0, 2)
    one.render(2)
    state = _state(one)
    _refused("rf_comm_export_features", one.export_features, ("color",))
    assert _same_state(_state(one), state)
    one.close()
    # the non-uniform state: a family that was not kept per tile count for the whole accumulation
    a = _handle(ADAPTIVE, CAP, aovs=False, direct=False)
    a.render_adaptive(_adaptive()[3], EVERY)
    assert not a.tile_samples_uniform()
    a.set_aovs(True)
    state = _state(a)
    _refused("AOVs", a.export_features, ("albedo",))
    _refused("direct", a.export_features, ("direct",))
    assert _same_state(_state(a), state)
    a.export_features(("color", "variance", "error", "samples"))
    a.close()
    assert (dst == MARK).all(), "a refused call wrote to its destination"
    assert _same_state(_state(r), before)


# ---------------------------------------------------------------------------------------- 7. the wait is real
def test_the_result_is_ready_for_torchs_stream_at_once():
    r, sums = _main()
    want = torch.from_numpy(_want(ALL, MAIN, sums, SPP)).cuda()
    want_pool, want_sum = torch.nn.functional.avg_pool2d(want[None], 4), want.sum(dim=(1, 2))
    torch.cuda.synchronize()
    for _ in range(3):
        got = r.export_features(ALL)                      # no torch.cuda.synchronize() between the call and the use
        pool, total = torch.nn.functional.avg_pool2d(got[None], 4), got.sum(dim=(1, 2))
        assert torch.equal(pool, want_pool) and torch.equal(total, want_sum)


# ---------------------------------------------------------------------------------------- 8. the root
WORLD = (72, 40)
WSPP = 6


@functools.lru_cache(maxsize=None)
def _whole(adaptive):
    """ONE handle without a tile shard over 72 x 40 -- after 6 samples, or after render_adaptive -- and what its own export gives, per form.  Read-only."""
    if not adaptive:
        r = _handle(WORLD, CAP)
        r.render(WSPP)
        target, counts = None, None
    else:
        probe = _handle(WORLD, CAP, tile_counts=True)
        probe.render(EVERY)
        est = probe.noise_estimate()
        probe.close()
        pixels = np.array([min(32, WORLD[0] - 32 * x) * min(32, WORLD[1] - 32 * y) for y in range(2) for x in range(3)], np.float32)
        target = float(np.float32(np.median((est["tile_sum"].reshape(-1) / pixels).astype(np.float32))))
        r = _handle(WORLD, CAP, tile_counts=True)
        res = r.render_adaptive(target, EVERY)
        assert res["min_tile_samples"] < res["max_tile_samples"]
        counts = r.read_tile_samples()
    out = {(layout, dtype): r.export_features(ALL, layout=layout, dtype=dtype).cpu().numpy() for layout, dtype in FORMS}
    out["sparse"] = r.export_features(SPARSE[0], dtype="f16").cpu().numpy()
    r.close()
    return out, target, counts


def _local_world(world, script, **handle):
    """N tile-sharded handles and N communicators of the local test transport in one process, one host thread per rank (tests/test_gpu_gather_direct.py's form)"""
    uid = rf.comm_unique_id()
    out, errors = {}, []

    def rank_main(rank):
        try:
            r = _handle(WORLD, CAP, **handle)
            r.set_tile_shard(rank, world)
            comm = rf.TileComm(uid, rank, world, 0)
            assert comm.local_transport()
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
    return out


def _check_root(comm, r, want, what):
    for layout, dtype in FORMS:
        got = _guarded(functools.partial(comm.export_features, r), WORLD, ALL, layout, dtype)
        assert fr.same(got, want[(layout, dtype)]), (what, layout, dtype, fr.first_difference(got, want[(layout, dtype)]))
    got = _guarded(functools.partial(comm.export_features, r), WORLD, SPARSE[0], "chw", "f16", 1)
    assert fr.same(got, want["sparse"]), (what, "sparse")


@pytest.mark.parametrize("world", [2, 3])
def test_the_root_exports_what_the_whole_frame_handle_exports(monkeypatch, world):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "60")
    want, _, _ = _whole(False)
    root = world - 1

    def script(rank, r, comm, out):
        r.render(WSPP)
        assert bool(r.gather_frame(comm, root=root, aovs=True, moments=True, direct=True)) == (rank == root)
        if rank != root:
            _refused("was not the root", comm.export_features, r, ("color",))
        else:
            _check_root(comm, r, want, world)
        # a gather without the AOVs and D: their channels are refused on the root, COLOR and VARIANCE are served
        r.gather_frame(comm, root=root, moments=True)
        if rank == root:
            _refused("AOVs", comm.export_features, r, ("albedo",))
            _refused("direct", comm.export_features, r, ("indirect",))
            got = comm.export_features(r, ("color", "variance", "error", "samples"), layout="hwc").cpu().numpy()
            pick = [i for i, n in enumerate(rf.feature_channels(ALL)[0]) if n.split(".")[0] in ("color", "variance", "error", "samples")]
            assert fr.same(got, np.ascontiguousarray(want[("hwc", "f32")][..., pick]))
            r.gather_frame(comm, root=root)
            _refused("moments", comm.export_features, r, ("error",))
            out["root finished"] = rank
        else:
            r.gather_frame(comm, root=root)

    assert _local_world(world, script)["root finished"] == root


def test_the_root_exports_an_adaptively_sampled_frame_per_tile_count(monkeypatch):
    monkeypatch.setenv("RF_COMM_TRANSPORT", "local")
    monkeypatch.setenv("RF_COMM_TIMEOUT_S", "60")
    want, target, counts = _whole(True)
    world, root = 3, 0

    def script(rank, r, comm, out):
        comm.render_adaptive(r, target, EVERY)
        assert bool(r.gather_frame(comm, root=root, aovs=True, moments=True, direct=True, tile_counts=True)) == (rank == root)
        if rank == root:
            assert np.array_equal(comm.read_tile_samples(), counts) and counts.min() < counts.max()
            _check_root(comm, r, want, "adaptive")
            out["root finished"] = rank

    assert _local_world(world, script, tile_counts=True)["root finished"] == root


def test_rccl_world_size_one(monkeypatch):
    """RCCL itself: a world-size-1 communicator, the planes sent to itself (loop-back) and read in place"""
    monkeypatch.delenv("RF_COMM_TRANSPORT", raising=False)
    want, _, _ = _whole(False)
    r = _handle(WORLD, CAP)
    comm = rf.TileComm(rf.comm_unique_id(), 0, 1, 0)
    assert not comm.local_transport()
    r.render(WSPP)
    for loopback in (True, False):
        assert r.gather_frame(comm, root=0, loopback=loopback, aovs=True, moments=True, direct=True)
        _check_root(comm, r, want, ("rccl", loopback))
    n = C.c_uint32(0)
    out = torch.empty((1, 40, 72), device="cuda")
    rf.check(rf._ffi.lib.rf_comm_export_features(comm._h, r._h, C.byref(rf._ffi.FeatureRequest(0x200, 0, 0, 0)), C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(n)))
    assert n.value == WSPP
    comm.close()
    r.close()
