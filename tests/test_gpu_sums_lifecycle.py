"""The life cycle of a handle's sums on the GPU (-m gpu): every event that restarts an accumulation (a parameter change, a resize, a tile shard, binding or unbinding
an accumulation buffer) leaves the image, the first-hit AOV sums, the radiance second moments, the denoised snapshot and the per-tile sample counts in the state of a
twin handle that never held them -- the reads report nothing, and the next render() gives the twin's sums bit for bit.  A characterisation of the host bookkeeping:
the twin is the reference, nothing here is compared against a tolerance."""
import numpy as np
import pytest
import torch

import rayfinder_amd as rf
import test_gpu_adaptive as adaptive     # the frame, the target and the oracle cache of the tile-adaptive tests (computed once per process)
from conftest import bits

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
W, H, SPP, BOUNCES, EXPOSURE = 64, 48, 12, 2, 0.25      # 2 x 2 tiles; the lower row is half outside the frame (48 = 32 + 16): padded and valid pixels differ
FIRST, SECOND = 3, 4                                    # samples before and after the event


def _params(w, h, spp, bounces, exposure):
    return rf.make_render_parameters(w, h, rf.fly_camera(w, h), spp, bounces, rf.make_sky(), exposure)


def _bind(r, keep):
    _, nbytes = r.accumulation_device_buffer()
    buf = torch.zeros(nbytes // 4 + 1024, dtype=torch.float32, device="cuda")     # room to spare
    keep.append(buf)                                                               # (the handle renders into it: alive as long as the handle)
    r.bind_accumulation_buffer(buf.data_ptr(), buf.numel() * 4)


def _bind_unbind(r, keep):
    _bind(r, keep)
    r.bind_accumulation_buffer(None, 0)


def _shard_and_back(r, keep):
    r.set_tile_shard(0, 2)
    r.set_tile_shard(0, 1)


# name -> (the event, a tile shard is set afterwards)
EVENTS = {
    "exposure": (lambda r, keep: r.set_render_parameters(_params(W, H, SPP, BOUNCES, 0.5)), False),
    "smaller": (lambda r, keep: r.set_render_parameters(_params(40, 24, SPP, BOUNCES, EXPOSURE)), False),
    "shard": (lambda r, keep: r.set_tile_shard(1, 2), True),
    "shard_and_back": (_shard_and_back, False),
    "bind": (_bind, False),
    "bind_unbind": (_bind_unbind, False),
}


def _bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _reads(r, whole_frame):
    """Everything the handle reports about its sums, as bit patterns / integers"""
    img, acc = r.read_accumulation()
    aov = r.read_aovs()
    q, n = r.read_moments()
    out = dict(acc=acc, aov_n=aov["samples"], n=n, S=bits(img), Q=bits(q), mean=bits(r.read_mean()), bgra=r.read_tonemapped(),
               counts=r.read_tile_samples().reshape(-1).astype(np.int64))
    for k in ("albedo", "normal", "depth", "coverage"):
        out["aov_" + k] = bits(aov[k])
    if whole_frame:
        est = r.noise_estimate()
        for k, v in est.items():
            out["est_" + k] = bits(v) if isinstance(v, np.ndarray) else (_bits64(v) if isinstance(v, float) else v)
        r.denoise()
        rgb, bgra, dn = r.read_denoised()
        out.update(den_rgb=bits(rgb), den_bgra=bgra, den_n=dn)
    return out


def _differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("event", list(EVENTS))
def test_an_event_leaves_the_sums_as_a_twin_that_never_held_them(duck_pt, event):
    apply, sharded = EVENTS[event]
    keep = []
    a = rf.ReferencePathTracer(_params(W, H, SPP, BOUNCES, EXPOSURE), duck_pt.scene())
    b = rf.ReferencePathTracer(_params(W, H, SPP, BOUNCES, EXPOSURE), duck_pt.scene())
    try:
        a.set_aovs(True)
        a.set_moments(True)
        a.render(FIRST)
        a.denoise()
        assert a.read_denoised()[2] == FIRST
        apply(a, keep)
        # right after the event: nothing is reported
        img, acc = a.read_accumulation()
        assert acc == 0 and not bits(img).any()
        aov = a.read_aovs()
        assert aov["samples"] == 0 and not any(bits(aov[k]).any() for k in ("albedo", "normal", "depth", "coverage"))
        q, n = a.read_moments()
        assert n == 0 and not bits(q).any()
        with pytest.raises(rf.RayfinderError) as err:
            a.read_denoised()
        assert err.value.status == INVALID
        assert not a.read_tile_samples().any()

        b.render(FIRST)                                   # (advances the frame counter as A's did)
        apply(b, keep)
        assert np.array_equal(a.read_tonemapped(), b.read_tonemapped())
        assert np.array_equal(bits(a.read_mean()), bits(b.read_mean()))
        b.set_aovs(True)
        b.set_moments(True)

        a.render(SECOND)
        b.render(SECOND)
        got, want = _reads(a, not sharded), _reads(b, not sharded)
        assert got["acc"] == got["aov_n"] == got["n"] == SECOND
        assert want["acc"] == want["aov_n"] == want["n"] == SECOND
        assert got["S"].any() and got["Q"].any() and got["aov_coverage"].any()       # (a comparison of real sums)
        assert _differing(got, want) == []
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("event", ["exposure", "bind"])
def test_an_event_ends_the_non_uniform_state(duck_pt, event):
    aw, ah, spp, bounces, every = adaptive.W, adaptive.H, adaptive.SPP, adaptive.BOUNCES, adaptive.EVERY
    apply = {"exposure": lambda r, keep: r.set_render_parameters(_params(aw, ah, spp, bounces, 0.5)), "bind": _bind}[event]
    keep = []
    a = adaptive._renderer(duck_pt)                       # moments only
    b = adaptive._renderer(duck_pt, moments=False)
    try:
        res = a.render_adaptive(adaptive._target(), every, every, 16)
        assert 0 < res["stopped_tiles"] < res["tiles"] and res["max_tile_samples"] == 16
        assert len(set(a.read_tile_samples().reshape(-1).tolist())) > 1
        with pytest.raises(rf.RayfinderError) as err:
            a.render(1)
        assert err.value.status == INVALID
        apply(a, keep)
        assert not a.read_tile_samples().any() and a.read_accumulation()[1] == 0 and a.read_moments()[1] == 0
        a.render(SECOND)

        b.render(16)                                      # (the leading count: advances the frame counter as A's call did)
        apply(b, keep)
        b.set_moments(True)
        b.render(SECOND)
        got, want = {}, {}
        for r, out in ((a, got), (b, want)):
            img, acc = r.read_accumulation()
            q, n = r.read_moments()
            out.update(acc=acc, n=n, S=bits(img), Q=bits(q), mean=bits(r.read_mean()), bgra=r.read_tonemapped(), counts=r.read_tile_samples().reshape(-1).astype(np.int64))
        assert got["acc"] == got["n"] == SECOND and got["counts"].tolist() == [SECOND] * adaptive.TILES
        assert got["S"].any() and got["Q"].any()
        assert _differing(got, want) == []
    finally:
        a.close()
        b.close()
