"""The handle's bookkeeping model-checked on the GPU (-m gpu): one ReferencePathTracer and one HandleModel (tests/handle_model.py: include/rayfinder_amd.h composed
from the restatements over the CPU oracle) walk through the same seeded random call sequences (tests/handle_walk.py), and after EVERY call
  1. the outcome is the same: OK, or RF_ERROR_INVALID_ARGUMENT with the words the header promises in the message, and the same returned value;
  2. observe() of the handle -- every sum with its count, the per-tile counts, the mean, the texels, both snapshots, primary_rays -- equals the model's, floats as bit
     patterns, texels and counts as integers;
  3. after a refused call the handle's observe() is its own previous one (so that a mistake of the model cannot hide a state change).
Every seed also draws a scheduling (batch depth, slot order, accumulate kernel, sample permutation) that must be invisible.  Nothing is compared against a tolerance.
A failing walk prints its seed, the index of the first call that differs, the observables that differ and the calls so far as Python lines that replay them."""
import numpy as np
import pytest

import handle_walk as hw
import rayfinder_amd as rf
from conftest import DUCK
from handle_model import bits, differing, estimate_scalars

pytestmark = pytest.mark.gpu
INVALID = rf._ffi.RF_ERROR_INVALID_ARGUMENT
_PT = []


def _params(exposure):
    _, camera, _ = hw.frame()
    return rf.make_render_parameters(hw.W, hw.H, rf.camera_from_array(camera), hw.SPP, hw.BOUNCES, rf.make_sky(), exposure)


def new_handle(scheduling):
    if not _PT:
        _PT.append(rf.PtFormat.from_gltf(DUCK))
    r = rf.ReferencePathTracer(_params(hw.EXPOSURE), _PT[0].scene(), max_paths_in_flight=scheduling["max_paths_in_flight"])
    for k, v in scheduling["options"].items():
        r.set_option(k, v)
    return r


def _bind(r, keep):
    import torch
    _, nbytes = r.accumulation_device_buffer()
    buf = torch.zeros(hw.TILES * 1024 * 4 + 1024, dtype=torch.float32, device="cuda")   # room for the whole frame, whatever the shard: the handle renders into it
    assert buf.numel() * 4 >= nbytes
    keep.append(buf)
    r.bind_accumulation_buffer(buf.data_ptr(), buf.numel() * 4)


def apply_gpu(r, call, keep):
    """One call of a walk on the handle -> ("ok", value) | ("refused", the message); any status but RF_ERROR_INVALID_ARGUMENT raises"""
    name, args = call[0], call[1:]
    try:
        value = None
        if name == "render_until":
            frames, last = r.render_until(*args)
            value = dict(frames=frames, last=estimate_scalars(last))
        elif name == "render_adaptive":
            res = r.render_adaptive(*args)
            value = {k: int(v) for k, v in res.items() if k != "last"}
            value["last"] = estimate_scalars(res["last"])
        elif name == "noise_estimate":
            e = r.noise_estimate()
            value = estimate_scalars(e)
            value.update(error_map=bits(e["error_map"]), tile_sum=bits(e["tile_sum"]), tile_max=bits(e["tile_max"]))
        elif name == "set_aovs":
            rf.check(rf.lib.rf_renderer_set_aovs(r._h, args[0]))
        elif name == "set_buckets":
            rf.check(rf.lib.rf_renderer_set_buckets(r._h, args[0]))
        elif name == "set_exposure":
            r.set_render_parameters(_params(args[0]))
        elif name == "bind":
            _bind(r, keep)
        elif name == "unbind":
            r.bind_accumulation_buffer(None, 0)
        elif name in ("denoise", "denoise_robust"):
            getattr(r, name)(iterations=args[0])
        else:
            getattr(r, name)(*args)
        return ("ok", value)
    except rf.RayfinderError as e:
        if e.status != INVALID:
            raise
        return ("refused", str(e))


def observe_gpu(r):
    """handle_model.HandleModel.observe() of the handle (and S_a, the accumulation's fourth channel, which the header leaves open: compared with the handle's own only)"""
    s, acc = r.read_accumulation()
    q, qn = r.read_moments()
    a = r.read_aovs()
    b, bn = r.read_buckets()
    counts = r.read_tile_samples().reshape(-1).astype(np.int64)
    out = dict(acc=acc, S=bits(s[..., :3]), S_a=bits(s[..., 3]), Q=bits(q), q_n=qn, AC=bits(np.concatenate([a["albedo"], a["coverage"][..., None]], -1)),
               ND=bits(np.concatenate([a["normal"], a["depth"][..., None]], -1)), aov_n=a["samples"], B=bits(b), K=b.shape[0], b_n=bn, counts=counts,
               uniform=bool(r.tile_samples_uniform()), mean=bits(r.read_mean()), bgra=r.read_tonemapped(), primary_rays=int(r.stats()["primary_rays"]))
    try:
        rgb, bgra, n = r.read_denoised()
        out.update(has_denoised=True, den_rgb=bits(rgb), den_bgra=bgra, den_n=n)
    except rf.RayfinderError as e:
        assert e.status == INVALID
        out["has_denoised"] = False
    try:
        m = r.read_robust_mean()
        out.update(has_robust=True, rob_mean=bits(m["mean"]), rob_trim=m["trim"], rob_bgra=m["bgra8"], rob_n=m["samples"])
    except rf.RayfinderError as e:
        assert e.status == INVALID
        out["has_robust"] = False
    return out


def against_model(now, model):
    """The observables in which a reading of the handle (observe_gpu) differs from the model's"""
    return differing({k: v for k, v in now.items() if k != "S_a"}, model.observe())


def _same_value(a, b):
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same_value(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


def run_walk(calls, scheduling, seed=None):
    """Both sides through `calls`; the first disagreement fails with the replay"""
    model, r, keep = hw.new_model(), new_handle(scheduling), []
    try:
        before = observe_gpu(r)
        assert against_model(before, model) == [], "a fresh handle"
        for i, call in enumerate(calls):
            want, got = hw.apply(model, call), apply_gpu(r, call, keep)
            now = observe_gpu(r)
            problems = []
            if got[0] != want[0]:
                problems.append(f"outcome: the handle {got}, the model {want}")
            elif got[0] == "refused":
                problems += [f"the message lacks {w!r}: {got[1]}" for w in (want[1] or ()) if w not in got[1]]
                problems += [f"a refused call changed {k}" for k in differing(now, before)]
            elif not _same_value(got[1], want[1]):
                problems.append(f"returned value: the handle {got[1]}, the model {want[1]}")
            problems += [f"observable {k} differs" for k in against_model(now, model)]
            if problems:
                pytest.fail(f"seed {seed}, call {i} {call}: " + "; ".join(problems) + "\n" + hw.replay_lines(seed, calls[:i + 1], scheduling), pytrace=False)
            before = now
    finally:
        r.close()


@pytest.mark.parametrize("seed", hw.SEEDS)
def test_the_handle_follows_the_model_through_a_seeded_walk(seed):
    calls, scheduling = hw.walk(seed)
    run_walk(calls, scheduling, seed)
