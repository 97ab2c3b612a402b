"""Seeded random call sequences for one renderer handle, drawn from the state of tests/handle_model.py's model so that they go somewhere: walk(seed, length) is the
call list of one walk plus a scheduling (batch depth, slot order, accumulate kernel, sample permutation) that must be invisible.  apply() plays one call on a model;
tests/test_gpu_handle_walk.py has the twin that plays it on a GPU handle.  tests/test_handle_model.py holds the walk set to the coverage conditions it must meet,
computed from the model alone."""
import functools

import numpy as np

from adaptive_restatement import tile_errors
from conftest import DUCK, oracle_scene_from_pt
from handle_model import AOV_FIRST_HIT, AOV_TILE_COUNTS, BUCKETS_TILE_COUNTS, HandleModel
from noise_restatement import estimate

W, H, SPP, BOUNCES, EXPOSURE = 72, 40, 24, 2, 0.25          # 3 x 2 tiles, both edges ragged (72 = 2 x 32 + 8, 40 = 32 + 8)
TILES = 6
SEEDS = tuple(range(16))
LENGTH = 20
SEED_BASE = 1000
HUGE = 1.0e9
BIT = BUCKETS_TILE_COUNTS
STEPS = (1, 2, 3, 5, 8, 30)
SHARDS = ((0, 1), (0, 2), (1, 2))
BUCKET_ARGS = (0, 3, 5, 3 | BIT, 5 | BIT, 4, 17, 0x100, 9 | 0x200)       # the last four are invalid
AOV_ARGS = (0, AOV_FIRST_HIT, AOV_FIRST_HIT | AOV_TILE_COUNTS, AOV_TILE_COUNTS)   # the last is invalid
EXPOSURES = (0.25, 0.5, 1.0)
MAX_PATHS = (0, 4 * TILES * 1024, 24 * TILES * 1024)
STATE_CHANGING = ("render", "render_until", "render_adaptive", "set_moments", "set_aovs", "set_buckets", "set_exposure", "set_tile_shard", "bind", "unbind")
QUERIES = ("noise_estimate", "denoise", "robust_mean", "denoise_robust")


@functools.lru_cache(maxsize=None)
def frame():
    """The walks' frame through the oracle: (OracleScene over Duck's arrays, camera (19 floats), sky state (40 floats)); one per process, so one sample cache"""
    import rayfinder_amd as rf                                # host code only: the .glb ingest and the BVH build the bit-exact GPU tests feed the oracle with
    pt = rf.PtFormat.from_gltf(DUCK)
    scene, _ = oracle_scene_from_pt(pt)
    return scene, rf.camera_to_array(rf.fly_camera(W, H)), rf.aligned_sky_state(rf.make_sky())


def new_model():
    scene, camera, sky = frame()
    return HandleModel(scene, W, H, SPP, BOUNCES, EXPOSURE, camera, sky)


def apply(model, call):
    """One call of a walk on the model -> ("ok", value) | ("refused", keyword)"""
    name, args = call[0], call[1:]
    if name == "set_exposure":
        return model.set_render_parameters(*args)
    if name == "bind":
        return model.bind_accumulation_buffer(True)
    if name == "unbind":
        return model.bind_accumulation_buffer(False)
    if name in ("denoise", "denoise_robust"):
        return getattr(model, name)(iterations=args[0])
    return getattr(model, name)(*args)


def _median_target(model, every, min_samples, max_samples):
    """The median of the model's own errors of the active tiles at the call's first check: about half of them stop there.  None where no check would be made."""
    cap = SPP if max_samples == 0 else min(max_samples, SPP)
    L = model.L
    while L < cap:
        L += min(every, cap - L)
        if L >= max(2, min_samples):
            break
    else:
        return None
    if L < max(2, min_samples):
        return None
    active = [t for t in range(TILES) if model.counts[t] == model.L]
    errors = tile_errors(estimate(model._sum("S", 0, L), model._sum("Q", 0, L), L))[active]
    return float(np.float32(np.median(errors)))


def _adaptive_runs(m):
    """render_adaptive would be accepted with valid arguments"""
    return (m.moments_on and (m.L == 0 or m.q_start == 0) and m.world == 1 and (not m.K or (m.bucket_bit and (m.L == 0 or m.b_start == 0)))
            and (not m._aov_on() or (m._aov_bit() and (m.L == 0 or m.a_start == 0))))


def _draw(rng, m):
    """One call, drawn from the model's state"""
    non_uniform, runs = m.non_uniform(), _adaptive_runs(m)
    would_run = lambda reasons: 2.0 if not reasons else 0.4              # noqa: E731  (a query that would run is drawn more often than one that would be refused)
    per_tile_buckets = non_uniform and m.K and m.bucket_bit
    weights = dict(render=1.0 if non_uniform else 4.0, render_until=1.0, render_adaptive=3.0 if runs and m.L < SPP else 0.8,
                   set_moments=3.0 if not m.moments_on and m.L == 0 else 1.0 if not m.moments_on else 0.15,
                   set_aovs=0.5 if m._aov_on() and m.L > 0 else 1.2, set_buckets=0.5 if non_uniform or (m.K and m.L > 0) else 1.5, set_exposure=0.9 if non_uniform else 0.4,
                   set_tile_shard=2.5 if m.world != 1 else 0.5, bind=0.3, unbind=1.5 if m.bound else 0.1,
                   noise_estimate=0.8, denoise=1.0 * would_run(m._denoise_reasons()),
                   robust_mean=3.0 if per_tile_buckets else 0.6 * would_run(m._robust_reasons()),
                   denoise_robust=(3.0 if non_uniform else 1.0) * would_run(m._denoise_reasons() + m._robust_reasons()))
    pick = lambda options: options[int(rng.integers(len(options)))]      # noqa: E731
    # calls that only this state makes possible: drawn on purpose now and then, so that the walks reach the compound situations
    purposeful = []
    if not non_uniform and m.L > 0:
        if m.K:
            purposeful.append(("set_buckets", (8 - m.K) | (BIT if m.bucket_bit else 0)))                  # another K mid-accumulation (3 <-> 5)
            purposeful.append(("set_buckets", m.K | (0 if m.bucket_bit else BIT)))                        # the tile bit alone
        if not m.moments_on:
            purposeful.append(("set_moments", 1))                                                         # the moments on partway
        if m._aov_on():
            purposeful.append(("set_aovs", m.aov_flags ^ AOV_TILE_COUNTS))                                # between the two valid values
        if m.L == SPP:
            purposeful.append(("render", pick(STEPS)))
    if runs and m.L < SPP and rng.random() < 0.4:
        every, min_samples = pick(((2, 0), (3, 0))) if m.K == 5 and rng.random() < 0.4 else (4, 8)       # tiles that stop below K = 5 | every tile with K samples or more
        target = _median_target(m, every, min_samples, 0)
        if target is not None:
            purposeful.append(("render_adaptive", target, every, min_samples, pick((0, 0, 16))))
    if per_tile_buckets and rng.random() < 0.5:
        purposeful.append(("robust_mean",))
    if m.L > 0 and not m._robust_reasons() and rng.random() < 0.3:
        purposeful.append(("robust_mean",))
    if m.L > 0 and not m._denoise_reasons() + m._robust_reasons():
        purposeful.append(("denoise_robust", pick((0, 2, 5))))
    if non_uniform and rng.random() < 0.25:
        purposeful.append(("set_exposure", pick([e for e in EXPOSURES if e != m.exposure])))          # an event ends the non-uniform state
    if m.world != 1:
        purposeful.append(("set_tile_shard", 0, 1))
    if purposeful and rng.random() < 0.4:
        return pick(purposeful)
    names = list(weights)
    p = np.array([weights[k] for k in names])
    name = names[int(rng.choice(len(names), p=p / p.sum()))]
    if name == "render":
        return ("render", pick(STEPS))
    if name == "render_until":
        every = pick((0, 1, 2, 4, 5))
        return ("render_until", pick((0.0, HUGE, 0.05)), every, pick((3, 8, 0xFFFFFFFF)))
    if name == "render_adaptive":
        every, min_samples, max_samples = pick((0, 2, 2, 3, 4, 4, 4, 8)), pick((0, 0, 4, 8)), pick((0, 0, 8, 16))
        kind = pick(("zero", "huge", "median", "median", "median", "median", "median", "negative"))
        target = dict(zero=0.0, huge=HUGE, negative=-1.0).get(kind)
        if kind == "median":
            target = _median_target(m, every, min_samples, max_samples) if runs and every else 0.05
            target = 0.05 if target is None else target
        return ("render_adaptive", target, every, min_samples, max_samples)
    if name == "set_moments":
        return ("set_moments", int(rng.random() < 0.8) if not m.moments_on else int(rng.random() < 0.3))
    if name == "set_aovs":
        return ("set_aovs", AOV_ARGS[int(rng.choice(4, p=(0.15, 0.3, 0.4, 0.15)))])
    if name == "set_buckets":
        return ("set_buckets", BUCKET_ARGS[int(rng.choice(9, p=(0.1, 0.1, 0.1, 0.25, 0.25, 0.05, 0.05, 0.05, 0.05)))])
    if name == "set_exposure":
        return ("set_exposure", pick(EXPOSURES))
    if name == "set_tile_shard":
        return ("set_tile_shard",) + ((0, 1) if m.world != 1 and rng.random() < 0.7 else pick(SHARDS))
    if name in ("denoise", "denoise_robust"):
        return (name, pick((0, 2, 5)))
    return (name,)


@functools.lru_cache(maxsize=None)
def walk(seed, length=LENGTH):
    """-> (the walk's calls, a tuple of tuples; its scheduling: dict(max_paths_in_flight, options))"""
    rng = np.random.default_rng(SEED_BASE + seed)
    scheduling = dict(max_paths_in_flight=MAX_PATHS[int(rng.integers(3))],
                      options=dict(slot_group_shift=(0, 2, -1)[int(rng.integers(3))], accumulate_runs=(1, 0)[int(rng.integers(2))], sample_sort=(1, 0)[int(rng.integers(2))]))
    model = new_model()
    calls = []
    # most walks open with the switches that the interesting calls need from the first sample
    for call, chance in ((("set_moments", 1), 0.85), (("set_aovs", AOV_FIRST_HIT | AOV_TILE_COUNTS), 0.7), (("set_buckets", (3, 5, 5)[int(rng.integers(3))] | BIT), 0.7)):
        if rng.random() < chance and len(calls) < length:
            calls.append(call)
            apply(model, call)
    while len(calls) < length:
        call = _draw(rng, model)
        calls.append(call)
        apply(model, call)
    return tuple(calls), scheduling


def replay_lines(seed, calls, scheduling):
    """The calls so far as lines of Python that replay them against both sides (run from tests/, on the GPU machine)"""
    lines = ["import handle_walk, test_gpu_handle_walk as g",
             f"model, handle, keep = handle_walk.new_model(), g.new_handle({scheduling!r}), []   # seed {seed}"]
    for i, call in enumerate(calls):
        lines.append(f"print({i}, handle_walk.apply(model, {call!r}), g.apply_gpu(handle, {call!r}, keep), g.against_model(g.observe_gpu(handle), model))")
    return "\n".join(lines)
