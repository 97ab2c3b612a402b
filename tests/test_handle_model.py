"""The handle model (tests/handle_model.py) and the walk set (tests/handle_walk.py) on the CPU: the model is held to what the suite already trusts -- the oracle's
render and the restatements' sums -- and the seeded walks to the coverage conditions below, computed from the model alone.  The conditions are conditions, not
measurements: the generator's weights are tuned until they hold, the thresholds never.

One condition cannot be met as a whole: "every state-changing call kind is refused at least once".  include/rayfinder_amd.h gives set_moments, set_render_parameters
(an exposure) and binding / unbinding a buffer that is large enough no RF_ERROR_INVALID_ARGUMENT refusal on a valid handle, so NEVER_REFUSED lists them and they
are held to the accepted half alone."""
import functools

import numpy as np

import handle_walk as hw
from adaptive_restatement import play, prefix_sums, tile_errors, tile_slices
from aov_restatement import aov_sums
from handle_model import AOV_FIRST_HIT, AOV_TILE_COUNTS, bits, differing
from noise_restatement import estimate, oracle_samples
from oracle import orc
from robust_restatement import bucket_sums

NEVER_REFUSED = ("set_moments", "set_exposure", "bind", "unbind")
EVENTS = ("moments on partway", "AOV flags changed between the valid values mid-accumulation", "K changed mid-accumulation", "a second adaptive call continues",
          "a batch shorter than K after a non-zero bucket phase", "robust mean refused for a tile below K", "denoise_robust runs in the non-uniform state",
          "a shard set and taken back", "render calls after the accumulation ran to spp", "the tile bit alone changed over non-zero bucket sums")


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_a_fresh_models_sums_are_the_oracles_and_the_restatements():
    n, k = 7, 3
    m = hw.new_model()
    for call in (("set_moments", 1), ("set_aovs", AOV_FIRST_HIT), ("set_buckets", k), ("render", n)):
        assert hw.apply(m, call)[0] == "ok"
    scene, _, _ = hw.frame()
    samples = list(oracle_samples(orc, scene, m.rp, range(n)))
    S, Q = prefix_sums(samples)
    ref, _ = orc.render(scene, m.rp, 0, n)
    ac, nd = aov_sums(scene, m.rp, range(n))
    (s, acc), (q, qn), (a, d, an), (b, kk, bn) = m.read_accumulation(), m.read_moments(), m.read_aovs(), m.read_buckets()
    assert acc == qn == an == bn == n and kk == k and m.frame_count == n
    assert _same(s[..., :3], ref[..., :3]) and _same(s, S[n]) and _same(q, Q[n]) and _same(a, ac) and _same(d, nd) and _same(b, bucket_sums(samples, k))
    assert s[..., :3].any() and q.any() and a[..., 3].any() and b[k - 1].any()
    assert m.primary_rays == n * hw.W * hw.H and m.read_tile_samples().tolist() == [n] * hw.TILES and m.tile_samples_uniform()


def test_after_an_adaptive_call_every_tile_holds_the_uniform_sums_at_its_own_count():
    """The header's defining property, and the issue's figure for this frame: the median target at check_every = 4, min_samples = 8 leaves [16 24 8 8 16 8]"""
    k = 5
    m = hw.new_model()
    for call in (("set_moments", 1), ("set_aovs", AOV_FIRST_HIT | AOV_TILE_COUNTS), ("set_buckets", k | hw.BIT)):
        hw.apply(m, call)
    target = hw._median_target(m, 4, 8, 0)
    scene, _, _ = hw.frame()
    samples = list(oracle_samples(orc, scene, m.rp, range(hw.SPP)))
    S, Q = prefix_sums(samples)
    assert target == float(np.float32(np.median(tile_errors(estimate(S[8], Q[8], 8)))))
    outcome, value = hw.apply(m, ("render_adaptive", target, 4, 8, 0))
    counts = m.read_tile_samples()
    assert outcome == "ok" and counts.tolist() == [16, 24, 8, 8, 16, 8] and not m.tile_samples_uniform() and m.L == 24 and m.frame_count == 24
    want = play(S, Q, hw.W, hw.H, target, 4, min_samples=8)
    assert value["pixel_samples"] == want["pixel_samples"] == m.primary_rays and value["stopped_tiles"] == want["stopped_tiles"] == 5
    got = dict(S=m.read_accumulation()[0], Q=m.read_moments()[0], AC=m.read_aovs()[0], ND=m.read_aovs()[1], B=m.read_buckets()[0])
    assert m.read_moments()[1] == m.read_aovs()[2] == m.read_buckets()[2] == 24
    uniform = {}
    for c in sorted(set(counts.tolist())):                                   # a fresh model rendered uniformly to each count
        u = hw.new_model()
        for call in (("set_moments", 1), ("set_aovs", AOV_FIRST_HIT), ("set_buckets", k), ("render", c)):
            hw.apply(u, call)
        uniform[c] = dict(S=u.read_accumulation()[0], Q=u.read_moments()[0], AC=u.read_aovs()[0], ND=u.read_aovs()[1], B=u.read_buckets()[0])
    for t, (rows, cols) in enumerate(tile_slices(hw.W, hw.H)):
        for name in got:
            assert _same(got[name][..., rows, cols, :], uniform[int(counts[t])][name][..., rows, cols, :]), (t, name)
    assert _same(got["S"], want["S"]) and _same(got["Q"], want["Q"])


def test_a_refused_call_changes_nothing():
    m = hw.new_model()
    for call in (("set_moments", 1), ("render", 3)):
        hw.apply(m, call)
    before, frame = m.observe(), m.frame_count
    for call in (("set_buckets", 4), ("set_aovs", AOV_TILE_COUNTS), ("render_adaptive", -1.0, 4, 0, 0), ("render_adaptive", 0.1, 0, 0, 0), ("denoise", 5), ("robust_mean",),
                 ("render_until", 0.0, 0, 8)):
        assert hw.apply(m, call)[0] == "refused", call
        assert differing(m.observe(), before) == [] and m.frame_count == frame


def test_walks_are_deterministic():
    first = hw.walk.__wrapped__(3, hw.LENGTH)
    assert first == hw.walk.__wrapped__(3, hw.LENGTH) and first == hw.walk(3)
    assert len(first[0]) == hw.LENGTH and first != hw.walk(4)


@functools.lru_cache(maxsize=None)
def survey():
    """Every seeded walk through the model alone -> per seed: dict(kinds, accepted, refused, events, entered, left, frames, render_refused_non_uniform)"""
    out = {}
    for seed in hw.SEEDS:
        calls, _ = hw.walk(seed)
        m = hw.new_model()
        s = dict(kinds=[c[0] for c in calls], accepted=[], refused=[], events=set(), entered=False, left=False, render_refused_non_uniform=False, shard_set=False)
        for call in calls:
            name = call[0]
            was = dict(non_uniform=m.non_uniform(), L=m.L, K=m.K, flags=m.aov_flags, moments=m.moments_on, world=m.world, b_start=m.b_start, bit=m.bucket_bit,
                       tile_below_k=any(isinstance(r, tuple) and len(r) == 2 for r in m._robust_reasons()))
            outcome, _ = hw.apply(m, call)
            (s["accepted"] if outcome == "ok" else s["refused"]).append(name)
            now = m.non_uniform()
            s["entered"] |= now and not was["non_uniform"]
            s["left"] |= was["non_uniform"] and not now
            if outcome == "refused":
                s["render_refused_non_uniform"] |= name == "render" and was["non_uniform"]
                if name == "robust_mean" and was["tile_below_k"]:
                    s["events"].add(EVENTS[5])
                continue
            if name == "set_moments" and m.moments_on and not was["moments"] and was["L"] > 0:
                s["events"].add(EVENTS[0])
            if name == "set_aovs" and was["L"] > 0 and {was["flags"], m.aov_flags} == {AOV_FIRST_HIT, AOV_FIRST_HIT | AOV_TILE_COUNTS}:
                s["events"].add(EVENTS[1])
            if name == "set_buckets" and was["L"] > 0 and was["K"] and m.K and was["K"] != m.K:
                s["events"].add(EVENTS[2])
            if name == "set_buckets" and was["K"] == m.K and m.K and was["bit"] != m.bucket_bit and was["L"] > was["b_start"]:
                s["events"].add(EVENTS[9])
            if name == "render_adaptive" and was["non_uniform"] and m.L > was["L"]:
                s["events"].add(EVENTS[3])
            if name in ("render", "render_until", "render_adaptive") and m.K and m.L > was["L"]:
                step = m.L - was["L"] if name == "render" else call[2]
                L = was["L"]
                while L < m.L:                                               # the batches' sizes: the call's steps
                    n = min(step, m.L - L)
                    if n < m.K and (L - was["b_start"]) % m.K != 0:
                        s["events"].add(EVENTS[4])
                    L += n
            if name == "denoise_robust" and was["non_uniform"]:
                s["events"].add(EVENTS[6])
            if name == "set_tile_shard":
                if m.world != 1:
                    s["shard_set"] = True
                elif s["shard_set"] and was["world"] != 1:
                    s["events"].add(EVENTS[7])
            if name == "render" and was["L"] == hw.SPP:
                s["events"].add(EVENTS[8])
        s["frames"] = len(m.frames_traced)
        out[seed] = s
    return out


def unmet(sv):
    """The conditions the walk set misses, in words"""
    kinds = hw.STATE_CHANGING + hw.QUERIES
    accepted = {k: sum(s["accepted"].count(k) for s in sv.values()) for k in kinds}
    refused = {k: sum(s["refused"].count(k) for s in sv.values()) for k in kinds}
    missed = [f"{k} is never accepted" for k in kinds if accepted[k] < 1]
    missed += [f"{k} is never refused" for k in kinds if refused[k] < 1 and k not in NEVER_REFUSED]
    if not any(s["render_refused_non_uniform"] for s in sv.values()):
        missed.append("render is never refused in the non-uniform state")
    entered = [s for s in sv.values() if s["entered"]]
    if 2 * len(entered) < len(sv):
        missed.append(f"the non-uniform state is entered in {len(entered)} of {len(sv)} walks")
    if 3 * sum(s["left"] for s in entered) < len(entered):
        missed.append(f"the non-uniform state is left again in {sum(s['left'] for s in entered)} of {len(entered)} walks")
    missed += [f"no walk reaches: {e}" for e in EVENTS if not any(e in s["events"] for s in sv.values())]
    if 2 * sum(refused.values()) > sum(accepted.values()) + sum(refused.values()):
        missed.append(f"{sum(refused.values())} of {sum(accepted.values()) + sum(refused.values())} calls are refused")
    missed += [f"walk {seed} traces {s['frames']} frames" for seed, s in sv.items() if s["frames"] > 120]
    return missed, accepted, refused


def test_the_walk_set_meets_its_conditions():
    sv = survey()
    missed, accepted, refused = unmet(sv)
    for seed, s in sv.items():
        print(seed, "frames", s["frames"], "entered", s["entered"], "left", s["left"], "refused", len(s["refused"]), sorted(s["events"]))
        print("   ", " ".join(s["kinds"]))
    print("accepted", accepted)
    print("refused ", refused)
    assert missed == []
