"""Hand-written call sequences over the walks' frame (tests/handle_walk.py: Duck, 72 x 40, 24 spp), each ending in the refusal it is after: the refusals the handle
model (tests/handle_model.py) does not have -- the direct sums, denoise_split, export_features, rf_comm_render_adaptive's checks, bad words to the set calls, reads
without a snapshot, every call that needs the whole frame under a tile shard -- and one of each wording the walks may or may not draw.  tools/record_refusals.py plays
them on a GPU handle and records what rf_last_error_message() says (tests/golden/refusals_parent.json); tests/test_books.py plays them through tests/books_main.cpp.

A call is a tuple in handle_walk's form; beside the walk's kinds: ("set_direct", word), ("denoise_split",), ("export_features", channel names), ("read_denoised",),
("read_robust_mean",) and ("check_adaptive", target, check_every, 1): rf_comm_render_adaptive on a communicator of one rank, refused before anything is exchanged."""
FIRST_HIT, TILE_COUNTS, SHARD_TILE_COUNTS = 0x1, 0x100, 0x400
# the median of the model's tile errors at 8 samples (handle_walk._median_target of a fresh model, check_every = 4, min_samples = 8): render_adaptive from nothing
# leaves the counts [16, 24, 8, 8, 16, 8] (tests/test_handle_model.py) -- the non-uniform state; at check_every = 2, min_samples = 0: [8, 16, 2, 2, 8, 2], tiles below K = 5
MEDIAN_AT_8, MEDIAN_AT_2 = 0.026662258431315422, 0.040076084434986115
ADAPTIVE = ("render_adaptive", MEDIAN_AT_8, 4, 8, 0)
MOMENTS, AOVS, AOVS_BIT, DIRECT, DIRECT_BIT = ("set_moments", 1), ("set_aovs", FIRST_HIT), ("set_aovs", FIRST_HIT | TILE_COUNTS), ("set_direct", 1), ("set_direct", 1 | TILE_COUNTS)
SHARD = ("set_tile_shard", 0, 2)
NON_UNIFORM = [MOMENTS, ADAPTIVE]                       # nothing but the moments kept
EVERYTHING_PER_TILE = [MOMENTS, AOVS_BIT, DIRECT_BIT, ("set_buckets", 5 | TILE_COUNTS)]

# what a feature channel reads (rf_feature_request.hpp: kFeatureReadsS = 1, Q = 2, the AOVs = 4, D = 8) and whether it needs two samples
FEATURE_READS = dict(color=(1, False), albedo=(4, False), normal=(4, False), depth=(4, False), coverage=(4, False), direct=(8, False), indirect=(1 | 8, False),
                     variance=(1 | 2, True), error=(1 | 2, True), samples=(0, False))


def feature_reads(channels):
    reads, two = 0, False
    for c in channels:
        reads, two = reads | FEATURE_READS[c][0], two or FEATURE_READS[c][1]
    return reads, two


CASES = {
    # ---- the direct sums and the split denoiser
    "split: the direct sums are off": [AOVS, ("render", 2), ("denoise_split",)],
    "split: the AOVs are off": [DIRECT, ("render", 2), ("denoise_split",)],
    "split: no sample": [AOVS, DIRECT, ("denoise_split",)],
    "split: the AOVs came on partway": [DIRECT, ("render", 2), AOVS, ("render", 1), ("denoise_split",)],
    "split: the direct sums came on partway": [AOVS, ("render", 2), DIRECT, ("render", 1), ("denoise_split",)],
    "split: non-uniform, nothing kept per tile": NON_UNIFORM + [("denoise_split",)],
    "split: non-uniform, the AOVs alone kept per tile": [MOMENTS, AOVS_BIT, ADAPTIVE, ("denoise_split",)],
    "adaptive: the direct sums without their bit": [MOMENTS, DIRECT, ADAPTIVE],
    "adaptive: the direct sums came on partway": [MOMENTS, ("render", 2), DIRECT_BIT, ADAPTIVE],
    "set_direct: on, non-uniform": NON_UNIFORM + [DIRECT],
    "set_direct: on with the bit, non-uniform": NON_UNIFORM + [DIRECT_BIT],
    "set_direct: the bit alone": [("set_direct", TILE_COUNTS)],
    "set_direct: an unknown bit": [("set_direct", 2)],
    # ---- bad words to the other set calls
    "set_buckets: even": [("set_buckets", 4)],
    "set_buckets: one": [("set_buckets", 1)],
    "set_buckets: too many": [("set_buckets", 17)],
    "set_buckets: the bit alone": [("set_buckets", TILE_COUNTS)],
    "set_buckets: an unknown bit": [("set_buckets", 9 | 0x200)],
    "set_buckets: the shard bit without the tile bit": [("set_buckets", 3 | SHARD_TILE_COUNTS)],
    "set_buckets: on, non-uniform": NON_UNIFORM + [("set_buckets", 3)],
    "set_aovs: the bit alone": [("set_aovs", TILE_COUNTS)],
    "set_aovs: an unknown bit": [("set_aovs", 2)],
    "set_tile_shard: rank beyond the world": [("set_tile_shard", 2, 2)],
    "set_tile_shard: no world": [("set_tile_shard", 0, 0)],
    "set_tile_shard: non-uniform": NON_UNIFORM + [SHARD],
    # ---- export_features
    "features: the AOVs are off": [("render", 2), ("export_features", ("color", "albedo"))],
    "features: the direct sums are off": [("render", 2), ("export_features", ("indirect",))],
    "features: the moments are off": [("render", 2), ("export_features", ("variance",))],
    "features: no sample": [AOVS, ("export_features", ("albedo",))],
    "features: the AOVs came on partway": [("render", 1), AOVS, ("render", 1), ("export_features", ("normal",))],
    "features: the direct sums came on partway": [("render", 1), DIRECT, ("render", 1), ("export_features", ("direct",))],
    "features: the moments came on partway": [("render", 1), MOMENTS, ("render", 1), ("export_features", ("error",))],
    "features: one sample": [MOMENTS, ("render", 1), ("export_features", ("variance",))],
    "features: non-uniform, the AOVs off": NON_UNIFORM + [("export_features", ("depth",))],
    # ---- rf_comm_render_adaptive's checks
    "sharded: the buckets with the tile bit alone": [MOMENTS, ("set_buckets", 3 | TILE_COUNTS), ("check_adaptive", 0.1, 4, 1)],
    "sharded: the buckets without a bit": [MOMENTS, ("set_buckets", 3), ("check_adaptive", 0.1, 4, 1)],
    "sharded: the buckets with both bits, the moments off": [("set_buckets", 3 | TILE_COUNTS | SHARD_TILE_COUNTS), ("check_adaptive", 0.1, 4, 1)],
    "sharded: the AOVs without their bit": [MOMENTS, AOVS, ("check_adaptive", 0.1, 4, 1)],
    "sharded: the direct sums without their bit": [MOMENTS, DIRECT, ("check_adaptive", 0.1, 4, 1)],
    "sharded: check_every 0": [MOMENTS, ("check_adaptive", 0.1, 0, 1)],
    "sharded: a negative target": [MOMENTS, ("check_adaptive", -1.0, 4, 1)],
    "sharded: the buckets came on partway": [MOMENTS, ("render", 2), ("set_buckets", 3 | TILE_COUNTS | SHARD_TILE_COUNTS), ("check_adaptive", 0.1, 4, 1)],
    # ---- reads without a snapshot
    "read_denoised: none yet": [("read_denoised",)],
    "read_robust_mean: none yet": [("read_robust_mean",)],
    "read_denoised: dropped with the AOV sums": [AOVS, ("render", 2), ("denoise", 2), AOVS_BIT, ("read_denoised",)],
    "read_denoised: dropped with the direct sums": [AOVS, DIRECT, ("render", 2), ("denoise_split",), ("set_direct", 0), ("read_denoised",)],
    "read_denoised: dropped with the accumulation": [AOVS, ("render", 2), ("denoise", 2), ("set_exposure", 0.5), ("read_denoised",)],
    "read_robust_mean: dropped with the bucket sums": [("set_buckets", 3), ("render", 3), ("robust_mean",), ("set_buckets", 5), ("read_robust_mean",)],
    "read_robust_mean: dropped with the accumulation": [("set_buckets", 3), ("render", 3), ("robust_mean",), SHARD, ("read_robust_mean",)],
    # ---- every call that needs the whole frame, under a tile shard
    "shard: denoise": [AOVS, SHARD, ("render", 2), ("denoise", 2)],
    "shard: denoise_split": [AOVS, DIRECT, SHARD, ("render", 2), ("denoise_split",)],
    "shard: export_features": [SHARD, ("render", 2), ("export_features", ("color",))],
    "shard: robust_mean": [("set_buckets", 3), SHARD, ("render", 3), ("robust_mean",)],
    "shard: denoise_robust": [AOVS, ("set_buckets", 3), SHARD, ("render", 3), ("denoise_robust", 2)],
    "shard: noise_estimate": [MOMENTS, SHARD, ("render", 2), ("noise_estimate",)],
    "shard: render_until": [MOMENTS, SHARD, ("render_until", 0.0, 2, 4)],
    "shard: render_adaptive": [MOMENTS, SHARD, ADAPTIVE],
    # ---- one of each wording of the calls the walks draw from
    "render: non-uniform": NON_UNIFORM + [("render", 1)],
    "render_until: the moments are off": [("render_until", 0.0, 2, 4)],
    "render_until: non-uniform": NON_UNIFORM + [("render_until", 0.0, 2, 4)],
    "render_until: check_every 0": [MOMENTS, ("render_until", 0.0, 0, 4)],
    "render_until: the moments came on partway": [("render", 2), MOMENTS, ("render_until", 0.0, 2, 4)],
    "noise_estimate: the moments are off": [("render", 2), ("noise_estimate",)],
    "noise_estimate: the moments came on partway": [("render", 2), MOMENTS, ("render", 2), ("noise_estimate",)],
    "noise_estimate: one sample": [MOMENTS, ("render", 1), ("noise_estimate",)],
    "denoise: the AOVs are off": [("render", 2), ("denoise", 2)],
    "denoise: no sample": [AOVS, ("denoise", 2)],
    "denoise: the AOVs came on partway": [("render", 2), AOVS, ("render", 1), ("denoise", 2)],
    "denoise: non-uniform, the AOVs off": NON_UNIFORM + [("denoise", 2)],
    "robust_mean: the buckets are off": [("render", 2), ("robust_mean",)],
    "robust_mean: fewer samples than buckets": [("set_buckets", 5), ("render", 3), ("robust_mean",)],
    "robust_mean: the buckets came on partway": [("render", 2), ("set_buckets", 3), ("render", 4), ("robust_mean",)],
    "robust_mean: non-uniform, the buckets off": NON_UNIFORM + [("robust_mean",)],
    "robust_mean: a tile below K": [MOMENTS, ("set_buckets", 5 | TILE_COUNTS), ("render_adaptive", MEDIAN_AT_2, 2, 0, 0), ("robust_mean",)],
    "denoise_robust: the AOVs are off": [("set_buckets", 3), ("render", 3), ("denoise_robust", 2)],
    "denoise_robust: the buckets are off": [AOVS, ("render", 3), ("denoise_robust", 2)],
    "denoise_robust: non-uniform, the AOVs off": NON_UNIFORM + [("denoise_robust", 2)],
    "denoise_robust: non-uniform, the buckets off": [MOMENTS, AOVS_BIT, ADAPTIVE, ("denoise_robust", 2)],
    "adaptive: the moments are off": [ADAPTIVE],
    "adaptive: the buckets without their bit": [MOMENTS, ("set_buckets", 3), ADAPTIVE],
    "adaptive: the AOVs without their bit": [MOMENTS, AOVS, ADAPTIVE],
    "adaptive: check_every 0": [MOMENTS, ("render_adaptive", 0.1, 0, 0, 0)],
    "adaptive: a negative target": [MOMENTS, ("render_adaptive", -1.0, 4, 0, 0)],
    "adaptive: a target that is no number": [MOMENTS, ("render_adaptive", float("nan"), 4, 0, 0)],
    "adaptive: the moments came on partway": [("render", 2), MOMENTS, ADAPTIVE],
    "adaptive: the AOVs came on partway": [MOMENTS, ("render", 2), AOVS_BIT, ADAPTIVE],
    "adaptive: the buckets came on partway": [MOMENTS, ("render", 2), ("set_buckets", 3 | TILE_COUNTS), ADAPTIVE],
    "adaptive: a shard and a switch at fault": [MOMENTS, AOVS, SHARD, ADAPTIVE],
    "adaptive: a shard and an argument at fault": [MOMENTS, SHARD, ("render_adaptive", 0.1, 0, 0, 0)],
    # (everything kept per tile count: the reads run in the non-uniform state; another K is refused there all the same)
    "set_buckets: another K, non-uniform with everything kept per tile": EVERYTHING_PER_TILE + [ADAPTIVE, ("denoise_split",), ("set_buckets", 3)],
}
