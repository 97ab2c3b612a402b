// rf_books.cpp -- the accumulation's books and refusals (rf_books.hpp).  Host only.
#include "rf_books.hpp"

#include "rf_feature_request.hpp" // kFeatureReads*

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <utility>

namespace rf
{
namespace
{
using Books = AccumulationBooks;
enum class Drops
{
    Nothing,
    Denoised,
    RobustMean
};
// What the messages call a family, and what its restart takes with it
struct FamilyWords
{
    const char* name;    // "... needs the first-hit AOVs"
    const char* hint;    // its set call
    const char* count;   // "the AOV sample count"
    const char* them;    // "turn the AOVs on"
    const char* perTile; // the word that keeps it per tile count, where a bit says so
    bool        alwaysPerTile;
    Drops       drops; // the snapshot made from these sums
};
const FamilyWords kWords[Books::kFamilies] = {
    {"the image", "", "", "", "", true, Drops::Nothing},
    {"the first-hit AOVs", "rf_renderer_set_aovs", "AOV", "the AOVs", "RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS", false, Drops::Denoised},
    {"the radiance second moments", "rf_renderer_set_moments", "moment", "the moments", "", true, Drops::Nothing}, // (render_adaptive needs them)
    {"the direct sums", "rf_renderer_set_direct", "direct", "the direct sums", "1 | RF_DIRECT_TILE_COUNTS", false, Drops::Denoised},
    {"the bucket sums", "rf_renderer_set_buckets", "bucket", "the buckets", "", false, Drops::RobustMean},
};
constexpr Books::Family kSwitched[] = {Books::kAovs, Books::kMoments, Books::kDirect, Books::kBuckets}; // every family but the image
std::string str(uint32_t n) { return std::to_string(n); }
} // namespace

AccumulationBooks::AccumulationBooks() { mSums[kImage].on = true, mSums[kImage].word = 1u; }

// ---- counters and tiles
void AccumulationBooks::requireUniform(const char* what, const std::string& unless) const
{
    if (nonUniform() || frameNonUniform())
        throw std::invalid_argument(std::string(what) + ": the tiles hold different sample counts after rf_renderer_render_adaptive" + unless +
                                    " (continue with render_adaptive, or restart the accumulation with rf_renderer_set_render_parameters)");
}

std::vector<uint32_t> AccumulationBooks::tileCounts() const { return nonUniform() ? mTileSamples : std::vector<uint32_t>(mShardTiles, mAccumulated); }

uint32_t AccumulationBooks::minTileSamples() const
{
    // (frameLeadingSamples != 0: rf_comm_render_adaptive has settled the frame's figures since the accumulation was restarted)
    if (mFrameLeadingSamples != 0u) return mFrameMinTileSamples;
    return nonUniform() ? leastOwnTile() : mAccumulated;
}

bool AccumulationBooks::tileCounts(Family f) const { return mSums[f].on && (kWords[f].alwaysPerTile || (mSums[f].word & kWordTileCounts) != 0u); }
bool AccumulationBooks::shardTileCounts(Family f) const { return mSums[f].on && (kWords[f].alwaysPerTile || (mSums[f].word & kWordShardTileCounts) != 0u); }

// ---- transitions
// the sums start again: zeroed before the next sample, sized for the shard then
void AccumulationBooks::restart(Family f)
{
    mSums[f].samples = 0;
    mSums[f].dirty = true;
    if (kWords[f].drops == Drops::Denoised) mDenoised.valid = false;
    if (kWords[f].drops == Drops::RobustMean) mRobust.valid = false;
    if (f == kAovs) mTemporal.valid = false; // (the temporal result is made from S and the AOV sums; S never restarts without them.  The temporal HISTORY stays)
}

void AccumulationBooks::restartAccumulation()
{
    mAccumulated = 0;
    mTileSamples.clear();
    mFrameLeadingSamples = mFrameMinTileSamples = 0;
    for (uint32_t f = 0; f < kFamilies; ++f) restart(static_cast<Family>(f));
}

AccumulationBooks::Change AccumulationBooks::set(Family f, uint32_t word, uint32_t planes)
{
    if (word == mSums[f].word) return Change::Unchanged;
    mSums[f].word = word;
    mSums[f].on = (word & (f == kBuckets ? kWordOn : 1u)) != 0u;
    mSums[f].planes = planes;
    restart(f);
    return mSums[f].on ? Change::Restarted : Change::RestartedOff;
}

AccumulationBooks::Change AccumulationBooks::setAovs(uint32_t word) { return set(kAovs, word, 1u); }
AccumulationBooks::Change AccumulationBooks::setMoments(bool enabled) { return set(kMoments, enabled ? 1u : 0u, 1u); }

AccumulationBooks::Change AccumulationBooks::setDirect(uint32_t word)
{
    if ((word & ~(1u | kWordTileCounts)) != 0u || word == kWordTileCounts)
        throw std::invalid_argument("set_direct: the word must be 0 (off), 1 (on) or 1 | RF_DIRECT_TILE_COUNTS (the bit says how D is kept: valid only together with 1)");
    // (with the bit too: D must hold every tile's samples from the tile's first one on, and the tiles below the leading count get no more)
    if ((word & 1u) != 0u) requireUniform("rf_renderer_set_direct", ": the direct sums keep ONE sample count for the frame");
    return set(kDirect, word, 1u);
}

AccumulationBooks::Change AccumulationBooks::setBuckets(uint32_t word)
{
    // the low byte is K, HOW starts at bit 8 (as in the AOV flags word)
    const uint32_t K = word & kWordOn;
    const bool     tileCounts = (word & kWordTileCounts) != 0u, shardTileCounts = (word & kWordShardTileCounts) != 0u;
    if ((word & ~(kWordOn | kWordTileCounts | kWordShardTileCounts)) != 0u || (K == 0u && tileCounts) || (K != 0u && (K % 2u == 0u || K < 3u || K > kMaxBuckets)) ||
        (shardTileCounts && !tileCounts))
        throw std::invalid_argument("set_buckets: K must be 0 (off) or odd with 3 <= K <= 15, alone or ORed with RF_BUCKETS_TILE_COUNTS (K > 0 only), and with "
                                    "RF_BUCKETS_SHARD_TILE_COUNTS on top of that bit only");
    if (K != 0u) requireUniform("rf_renderer_set_buckets", ": the bucket sums keep ONE sample count for the frame");
    return set(kBuckets, word, K != 0u ? K : 1u); // (a change of either bit alone clears the sums too)
}

void AccumulationBooks::recordStep(uint32_t n)
{
    mFrameCount += n;
    mAccumulated += n;
    for (Sums& s : mSums)
        if (s.on) s.samples += n;
}

uint32_t AccumulationBooks::framesToTrace(uint32_t numFrames)
{
    if (numFrames != 0u && (mAccumulated >= mSampleCap || mShardTiles == 0u))
    {
        mFrameCount += numFrames;
        return 0u;
    }
    return std::min(numFrames, mSampleCap - mAccumulated);
}

uint32_t AccumulationBooks::settleTileSamples(const std::vector<uint32_t>& counts)
{
    const uint32_t stopped = static_cast<uint32_t>(std::count_if(counts.begin(), counts.end(), [&](uint32_t c) { return c != mAccumulated; }));
    if (stopped == 0u) mTileSamples.clear(); // every tile of the handle at its leading count: its per-tile reads take the ordinary form
    else mTileSamples = counts;
    return stopped;
}

uint32_t AccumulationBooks::settleFrameTileSamples(uint32_t leading, uint32_t minimum, uint32_t skipFrames)
{
    mFrameLeadingSamples = leading, mFrameMinTileSamples = minimum;
    mFrameCount += skipFrames;
    uint32_t below = 0;
    for (uint32_t k = 0; k < mShardTiles; ++k) below += tileCount(k) < leading ? 1u : 0u;
    return below;
}

// ---- the shared pieces of the refusals
void AccumulationBooks::requireOn(const std::string& what, Family f) const
{
    if (!on(f)) throw std::invalid_argument(what + " needs " + kWords[f].name + ": turn them on (" + kWords[f].hint + ") before the first sample");
}

// (a dirty family's count is 0 and a dirty image's accumulated count is 0 -- Sums -- so the counts print as they are)
void AccumulationBooks::requireCovers(const std::string& what, Family f) const
{
    if (!covers(f))
        throw std::invalid_argument(what + ": the " + kWords[f].count + " sample count (" + str(mSums[f].samples) + ") differs from the accumulated sample count (" +
                                    str(mAccumulated) + "): turn " + kWords[f].them + " on before the first sample");
}

void AccumulationBooks::requireCoversIfAny(const std::string& what, Family f) const
{
    if (!on(f) || mAccumulated == 0u || covers(f)) return;
    const std::string which = f == kMoments ? "the moments do not cover the accumulation (turned on partway through)"
                                            : std::string("the ") + kWords[f].count + " sample count does not cover the accumulation (" + kWords[f].them + " were turned on partway through)";
    throw std::invalid_argument(what + ": " + which + ": restart the accumulation first");
}

void AccumulationBooks::requireWholeFrame(const std::string& what, const char* instead) const
{
    if (mWorldSize != 1u) throw std::invalid_argument(what + " needs the whole frame: a tile shard is set" + instead);
}

void AccumulationBooks::requireSamples(const std::string& what) const
{
    if (mAccumulated == 0u) throw std::invalid_argument(what + ": no sample has been accumulated");
}

// the non-uniform state: a per-tile read divides each pixel by its tile's own count, which every family it reads must have been kept for, from the first sample on
void AccumulationBooks::requireKeptPerTile(const char* api, std::initializer_list<Family> families) const
{
    if (!nonUniform() || std::all_of(families.begin(), families.end(), [&](Family f) { return tileCounts(f) && covers(f); })) return;
    std::string names, words;
    for (const Family f : families)
    {
        names += std::string(names.empty() ? "" : " and ") + kWords[f].name;
        words += std::string(words.empty() ? "" : " and ") + kWords[f].perTile + " (" + kWords[f].hint + ")";
    }
    requireUniform(api, ", and " + names + " were not " + (families.size() > 1 ? "both " : "") + "kept with per-tile counts for the whole accumulation: set " + words +
                            " before the first sample and " + api + " runs in this state");
}

void AccumulationBooks::requireTileBit(Family f, const char* them) const
{
    if (on(f) && !tileCounts(f))
        throw std::invalid_argument(std::string("render_adaptive: ") + kWords[f].name + " are on (" + kWords[f].hint + "), and they keep ONE sample count for the frame: turn " +
                                    them + " off (" + kWords[f].hint + "(r, 0)) before sampling adaptively");
}

// ---- the refusals
void AccumulationBooks::refuseSetTileShard(uint32_t rank, uint32_t worldSize) const
{
    if (worldSize == 0 || rank >= worldSize) throw std::runtime_error("invalid tile shard");
    requireUniform("rf_renderer_set_tile_shard");
}

// The denoisers: the non-uniform state's refusal before any other, then each needed family on, the whole frame, a sample, each family covering
void AccumulationBooks::refuseDenoiseWith(const char* what, const char* api, bool uniformOtherwise, const char* instead, std::initializer_list<Family> perTile,
                                          std::initializer_list<Family> needed) const
{
    requireKeptPerTile(api, perTile);
    if (uniformOtherwise && !nonUniform()) requireUniform(api);
    for (const Family f : needed) requireOn(what, f);
    requireWholeFrame(what, instead);
    requireSamples(what);
    for (const Family f : needed) requireCovers(what, f);
}

void AccumulationBooks::refuseDenoise() const
{
    refuseDenoiseWith("denoise", "rf_renderer_denoise", false, " (use rf_denoise_images on the gathered sums)", {kAovs}, {kAovs});
}

void AccumulationBooks::refuseDenoiseSplit() const
{
    refuseDenoiseWith("denoise_split", "rf_renderer_denoise_split", true, " (use rf_denoise_split_images on the sum of the ranks' reads)", {kDirect, kAovs}, {kAovs, kDirect});
}

// rf_renderer_denoise's refusals, then the robust mean's
void AccumulationBooks::refuseDenoiseRobust() const
{
    refuseDenoiseWith("denoise_robust", "rf_renderer_denoise_robust", true, "", {kAovs}, {kAovs});
    refuseRobustMean();
}

void AccumulationBooks::refuseRobustMean() const
{
    const std::string what = "robust_mean";
    const uint32_t    K = buckets();
    // the non-uniform state: the planes follow the per-tile counts when the buckets carry kWordTileCounts (they were on before render_adaptive made the state)
    const bool perTile = bucketsPerTile();
    if (!perTile) requireUniform("rf_renderer_robust_mean");
    requireOn(what, kBuckets);
    requireWholeFrame(what, " (use rf_robust_mean_images on the sum of the ranks' bucket reads)");
    // (first: with nothing accumulated the counts agree, at 0, and there is still nothing to combine)
    if (mAccumulated < K) throw std::invalid_argument(what + ": every one of the " + str(K) + " buckets needs a sample, and only " + str(mAccumulated) + " are accumulated");
    requireCovers(what, kBuckets);
    // what the state adds on top: every bucket of every tile needs a sample
    if (perTile && leastOwnTile() < K)
        throw std::invalid_argument(what + ": every one of the " + str(K) + " buckets of every tile needs a sample, and the smallest tile count is " + str(leastOwnTile()) +
                                    " (sample adaptively with min_samples >= K)");
}

void AccumulationBooks::refuseNoiseEstimate() const
{
    requireOn("the noise estimate", kMoments);
    requireWholeFrame("the noise estimate", " (use rf_noise_estimate_images on the ranks' sums)");
    requireCovers("noise estimate", kMoments);
    if (mAccumulated < 2u) throw std::invalid_argument("noise estimate: a variance needs at least 2 accumulated samples");
}

void AccumulationBooks::refuseRenderUntil(uint32_t checkEvery) const
{
    requireOn("render_until", kMoments);
    requireUniform("rf_renderer_render_until"); // (first: under a tile shard this is the state rf_comm_render_adaptive left)
    requireWholeFrame("render_until");
    if (checkEvery == 0u) throw std::invalid_argument("render_until: check_every must be >= 1");
    requireCoversIfAny("render_until", kMoments);
}

// render_adaptive in two halves, the switches and the arguments: rf_renderer_render_adaptive refuses a tile shard between them
void AccumulationBooks::refuseAdaptiveSwitches(bool sharded) const
{
    requireTileBit(kDirect, "them");
    if (tileCounts(kBuckets) && sharded && !shardTileCounts(kBuckets))
        throw std::invalid_argument("render_adaptive: the bucket sums are on (rf_renderer_set_buckets), and RF_BUCKETS_TILE_COUNTS covers rf_renderer_render_adaptive only: "
                                    "bucket planes under a tile shard are not kept per tile count; turn the buckets off (rf_renderer_set_buckets(r, 0)) first");
    requireTileBit(kBuckets, "the buckets");
    requireOn("render_adaptive", kMoments);
    if (on(kAovs) && !tileCounts(kAovs))
        throw std::invalid_argument("render_adaptive: the first-hit AOVs are on without RF_AOV_TILE_COUNTS (their sums and the denoiser then keep ONE sample count): set "
                                    "RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS before the first sample, or turn the AOVs off");
}

void AccumulationBooks::refuseAdaptiveArguments(uint32_t checkEvery, float targetTileError) const
{
    if (checkEvery == 0u) throw std::invalid_argument("render_adaptive: check_every must be >= 1");
    if (!std::isfinite(targetTileError) || targetTileError < 0.0f) throw std::invalid_argument("render_adaptive: target_tile_error must be finite and >= 0");
    for (const Family f : {kMoments, kAovs, kBuckets, kDirect}) requireCoversIfAny("render_adaptive", f);
}

void AccumulationBooks::refuseAdaptive(uint32_t checkEvery, float targetTileError, bool sharded) const
{
    refuseAdaptiveSwitches(sharded);
    refuseAdaptiveArguments(checkEvery, targetTileError);
}

// (the order of the checks, and so which message a call with several faults gets, is the one this call always had)
void AccumulationBooks::refuseRenderAdaptive(uint32_t checkEvery, float targetTileError) const
{
    refuseAdaptiveSwitches(false);
    requireWholeFrame("render_adaptive", " (rf_comm_render_adaptive samples a sharded frame adaptively)");
    refuseAdaptiveArguments(checkEvery, targetTileError);
}

void AccumulationBooks::refuseExportFeatures(uint32_t reads, bool twoSamples) const
{
    const std::string what = "export_features";
    requireWholeFrame(what, " (gather the frame -- rf_renderer_gather_frame -- and call rf_comm_export_features on the root)");
    requireSamples(what);
    // each selected channel's family: on, covering the accumulation and -- in the non-uniform state -- kept per tile count
    const std::pair<uint32_t, Family> selected[] = {{kFeatureReadsAovs, kAovs}, {kFeatureReadsD, kDirect}, {kFeatureReadsQ, kMoments}};
    for (const auto& [bit, f] : selected)
    {
        if (!(reads & bit)) continue;
        const std::string name = kWords[f].name;
        requireOn(what + ": a selected channel", f);
        if (!covers(f))
            throw std::invalid_argument(what + ": the sample count of " + name + " (" + str(mSums[f].samples) + ") differs from the accumulated sample count (" + str(mAccumulated) +
                                        "): turn them on before the first sample");
        if (nonUniform() && !tileCounts(f))
            requireUniform("rf_renderer_export_features", ", and " + name + " were not kept with per-tile counts (" + kWords[f].hint + " with the tile-count bit before the first sample)");
    }
    if (!twoSamples) return;
    if (mAccumulated < 2u) throw std::invalid_argument(what + ": RF_FEATURE_VARIANCE / RF_FEATURE_ERROR need at least 2 accumulated samples");
    if (nonUniform() && leastOwnTile() < 2u) throw std::invalid_argument(what + ": RF_FEATURE_VARIANCE / RF_FEATURE_ERROR need at least 2 samples in every tile");
}

void AccumulationBooks::refuseReadDenoised() const
{
    if (!mDenoised.valid) throw std::invalid_argument("no denoised image: call rf_renderer_denoise first (the image is dropped when the accumulation or the AOVs are cleared)");
}

void AccumulationBooks::refuseReadRobustMean() const
{
    if (!mRobust.valid) throw std::invalid_argument("no robust mean: call rf_renderer_robust_mean first (the image is dropped when the accumulation or the bucket sums are cleared)");
}

// The temporal history.  The count check is skipped while nothing is accumulated: the two counts then agree, at 0 (a family's count never exceeds the accumulated one),
// and "no sample" is the message.
void AccumulationBooks::refuseTemporalAccumulate(bool denoise) const
{
    const std::string what = denoise ? "denoise_temporal" : "temporal_accumulate";
    requireOn(what, kAovs);
    if (mAccumulated != 0u) requireCovers(what, kAovs);
    requireSamples(what);
    requireWholeFrame(what, " (use rf_temporal_images on the gathered sums)");
    requireUniform(denoise ? "rf_renderer_denoise_temporal" : "rf_renderer_temporal_accumulate");
}

void AccumulationBooks::refuseTemporalCommit() const
{
    if (!mTemporal.valid)
        throw std::invalid_argument("no temporal result to commit: call rf_renderer_temporal_accumulate first (the result is dropped when the accumulation or the AOVs are "
                                    "cleared, and a commit takes it)");
}

void AccumulationBooks::refuseReadTemporal() const
{
    if (!mTemporal.valid)
        throw std::invalid_argument("no temporal result: call rf_renderer_temporal_accumulate first (the result is dropped when the accumulation or the AOVs are cleared, "
                                    "and a commit takes it)");
}

void AccumulationBooks::requireShardRobustMean() const
{
    if (!on(kBuckets) || !covers(kBuckets) || mAccumulated < buckets()) throw std::logic_error("enqueueShardRobustMean: the bucket sums do not cover the accumulation");
}

void AccumulationBooks::requireSlotAddressing(bool shardSlots) const
{
    if (!shardSlots && mWorldSize != 1u) throw std::logic_error("a tile shard's sums are addressed by slot");
}

// ---- views
AccumulationBooks::Checkpoint AccumulationBooks::checkpoint() const
{
    Checkpoint c;
    c.frameCount = mFrameCount, c.accumulated = mAccumulated, c.frameLeadingSamples = mFrameLeadingSamples, c.frameMinTileSamples = mFrameMinTileSamples;
    for (uint32_t f = 0; f < kFamilies; ++f) c.word[f] = mSums[f].word, c.family[f] = {mSums[f].on, (!mSums[f].on || mSums[f].dirty) ? 0u : mSums[f].samples};
    c.tileSamples = tileCounts();
    return c;
}

void AccumulationBooks::adopt(const Checkpoint& c)
{
    if (c.tileSamples.size() != mShardTiles) throw std::logic_error("checkpointAdopt: one count per tile of the shard");
    mFrameCount = c.frameCount;
    mAccumulated = c.accumulated;
    mSums[kImage].samples = c.accumulated; // (the image keeps no count of its own)
    for (const Family f : kSwitched)
        if (mSums[f].on) mSums[f].samples = c.family[f].samples;
    settleTileSamples(c.tileSamples); // (stored only while they differ from the accumulated count)
    mFrameLeadingSamples = c.frameLeadingSamples, mFrameMinTileSamples = c.frameMinTileSamples;
}
} // namespace rf
