// rf_books.hpp -- the books of one handle's accumulation and the refusals that rest on them: which samples every sum holds, which tile holds how many, which
// snapshot is valid, and which call the handle turns down in which state, with which words.  Host only: no device memory, no HIP header, no HIP runtime call -- the unit
// links into a program without libamdhip64 (tests/books_main.cpp walks it against the handle model).  The renderer (rf_renderer.hip) keeps the storage half: the
// buffers, their sizing and zeroing, and every enqueue.
#pragma once

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

namespace rf
{
// One sum over the samples of an accumulation: on or off, its own sample count, and whether it holds exactly the accumulated samples (on from the first sample, at least
// one accumulated: what the frame gather requires before it sends the sum) -- Renderer::ShardSums::Channel
struct SumCoverage
{
    bool     on, coversAccumulation;
    uint32_t samples;
};
// ... and as a checkpoint carries it -- Renderer::CheckpointBooks::Family
struct SumCount
{
    bool     on;
    uint32_t samples; // 0: restarted (its read returns zeros)
};

class AccumulationBooks
{
public:
    // The five families of sums, in the checkpoint's order: the image S (always on), the first-hit AOV sums (two buffers), the radiance second moments Q, the direct
    // sums D, the K bucket planes.  The one enumeration of them: everything that concerns every family is a loop over it.
    enum Family : uint32_t
    {
        kImage,
        kAovs,
        kMoments,
        kDirect,
        kBuckets,
        kFamilies
    };
    // the words of the set calls share their layout: the low byte says whether the family is on (the buckets: K), the bits above it how it is kept
    static constexpr uint32_t kWordOn = 0xFFu, kWordTileCounts = 0x100u, kWordShardTileCounts = 0x400u, kMaxBuckets = 15u;

    // One family's books.  All of a family's sums are compact tile-major float4 buffers of the shard, summed in sample order.
    // What the driver relies on (restartAccumulation, the set calls, zeroed and recordStep are the only writers):
    //   * dirty is raised only together with samples = 0, and cleared only by the zeroing in front of the next sample: dirty implies samples == 0;
    //   * the image's dirty flag is raised only by restartAccumulation, which sets accumulated = 0 and restarts every family: a dirty image implies
    //     accumulated == 0 and every family dirty.  (A read may zero a dirty image and clear the flag before any sample: accumulated == 0 does not imply dirty);
    //   * hence covers() with accumulated != 0 says that the family was on for every sample of the accumulation, whatever the image's flag says.
    struct Sums
    {
        bool     on = false;
        bool     dirty = true; // restarted: to be zeroed before the next sample
        uint32_t samples = 0;  // samples summed since it was last restarted (the image: the accumulated count)
        uint32_t planes = 1;   // float4 per pixel in each buffer, plane after plane (the bucket sums: K)
        uint32_t word = 0;     // as the caller set it (rf_renderer_set_aovs / set_moments / set_direct / set_buckets)
    };
    // what a set call did: nothing, or the family's sums start again -- and the family is now off (the renderer synchronises and releases buffers, nothing more)
    enum class Change
    {
        Unchanged,
        Restarted,
        RestartedOff
    };

    AccumulationBooks();

    // ---- counters and shard
    uint32_t frameCount() const { return mFrameCount; }
    uint32_t accumulated() const { return mAccumulated; } // the leading count L
    uint32_t rank() const { return mRank; }
    uint32_t worldSize() const { return mWorldSize; }
    uint32_t shardTiles() const { return mShardTiles; }
    void     setSampleCap(uint32_t samplesPerPixel) { mSampleCap = samplesPerPixel; }
    void     setShard(uint32_t rank, uint32_t worldSize) { mRank = rank, mWorldSize = worldSize, mTemporalHistory = false; } // (refuseSetTileShard has passed; the temporal history goes)
    void     setShardTiles(uint32_t numTiles) { mShardTiles = numTiles; }                          // (the caller restarts the accumulation)
    // Tile-adaptive sampling.  The per-tile counts, by slot of the shard; EMPTY = the uniform state: every tile holds `accumulated` samples (the only state a handle that
    // never called render_adaptive is ever in).  Non-empty: the counts differ, `accumulated` is the leading count L, and the tiles still at L are the only ones a later
    // render_adaptive samples.  Cleared by restartAccumulation.
    bool                  nonUniform() const { return !mTileSamples.empty(); } // this handle's own tiles: which form its per-tile reads take
    // Under a tile shard (rf_comm_render_adaptive) the FRAME's largest and smallest tile count over all ranks, as the call's all-reduces left them on every rank: while
    // they differ the frame is non-uniform, on a rank whose own tiles share one count too.  Both 0: no such call since the accumulation was restarted.
    bool                  frameNonUniform() const { return mFrameLeadingSamples != mFrameMinTileSamples; }
    void                  requireUniform(const char* what, const std::string& unless = "") const;
    const std::vector<uint32_t>& tileSamples() const { return mTileSamples; }
    uint32_t              tileCount(size_t slot) const { return nonUniform() ? mTileSamples[slot] : mAccumulated; }
    std::vector<uint32_t> tileCounts() const; // one count per slot, the uniform state too
    uint32_t              minTileSamples() const; // the smallest tile count known to the rank (Renderer::ShardSums::minTileSamples)

    // ---- the table of families
    const Sums& sums(Family f) const { return mSums[f]; }
    bool        on(Family f) const { return mSums[f].on; }
    bool        covers(Family f) const { return !mSums[f].dirty && mSums[f].samples == mAccumulated; }
    bool        empty(Family f) const { return !mSums[f].on || mSums[f].dirty || mSums[f].samples == 0u; }
    uint32_t    readCount(Family f) const { return empty(f) ? 0u : mSums[f].samples; } // what the family's read reports
    bool        tileCounts(Family f) const;      // on, and kept per tile count under render_adaptive (the image and the moments always are)
    bool        shardTileCounts(Family f) const; // ... and under a tile shard too (kWordShardTileCounts)
    uint32_t    buckets() const { return on(kBuckets) ? mSums[kBuckets].planes : 0u; } // K
    bool        bucketsPerTile() const { return nonUniform() && !frameNonUniform() && tileCounts(kBuckets); }
    // before the first sample after a restart the renderer asks whether the family is stale, zeroes its buffers, and says so
    bool stale(Family f) const { return mSums[f].on && mSums[f].dirty; }
    void zeroed(Family f) { mSums[f].dirty = false; }

    // ---- snapshots: the denoised image (filtered with the AOV sums as guides, the split one from the direct sums too) and the robust mean (combined from the bucket
    // sums); each is dropped when a family it was made from restarts
    bool     denoisedValid() const { return mDenoised.valid; }
    bool     robustValid() const { return mRobust.valid; }
    uint32_t denoisedSamples() const { return mDenoised.samples; }
    uint32_t robustSamples() const { return mRobust.samples; }
    void     noteDenoised() { mDenoised = {true, mAccumulated}; } // (the snapshot's sample count is the leading count)
    void     noteRobustMean() { mRobust = {true, mAccumulated}; }
    // ... and the temporal result (rf_renderer_temporal_accumulate: the current view's sums blended with the reprojected history), tracked as the denoised image is and
    // dropped with the AOV sums; and the temporal HISTORY, which is not a snapshot of this accumulation: a commit makes the result the history (the result is then gone),
    // restartAccumulation leaves it -- that is its purpose --, and a new frame size (frameResized), a tile shard (setShard) and resetTemporal drop it.
    bool     temporalValid() const { return mTemporal.valid; }
    uint32_t temporalSamples() const { return mTemporal.samples; }
    bool     temporalHistory() const { return mTemporalHistory; }
    void     noteTemporal() { mTemporal = {true, mAccumulated}; }
    void     commitTemporal() { mTemporal.valid = false, mTemporalHistory = true; } // (refuseTemporalCommit has passed)
    void     resetTemporal() { mTemporal.valid = false, mTemporalHistory = false; }
    void     frameResized() { mTemporalHistory = false; } // (the caller restarts the accumulation)

    // ---- transitions
    // A new accumulation (new parameters, another shard, another accumulation buffer): no sample, every tile at the same count, every sum to be zeroed before the
    // next sample, no snapshot.  The frame counter stays.
    void   restartAccumulation();
    // The set calls: the word is checked (std::invalid_argument), then compared with the one in force; any change of the value restarts the family's sums, a change
    // of a "how" bit alone included.  setAovs takes the word as rf_renderer_set_aovs has checked it.
    Change setAovs(uint32_t word);
    Change setMoments(bool enabled);
    Change setDirect(uint32_t word);
    Change setBuckets(uint32_t word);
    // a batch of n samples has been enqueued: the frame counter, the accumulated count, and the count of every family that is on
    void     recordStep(uint32_t n);
    // rf_renderer_render: of `numFrames` frames still to go, how many to trace now.  0: none -- the accumulation is full or the shard holds no tile, and the rest of
    // them has moved the frame counter alone (reference_path_tracer.cpp:577-591: calls past spp only advance frameCount)
    uint32_t framesToTrace(uint32_t numFrames);
    // the adaptive loop: the counts by slot after a step (non-uniform from here on, should an estimate throw), and as the loop leaves them -- every tile of the handle
    // at its leading count: the ordinary form again.  -> the tiles below the leading count
    void     setTileSamples(const std::vector<uint32_t>& counts) { mTileSamples = counts; }
    uint32_t settleTileSamples(const std::vector<uint32_t>& counts);
    // what follows the loop under a shard (Renderer::settleFrameTileSamples) -> how many of the shard's tiles are below `leading`
    uint32_t settleFrameTileSamples(uint32_t leading, uint32_t minimum, uint32_t skipFrames);

    // ---- refusals, one per call; the order of the checks inside each is part of the interface (a call with several faults gets the message it always got), and so is
    // each exception's type (rf_c_api.cpp maps types to status codes)
    void refuseRender() const { requireUniform("rf_renderer_render"); }
    void refuseSetTileShard(uint32_t rank, uint32_t worldSize) const;
    void refuseDenoise() const;
    void refuseDenoiseSplit() const;
    void refuseDenoiseRobust() const;
    void refuseRobustMean() const;
    void refuseNoiseEstimate() const;
    void refuseRenderUntil(uint32_t checkEvery) const;
    // what rf_renderer_render_adaptive and rf_comm_render_adaptive check alike before anything is traced (or exchanged); sharded: the call is the latter's
    void refuseAdaptive(uint32_t checkEvery, float targetTileError, bool sharded) const;
    void refuseRenderAdaptive(uint32_t checkEvery, float targetTileError) const;
    // reads: kFeatureReads* of the selected channels (rf_feature_request.hpp); twoSamples: VARIANCE / ERROR are among them
    void refuseExportFeatures(uint32_t reads, bool twoSamples) const;
    void refuseReadDenoised() const;
    void refuseReadRobustMean() const;
    // the temporal history: the AOVs on, their count the accumulated count, a sample, the whole frame, the uniform state -- in that order; denoise: the call is
    // rf_renderer_denoise_temporal (whose second half, the denoiser's own refusals, these imply)
    void refuseTemporalAccumulate(bool denoise = false) const;
    void refuseTemporalCommit() const;
    void refuseReadTemporal() const;
    void requireShardRobustMean() const;               // Renderer::enqueueShardRobustMean: the caller has checked, so std::logic_error
    void requireSlotAddressing(bool shardSlots) const; // Renderer::renderAdaptiveFrom

    // ---- views
    SumCoverage shardChannel(Family f) const { return {on(f), on(f) && mAccumulated != 0u && covers(f), mSums[f].samples}; }
    struct Checkpoint
    {
        uint32_t              frameCount = 0, accumulated = 0, frameLeadingSamples = 0, frameMinTileSamples = 0;
        uint32_t              word[kFamilies] = {};
        SumCount              family[kFamilies] = {};
        std::vector<uint32_t> tileSamples; // one count per slot (the uniform state: the accumulated count)
    };
    Checkpoint checkpoint() const;
    // the books of a load whose planes lie in device memory and have been verified (the words are the handle's own: a load has set them through the set calls)
    void       adopt(const Checkpoint& c);

private:
    struct Snapshot
    {
        bool     valid = false;
        uint32_t samples = 0;
    };
    void     restart(Family f);
    uint32_t leastOwnTile() const { return *std::min_element(mTileSamples.begin(), mTileSamples.end()); } // (the non-uniform state)
    Change set(Family f, uint32_t word, uint32_t planes);
    // the shared pieces of the refusals
    void requireOn(const std::string& what, Family f) const;
    void requireCovers(const std::string& what, Family f) const;          // its count is the accumulated count
    void requireCoversIfAny(const std::string& what, Family f) const;     // ... unless nothing is accumulated yet
    void requireWholeFrame(const std::string& what, const char* instead = "") const;
    void requireSamples(const std::string& what) const;
    void requireKeptPerTile(const char* api, std::initializer_list<Family> families) const; // the non-uniform state: every one of them on, with its tile-count bit, covering
    void requireTileBit(Family f, const char* them) const;                // render_adaptive: a family that is on keeps ONE count without its bit
    void refuseAdaptiveSwitches(bool sharded) const;
    void refuseAdaptiveArguments(uint32_t checkEvery, float targetTileError) const;
    void refuseDenoiseWith(const char* what, const char* api, bool uniformOtherwise, const char* instead, std::initializer_list<Family> perTile,
                           std::initializer_list<Family> needed) const;

    uint32_t              mFrameCount = 0, mAccumulated = 0;
    uint32_t              mRank = 0, mWorldSize = 1, mShardTiles = 0, mSampleCap = 0;
    std::vector<uint32_t> mTileSamples;
    uint32_t              mFrameLeadingSamples = 0, mFrameMinTileSamples = 0;
    Sums                  mSums[kFamilies];
    Snapshot              mDenoised, mRobust, mTemporal;
    bool                  mTemporalHistory = false;
};
} // namespace rf
