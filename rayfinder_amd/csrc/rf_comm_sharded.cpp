// rf_comm_sharded.cpp -- a tile-sharded handle's calls over its communicator (rf_comm.hpp: gatherFrame, renderAdaptive).  Host code only.
#include "../../include/rayfinder_amd.h" // RF_GATHER_*

#include "rf_comm.hpp"

#include <stdexcept>
#include <string>

namespace rf
{
namespace
{
void require(bool cond, const char* what)
{
    if (!cond) throw std::invalid_argument(what);
}

// the handle's shard is the communicator's rank, and the exchange is enqueued on the handle's stream with the communicator's device current: they must be one device
void requireOneRank(const Renderer& h, const TileComm& comm)
{
    require(h.shardRank() == comm.rank() && h.shardWorldSize() == comm.worldSize(),
            "the renderer's tile shard differs from the communicator's rank / world size (call rf_renderer_set_tile_shard first)");
    require(h.deviceOrdinal() == comm.deviceOrdinal(), "the renderer and the communicator are on different devices");
}
} // namespace

const void* gatherFrame(Renderer& h, TileComm& comm, uint32_t root, uint32_t flags)
{
    require(root < comm.worldSize(), "gather root out of range");
    requireOneRank(h, comm);
    if (!(flags & RF_GATHER_TILE_COUNTS)) h.requireUniformTileSamples("rf_renderer_gather_frame"); // (such an exchange carries no per-tile counts)
    // ... and the robust mean is combined with ONE count whatever else travels: a whole-frame handle (world size 1) can be in the non-uniform state with its bucket
    // planes kept per tile count (RF_BUCKETS_TILE_COUNTS, rf_renderer_render_adaptive), and the accumulated count is then only the leading tiles' -- unless the buckets
    // carry RF_BUCKETS_SHARD_TILE_COUNTS: the rank's combine then takes one count per slot, the counts the gather sends (the flag is there: checked above)
    const Renderer::ShardSums s = h.shardSums();
    const bool                robustPerSlot = (flags & RF_GATHER_ROBUST_MEAN) && !h.tileSamplesUniform();
    if (robustPerSlot && !s.bucketsShardTileCounts)
        throw std::invalid_argument("rf_renderer_gather_frame: RF_GATHER_ROBUST_MEAN: the tiles hold different sample counts after rf_renderer_render_adaptive, and the gathered "
                                    "robust mean is combined with ONE count for the frame (rf_renderer_robust_mean combines a whole-frame handle per tile count; or restart "
                                    "the accumulation with rf_renderer_set_render_parameters)");
    // the extra planes: a sum travels only when it holds exactly the accumulated samples (a rank whose shard has no tile has nothing to send and nothing to check
    // but the switch).  Refused before anything is enqueued or cleared.
    uint32_t                  planeMask = kPlaneMaskImage;
    const auto                differs = [&](const char* flag, const char* count, uint32_t samples, const char* name) {
        return std::invalid_argument(std::string("rf_renderer_gather_frame: ") + flag + ": the " + count + " sample count (" + std::to_string(samples) +
                                     ") differs from the accumulated sample count (" + std::to_string(s.accumulated) + "): turn the " + name + " on before the first sample");
    };
    if (flags & RF_GATHER_AOVS)
    {
        require(s.aovs.on, "rf_renderer_gather_frame: RF_GATHER_AOVS needs the first-hit AOVs: turn them on (rf_renderer_set_aovs) before the first sample");
        require(!s.ownsTiles || s.accumulated != 0u, "rf_renderer_gather_frame: RF_GATHER_AOVS: no sample has been accumulated");
        if (s.ownsTiles && !s.aovs.coversAccumulation) throw differs("RF_GATHER_AOVS", "AOV", s.aovs.samples, "AOVs");
        planeMask |= kPlaneMaskAovs;
    }
    if (flags & RF_GATHER_MOMENTS)
    {
        require(s.moments.on, "rf_renderer_gather_frame: RF_GATHER_MOMENTS needs the radiance second moments: turn them on (rf_renderer_set_moments) before the first sample");
        require(!s.ownsTiles || s.accumulated != 0u, "rf_renderer_gather_frame: RF_GATHER_MOMENTS: no sample has been accumulated");
        if (s.ownsTiles && !s.moments.coversAccumulation) throw differs("RF_GATHER_MOMENTS", "moment", s.moments.samples, "moments");
        planeMask |= kPlaneMaskMoments;
    }
    // the robust mean: the buckets must cover the accumulation, and every bucket needs a sample (N >= K) -- in the non-uniform state (refused above without
    // RF_BUCKETS_SHARD_TILE_COUNTS) every bucket of every tile: the smallest count the rank knows of, after rf_comm_render_adaptive the FRAME's, which every rank holds
    // -- one without a tile too --, so that all ranks are refused alike and no peer waits for an exchange
    if (flags & RF_GATHER_ROBUST_MEAN)
    {
        require(s.buckets.on, "rf_renderer_gather_frame: RF_GATHER_ROBUST_MEAN needs the bucket sums: turn them on (rf_renderer_set_buckets) before the first sample");
        require(!s.ownsTiles || s.accumulated != 0u, "rf_renderer_gather_frame: RF_GATHER_ROBUST_MEAN: no sample has been accumulated");
        if (s.ownsTiles && !s.buckets.coversAccumulation) throw differs("RF_GATHER_ROBUST_MEAN", "bucket", s.buckets.samples, "buckets");
        if (s.ownsTiles && s.accumulated < s.bucketsK)
            throw std::invalid_argument("rf_renderer_gather_frame: RF_GATHER_ROBUST_MEAN: every one of the " + std::to_string(s.bucketsK) + " buckets needs a sample, and only " +
                                        std::to_string(s.accumulated) + " are accumulated");
        if (robustPerSlot && s.minTileSamples < s.bucketsK)
            throw std::invalid_argument("rf_renderer_gather_frame: RF_GATHER_ROBUST_MEAN: every one of the " + std::to_string(s.bucketsK) +
                                        " buckets of every tile needs a sample, and the smallest tile count is " + std::to_string(s.minTileSamples) +
                                        " (sample adaptively with min_samples >= K)");
        planeMask |= kPlaneMaskRobustMean;
    }
    // the direct sums, a sum plane like the AOVs' and the moments'; in the non-uniform state (the counts travel: checked above) D must have been kept per tile count
    if (flags & RF_GATHER_DIRECT)
    {
        require(s.direct.on, "rf_renderer_gather_frame: RF_GATHER_DIRECT needs the direct sums: turn them on (rf_renderer_set_direct) before the first sample");
        require(!s.ownsTiles || s.accumulated != 0u, "rf_renderer_gather_frame: RF_GATHER_DIRECT: no sample has been accumulated");
        if (s.ownsTiles && !s.direct.coversAccumulation) throw differs("RF_GATHER_DIRECT", "direct", s.direct.samples, "direct sums");
        require(h.tileSamplesUniform() || s.directTileCounts,
                "rf_renderer_gather_frame: RF_GATHER_DIRECT: the tiles hold different sample counts, and the direct sums were not kept per tile count: set "
                "1 | RF_DIRECT_TILE_COUNTS (rf_renderer_set_direct) before the first sample");
        planeMask |= kPlaneMaskDirect;
    }
    h.clearAccumulationIfStale(); // nothing rendered since the last reset: send zeros, not the previous frame
    // the shard's per-tile counts, in slot order, from device memory (the ordinary state: every tile at the accumulated count)
    const uint32_t* counts = nullptr;
    if (flags & RF_GATHER_TILE_COUNTS) planeMask |= kGatherMaskTileCounts, counts = h.shardTileSamplesDevice();
    // every check of the handle's state is behind us: the rank's own combine goes onto the handle's stream in front of the exchange, and its output travels as plane 4.
    // (The communicator's own checks -- an aborted transport, the plane mask, a null buffer: gatherPlanes -- follow it, as they follow the clearing above; a gather
    // they refuse has written the handle's own plane-4 buffer and nothing else.)
    const void* planes[kGatherPlanes] = {s.planes[0], s.planes[1], s.planes[2], s.planes[3], nullptr, s.directPlane};
    if (flags & RF_GATHER_ROBUST_MEAN) planes[kPlaneRobustMean] = h.enqueueShardRobustMean(robustPerSlot ? counts : nullptr);
    return comm.gatherPlanes(planes, planeMask, s.accumulated, h.width(), h.height(), root, h.streamHandle(), (flags & RF_GATHER_LOOPBACK) != 0, counts, s.bucketsK);
}

ShardedAdaptiveResult renderAdaptive(Renderer& h, TileComm& comm, const AdaptiveParameters& p)
{
    h.checkAdaptive(p, true);
    requireOneRank(h, comm);
    void* const stream = h.streamHandle();
    // the frame's leading count: the largest accumulated count of any rank.  From here the loop is this rank's own: a tile's stop reads its own sums alone
    const uint32_t        leading = static_cast<uint32_t>(comm.allReduceMax(static_cast<double>(h.accumulatedSampleCount()), stream));
    ShardedAdaptiveResult out;
    AdaptiveResult&       a = out.rank = h.renderAdaptiveFrom(p, leading, true);
    // the frame's figures (exact in a double; a minimum as the maximum of the negated value; a rank without a tile has no minimum to offer)
    const double noTile = -4294967296.0;
    out.frameLeadingSamples = static_cast<uint32_t>(comm.allReduceMax(a.tiles ? static_cast<double>(a.maxTileSamples) : 0.0, stream));
    out.frameMinTileSamples = static_cast<uint32_t>(-comm.allReduceMax(a.tiles ? -static_cast<double>(a.minTileSamples) : noTile, stream));
    out.maxRankPixelSamples = static_cast<uint64_t>(comm.allReduceMax(static_cast<double>(a.tracedPixelSamples), stream));
    // the frame's leading tiles moved the frame counter of the ranks that hold them by frameLeading - leading; a rank that stopped earlier, or never started, follows
    a.stoppedTiles = h.settleFrameTileSamples(out.frameLeadingSamples, out.frameMinTileSamples, out.frameLeadingSamples - leading - a.framesTraced);
    return out;
}
} // namespace rf
