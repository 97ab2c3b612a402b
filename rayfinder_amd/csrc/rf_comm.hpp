// rf_comm.hpp -- the multi-GPU frame exchange: one RCCL gather of tile shards at frame end + a device un-tile.
//
// No reference counterpart (the reference is single-device: src/pt/reference_path_tracer.cpp:565-595 draws one
// full-screen quad on one WGPUDevice).  Contract: the image is cut into 32x32
// tiles dealt to ranks by tilesForRank(); every rank renders its tiles into a compact tile-major float4 buffer;
// at frame end every rank sends that buffer to the root over RCCL (point-to-point ncclSend / ncclRecv in one
// group: all of the root's xGMI ingress links are used at once; no reduction, no ring), and the root turns the
// shards into the row-major width x height float4 image with one kernel.  One process (or host thread) per GPU.
// The same one group can carry the handle's other per-pixel sums (the first-hit AOV sums, the radiance second moments) as further PLANES, un-tiled by one kernel with
// the image; the root then denoises and estimates the gathered frame where it lies, in device memory (gatherPlanes, denoise, noiseEstimate below).
//
// Units: rf_comm.hip          the plans, TileComm (a gather as its steps, the un-tile kernels, the root-side calls) and the RCCL transport
//        rf_transport.hpp     what TileComm asks of a transport (internal)
//        rf_comm_local.cpp    the local test transport (RF_COMM_TRANSPORT=local)
//        rf_comm_sharded.cpp  gatherFrame / renderAdaptive below: a tile-sharded handle's calls over a communicator
#pragma once

#include "rf_renderer.hpp" // DenoiseParameters, NoiseEstimate

#include <cstdint>
#include <memory>
#include <vector>

namespace rf
{
constexpr uint32_t kCommIdBytes = 128; // NCCL_UNIQUE_ID_BYTES

// Where every tile of the frame lives in the root's staging area: shards are stored rank after rank, each
// rank's tiles in ascending tile id (the order of tilesForRank()).  Pure host arithmetic (tested on CPU).
struct GatherLayout
{
    uint32_t              tilesX = 0, tilesY = 0;
    std::vector<uint32_t> rankFirstTile; // world + 1 entries: staging offset of rank r's shard, in tiles
    std::vector<uint32_t> tileSlot;      // per tile id: staging position in tiles (rankFirstTile[owner] + index in the owner's list)
    std::vector<uint32_t> tileOwner;     // per tile id: owning rank
};
GatherLayout gatherLayout(uint32_t width, uint32_t height, uint32_t worldSize);

// The point-to-point operations ONE rank posts (inside one RCCL group) for a frame-end gather to `root`: what
// TileComm::gatherFrame() executes, as data.  Offsets and counts are in tiles (1024 float4 each): a receive lands
// at `offsetTiles` of the root's staging area, a send starts at `offsetTiles` (always 0) of the rank's own compact
// buffer.  Pure host arithmetic: the plan of every rank of a world can be checked without a GPU
// (tests/test_distributed_cpu.py: every send has its receive, the receives tile the staging area exactly).
struct GatherOp
{
    uint32_t isSend;      // 1: ncclSend to `peer`, 0: ncclRecv from `peer`
    uint32_t peer;
    uint32_t offsetTiles;
    uint32_t countTiles;
};
std::vector<GatherOp> gatherPlan(const GatherLayout& layout, uint32_t worldSize, uint32_t rank, uint32_t root, bool loopback);

// The sums a gather can carry, one PLANE each, in this fixed order: the image S, the first-hit AOV sums AC = {albedo.rgb, coverage} and ND = {normal.xyz, depth},
// the radiance second moments Q and, behind plane 4, the direct radiance sums D.  Every plane is a compact tile-major float4 buffer of the rank's shard, and has its own
// staging area (GatherLayout) and its own row-major image on the root.  A plane mask has bit p set for every carried plane; plane 0 always travels.
// Plane 4 is no sum: the robust mean of the rank's own pixels, {M.rgb, float(c)} (Renderer::enqueueShardRobustMean: the combine is per pixel, so every rank runs it over its
// own bucket planes BEFORE the exchange and one plane travels instead of K).  It is staged like the others; the root's un-tile splits it into a row-major {M.rgb, 1}
// image and a row-major uint8 trim image.  The SUM planes -- kPlaneIsSum: {0, 1, 2, 3, 5}, kSumPlanes of them -- are the ones readPlane / planeDevice serve and the one
// kUntilePlanes launch un-tiles; whoever asks "is p a sum plane" asks isSumPlane(p).
constexpr uint32_t kGatherPlanes = 6, kSumPlanes = 5;
constexpr uint32_t kPlaneImage = 0, kPlaneAlbedoCoverage = 1, kPlaneNormalDepth = 2, kPlaneMoments = 3, kPlaneRobustMean = 4, kPlaneDirect = 5;
constexpr bool     kPlaneIsSum[kGatherPlanes] = {true, true, true, true, false, true};
constexpr bool     isSumPlane(uint32_t plane) { return plane < kGatherPlanes && kPlaneIsSum[plane]; }
constexpr uint32_t kPlaneMaskImage = 1u << kPlaneImage, kPlaneMaskAovs = (1u << kPlaneAlbedoCoverage) | (1u << kPlaneNormalDepth), kPlaneMaskMoments = 1u << kPlaneMoments,
                   kPlaneMaskRobustMean = 1u << kPlaneRobustMean, kPlaneMaskDirect = 1u << kPlaneDirect;

// gatherPlan() once per carried plane, still ONE group: on the root, for each plane in order, the receives of that plane in rank order; on a sender, its sends in plane
// order -- so per (source, destination) pair the k-th send meets the k-th receive, which is what both RCCL's grouped point-to-point calls and the local transport's
// FIFO matching rely on.  offsetTiles counts from the start of THAT plane's staging area (receive) or compact buffer (send).  With planeMask == kPlaneMaskImage the
// list is gatherPlan()'s with plane = 0.  Plane 5 comes behind all of that as a whole -- its receives, then its send: the list with it is the list without it followed by
// gatherPlan()'s with plane = 5, and the pairing rule holds as before.  Pure host arithmetic (tests/test_gather_sums_api.py, tests/test_gather_direct_api.py).
struct GatherPlaneOp
{
    uint32_t isSend, peer, plane, offsetTiles, countTiles;
};
std::vector<GatherPlaneOp> gatherPlanPlanes(const GatherLayout& layout, uint32_t worldSize, uint32_t rank, uint32_t root, bool loopback, uint32_t planeMask);

// A gather can also carry the per-tile sample counts of the shards (tile-adaptive sampling across ranks): bit kGatherPlanes of the plane mask.  Every sender then sends,
// in the same one group and behind its planes, one uint32 per tile of its shard in slot order; the root stages them rank after rank.  gatherPlanCounts: those
// operations -- gatherPlan()'s with offsetTiles / countTiles counting uint32 WORDS of the count staging area (receive) or of the rank's count array (send).
constexpr uint32_t kGatherMaskTileCounts = 1u << kGatherPlanes;
std::vector<GatherOp> gatherPlanCounts(const GatherLayout& layout, uint32_t worldSize, uint32_t rank, uint32_t root, bool loopback);

// HIP devices this process sees (0 without a GPU or a driver; never throws)
int deviceCount();

class TileComm
{
public:
    // rank 0 calls uniqueId() and hands the 128 bytes to the other ranks through the host application's own
    // channel (file, socket, torch.distributed store ...); then every rank constructs its TileComm (collective).
    static void uniqueId(uint8_t out[kCommIdBytes]);
    TileComm(const uint8_t id[kCommIdBytes], uint32_t rank, uint32_t worldSize, int deviceOrdinal);
    ~TileComm();
    TileComm(const TileComm&) = delete;
    TileComm& operator=(const TileComm&) = delete;

    uint32_t rank() const;
    uint32_t worldSize() const;
    int      deviceOrdinal() const;
    // What RCCL itself reports for this communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): proof of how
    // many ranks the exchange really spans.
    void rcclInfo(uint32_t& count, uint32_t& userRank, int& device) const;
    // true: this communicator runs on the LOCAL test transport (RF_COMM_TRANSPORT=local when its id was made: N ranks in one process, one host thread each,
    // every send / receive pair a device-to-device copy -- the same plan, staging offsets and un-tile; rf_comm_local.cpp), not on RCCL
    bool localTransport() const;

    // Frame-end exchange, enqueued on `stream` (a hipStream_t: the renderer's, so the exchange is ordered behind
    // the frame's kernels).  compactDevice: this rank's tile-major buffer (tilesForRank(...).size() * 1024 float4).
    // On the root the row-major width * height float4 image is produced in device memory owned by this object
    // (returned; valid until the next gather); other ranks get nullptr.  loopback: the root's own shard also
    // travels through ncclSend / ncclRecv (to itself) instead of being read in place -- the world-size-1 self-test.
    const void* gatherFrame(const void* compactDevice, uint32_t width, uint32_t height, uint32_t root, void* stream, bool loopback = false);
    // The same exchange carrying every plane of planeMask (plane 0 included) in the one group: compactDevice[p] is this rank's tile-major buffer of plane p (unused
    // entries ignored).  The root stages each plane in its own area of one allocation and un-tiles them all with ONE kernel (kUntilePlanes) into one row-major image per
    // plane; -> the image of plane 0 on the root, nullptr elsewhere.  planeMask == kPlaneMaskImage enqueues exactly what gatherFrame() enqueues.  `samples`: the sample
    // count N of the sums, recorded on the root for denoise() / noiseEstimate().  Every gather replaces the record of the one before (planes, frame size, N) and drops
    // the denoised snapshot.
    // planeMask & kGatherMaskTileCounts: tileCountsDevice, this rank's per-tile sample counts in slot order (device memory, one uint32 per tile of the shard), travels too;
    // the root assembles one count per tile of the frame (kUntileCounts), waits for the exchange, and records N = the largest count instead of `samples`.
    // planeMask & kPlaneMaskRobustMean: compactDevice[4] is the rank's {M.rgb, float(c)} buffer; it is un-tiled by a launch of its own (kUntileRobust) behind the one of
    // the sum planes, and `robustK` -- the K of the combine -- is recorded on the root for readRobustMean().
    // planeMask & kPlaneMaskDirect: compactDevice[5] is the rank's D; it travels behind plane 4 and is un-tiled with the other sum planes, one more blockIdx.y of their launch.
    const void* gatherPlanes(const void* const compactDevice[kGatherPlanes], uint32_t planeMask, uint32_t samples, uint32_t width, uint32_t height, uint32_t root, void* stream,
                             bool loopback = false, const uint32_t* tileCountsDevice = nullptr, uint32_t robustK = 0);
    // Device time of the LAST gatherFrame() on the caller's stream, HIP events around it: from the moment the rank's queued frame kernels have drained and the
    // exchange starts to the end of its sends / receives (+ the un-tile on the root).  Waits for that exchange; -1 before the first one.
    double lastExchangeMs();
    // Root: wait for the stream and copy the gathered image to the host (width * height * 4 floats, row-major).
    void readFrame(float* dstHost, void* stream);

    // ---- the root's side of the last gather.  Each of these throws std::invalid_argument that says which case applies when this rank was not the root of the last
    // gather, when no gather has been made, or when the last gather did not carry the planes the call needs.
    // What the last gather left on this rank: the carried planes, the frame size and N.
    void gatheredPlanes(uint32_t& planeMask, uint32_t& width, uint32_t& height, uint32_t& samples) const;
    // The row-major width * height float4 image of plane `plane` in device memory (owned by this object; valid until the next gather)
    const void* planeDevice(uint32_t plane) const;
    // Wait for the stream and copy that image to the host (width * height * 4 floats)
    void readPlane(uint32_t plane, float* dstHost, void* stream);
    // The a-trous denoiser (rf_denoise.hpp: enqueueDenoise, row-major, N) over the gathered planes 0, 1, 2 where they lie, enqueued on `stream`; the snapshot lives in a
    // DenoiseWork of this object until the next gather.  Needs kPlaneMaskAovs.
    void denoise(const DenoiseParameters& params, float exposure, void* stream);
    void readDenoised(float* rgba, uint32_t* bgra8, uint32_t* sampleCount, void* stream);
    // The noise estimate (rf_noise.hpp: runNoiseEstimate, row-major, N) over the gathered planes 0 and 3; enqueued on `stream`, then waited for.  Needs kPlaneMaskMoments and N >= 2.
    NoiseEstimate noiseEstimate(float* errorMap, float* tileSum, float* tileMax, void* stream);
    // After a gather with kGatherMaskTileCounts, denoise() and noiseEstimate() take each tile's own count (every count >= 1 / >= 2), and:
    // the gathered counts, one per tile of the frame (tileSamples may be nullptr) -> the number of tiles
    uint32_t readTileSamples(uint32_t* tileSamples) const;
    // row-major width * height * 4 floats {S.rgb / float(the tile's count), 1}, {0, 0, 0, 1} in a tile without a sample; enqueued on `stream`, then waited for
    void readMean(float* rgba, void* stream);
    // After a gather with kPlaneMaskRobustMean: the gathered robust mean as the gather left it (row-major width * height: 4 floats {M.rgb, 1}, BGRA8 texels -- kTonemap
    // over M with accumulatedSamples = 1 and `exposure`, enqueued on `stream` --, one trim byte; any pointer may be nullptr), the K of the combine and N.  Waits for the stream.
    void readRobustMean(float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* K, uint32_t* sampleCount, float exposure, void* stream);
    // denoise() with prep's colour = the gathered M instead of S / N (Renderer::denoiseRobust's filter over row-major planes); needs kPlaneMaskAovs | kPlaneMaskRobustMean.
    // The snapshot is denoise()'s: readDenoised.
    void denoiseRobust(const DenoiseParameters& params, float exposure, void* stream);
    // After a gather with kPlaneMaskDirect: the split-component filter (rf_denoise.hpp: enqueueDenoiseSplit, row-major) over the gathered S, D, AC and ND where they lie, per
    // tile count when the counts travelled; needs kPlaneMaskAovs | kPlaneMaskDirect.  The snapshot is denoise()'s: readDenoised.
    void denoiseSplit(const DenoiseParameters& direct, const DenoiseParameters& indirect, float exposure, void* stream);
    // The two components of the gathered frame, row-major width * height * 4 floats each (either may be nullptr, not both): direct = {D.rgb / float(n), 1} and
    // indirect = {(S.rgb - D.rgb) / float(n), 1}, n = N or, gathered with the counts, the pixel's tile's count ({0, 0, 0, 1} for both in a tile without a sample: readMean's
    // rule; without the counts N = 0 is refused).  One kernel (rf_noise.hpp: enqueueSplitMeanRows) on `stream`, then waited for.  Needs kPlaneMaskDirect.
    void readSplit(float* directRgba, float* indirectRgba, void* stream);
    // The feature export (rf_features.hpp; the definition: include/rayfinder_amd.h) over the gathered row-major planes 0 .. 3 and 5 where they lie, per tile count when the
    // counts travelled: into `dstDevice` (caller-owned memory of this device), enqueued on `stream`, then waited for; -> N.  Needs the planes the request's channels read;
    // VARIANCE / ERROR need every count >= 2.
    uint32_t exportFeatures(const FeatureRequest& request, void* dstDevice, uint64_t dstBytes, void* stream);
    // Max over ranks of a host double / barrier (timing plumbing for callers that have no other collective layer).
    double allReduceMax(double value, void* stream);

private:
    struct Impl;
    std::unique_ptr<Impl> mImpl;
};

// ---- a tile-sharded handle's calls over its communicator (rf_renderer_gather_frame, rf_comm_render_adaptive).  Every refusal (std::invalid_argument) comes before
// the first collective: a refused rank leaves no peer waiting as long as the ranks pass the same arguments.
// The frame-end gather of the handle's sums on its own stream; `flags`: RF_GATHER_* (include/rayfinder_amd.h).  -> the root's image (plane 0), nullptr elsewhere
const void* gatherFrame(Renderer& handle, TileComm& comm, uint32_t root, uint32_t flags);
// Tile-adaptive sampling of the sharded frame: Renderer::renderAdaptiveFrom on every rank from the frame's leading count, then the frame's figures, the same on every rank
struct ShardedAdaptiveResult
{
    AdaptiveResult rank; // this rank's tiles; stoppedTiles: those below the FRAME's leading count
    uint32_t       frameLeadingSamples = 0, frameMinTileSamples = 0;
    uint64_t       maxRankPixelSamples = 0; // the pixel samples traced by the busiest rank
};
ShardedAdaptiveResult renderAdaptive(Renderer& handle, TileComm& comm, const AdaptiveParameters& params);
} // namespace rf
