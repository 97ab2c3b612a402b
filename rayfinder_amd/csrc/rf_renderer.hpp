// rf_renderer.hpp -- host interface of the MI355X wavefront path tracer.
//
// Mirrors the reference's renderer seam (src/pt/reference_path_tracer.hpp:26-76):
//   ReferencePathTracer(desc, gpu, scene)  -> Renderer(desc, scene)      copies the scene to HBM
//   setRenderParameters(params)            -> setRenderParameters        resets accumulation on change
//   render(...)  (one sample per call)     -> render(numFrames)          n calls without host sync
//   averageRenderpassDurationMs()          -> averageRenderpassDurationMs (30-deep moving average)
//   renderProgressPercentage()             -> renderProgressPercentage
// plus what an offline renderer needs and the reference never exposed: read-back of the float
// accumulation buffer, the tonemapped image, per-kernel statistics, tile sharding for multi-GPU,
// and the bvh-visualizer node-visit pass (src/bvh-visualizer/main.cpp:60-78) on the GPU.
#pragma once

#include "rf_books.hpp" // SumCoverage, SumCount
#include "rf_bvh.hpp" // SceneView
#include "rf_ray_query_request.hpp"
#include "rf_sky.hpp"
#include "rf_types.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <memory>
#include <span>
#include <string>
#include <vector>

struct rf_launch_plan; // include/rayfinder_amd.h

namespace rf
{
struct FeatureRequest; // rf_feature_request.hpp

struct SamplingParams
{
    uint32_t numSamplesPerPixel = 128;
    uint32_t numBounces = 4;
    bool     operator==(const SamplingParams&) const = default;
};

struct RenderParameters
{
    uint32_t       width = 0, height = 0;
    Camera         camera{};
    SamplingParams samplingParams;
    Sky            sky;
    float          exposure = 1.0f;
};
bool operator==(const RenderParameters& a, const RenderParameters& b);

struct RendererDescriptor
{
    RenderParameters renderParams;
    uint32_t         maxWidth = 0, maxHeight = 0;
    int              deviceOrdinal = 0;
    // Paths kept in flight per batch (several samples of every pixel are traced together so that
    // deep bounces still fill the chip). 0 = default (about 8M).
    uint64_t maxPathsInFlight = 0;
};

// Ray/traversal statistics since the last resetStats().  Node visits and triangle tests are only
// counted while counting is enabled (it selects the counting build of the traversal kernels).
struct RenderStats
{
    uint64_t primaryRays = 0, closestRays = 0, shadowRays = 0;
    uint64_t closestNodeVisits = 0, closestTriangleTests = 0;
    uint64_t shadowNodeVisits = 0, shadowTriangleTests = 0;
    uint64_t paths = 0;
    uint32_t stackHighWater = 0;
    // batch depth actually used (round 6): samples of every pixel traced together in the MOST RECENT batch, paths in it, and batches traced since the last reset.  A render call
    // that does not get the configured depth (device memory short: another handle, a co-tenant) traces the same samples in more, shallower batches -- same image, shorter
    // launches: a loss of speed that used to be said on stderr only
    uint32_t batchSamplesUsed = 0, batchesTraced = 0;
    uint64_t batchPathsUsed = 0;
    uint64_t closestRecordFetches = 0, shadowRecordFetches = 0; // 64-B BVH records fetched (counting build)
    uint64_t abandonedRays = 0;  // rays whose traversal stack outgrew 96 entries (reference: undefined past 32); every build
    uint64_t scalarRedoRays = 0; // rays redone by the reference-ordered scalar traversal (irregular rays, LDS stack overflow); every build
    uint64_t primaryListRays = 0;     // bounce-1 rays of the batches whose primary launch ran over the per-pixel leaf lists (rf_primary_lists.hip); 0: every batch kept the kTraceWide launch
    uint64_t primaryFallbackRays = 0; // of those: handed on to the kTraceWide launch (a pixel without a list, a ray that is not class A)
    uint64_t primaryFusedRays = 0;    // ... of the batches that generated, intersected and shaded them in one kernel (kPrimaryFused); 0: every batch kept kRaygen, kTraceLeafLists and kShade
    uint64_t shadowRaysSelfAnswered = 0; // of shadowRays: stopped by the triangle they start on, found by kShade's own test (kShadeSelfShadow); never queued for an any-hit launch
    uint64_t shadowRaysHintAnswered = 0; // of shadowRays: answered by kShadowHint at the leaf the occluder grid named (never entered the traversal); every build
    // hipEvent-timed kernel time (ms) and launch counts, per kernel class, while timing is enabled
    double   msRaygen = 0, msClosest = 0, msShade = 0, msShadow = 0, msAccumulate = 0;
    uint32_t launchesRaygen = 0, launchesClosest = 0, launchesShade = 0, launchesShadow = 0, launchesAccumulate = 0;
    // per bounce (index b = bounce b+1; bounces past kMaxBounceStats are folded into the last entry):
    // queue occupancy = rays traced, and kernel time while timing is enabled
    static constexpr uint32_t kMaxBounceStats = 32;
    uint64_t closestRaysByBounce[kMaxBounceStats] = {}, shadowRaysByBounce[kMaxBounceStats] = {};
    double   msClosestByBounce[kMaxBounceStats] = {}, msShadowByBounce[kMaxBounceStats] = {};
};

constexpr uint32_t kTileSize = 32; // shard tile edge in pixels (32x32 = 16 waves of 8x8 pixels)

// The grid of kTileSize x kTileSize tiles over a width x height frame: tile t = tile_y * tilesX + tile_x; the last column and the last row may reach past the frame.
// The one place that knows the tile arithmetic of the host code (the kernels' own: rf_kernels.hpp).
struct TileGrid
{
    uint32_t width, height, tilesX, tilesY;
    TileGrid(uint32_t w, uint32_t h) : width(w), height(h), tilesX((w + kTileSize - 1) / kTileSize), tilesY((h + kTileSize - 1) / kTileSize) {}
    uint32_t count() const { return tilesX * tilesY; }
    uint32_t pixelsInFrame(uint32_t tile) const
    {
        const uint32_t x0 = (tile % tilesX) * kTileSize, y0 = (tile / tilesX) * kTileSize;
        return std::min(kTileSize, width - x0) * std::min(kTileSize, height - y0);
    }
    // before[i] = the in-frame pixels of tiles[0 .. i) (tiles.size() + 1 entries: kRaygen's queue positions, FrameParams::tileValidBefore) and their total
    struct Prefix
    {
        std::vector<uint32_t> before;
        uint64_t              total = 0;
    };
    Prefix validPrefix(std::span<const uint32_t> tiles) const
    {
        Prefix p;
        p.before.reserve(tiles.size() + 1);
        for (const uint32_t t : tiles)
        {
            p.before.push_back(static_cast<uint32_t>(p.total));
            p.total += pixelsInFrame(t);
        }
        p.before.push_back(static_cast<uint32_t>(p.total));
        return p;
    }
};

// Deterministic tile -> rank assignment (tiles along a Z-order curve dealt round-robin: equal counts +-1, every compact block of the image split over all ranks).
std::vector<uint32_t> tilesForRank(uint32_t width, uint32_t height, uint32_t rank, uint32_t worldSize);
// compact tile-major float4 buffer -> row-major width*height*4 image (pixels of other ranks' tiles untouched)
void untileHost(const float* compact, const uint32_t* tileIds, uint32_t numTiles, uint32_t width, uint32_t height, float* image);
// the same for texels of any size (float4 sums: 16 bytes, BGRA8: 4)
void untileHostTexels(const void* compact, const uint32_t* tileIds, uint32_t numTiles, uint32_t width, uint32_t height, size_t texelBytes, void* image);

// Edge-aware a-trous denoiser (rf_denoise.hip): iterations 0..8, every sigma finite and > 0 (the C ABI checks them before any device call)
struct DenoiseParameters
{
    uint32_t iterations = 5;
    float    sigmaColor = 1.0f, sigmaNormal = 0.1f, sigmaDepth = 0.1f;
};
// The denoiser over host-assembled row-major width*height*4 sums ({color, -}, {albedo, coverage}, {normal, depth}) of `samples` samples, on device
// `deviceOrdinal`: the mean RGBA (.w = 1) and / or its BGRA8 under `exposure` (NULL = skip).  Synchronous; allocates and frees its own device memory.
void denoiseImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* albedoCoverage, const float* normalDepth,
                   const DenoiseParameters& params, float exposure, float* outRgba, uint32_t* outBgra8);
// The same with one sample count per tile of the 32 x 32 grid (tileSamples[t] > 0, tile t = tile_y * ceil(width / 32) + tile_x): prep's Nf = float(tileSamples[t]) for
// the pixels of tile t.  tileSamples == nullptr: `samples` for every tile.
void denoiseTiles(int deviceOrdinal, uint32_t width, uint32_t height, const uint32_t* tileSamples, uint32_t samples, const float* colorSum, const float* albedoCoverage,
                  const float* normalDepth, const DenoiseParameters& params, float exposure, float* outRgba, uint32_t* outBgra8);

// The split-component denoiser over host-assembled row-major sums: colorSum = S, directSum = D (the layout of S), the rest as denoiseImages.  Synchronous.
struct SplitDenoiseDefaults
{
    DenoiseParameters direct, indirect;
};
SplitDenoiseDefaults splitDenoiseDefaults();
void denoiseSplitImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* directSum, const float* albedoCoverage,
                        const float* normalDepth, const DenoiseParameters& direct, const DenoiseParameters& indirect, float exposure, float* outRgba, uint32_t* outBgra8);
// The same with one sample count per tile of the 32 x 32 grid (tileSamples[t] > 0, as denoiseTiles takes them): prep's Nf = float(tileSamples[t]) for S, D and the AOV
// sums of the pixels of tile t.  tileSamples == nullptr: `samples` for every tile.
void denoiseSplitTiles(int deviceOrdinal, uint32_t width, uint32_t height, const uint32_t* tileSamples, uint32_t samples, const float* colorSum, const float* directSum,
                       const float* albedoCoverage, const float* normalDepth, const DenoiseParameters& direct, const DenoiseParameters& indirect, float exposure,
                       float* outRgba, uint32_t* outBgra8);

// The feature export (rf_features.hip; the definition: include/rayfinder_amd.h) over host-assembled row-major width*height*4 sums (NULL where no selected channel reads
// them) on device `deviceOrdinal`, into host memory: width * height * C elements.  tileSamples as denoiseTiles takes them, nullptr: `samples` for every pixel.
// Synchronous; allocates and frees its own device memory.  The arguments have passed checkFeatureImages (rf_feature_request.hpp).
void exportFeaturesImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const uint32_t* tileSamples, const float* colorSum, const float* sumSq,
                          const float* albedoCoverage, const float* normalDepth, const float* directSum, const FeatureRequest& request, void* outHost);

// The firefly-robust mean (rf_robust.hip; the definition: include/rayfinder_amd.h) over host-assembled bucket planes -- K x width*height*4 floats, plane after plane,
// each row-major -- of `samples` >= K samples, on device `deviceOrdinal`: the mean RGBA (.w = 1), its BGRA8 under `exposure` and the trim count of every pixel
// (NULL = skip).  K odd, 3 .. 15.  Synchronous; allocates and frees its own device memory.
void robustMeanImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t K, uint32_t samples, const float* buckets, float exposure, float* outRgba,
                      uint32_t* outBgra8, uint8_t* outTrim);
// The same with one sample count >= K per 32x32 tile (host memory, ceil(width / 32) * ceil(height / 32) words, tile_y * ceil(width / 32) + tile_x): the bucket planes of
// a frame of renderAdaptive with kBucketsTileCounts
void robustMeanTiles(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t K, const uint32_t* tileSamples, const float* buckets, float exposure, float* outRgba,
                     uint32_t* outBgra8, uint8_t* outTrim);

// The temporal history (rf_temporal.hip; the definition: include/rayfinder_amd.h, "Temporal history"): maxHistory and depthTolerance finite and > 0, minNormalDot in
// [-1, 1] (the C ABI checks them before any device call)
struct TemporalParameters
{
    float maxHistory = 64.0f, depthTolerance = 0.05f, minNormalDot = 0.9f;
};
// The reprojection over host-assembled row-major width*height*4 sums of `samples` samples seen by `camera`, and a history of the same size -- histColor = {mean rgb,
// effective sample count}, histGeometry = {unit normal, depth}, histCamera: all three nullptr (no history) or all three given -- on device `deviceOrdinal`: outColor =
// {T.rgb, T.w}, outGeometry = {n, z}, the BGRA8 of T.rgb under `exposure` (NULL = skip).  Synchronous; allocates and frees its own device memory.
void temporalImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* albedoCoverage, const float* normalDepth,
                    const Camera& camera, const float* histColor, const float* histGeometry, const Camera* histCamera, const TemporalParameters& params, float exposure,
                    float* outColor, float* outGeometry, uint32_t* outBgra8);

// The noise estimate over the accumulation and the radiance second moments (rf_noise.hip; the definition: include/rayfinder_amd.h)
struct NoiseEstimate
{
    double   meanError = 0.0;
    float    maxError = 0.0f;
    uint32_t worstTile = 0, samples = 0;
    uint64_t pixels = 0, nonfinitePixels = 0;
};
// The estimate over host-assembled row-major width*height*4 sums (the accumulation and the second moments) of `samples` >= 2 samples, on device `deviceOrdinal`:
// errorMap (width * height), tileSum, tileMax (one entry per tile of the 32 x 32 grid) are host pointers, NULL = skip.  Synchronous; allocates and frees its own
// device memory.
NoiseEstimate noiseEstimateImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* sumSq, float* errorMap,
                                  float* tileSum, float* tileMax);

// The same with one sample count per tile of the 32 x 32 grid (tileSamples[t] >= 2, tile t = tile_y * ceil(width / 32) + tile_x): Nf = float(tileSamples[t]) for the
// pixels of tile t.  tileSamples == nullptr: `samples` for every tile.  The result's `samples` is `samples` as given.
NoiseEstimate noiseEstimateTiles(int deviceOrdinal, uint32_t width, uint32_t height, const uint32_t* tileSamples, uint32_t samples, const float* colorSum, const float* sumSq,
                                 float* errorMap, float* tileSum, float* tileMax);

// Tile-adaptive sampling (rf_renderer_render_adaptive; the loop: include/rayfinder_amd.h)
struct AdaptiveParameters
{
    float    targetTileError = 0.0f;
    uint32_t checkEvery = 8, minSamples = 0, maxSamples = 0; // maxSamples 0: numSamplesPerPixel
};
struct AdaptiveResult
{
    uint32_t      estimatePasses = 0;
    uint32_t      tiles = 0, stoppedTiles = 0; // stopped: tiles below the leading count
    uint32_t      minTileSamples = 0, maxTileSamples = 0;
    uint64_t      pixelSamples = 0;            // sum over the tiles of in-frame pixels x sample count
    uint64_t      tracedPixelSamples = 0;      // of those, the ones this call traced
    uint32_t      framesTraced = 0;            // how far the call moved the handle's frame counter
    NoiseEstimate last;                        // the last pass's estimate, over the tiles that were active in it (samples = 0: no pass was made)
};

class Renderer
{
public:
    Renderer(const RendererDescriptor& desc, const SceneView& scene);
    ~Renderer();
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    void  setRenderParameters(const RenderParameters& params);
    void  render(uint32_t numFrames);
    float averageRenderpassDurationMs() const;
    float renderProgressPercentage() const;

    // Multi-GPU: render only this rank's tiles. Resets accumulation.
    void setTileShard(uint32_t rank, uint32_t worldSize);
    std::span<const uint32_t> shardTiles() const;

    uint32_t accumulatedSampleCount() const;
    uint32_t width() const;
    uint32_t height() const;
    uint32_t shardRank() const;
    uint32_t shardWorldSize() const;
    int      deviceOrdinal() const;
    float    exposure() const; // of the current render parameters: what the display transforms scale by
    // The handle's HIP stream (a hipStream_t): work a caller wants ordered behind the frame's kernels (the RCCL
    // frame exchange, rf_comm.hpp) is enqueued here.
    void* streamHandle() const;
    // Row-major width*height*4 floats (sum of samples, 16-B stride as the reference's
    // array<vec3f>); pixels outside this rank's tiles are zero.
    void readAccumulation(float* dst);
    // First-hit AOVs (rf_renderer_set_aovs / rf_renderer_read_aovs): flags 0 = off (default), kAovFirstHit = on, kAovFirstHit | kAovTileCounts = on and kept per tile
    // count under renderAdaptive (until that is called: exactly kAovFirstHit).  Any change of the flags value clears the sums.
    // Read: row-major width*height*4 floats each ({albedo.rgb, coverage} and {normal.xyz, depth} SUMS, this rank's pixels; NULL = skip) and the AOV sample count.
    static constexpr uint32_t kAovFirstHit = 1u, kAovTileCounts = 0x100u;
    void     setAovs(uint32_t flags);
    uint32_t aovFlags() const;
    void     readAovs(float* albedoCoverage, float* normalDepth, uint32_t* sampleCount);
    // Edge-aware a-trous denoiser over the accumulation and the first-hit AOVs (rf_renderer_denoise; the arithmetic: include/rayfinder_amd.h).  denoise enqueues on the
    // handle's stream and keeps a snapshot (allocated on the first call); it throws std::invalid_argument when the AOVs are off, their count differs from the
    // accumulated count, nothing is accumulated or a tile shard is set.  In the non-uniform state it runs when the AOVs carry kAovTileCounts and cover the accumulation
    // (prep then divides each pixel by its tile's count; the snapshot's count is the leading count; the call first waits for the stream and copies the counts to the
    // device, as the other per-tile reads do), and refuses as requireUniformTileSamples does otherwise.
    // readDenoised: row-major width*height*4 mean floats and / or BGRA8 (NULL = skip) and the snapshot's sample count; std::invalid_argument without a snapshot
    // (none yet, or cleared with the AOV sums).
    void denoise(const DenoiseParameters& params);
    void readDenoised(float* rgba, uint32_t* bgra8, uint32_t* sampleCount);
    // Radiance second moments (rf_renderer_set_moments / rf_renderer_read_moments): off by default.  While on, one more compact tile-major float4 buffer holds
    // {sum r.x r.x, sum r.y r.y, sum r.z r.z, 0} over the samples traced since it was last cleared (with the image, or when the switch changes), in sample order.
    // Read: row-major width*height*4 floats (this rank's pixels; NULL = skip) and the moment sample count.
    void     setMoments(bool enabled);
    bool     momentsEnabled() const;
    void     readMoments(float* sumSq, uint32_t* sampleCount);
    // Direct radiance sums (rf_renderer_set_direct / rf_renderer_read_direct): off by default.  While on, one more compact tile-major float4 buffer holds D = the sum, in
    // sample order, of each sample's radiance as it stands after bounce 1 -- what the image of a handle with numBounces = 1 holds, bit for bit -- over the samples traced
    // since it was last cleared (with the image, or when the switch changes).  Indirect light is S - D, formed by whoever needs it.  One more launch per batch, behind
    // bounce 1's shadow launch.  The word is 0 = off, kDirectOn = on, kDirectOn | kDirectTileCounts = on and kept per tile count under renderAdaptive /
    // renderAdaptiveFrom (until one of them is called: exactly kDirectOn): D of tile t is then that of its first tileSamples[t] samples, as S and Q are, added through
    // the tile list's radiance-sum kernels (rf_sums.hpp).  Without the bit renderAdaptive / checkAdaptive refuse while D is on.  Any change of the word clears D and
    // drops a split-denoised snapshot; turning D on is refused in the non-uniform state, with or without the bit.  std::invalid_argument for any other word.
    // Read: row-major width*height*4 floats (this rank's pixels; NULL = skip) and the direct sample count (the non-uniform state: the leading count).
    static constexpr uint32_t kDirectOn = 1u, kDirectTileCounts = 0x100u;
    void     setDirect(uint32_t flags);
    bool     directEnabled() const;
    uint32_t directFlags() const;
    void     readDirect(float* directSum, uint32_t* sampleCount);
    // The split-component denoiser (rf_renderer_denoise_split; the arithmetic: include/rayfinder_amd.h): D and S - D demodulated and filtered separately, each with its
    // own parameters, and recombined; the result is denoise's snapshot (readDenoised).  std::invalid_argument when the AOVs or the direct sums are off or do not cover
    // the accumulation, nothing is accumulated or a tile shard is set.  In the non-uniform state it runs when D carries kDirectTileCounts, the AOVs carry kAovTileCounts
    // and both cover the accumulation (prep then divides each pixel by its tile's count; the snapshot's count is the leading count; the call first waits for the
    // stream and copies the counts to the device), and refuses as requireUniformTileSamples does otherwise -- before any other check.
    void denoiseSplit(const DenoiseParameters& direct, const DenoiseParameters& indirect);
    // The feature export (rf_renderer_export_features; the definition: include/rayfinder_amd.h): the request's channels of the handle's own tile-major sums into
    // `dstDevice` (caller-owned memory of the handle's device, dstBytes of it), enqueued on the handle's stream and waited for; -> the accumulated (leading) count.  In the
    // non-uniform state every pixel takes its tile's count (uploadTileSamples, as the other per-tile reads).  Read-only.  std::invalid_argument, before any launch: a
    // destination that is too small or not device memory of this device, a tile shard, no sample, a selected channel whose family is off, does not cover the accumulation
    // or -- in the non-uniform state -- was kept without its tile-count bit, VARIANCE / ERROR below 2 samples.
    uint32_t exportFeatures(const FeatureRequest& request, void* dstDevice, uint64_t dstBytes);
    // Bucket sums (rf_renderer_set_buckets / rf_renderer_read_buckets): K = 0 off (the default), else odd, 3 .. 15.  While on, K more compact tile-major float4 planes
    // in one allocation: plane b holds {sum r.x, sum r.y, sum r.z, 0} over the samples whose ordinal -- the bucket sample count just before the sample -- is b mod K,
    // in sample order.  Their own sample count; cleared with the image and whenever the word changes.  The word is K, or K | kBucketsTileCounts (K > 0): until
    // renderAdaptive is called the same handle; renderAdaptive then runs with the buckets on, the planes of tile t hold its first tileSamples[t] samples (sample j of the
    // tile in plane j mod K), and robustMean / denoiseRobust combine every pixel with its tile's count.  Without the bit renderAdaptive / checkAdaptive refuse while the
    // buckets are on.  std::invalid_argument for a bad word, and for K > 0 in the non-uniform state.
    // K | kBucketsTileCounts | kBucketsShardTileCounts (valid only with the first bit): the per-tile-count planes are also kept under a tile shard -- checkAdaptive(p, true)
    // passes, renderAdaptiveFrom adds the bucket sums through the shard's slot list -- and they may leave the handle through the frame gather (enqueueShardRobustMean with
    // one count per slot).  On a whole-frame handle nothing else changes.  A change of either bit alone clears the sums like a change of K.
    // Read: K x width*height*4 floats, plane after plane, each row-major (this rank's pixels; NULL = skip), K and the bucket sample count (the leading count).
    static constexpr uint32_t kBucketsTileCounts = 0x100u, kBucketsShardTileCounts = 0x400u;
    void     setBuckets(uint32_t word);
    uint32_t buckets() const;
    bool     bucketsPerTile() const; // the non-uniform state of a whole-frame handle whose buckets carry kBucketsTileCounts
    void     readBuckets(float* planes, uint32_t* K, uint32_t* sampleCount);
    // The robust mean over the handle's own bucket sums (rf_renderer_robust_mean; the arithmetic: include/rayfinder_amd.h): enqueued on the handle's stream, keeps a
    // snapshot (allocated by the first call, dropped whenever the bucket sums are cleared).  std::invalid_argument when the buckets are off, their count differs from
    // the accumulated count or is below K, a tile shard is set or the tiles hold different counts -- unless bucketsPerTile(): then every pixel is combined with its
    // tile's count (refused when a tile holds fewer than K samples) and the snapshot's count is the leading count.
    // readRobustMean: row-major width*height*4 mean floats, BGRA8, one trim count per pixel (NULL = skip) and the snapshot's sample count; std::invalid_argument
    // without a snapshot.
    void robustMean();
    void readRobustMean(float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* sampleCount);
    // robustMean, then the a-trous filter of denoise with prep's colour c = M.rgb: the result is denoise's snapshot (readDenoised).  Refused as denoise and robustMean are
    // (the non-uniform state: the AOVs with kAovTileCounts and the buckets with kBucketsTileCounts, both covering the accumulation; prep divides by each tile's count).
    void denoiseRobust(const DenoiseParameters& params);
    // The temporal history (rf_renderer_temporal_*; the arithmetic: include/rayfinder_amd.h, "Temporal history").  temporalAccumulate: the current view's sums blended
    // with the kept history reprojected into the current camera, enqueued on the handle's stream; keeps a snapshot (T, G, texels, camera, count: allocated by the first
    // call, dropped whenever the AOV sums are cleared); a later call in the same accumulation recomputes from the same history.  std::invalid_argument when the AOVs
    // are off or do not cover the accumulation, nothing is accumulated, a tile shard is set or the tiles hold different counts.
    // temporalCommit: the result becomes the history (a swap of roles, no copy) and the snapshot is gone; std::invalid_argument without a result.  The history survives
    // a restart of the accumulation; a change of the frame size, a tile shard and temporalReset drop it.
    // readTemporal: row-major width*height*4 floats {T.rgb, T.w}, BGRA8, width*height*4 floats {n, z} (NULL = skip) and the snapshot's sample count;
    // std::invalid_argument without a result.
    void temporalAccumulate(const TemporalParameters& params);
    void temporalCommit();
    void temporalReset();
    void readTemporal(float* rgba, uint32_t* bgra8, float* geometry, uint32_t* sampleCount);
    // temporalAccumulate, then the a-trous filter of denoise with prep's colour c = T.rgb: the result is denoise's snapshot (readDenoised).  Refused as either half is.
    void denoiseTemporal(const TemporalParameters& temporal, const DenoiseParameters& params);
    // The noise estimate over the handle's own sums (rf_renderer_noise_estimate): enqueued on the handle's stream, then waited for.  std::invalid_argument when the
    // moments are off, their count differs from the accumulated count, fewer than 2 samples are accumulated or a tile shard is set.  Host pointers, NULL = skip.
    NoiseEstimate noiseEstimate(float* errorMap, float* tileSum, float* tileMax);
    // render() in steps of checkEvery frames with an estimate after each step (once 2 samples are accumulated), until the mean error is <= target, maxFrames frames
    // have been rendered or the accumulation is full.  -> frames rendered; *last: the last estimate (samples = 0: none was made).  Needs the moments on (covering
    // the whole accumulation), no tile shard and checkEvery >= 1.
    uint32_t renderUntil(float targetMeanError, uint32_t checkEvery, uint32_t maxFrames, NoiseEstimate* last);
    // Tile-adaptive sampling: keep sampling only the 32 x 32 tiles whose mean error is still above the target.  Afterwards the tiles may hold different sample counts
    // (the non-uniform state): render, renderUntil, setTileShard and the frame gather then throw std::invalid_argument (requireUniformTileSamples), as does denoise
    // unless the AOVs were kept with kAovTileCounts; the reads report the leading count, and readTileSamples / readMean / readTonemapped / noiseEstimate / denoise honour
    // the per-tile counts.  With kAovFirstHit | kAovTileCounts the AOV sums of tile t are those of its first tileSamples[t] samples, as S and Q are.
    // With K | kBucketsTileCounts the bucket planes of tile t are those of its first tileSamples[t] samples too, and robustMean / denoiseRobust honour the counts.
    // With kDirectOn | kDirectTileCounts so is D of tile t, and denoiseSplit honours the counts (given the AOVs' bit as well).
    // std::invalid_argument when the moments are off or do not cover the accumulation, the AOVs are on without kAovTileCounts or do not cover it, the buckets are on
    // without kBucketsTileCounts or do not cover it, the direct sums are on without kDirectTileCounts or do not cover it, a tile shard is set,
    // checkEvery is 0 or the target is negative or not finite.
    AdaptiveResult renderAdaptive(const AdaptiveParameters& params);
    // The same over a tile shard, one rank's part of rf_comm_render_adaptive (renderAdaptive of rf_comm.hpp makes the exchanges around it).  checkAdaptive: renderAdaptive's
    // checks but the shard's, throwing before anything is traced -- there, before the first collective.  renderAdaptiveFrom: the loop over this handle's tiles with `leading`
    // the FRAME's leading count (the largest accumulated count over the ranks): the active tiles are those at `leading` -- none when this handle's own count is lower -- and
    // the result speaks of this handle's tiles (stoppedTiles: below its own accumulated count); shardSlots: the sums are addressed through each listed tile's slot in the
    // shard (always so through rf_comm_render_adaptive, at world size 1 as well).
    // sharded: the call is rf_comm_render_adaptive's, which the buckets refuse (kBucketsTileCounts covers renderAdaptive alone) unless they carry
    // kBucketsShardTileCounts as well.
    void           checkAdaptive(const AdaptiveParameters& params, bool sharded = false) const;
    AdaptiveResult renderAdaptiveFrom(const AdaptiveParameters& params, uint32_t leading, bool shardSlots);
    // What follows the loop once the ranks have agreed on the frame: its largest and smallest tile count, the same on every rank -- while they differ the handle is in the
    // non-uniform state (requireUniformTileSamples) whatever its own tiles hold; cleared with the accumulation -- and `skipFrames` more on the frame counter without
    // tracing: a rank whose tiles all stopped while the frame's leading tiles went on stays in step with them, so the next sample any rank traces (after a restart of the
    // accumulation too) is the one a handle without a shard would trace.  -> how many of the shard's tiles are below `leading`
    uint32_t       settleFrameTileSamples(uint32_t leading, uint32_t minimum, uint32_t skipFrames);
    // The counts of the shard's tiles in slot order (the order of shardTiles()) in device memory, for the frame gather; waits for the stream.  Valid until the next
    // per-tile read or gather of this handle.
    const uint32_t* shardTileSamplesDevice();
    bool           tileSamplesUniform() const;
    void           requireUniformTileSamples(const char* what) const;
    // one count per tile of the frame's grid (tile_y * ceil(width / 32) + tile_x); a tile outside this rank's shard: 0.  -> the number of tiles
    uint32_t readTileSamples(uint32_t* tileSamples) const;
    // Row-major width*height*4 floats {S.rgb / float(the tile's count), 1}; rgb 0 where the tile has no sample; pixels outside this rank's tiles are zero.
    void readMean(float* rgba);
    // Device pointer of the compact tile-major accumulation buffer (numTiles*1024 float4) and a
    // way to render into caller-owned device memory (e.g. a torch tensor used for the RCCL gather).
    void*    accumulationDevicePointer() const;
    // The compact tile-major sums of the shard as the frame gather sees them (rf_comm.hpp: planes 0 .. 3 = S, {albedo.rgb, coverage}, {normal.xyz, depth}, Q; plane 5 = D): each
    // plane's device pointer -- nullptr while its channel is off or has not been sized yet -- and per channel whether it is on, whether it holds exactly the accumulated
    // samples (on from the first sample, at least one accumulated: what the gather requires before it sends them) and its own sample count.
    struct ShardSums
    {
        using Channel = SumCoverage; // on, coversAccumulation, samples
        const void* planes[4];
        Channel     aovs, moments;
        uint32_t    accumulated;
        bool        ownsTiles;
        Channel     buckets;  // the bucket sums: on, covering the accumulation, their own sample count
        uint32_t    bucketsK; // K while they are on, else 0
        bool        bucketsShardTileCounts; // the buckets carry kBucketsShardTileCounts: the planes follow the per-slot counts and may be gathered in the non-uniform state
        // the smallest tile count known to the rank: the frame's minimum after rf_comm_render_adaptive (the same on every rank, one without a tile too), else the
        // smallest of the rank's own tiles (no tile: the accumulated count)
        uint32_t    minTileSamples;
        Channel     direct;           // the direct sums: on, covering the accumulation, their own sample count
        bool        directTileCounts; // D carries kDirectTileCounts: it follows the per-slot counts under rf_comm_render_adaptive
        const void* directPlane;      // D, shard-compact tile-major like planes[] (rf_comm.hpp: plane 5); nullptr while off or not sized yet
    };
    ShardSums shardSums() const;
    // The robust mean of the shard's own pixels, for the frame gather (rf_comm.hpp: plane 4): kRobustMeanShard over the shard-compact bucket planes with the accumulated
    // count, enqueued on the handle's stream -> the shard-compact tile-major buffer {M.rgb, float(c)} (owned by the handle: allocated by the first call, freed where the
    // bucket planes are -- setBuckets with another word --, regrown like them for a larger shard; nullptr and nothing enqueued when the shard holds no tile).  The caller has checked that the buckets cover the accumulation and that it holds >= K samples.
    // slotCounts != nullptr -- the non-uniform state; the caller has checked kBucketsShardTileCounts and that every tile holds >= K samples --: what
    // shardTileSamplesDevice() returned, and kRobustMeanShardTiles combines every slot with its own count.
    const void* enqueueShardRobustMean(const uint32_t* slotCounts = nullptr);
    // The checkpoint seam (rf_checkpoint.hip: the state digest, save and load are written against these three calls and the public reads alone).
    // checkpointBooks: waits for the stream, zeroes every restarted sum that is on as the next sample would (so that a restarted family lies in device memory as the
    // zeros its read returns), and -> the books a checkpoint carries and the compact tile-major planes as they lie (device pointers; nullptr: off, or a shard without a tile).
    // checkpointRestart: a new accumulation (restartAccumulation; the frame counter stays) and, zeroNow, every sum that is on sized for the shard and zeroed at once: what a load copies into.
    // checkpointAdopt: the books of a load whose planes lie in device memory and have been verified: the frame counter, the accumulated count, each family's own count,
    // the per-slot tile counts (stored only while they differ from the accumulated count) and the frame-level pair.
    struct CheckpointBooks
    {
        using Family = SumCount; // on, samples (0: restarted -- its read returns zeros)
        uint32_t              frameCount = 0, accumulated = 0, frameLeadingSamples = 0, frameMinTileSamples = 0;
        uint32_t              aovFlags = 0, moments = 0, directWord = 0, bucketsWord = 0;
        Family                family[5] = {}; // S, the AOVs, Q, D, the buckets
        std::vector<uint32_t> tileSamples;    // one count per tile of the shard, in slot order (the uniform state: the accumulated count)
        const void*           planes[20] = {}; // S, AC, ND, Q, D, bucket 0 .. 14
        uint32_t              camera[19] = {}, sky[6] = {}, numBounces = 0, samplesPerPixel = 0; // the render-parameter guard, as bit patterns, and the cap
        uint64_t              sceneCounts[4] = {}; // BVH nodes, triangles, textures, texels
        uint32_t              rootBounds[6] = {};  // the root node's box, as bit patterns
    };
    // prepare == false: the books alone, as they stand -- no device call, nothing zeroed, planes all nullptr (what a load compares a blob's guards with before it
    // touches anything).  checkpointScratch: device memory of at least `bytes` that the handle keeps between digests (the tile words and the tile table).
    CheckpointBooks checkpointBooks(bool prepare = true);
    void*           checkpointScratch(uint64_t bytes);
    void            checkpointRestart(bool zeroNow);
    void            checkpointAdopt(const CheckpointBooks& books);
    // Zero the accumulation buffer (on the handle's stream) if nothing has been rendered into it since the last reset, so that a
    // reader on the device (the frame exchange) never sees the previous frame's sums.
    void     clearAccumulationIfStale();
    // Device memory held: path state + queues (allocated on demand, kBytesPerPath per path slot), the batch depth in use, and
    // the resident scene (BVH layouts, triangles, shading records, textures).
    // rf_renderer_layout_info: layouts[0..15] = closest-hit, [16..31] = any-hit, [32..47] = any-hit launch starts at the occluder cache; misc = {hint levels, first look from bounce,
    // dense leaf min, legacy build}
    void     layoutInfo(uint32_t (&layouts)[48], uint32_t (&misc)[4], float& quadHalfAreaRatio, uint64_t& treeBytes) const;
    // rf_renderer_launch_plan: what the launches of bounce 1..numBounces of the handle's NEXT batch of numSamples samples would be, in its present state (the same
    // plans traceBatch enqueues from; nothing is enqueued).  std::invalid_argument for a bounce outside 1..numBounces or no sample.
    void     launchPlan(uint32_t bounce, uint32_t numSamples, ::rf_launch_plan& out) const;
    void     memoryInfo(uint64_t& pathStateBytes, uint64_t& pathsAllocated, uint64_t& maxPathsPerBatch, uint64_t& sceneBytes) const;
    uint64_t accumulationBytes() const;
    void     bindAccumulationBuffer(void* devicePtr, uint64_t bytes);
    // BGRA8 swap-chain image (wgsl:59-63), row-major.
    void readTonemapped(uint32_t* dstBgra8);
    // The same display transform for any row-major float4 SUM image in device memory (e.g. the frame a gather
    // assembled on the root rank): numPixels texels, divided by `samples`, scaled by the handle's exposure.
    void tonemapDeviceImage(const void* imageDevice, uint64_t numPixels, uint32_t samples, uint32_t* dstBgra8Host);

    // Deferred-lighting variant: numFrames frames of lighting pass + exponential resolve
    // (src/pt/deferred_renderer_lighting_pass.wgsl:96-186, deferred_renderer_resolve_pass.wgsl:33-54) over a
    // primary-ray G-buffer; uses the handle's camera, sky and exposure.  Its frame counter starts at 0 (frame 0
    // initialises the accumulation, resolve_pass.wgsl:41-44) and is independent of render()'s.
    void     renderDeferred(uint32_t numFrames);
    void     resetDeferred();
    uint32_t deferredFrameCount() const;
    // sampleBuffer / accumulationBuffer (width*height*3 floats, row-major) and the resolve pass's BGRA8 output; NULL = skip
    void readDeferred(float* sampleRgb, float* accumulationRgb, uint32_t* bgra8);

    void        setCounting(bool enabled);
    // Tuning knobs for A/B measurements inside one process ("traversal_variant": 0 = one ray per
    // thread kernels, 1 = persistent waves with lane refill).  Results never depend on them.
    void        setOption(const std::string& name, int64_t value);
    uint32_t    numBounces() const;
    void        setTiming(bool enabled);
    void        resetStats();
    RenderStats stats();
    void        synchronize();

    // bvh-visualizer pass: pinhole camera, u = j/W, v = 1-(i+1)/H, tMax = FLT_MAX.
    void tracePrimaryStats(const Camera& camera, uint32_t width, uint32_t height, uint32_t* nodesVisitedOut,
                           uint8_t* hitOut, float* tOut, uint32_t* triangleTestsOut);
    // Batch closest-hit / any-hit of caller rays (6 floats each) -- the GPU twin of the
    // reference's CPU query rayIntersectBvh (src/common/ray_intersection.hpp:43-49).
    void intersectRays(const float* rays6, uint64_t numRays, float tMax, uint32_t* triangleOut, float* tOut, float* uvOut,
                       float* pOut, uint32_t* nodesVisitedOut, uint32_t* triangleTestsOut);
    void occludedRays(const float* rays6, uint64_t numRays, float tMax, float* visibilityOut);
    // rf_renderer_cast_rays (the definition: include/rayfinder_amd.h): rays from caller-owned device memory through the production traversal, the hit and the surface
    // attributes at it into caller-owned device memory, in chunks of one path-state allocation; enqueued on the handle's stream, then waited for.  Read-only for the
    // handle's sums, books and statistics.  std::invalid_argument, before any launch, for what the header lists (the request's own checks: rf_ray_query_request.hpp)
    void castRays(const RayQueryRequest& request);

private:
    struct Impl;
    std::unique_ptr<Impl> mImpl;
};
} // namespace rf
