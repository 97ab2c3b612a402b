// rf_renderer.hip -- wavefront path tracer for MI355X (gfx950): the host driver (the kernels live in rf_trace.hip, rf_shade.hip and rf_sums.hip, what the
// units share in rf_kernels.hpp; the scene's device layouts are built and packed by host-only code, rf_scene_pack.cpp and rf_wide_build.cpp, and uploaded here; which
// kernel runs with which parameters is planned by host-only code too, rf_launch_policy.cpp, and enqueued here; the accumulation's books -- the counts, the switches, the
// snapshots' validity -- and every refusal that rests on them are host-only code as well, rf_books.cpp: this unit keeps the sums' storage and enqueues).
//
// The reference traces one full path per fragment-shader invocation
// (src/pt/reference_path_tracer.wgsl:34-64,180-234).  Here the same per-path arithmetic is cut
// into a wavefront pipeline so that every stage runs with full, coherent waves:
//
//   raygen            wgsl:42-54,236-245,594-616   S samples x all pixels of this rank's tiles
//   for bounce = 1..numBounces
//     traceClosest    wgsl:370-521                 queue of live paths -> hit record, origin <- p
//     shade           wgsl:189-228,247-319,546-592 miss: += throughput*sky, path ends
//                                                  hit : albedo, pending NEE term, next direction,
//                                                        throughput *= albedo; ballot-compacted queue
//     traceShadow     wgsl:321-368                 radiance += pending * visibility * invPdf
//   accumulate        wgsl:47-57                   image += radiance, samples in index order (f32)
//
// Path state lives in HBM as six float4 streams indexed by path slot (slot = sample*pixels +
// pixel, fixed for the life of the path); queues hold slot ids.  Because the reference reuses ONE
// blue-noise pair for lens, sun cone and every bounce (wgsl:52-55,194,209), cos/sin of 2*pi*u.y
// are evaluated once per path in raygen and carried in the .w lanes.
//
// Kernel grids are sized for the worst case (all paths alive) and read the live count from
// device memory, so a whole batch is enqueued without any host round trip.
#include "rayfinder_amd.h"
#include "rf_books.hpp"
#include "rf_denoise.hpp"
#include "rf_features.hpp"
#include "rf_kernels.hpp"
#include "rf_launch_policy.hpp"
#include "rf_noise.hpp"
#include "rf_ray_query.hpp"
#include "rf_robust.hpp"
#include "rf_temporal.hpp"
#include "rf_scene_pack.hpp"
#include "rf_sums.hpp"

#include <map>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace rf
{
bool operator==(const RenderParameters& a, const RenderParameters& b)
{
    return a.width == b.width && a.height == b.height && std::memcmp(&a.camera, &b.camera, sizeof(Camera)) == 0 &&
           a.samplingParams == b.samplingParams && a.sky == b.sky && a.exposure == b.exposure;
}

namespace
{
// Morton (Z-order) key of a tile position
uint32_t tileMortonKey(uint32_t tx, uint32_t ty)
{
    const auto spread = [](uint32_t v) {
        v &= 0xFFFFu;
        v = (v | (v << 8)) & 0x00FF00FFu;
        v = (v | (v << 4)) & 0x0F0F0F0Fu;
        v = (v | (v << 2)) & 0x33333333u;
        v = (v | (v << 1)) & 0x55555555u;
        return v;
    };
    return spread(tx) | (spread(ty) << 1);
}
} // namespace

std::vector<uint32_t> tilesForRank(uint32_t width, uint32_t height, uint32_t rank, uint32_t worldSize)
{
    const uint32_t tilesX = TileGrid(width, height).tilesX, n = TileGrid(width, height).count();
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    if (worldSize > 1)
    {
        // Tiles walked along a Z-order curve; each run of `world` consecutive tiles of the curve -- a compact block of the image
        // (4x2 tiles for 8 ranks, 2x2 for 4) -- is split over all ranks, and the deal is rotated by one rank from block to block so
        // that no rank always gets the same corner of a block (tile cost has a vertical gradient: a fixed position is a
        // systematic bias).  Every rank gets n/world +-1 tiles.  Neighbouring tiles cost about the same (sky vs interior), so the
        // ranks' loads are stratified samples of the frame: on the atrium at 1080p the busiest of 8 ranks traces 1.0 % more rays
        // than the mean, against 3.0 % for the hashed deal used before (3.6 % unrotated); the strong-scaling time is the
        // slowest rank's.
        std::stable_sort(order.begin(), order.end(), [tilesX](uint32_t a, uint32_t b) { return tileMortonKey(a % tilesX, a / tilesX) < tileMortonKey(b % tilesX, b / tilesX); });
    }
    std::vector<uint32_t> mine;
    for (uint32_t i = 0; i < n; ++i)
        if ((i % worldSize + i / worldSize) % worldSize == rank) mine.push_back(order[i]);
    std::sort(mine.begin(), mine.end());
    return mine;
}

void untileHost(const float* compact, const uint32_t* tileIds, uint32_t numTiles, uint32_t width, uint32_t height, float* image)
{
    untileHostTexels(compact, tileIds, numTiles, width, height, 4 * sizeof(float), image);
}

void untileHostTexels(const void* compact, const uint32_t* tileIds, uint32_t numTiles, uint32_t width, uint32_t height, size_t texelBytes, void* image)
{
    const uint32_t tilesX = TileGrid(width, height).tilesX;
    const auto*    src = static_cast<const unsigned char*>(compact);
    auto*          dst = static_cast<unsigned char*>(image);
    for (uint32_t t = 0; t < numTiles; ++t)
    {
        const uint32_t tx = tileIds[t] % tilesX, ty = tileIds[t] / tilesX;
        for (uint32_t w = 0; w < kTileSize * kTileSize; ++w)
        {
            const uint32_t block = w >> 6, lane = w & 63u;
            const uint32_t x = tx * kTileSize + (block & 3u) * 8u + (lane & 7u);
            const uint32_t y = ty * kTileSize + (block >> 2) * 8u + (lane >> 3);
            if (x >= width || y >= height) continue;
            std::memcpy(dst + texelBytes * (static_cast<size_t>(y) * width + x), src + texelBytes * (static_cast<size_t>(t) * 1024 + w), texelBytes);
        }
    }
}

using Books = AccumulationBooks;
static_assert(Renderer::kAovTileCounts == Books::kWordTileCounts && Renderer::kDirectTileCounts == Books::kWordTileCounts && Renderer::kBucketsTileCounts == Books::kWordTileCounts &&
              Renderer::kBucketsShardTileCounts == Books::kWordShardTileCounts && kMaxBuckets == Books::kMaxBuckets);

// The storage of one family of sums (its books: AccumulationBooks::Sums): compact tile-major float4 buffers of the shard -- the AOVs: {albedo.rgb, coverage}, {normal.xyz,
// depth}; the moments, the direct sums and the bucket planes: [0]; the image: none (Impl::image, the handle's own buffer or a bound one)
struct SumStorage
{
    uint32_t             numBuffers = 0;
    DeviceBuffer<float4> buffers[2];

    void release()
    {
        for (auto& b : buffers) b.release();
    }
    // before the first sample after a restart: room for `texels` (the stream is waited for before a smaller buffer is freed), then zeros
    void zero(hipStream_t stream, uint64_t texels)
    {
        if (numBuffers != 0u && buffers[0].count < texels)
        {
            RF_HIP(hipStreamSynchronize(stream)); // (a smaller buffer may still be read by the last batch or estimate)
            for (uint32_t i = 0; i < numBuffers; ++i) buffers[i].alloc(texels);
        }
        for (uint32_t i = 0; i < numBuffers; ++i) RF_HIP(hipMemsetAsync(buffers[i].ptr, 0, texels * sizeof(float4), stream));
    }
};

// ------------------------------------------------------------------------------------------------
struct Renderer::Impl
{
    int         device = 0;
    hipStream_t stream = nullptr;

    DeviceBuffer<float4>            nodes, triangles, wideNodes, wideCompact, wideHot, wideOwn, wideQuad;
    DeviceBuffer<uint4>             wideQuadHalf, wideQuadLocal, wideOct;
    DeviceBuffer<uint2>             bigLeaves;
    WideScene                       wide{};
    DeviceBuffer<float4>            attributes; // 4 per triangle (packed, see the constructor)
    DeviceBuffer<float4>            shadeRecords; // 8 per triangle: kShade's 128-byte record
    DeviceBuffer<TextureDescriptor> textureDescriptors;
    DeviceBuffer<uint32_t>          texels;
    DeviceBuffer<uint8_t>           blueNoise;
    DeviceBuffer<float>             albedoLut;
    DeviceScene                     scene{};

    RenderParameters params;
    SkyStateGpu      sky{};
    SunBasis         sunBasis{};

    void updateSunBasis() { pixarOnb(vec3(sky.sunDirection[0], sky.sunDirection[1], sky.sunDirection[2]), sunBasis.u, sunBasis.v); }
    uint32_t         maxWidth = 0, maxHeight = 0;
    // the frame counter, the accumulated count, the shard, the per-tile counts, every family's switch and count, both snapshots' validity: rf_books.hpp
    Books            books;
    // what the scene packing found (rf_scene_pack.hpp): the launch policy's facts, and a checkpoint's scene guard (checkpointBooks) -- the counts of BVH nodes,
    // triangles, textures and texels the handle was created with, and the root node's box
    SceneFacts       facts;
    DeviceBuffer<uint64_t> checkpointWork; // the state digest's tile words and, behind them, its tile table (checkpointScratch): grown on demand, kept

    std::vector<uint32_t>   tiles;
    DeviceBuffer<uint32_t>  tileIds; // the tile list of the next batch: the shard's own (configureShard) or an active list (uploadTileList), and behind the ids each tile's slot in the shard
    DeviceBuffer<uint32_t>  tileValidBefore; // prefix sum of the valid pixels of the shard's tiles (numTiles + 1): kRaygen's queue positions without an atomic (FrameParams)
    DeviceBuffer<float4>    ownedImage;
    float4*                 image = nullptr; // compact tile-major accumulation buffer
    uint64_t                imageBytes = 0;
    // The sums' storage, by family (off: nothing is allocated or launched).  The first-hit AOVs (rf_renderer_set_aovs); the radiance second moments
    // (rf_renderer_set_moments): {sum r r per channel, 0}; the direct sums (rf_renderer_set_direct): D = the sum of each sample's radiance as it stands after bounce 1 (the
    // primary miss's sky term, or the first hit's sun term times its visibility), in the image's layout and the image's order; the bucket sums (rf_renderer_set_buckets):
    // K planes of the shard's tiles x 1024 float4 each in one buffer, plane b = the radiance sum over the samples of ordinal b mod K (under render_adaptive with the
    // tile-count bit: of the TILE's samples -- every active tile holds the family's count of them)
    SumStorage              storage[Books::kFamilies] = {{0}, {2}, {1}, {1}, {1}};
    float4*                 aovAlbedoCoverage() const { return storage[Books::kAovs].buffers[0].ptr; }
    float4*                 aovNormalDepth() const { return storage[Books::kAovs].buffers[1].ptr; }
    float4*                 moments() const { return storage[Books::kMoments].buffers[0].ptr; }
    float4*                 direct() const { return storage[Books::kDirect].buffers[0].ptr; }
    float4*                 bucketPlanes() const { return storage[Books::kBuckets].buffers[0].ptr; }
    size_t                  bucketStride() const { return tiles.size() * 1024; }
    RobustWork              robustWork;
    DeviceBuffer<float4>    robustShard; // enqueueShardRobustMean's {M.rgb, float(c)} of the shard's pixels, shard-compact tile-major: what the frame gather sends as plane 4
    // the denoiser (rf_renderer_denoise): its work buffers, allocated by the first denoise, and the snapshot they hold (valid: the books)
    DenoiseWork             denoiseWork;
    // the temporal history (rf_renderer_temporal_accumulate): the result's and the history's planes, allocated by the first call (which of them is valid: the books)
    TemporalWork            temporalWork;
    NoiseWork               noiseWork; // the estimate's device buffers, allocated by the first rf_renderer_noise_estimate
    DeviceBuffer<uint32_t>  tileSamplesDevice; // the per-tile counts (the books') for the per-tile reads (mean, tonemap, estimate), uploaded by them
    DeviceBuffer<float4>    meanImage;         // rf_renderer_read_mean / the non-uniform rf_renderer_read_tonemapped: compact tile-major, allocated by the first read

    uint64_t                validPixels = 0;     // pixels of this rank's tiles that lie inside the frame
    unsigned long long      primaryRaysHost = 0; // samples traced x validPixels since the last resetStats()
    uint64_t                maxPaths = 0;
    DeviceBuffer<P3>        sRayO, sRayD, sRayD2, sThr, sThr2, sPending, sNoise, sNoise2; // queue-position arrays, packed xyz; rayD / thr / noise: double-buffered (PathStreams)
    DeviceBuffer<float4>    sRad, sHit;
    DeviceBuffer<float4>    sAov; // [2 slot, 2 slot + 1] the first-hit AOV record of each path (kShade<false, true>); allocated with the path state while the AOVs are on
    DeviceBuffer<uint32_t>  queueA, queueB, missQueue, missSlots, shadowList, queueCounts; // shadowList: kShade's list of the shadow rays its own-triangle test has not settled (kShadeSelfShadow)
    DeviceBuffer<DeviceCounters> counters;
    DeviceBuffer<DeviceCounters> castCounters; // what the traversal launches of rf_renderer_cast_rays count into: never read (the query's rays are not render rays)
    DeviceBuffer<uint32_t>       castWords;    // ... and their queue length and cursors, apart from queueCounts: [0] the count, [kLine ..) the launch's cursor lines
    DeviceBuffer<unsigned long long> bounceTotals; // 4 x kMaxBounceStats: closest-hit rays, shadow rays, shadow rays answered by kShadowFirstLook, shadow rays settled by kShade's own-triangle test

    // deferred-lighting variant: its own frame counter and buffers (array<array<f32, 3>>)
    uint32_t               deferredFrameCount = 0;
    DeviceBuffer<float>    deferredSample, deferredAccum;
    DeviceBuffer<uint32_t> deferredBgra;

    bool timing = false;
    LaunchOptions options; // every knob of the launch policy (rf_launch_policy.hpp): the plans are computed from these and policyInputs()
    uint32_t wideBlocks = 0;
    bool     wideBlocksForced = false; // option persistent_blocks: every persistent launch takes that grid
    uint32_t multiProcessors = 0;
    std::map<std::pair<const void*, uint32_t>, uint32_t> residentCache; // kernel, extra LDS -> workgroups the device holds at once
    uint32_t skyBlocks = 2048; // grid of the per-bounce kSky launches (grid-stride; set from the CU count)
    bool     occluderGridWarm = false;       // a batch has filled the occluder grid since it was allocated
    // kShadowFirstLook pays where most shadow rays are stopped by their cell's leaves; in a scene lit from everywhere it only adds a pass over the queue.  Every
    // batch reports {answered, rays} of its first looks (asynchronously: read when the copy has landed); below a quarter the next 16 batches go without.
    DeviceBuffer<unsigned long long> lookBatch;
    unsigned long long*              lookBatchHost = nullptr;
    hipEvent_t                       lookEvent = nullptr;
    bool                             lookPending = false;
    uint32_t                         firstLookHoldOff = 0;
    DeviceBuffer<uint32_t> occluderGrid;
    DeviceBuffer<uint32_t> primaryLists, primaryLengths; // [valid-pixel rank of the batch][capacity] leaf words / [rank] length word; allocated by the first batch that uses them
    DeviceBuffer<uint32_t> samplePerm;
    RenderStats hostStats;

    struct TimedLaunch
    {
        hipEvent_t start, stop;
        int        kind;
        uint32_t   bounce;
    };
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t>  eventPool;

    struct BatchTiming
    {
        hipEvent_t start, stop;
        uint32_t   samples;
    };
    std::vector<BatchTiming> pendingBatches;
    std::deque<float>        passDurationsMs;

    hipEvent_t getEvent()
    {
        if (!eventPool.empty())
        {
            hipEvent_t e = eventPool.back();
            eventPool.pop_back();
            return e;
        }
        hipEvent_t e;
        RF_HIP(hipEventCreate(&e));
        return e;
    }

    uint64_t allocatedPaths = 0;
    uint64_t effectivePaths = 0;       // batch depth the last render() call ended up with (<= maxPaths: less when less memory was free THEN)

    // bytes of path state + queues per path slot (eight packed xyz streams, two float4 streams, five u32 queues / lists): 148
    static constexpr uint64_t kBytesPerPath = 8 * sizeof(P3) + 2 * sizeof(float4) + 5 * sizeof(uint32_t);
    // ... plus the 32-byte AOV record while the first-hit AOVs are on
    static constexpr uint64_t kAovBytesPerPath = 2 * sizeof(float4);
    uint64_t bytesPerPath() const { return kBytesPerPath + (books.on(Books::kAovs) ? kAovBytesPerPath : 0u); }
    uint64_t pathStateBytes() const { return allocatedPaths * kBytesPerPath + sAov.count * sizeof(float4); }
    // the per-pixel leaf lists of bounce 1: capacity + 1 words per valid pixel of a batch (1080p at the default capacity of 64: 539 MB)
    uint64_t primaryListBytes() const { return (primaryLists.count + primaryLengths.count) * sizeof(uint32_t); }
    // What the launch policy reads besides the options, as the handle stands (active: the tile list of a batch of render_adaptive)
    PolicyInputs policyInputs(const ActiveTiles* active = nullptr) const
    {
        PolicyInputs in;
        in.facts = facts;
        const void* const present[] = {wide.nodes, wide.compact, wide.hot, wide.quad, wide.quadHalf, wide.quadLocal, wide.oct}; // by kLayoutBinary .. kLayoutOct
        for (int layout = kLayoutBinary; layout <= kLayoutOct; ++layout) in.layouts |= present[layout] != nullptr ? 1u << layout : 0u;
        in.rootLo = wide.rootLo, in.rootHi = wide.rootHi, in.originBound = wide.originBound;
        in.camera = params.camera, in.numBounces = params.samplingParams.numBounces;
        in.aovs = books.on(Books::kAovs), in.moments = books.on(Books::kMoments), in.buckets = books.on(Books::kBuckets);
        in.bucketPlanes = books.sums(Books::kBuckets).planes, in.bucketSamples = books.sums(Books::kBuckets).samples;
        in.numTiles = static_cast<uint32_t>(tiles.size()), in.validPixels = validPixels;
        if (active) in.active = *active;
        return in;
    }
    // the path state holds a batch of `paths` (the AOV records included while the AOVs are on)
    bool pathStateHolds(uint64_t paths) const { return paths <= allocatedPaths && (!books.on(Books::kAovs) || sAov.count >= 2 * paths); }

    void releasePathState()
    {
        sRayO.release(), sRayD.release(), sRayD2.release(), sThr.release(), sThr2.release(), sRad.release(), sHit.release();
        sPending.release(), sNoise.release(), sNoise2.release(), queueA.release(), queueB.release(), missQueue.release(), missSlots.release(), shadowList.release();
        sAov.release();
        allocatedPaths = 0;
    }

    // Path streams and queues are allocated on demand for the largest batch actually traced
    // (at most maxPaths): small renders stay small, big ones use the HBM that is there.
    // Returns false when the device is out of memory: nothing stays allocated then (allocatedPaths = 0), and the
    // caller retries with a smaller batch.  allocatedPaths is only raised once every buffer exists.
    bool ensurePathState(uint64_t paths)
    {
        if (pathStateHolds(paths)) return true;
        RF_HIP(hipStreamSynchronize(stream));
        releasePathState();
        const auto tryAlloc = [](auto& buf, uint64_t n) -> bool {
            void* p = nullptr;
            const hipError_t e = hipMalloc(&p, n * sizeof(*buf.ptr));
            if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
            {
                (void)hipGetLastError(); // clear the sticky error
                return false;
            }
            RF_HIP(e);
            buf.ptr = static_cast<decltype(buf.ptr)>(p);
            buf.count = n;
            return true;
        };
        const bool ok = tryAlloc(sRayO, paths) && tryAlloc(sRayD, paths) && tryAlloc(sRayD2, paths) && tryAlloc(sThr, paths) && tryAlloc(sThr2, paths) &&
                        tryAlloc(sRad, paths) && tryAlloc(sHit, paths) && tryAlloc(sPending, paths) && tryAlloc(sNoise, paths) && tryAlloc(sNoise2, paths) &&
                        tryAlloc(queueA, paths) && tryAlloc(queueB, paths) && tryAlloc(missQueue, paths) && tryAlloc(missSlots, paths) && tryAlloc(shadowList, paths) &&
                        (!books.on(Books::kAovs) || tryAlloc(sAov, 2 * paths));
        if (!ok)
        {
            releasePathState();
            return false;
        }
        allocatedPaths = paths;
        return true;
    }

    // Largest batch (in paths) the device can hold right now: what is free plus what the path state already holds, with a
    // tenth kept back for the allocator's granularity and for whoever else uses the device.
    uint64_t pathsThatFit()
    {
        size_t freeBytes = 0, totalBytes = 0;
        RF_HIP(hipMemGetInfo(&freeBytes, &totalBytes));
        // (the per-pixel leaf lists of bounce 1, where a batch would use them: what is not allocated yet comes off the budget)
        const uint64_t listsWanted = primaryListBytesWanted(options, policyInputs(), validPixels), listsHeld = primaryListBytes();
        const uint64_t budget = static_cast<uint64_t>(freeBytes) + pathStateBytes();
        const uint64_t reserve = listsWanted > listsHeld ? listsWanted - listsHeld : 0u;
        return (budget > reserve ? budget - reserve : 0u) / 10 * 9 / bytesPerPath();
    }

    void configureShard()
    {
        tiles = tilesForRank(params.width, params.height, books.rank(), books.worldSize());
        books.setShardTiles(static_cast<uint32_t>(tiles.size()));
        tileIds.alloc(2 * tiles.size());
        const uint64_t pixelsPadded = static_cast<uint64_t>(tiles.size()) * 1024;
        const TileGrid::Prefix valid = grid().validPrefix(tiles);
        validPixels = valid.total;
        tileValidBefore.alloc(valid.before.size());
        uploadTileList(tiles, nullptr);
        if (image == nullptr || image == ownedImage.ptr)
        {
            ownedImage.alloc(std::max<uint64_t>(pixelsPadded, 1));
            image = ownedImage.ptr;
        }
        else if (imageBytes < pixelsPadded * sizeof(float4))
        {
            throw std::runtime_error("bound accumulation buffer is too small for this shard");
        }
        if (image == ownedImage.ptr) imageBytes = pixelsPadded * sizeof(float4);
        books.restartAccumulation();
    }

    // Zero `bytes` of the image (on the stream) if no sample has gone into it since the accumulation was restarted.  The callers' byte counts, kept as they were:
    //   clearStaleSums (render, render_adaptive)    the shard's tiles x 1024 x 16
    //   meanOnDevice, readTonemapped                the same, from the 32-bit pixel count these two launch their kernels with
    //   clearAccumulationIfStale (the frame gather) min(the shard's tiles x 1024 x 16, imageBytes): a bound buffer is never written past the size its owner gave
    // (configureShard and bindAccumulationBuffer refuse a bound buffer smaller than the shard, so the first two stay inside it as well)
    void zeroImageIfStale(uint64_t bytes)
    {
        if (!books.stale(Books::kImage)) return;
        RF_HIP(hipMemsetAsync(image, 0, bytes, stream)); // wgsl:47-49
        books.zeroed(Books::kImage);
    }
    TileGrid grid() const { return TileGrid(params.width, params.height); }
    // row-major width * height * 4 floats <- a compact tile-major buffer of the shard; nullptr (nothing summed yet): all zeros, without a device copy
    void readCompact(const float4* device, float* dst) const
    {
        const size_t pixelsPadded = tiles.size() * 1024;
        std::memset(dst, 0, static_cast<size_t>(params.width) * params.height * 4 * sizeof(float));
        if (device == nullptr || pixelsPadded == 0) return;
        std::vector<float> compact(pixelsPadded * 4);
        RF_HIP(hipMemcpy(compact.data(), device, pixelsPadded * sizeof(float4), hipMemcpyDeviceToHost));
        untileHost(compact.data(), tiles.data(), static_cast<uint32_t>(tiles.size()), params.width, params.height, dst);
    }

    template<typename F>
    void launchTimed(int kind, F&& launch, uint32_t bounce = 0)
    {
        if (timing)
        {
            TimedLaunch t{getEvent(), getEvent(), kind, std::min(bounce, RenderStats::kMaxBounceStats - 1)};
            RF_HIP(hipEventRecord(t.start, stream));
            launch();
            RF_HIP(hipEventRecord(t.stop, stream));
            timed.push_back(t);
        }
        else
        {
            launch();
        }
    }

    void collectTimings()
    {
        if (timed.empty()) return;
        RF_HIP(hipStreamSynchronize(stream));
        for (const TimedLaunch& t : timed)
        {
            float ms = 0.0f;
            RF_HIP(hipEventElapsedTime(&ms, t.start, t.stop));
            switch (t.kind)
            {
            case 0: hostStats.msRaygen += ms; hostStats.launchesRaygen++; break;
            case 1: hostStats.msClosest += ms; hostStats.launchesClosest++; hostStats.msClosestByBounce[t.bounce] += ms; break;
            case 2: hostStats.msShade += ms; hostStats.launchesShade++; break;
            case 3: hostStats.msShadow += ms; hostStats.launchesShadow++; hostStats.msShadowByBounce[t.bounce] += ms; break;
            default: hostStats.msAccumulate += ms; hostStats.launchesAccumulate++; break;
            }
            eventPool.push_back(t.start);
            eventPool.push_back(t.stop);
        }
        timed.clear();
    }

    void collectBatchTimings()
    {
        for (const BatchTiming& b : pendingBatches)
        {
            RF_HIP(hipEventSynchronize(b.stop));
            float ms = 0.0f;
            RF_HIP(hipEventElapsedTime(&ms, b.start, b.stop));
            for (uint32_t i = 0; i < b.samples; ++i)
            {
                passDurationsMs.push_back(ms / static_cast<float>(b.samples));
                if (passDurationsMs.size() > 30) passDurationsMs.pop_front();
            }
            eventPool.push_back(b.start);
            eventPool.push_back(b.stop);
        }
        pendingBatches.clear();
    }

    // what a kTraceWide launch takes besides its plan: the streams, the queue with its count and cursor, the batch's geometry
    struct WideArgs
    {
        PathStreams     ps;
        const uint32_t* queue;
        const uint32_t* count;
        uint32_t*       cursor;
        float           tMax;
        dim3            grid;
        uint32_t        blocksWanted = 0; // != 0: the launch's worst-case workgroup count; the grid becomes min(this, what the device holds of the kernel launched)
        DeviceCounters* counters = nullptr; // nullptr: the handle's; a ray query's rays count into a block of their own (castRays), rf_stats never sees them
    };
    // Workgroups of THIS instantiation the device holds at once.  The persistent grid used to be sized once, from the closest-hit kernel (6 per CU: 80 VGPRs, 24 KB of LDS); the
    // any-hit instantiations need 63 ... 72 VGPRs and -- round 6: their stack holds child words only, 4 bytes per entry -- 12 KB: most of them fit 7 per CU.
    uint32_t residentBlocks(TraceWideKernel k, uint32_t extraLds)
    {
        const auto key = std::make_pair(reinterpret_cast<const void*>(k), extraLds);
        const auto it = residentCache.find(key);
        if (it != residentCache.end()) return it->second;
        int perCu = 0;
        RF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, reinterpret_cast<const void*>(k), kBlock, extraLds));
        const uint32_t n = static_cast<uint32_t>(std::max(perCu, 1)) * std::max(multiProcessors, 1u);
        residentCache[key] = n;
        return n;
    }
    // One kTraceWide launch, as its plan says
    void launchWide(const TraversalPlan& t, const WideScene& w, const WideArgs& a)
    {
        const TraceWideKernel k = traceWideKernel(t.anyHit, t.count, t.nearest, t.layout, t.dense);
        if (k == nullptr) throw std::logic_error("kTraceWide: record layout " + std::to_string(t.layout) + " is not compiled into this build");
        dim3 grid = a.grid;
        if (a.blocksWanted != 0u && !wideBlocksForced && !t.count) grid = dim3(std::min(a.blocksWanted, residentBlocks(k, t.extraLds)));
        hipLaunchKernelGGL(k, grid, dim3(kBlock), t.extraLds, stream, scene, w, sky, sunBasis, a.ps, a.queue, a.count, a.cursor, a.counters ? a.counters : counters.ptr, t.refillMin, t.leafVote, t.chunk, a.tMax, t.flags);
    }
    // Is a cached any-hit launch of the handle's NEXT batch free to run behind kShadowFirstLook, as far as the books a batch keeps go?  traceBatch's own bookkeeping,
    // foreseen without touching it (rf_renderer_launch_plan): a grid of another size starts cold, a report that has landed may start a hold-off, a running one counts down.
    bool nextBatchFirstLookReady(const BatchPlan& b) const
    {
        if (!b.occluderGrid || occluderGrid.count != b.occluderGridEntries || !occluderGridWarm) return false;
        if (lookPending && hipEventQuery(lookEvent) == hipSuccess) return !(lookBatchHost[1] != 0ull && lookBatchHost[0] * 4ull < lookBatchHost[1]) && firstLookHoldOff == 0u;
        return firstLookHoldOff <= 1u;
    }

    // Test hook (option query_variant = 2): arbitrary rays through the render path's persistent
    // traversal kernel.  closest: out0 = hit stream {tri, u, v, t}, out1 = rayO stream (offset hit
    // point); shadow: out0 = rad stream, .x != 0 iff the ray is unoccluded.
    void queryWide(const float* rays6, uint64_t n, float tMax, bool shadow, std::vector<float4>& out0, std::vector<float4>& out1)
    {
        if (n > 0xFFFFFFFFull) throw std::runtime_error("too many rays");
        const LaunchOptions& opt = options;
        const PolicyInputs   in = policyInputs();
        const uint32_t denseFlag = std::min(opt.optDenseLeafMin, 15u) << kFlagDenseLeafShift; // (the dense leaf phase, as in the render path)
        if (!ensurePathState(n)) throw std::runtime_error("out of device memory for the ray batch");
        std::vector<P3>       o(n), d(n);
        std::vector<uint32_t> ids(n);
        for (uint64_t i = 0; i < n; ++i)
        {
            o[i] = P3{rays6[6 * i], rays6[6 * i + 1], rays6[6 * i + 2]};
            d[i] = P3{rays6[6 * i + 3], rays6[6 * i + 4], rays6[6 * i + 5]};
            ids[i] = static_cast<uint32_t>(i);
        }
        // every copy goes through the handle's stream: ordered behind a batch that may still be in flight there
        RF_HIP(hipStreamSynchronize(stream));
        RF_HIP(hipMemcpyAsync(sRayO.ptr, o.data(), n * sizeof(P3), hipMemcpyHostToDevice, stream));
        RF_HIP(hipMemcpyAsync(sRayD.ptr, d.data(), n * sizeof(P3), hipMemcpyHostToDevice, stream));
        RF_HIP(hipMemcpyAsync(queueA.ptr, ids.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        const BatchCounters qc{nullptr, 0u}; // (no bounce: the queue's length, then the one launch's cursor)
        const uint32_t words = qc.words() + BatchCounters::kCursorWords;
        if (queueCounts.count < words) queueCounts.alloc(words);
        RF_HIP(hipMemsetAsync(queueCounts.ptr, 0, queueCounts.count * sizeof(uint32_t), stream));
        const uint32_t count = static_cast<uint32_t>(n);
        RF_HIP(hipMemcpyAsync(queueCounts.ptr, &count, sizeof count, hipMemcpyHostToDevice, stream));
        PathStreams ps{sRayO.ptr, sRayD.ptr, sThr.ptr, sRad.ptr, sHit.ptr, sPending.ptr, sNoise.ptr, sRayD2.ptr, sThr2.ptr, sNoise2.ptr};
        const dim3  grid(std::min<uint32_t>(static_cast<uint32_t>((n + kBlock - 1) / kBlock), wideBlocks));
        const WideArgs wa{ps, queueA.ptr, queueCounts.ptr + qc.queueWord(0), queueCounts.ptr + qc.cursorClosestWord(1), tMax, grid};
        if (shadow)
        {
            // rad = 0, pending = 1: rad.x becomes visibility * SOLAR_INV_PDF
            std::vector<P3> ones(n, P3{1.0f, 1.0f, 1.0f});
            RF_HIP(hipMemcpyAsync(sPending.ptr, ones.data(), n * sizeof(P3), hipMemcpyHostToDevice, stream));
            RF_HIP(hipMemsetAsync(sRad.ptr, 0, n * sizeof(float4), stream));
            RF_HIP(hipStreamSynchronize(stream)); // `ones` leaves scope before the launches are waited for
            // (the ray-query entry points take the layout the test asks for -- query_compact -- where the scene has it; the oct records serve closest-hit rays only)
            const int layout = layoutIfPresent(in, (opt.optQueryCompact == kLayoutOct || (!opt.shadowNearestFirst && opt.optQueryCompact < kLayoutQuad)) ? kLayoutBinary : opt.optQueryCompact);
            launchWide(resolveTraversal(opt, in, true, layout, false, opt.shadowNearestFirst, kFlagShadowDirFromStream | denseFlag, opt.optRefillMin, opt.optChunk, 0u, 0u), wide, wa);
        }
        else
        {
            // RF_DEBUG_QUERY_LIST=<file of n u32>: (read and uploaded BEFORE the timed span) the launch visits the rays in the order of that list (queue POSITIONS, as the any-hit launches behind kShadowFirstLook do) while
            // the rays stay where they are -- what a global order of a bounce's rays costs when only an index list is sorted (tools/gpu_sort_potential.py --indirect)
            WideScene wq = wide;
            wq.rayList = nullptr;
            if (const char* listPath = std::getenv("RF_DEBUG_QUERY_LIST"))
            {
                std::vector<uint32_t> list(n);
                FILE* f = std::fopen(listPath, "rb");
                if (f == nullptr || std::fread(list.data(), sizeof(uint32_t), n, f) != n) throw std::runtime_error("RF_DEBUG_QUERY_LIST: cannot read the ray list");
                std::fclose(f);
                RF_HIP(hipMemcpyAsync(queueB.ptr, list.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                RF_HIP(hipStreamSynchronize(stream));
                wq.rayList = queueB.ptr;
            }
            // RF_DEBUG_QUERY_MS: the traversal launch alone between two events (tools/gpu_sort_potential.py: what would an order of the rays be worth?)
            const bool timed = std::getenv("RF_DEBUG_QUERY_MS") != nullptr;
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (timed)
            {
                RF_HIP(hipEventCreate(&e0));
                RF_HIP(hipEventCreate(&e1));
                RF_HIP(hipEventRecord(e0, stream));
            }
            launchWide(resolveTraversal(opt, in, false, layoutIfPresent(in, opt.optQueryCompact), false, false, denseFlag, opt.optRefillMin, opt.optChunk, 0u, 0u), wq, wa);
            if (timed) RF_HIP(hipEventRecord(e1, stream));
            hipLaunchKernelGGL(hitPointsKernel(), dim3((count + 255) / 256), dim3(256), 0, stream, scene, sHit.ptr, sRayO.ptr, count);
            if (timed)
            {
                RF_HIP(hipStreamSynchronize(stream));
                float ms = 0.0f;
                RF_HIP(hipEventElapsedTime(&ms, e0, e1));
                std::fprintf(stderr, "[rf-query] closest-hit launch: %u rays, %.4f ms\n", count, ms);
                RF_HIP(hipEventDestroy(e0));
                RF_HIP(hipEventDestroy(e1));
            }
        }
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(stream));
        out0.resize(n);
        RF_HIP(hipMemcpy(out0.data(), shadow ? sRad.ptr : sHit.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
        if (!shadow)
        {
            std::vector<P3> packed(n);
            RF_HIP(hipMemcpy(packed.data(), sRayO.ptr, n * sizeof(P3), hipMemcpyDeviceToHost));
            out1.resize(n);
            for (uint64_t i = 0; i < n; ++i) out1[i] = make_float4(packed[i].x, packed[i].y, packed[i].z, 0.0f);
        }
    }

    // rf_renderer_cast_rays: chunk by chunk kCastLoad, the traversal launch the policy picks, kCastResolve (rf_ray_query.hip), all on the handle's stream with one wait at
    // the end.  The path state is scratch between render calls (as queryWide assumes); the queue words and the counter block are the query's own, the occluder grid and
    // the first-look bookkeeping are neither read nor written.  Every refusal has been made before the first launch (Renderer::castRays).
    void castRays(const RayQueryRequest& q, const ChunkPlan& chunks)
    {
        const bool          anyHit = q.kind == kRaysAny;
        const TraversalPlan t = planRayQuery(options, policyInputs(), anyHit);
        if (!ensurePathState(chunks.depth())) throw std::runtime_error("out of device memory for a chunk of " + std::to_string(chunks.depth()) + " rays (option cast_chunk makes the chunks smaller)");
        constexpr uint32_t kWords = BatchCounters::kLine + BatchCounters::kCursorWords;
        if (castWords.count < kWords) castWords.alloc(kWords);
        if (castCounters.count < 1) castCounters.alloc(1);
        RF_HIP(hipMemsetAsync(castCounters.ptr, 0, sizeof(DeviceCounters), stream));
        const PathStreams ps{sRayO.ptr, sRayD.ptr, sThr.ptr, sRad.ptr, sHit.ptr, sPending.ptr, sNoise.ptr, sRayD2.ptr, sThr2.ptr, sNoise2.ptr};
        WideScene         w = wide; // (no list of queue positions, no occluder grid: the render batches' own)
        w.rayList = nullptr, w.occGrid = nullptr;
        const uint32_t mask = q.mask();
        const auto     advanced = [&](uint32_t output, uint64_t firstRay) -> uint64_t { return q.outputs[output] ? q.outputs[output] + firstRay * kCastOutputWidth[output] * 4u : 0u; };
        for (uint64_t c = 0; c < chunks.count(); ++c)
        {
            const uint64_t firstRay = chunks.first(c);
            // (workgroup counts in 64 bits: a chunk may hold up to 2^32 - 1 rays, whatever the device's memory allows today)
            const uint32_t n = static_cast<uint32_t>(chunks.size(c));
            const uint32_t blocks = static_cast<uint32_t>((uint64_t{n} + kBlock - 1) / kBlock), castBlocks = static_cast<uint32_t>((uint64_t{n} + kCastBlock - 1) / kCastBlock);
            RF_HIP(hipMemsetAsync(castWords.ptr, 0, kWords * sizeof(uint32_t), stream)); // the cursors start at 0
            hipLaunchKernelGGL(castLoadKernel(anyHit), dim3(castBlocks), dim3(kCastBlock), 0, stream, reinterpret_cast<const float*>(q.origins + firstRay * q.originStride * 4u),
                               reinterpret_cast<const float*>(q.directions + firstRay * q.directionStride * 4u), q.originStride, q.directionStride, n, ps, queueA.ptr, castWords.ptr);
            if (t.kernel == kKernelWide)
                launchWide(t, w, WideArgs{ps, queueA.ptr, castWords.ptr, castWords.ptr + BatchCounters::kLine, q.tMax, dim3(std::min(blocks, wideBlocks)), blocks, castCounters.ptr});
            else hipLaunchKernelGGL(castScalarKernel(anyHit), dim3(blocks), dim3(kBlock), 0, stream, scene, ps, n, q.tMax);
            CastOutputs out{};
            out.triangle = reinterpret_cast<uint32_t*>(advanced(0, firstRay)), out.t = reinterpret_cast<float*>(advanced(1, firstRay));
            out.bary = reinterpret_cast<float*>(advanced(2, firstRay)), out.position = reinterpret_cast<float*>(advanced(3, firstRay));
            out.geometricNormal = reinterpret_cast<float*>(advanced(4, firstRay)), out.normal = reinterpret_cast<float*>(advanced(5, firstRay));
            out.texcoord = reinterpret_cast<float*>(advanced(6, firstRay)), out.albedo = reinterpret_cast<float*>(advanced(7, firstRay));
            out.texture = reinterpret_cast<uint32_t*>(advanced(8, firstRay)), out.visibility = reinterpret_cast<float*>(advanced(9, firstRay));
            hipLaunchKernelGGL(castResolveKernel(), dim3(castBlocks), dim3(kCastBlock), 0, stream, scene, sHit.ptr, sRad.ptr, out, n, mask);
        }
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(stream)); // the outputs may be used from any stream once the call returns
    }

    // Before the first sample of an accumulation: zero the sums that were cleared (the image, and the AOV sums / moments while they are on), sized for the shard
    void clearStaleSums(uint64_t pixelsPadded)
    {
        zeroImageIfStale(pixelsPadded * sizeof(float4));
        for (uint32_t i = Books::kAovs; i < Books::kFamilies; ++i)
        {
            const Books::Family f = static_cast<Books::Family>(i);
            if (!books.stale(f)) continue;
            storage[f].zero(stream, pixelsPadded * books.sums(f).planes);
            books.zeroed(f);
        }
    }

    // Samples per batch for `todo` samples of `pixelsPadded` path slots per sample (the shard's tiles, or the active tiles of render_adaptive), with the path state
    // for it allocated.
    uint32_t batchSamples(uint32_t todo, uint64_t pixelsPadded)
    {
        // equal batches (320 samples with room for 256 per batch -> 160 + 160, not 256 + 64): a small trailing batch has
        // short launches and, with few samples per pixel, less coherent waves
        // maxPaths is the CONFIGURED depth (the default or the caller's) and is never changed here: what a call has to give up
        // because memory is short at that moment (another handle alive, a shared GPU) is given up for that call only.
        uint32_t       n = 0;
        uint64_t       depth = maxPaths;
        for (;;)
        {
            const uint32_t perBatch = static_cast<uint32_t>(std::max<uint64_t>(1, depth / pixelsPadded));
            const uint32_t numBatches = (todo + perBatch - 1) / perBatch;
            n = (todo + numBatches - 1) / numBatches;
            const uint64_t need = static_cast<uint64_t>(n) * pixelsPadded;
            if (pathStateHolds(need)) break;
            // The batch depth is a speed knob, never a requirement: a device with less free memory than the
            // batch wants (a smaller or shared GPU, a second handle on this one) traces the same samples in more, smaller
            // batches -- same image.  First by what hipMemGetInfo reports, then by halving if hipMalloc still refuses.
            const uint64_t fit = pathsThatFit();
            if (need > fit && n > 1)
            {
                depth = std::max<uint64_t>(pixelsPadded, std::min(depth / 2, fit));
                continue;
            }
            if (ensurePathState(need)) break;
            if (n == 1) throw std::runtime_error("out of device memory: one sample of the frame (" + std::to_string(need * bytesPerPath() >> 20) + " MiB of path state) does not fit");
            depth = std::max<uint64_t>(pixelsPadded, depth / 2);
        }
        if (depth != effectivePaths)
        {
            // said once per change, not per batch: shallower batches are a silent loss of speed otherwise
            if (depth < maxPaths)
                std::fprintf(stderr, "[rf] device memory is short: batches of %llu paths instead of the configured %llu (%u samples per batch); same image, shorter launches\n",
                             static_cast<unsigned long long>(depth), static_cast<unsigned long long>(maxPaths), n);
            else if (effectivePaths != 0 && effectivePaths < maxPaths)
                std::fprintf(stderr, "[rf] device memory is back: batches of the configured %llu paths again\n", static_cast<unsigned long long>(maxPaths));
            effectivePaths = depth;
        }
        return n;
    }

    // the non-uniform counts on the device, for the per-tile reads (the stream is made idle first: an earlier read may still use the buffer)
    const uint32_t* uploadTileSamples()
    {
        RF_HIP(hipStreamSynchronize(stream));
        const std::vector<uint32_t>& tileSamples = books.tileSamples();
        if (tileSamplesDevice.count < tileSamples.size()) tileSamplesDevice.alloc(tileSamples.size());
        RF_HIP(hipMemcpy(tileSamplesDevice.ptr, tileSamples.data(), tileSamples.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        return tileSamplesDevice.ptr;
    }
    // the counts the per-tile reads take: the non-uniform state's, uploaded (the call first waits for the stream), or nullptr: the accumulated count for every pixel
    const uint32_t* nonUniformTileSamples() { return books.nonUniform() ? uploadTileSamples() : nullptr; }
    // What the post-process passes read (rf_frame_sums.hpp): the handle's own compact tile-major sums (a family that is off: nullptr) at the accumulated count;
    // tileSamples: the per-tile counts on the device, as the pass is to see them
    FrameSums frameSums(const uint32_t* tileSamples) const
    {
        return FrameSums{image, moments(), aovAlbedoCoverage(), aovNormalDepth(), direct(), params.width, params.height, grid().tilesX, books.accumulated(), tileSamples};
    }
    // kTileMean over the accumulation into meanImage, waited for: every pixel divided by its tile's count (uniform state: the accumulated count; nothing accumulated: 0)
    const float4* meanOnDevice()
    {
        const uint32_t n = static_cast<uint32_t>(tiles.size() * 1024);
        RF_HIP(hipStreamSynchronize(stream));
        if (meanImage.count < n) meanImage.alloc(n);
        zeroImageIfStale(static_cast<size_t>(n) * sizeof(float4));
        const uint32_t* counts = nonUniformTileSamples();
        hipLaunchKernelGGL(tileMeanKernel(), dim3((n + 255) / 256), dim3(256), 0, stream, static_cast<const float4*>(image), counts, books.accumulated(), n, meanImage.ptr);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(stream));
        return meanImage.ptr;
    }

    // tileIds / tileValidBefore <- a list of tile ids (ascending) of the shard's tiles and, behind the ids, their slots in the shard (slots == nullptr: 0, 1, ...: the
    // shard's own list).  The stream must be idle (the copies are synchronous).  -> pixels inside the frame
    uint64_t uploadTileList(const std::vector<uint32_t>& list, const std::vector<uint32_t>* slots)
    {
        const auto [before, valid] = grid().validPrefix(list);
        if (2 * list.size() > tileIds.count || before.size() > tileValidBefore.count || (slots && slots->size() != list.size())) throw std::logic_error("tile list longer than the shard's");
        std::vector<uint32_t> both(list);
        for (uint32_t k = 0; k < list.size(); ++k) both.push_back(slots ? (*slots)[k] : k);
        if (!both.empty()) RF_HIP(hipMemcpy(tileIds.ptr, both.data(), both.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        RF_HIP(hipMemcpy(tileValidBefore.ptr, before.data(), before.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        return valid;
    }

    // One batch of at most `todo` samples of `pixelsPadded` path slots each (the shard's tiles, or the `active` list of render_adaptive), and its books.  -> samples traced
    uint32_t step(uint32_t todo, uint64_t pixelsPadded, const ActiveTiles* active)
    {
        const uint32_t n = batchSamples(todo, pixelsPadded);
        traceBatch(books.frameCount(), n, active);
        hostStats.batchSamplesUsed = n, hostStats.batchPathsUsed = static_cast<uint64_t>(n) * pixelsPadded, ++hostStats.batchesTraced;
        books.recordStep(n);
        return n;
    }

    // ---- the launch groups of a bounce: they enqueue what the bounce's plan says, on the queues and words of BounceIo
    struct BounceIo
    {
        uint32_t      bounce;
        PathStreams   ps;
        uint32_t*     in;  // the bounce's queue
        uint32_t*     out; // the hits kShade appends: the next bounce's queue and this bounce's shadow rays
        BatchCounters words;
        uint32_t      blocks, itemBlocks; // workgroups for one thread per path / per kItems paths
        dim3          persistentGrid;
    };
    static dim3 cappedGrid(uint32_t blocks, uint32_t cap) { return dim3(cap ? std::min(blocks, cap) : blocks); }
    // Bounce 1 over the per-pixel leaf lists (BatchPlan::primaryLists): the lists for this batch's pixels, the walker over the whole queue, then the bounce's own
    // kTraceWide launch over the queue positions the walker handed on (WideScene::rayList; the walker has counted the queue's rays).  The bounce's OUTPUT queue is
    // free until kShade appends to it and holds that list meanwhile; its length is a device word, so an empty list costs one short launch.
    void enqueuePrimaryLists(const BatchPlan& b, const FrameParams& fp, const TraversalPlan& t, const BounceIo& io)
    {
        uint32_t* const countIn = io.words.queueCount(0);
        hipLaunchKernelGGL(pixelLeafListsKernel(), dim3((fp.pixelsPadded + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, fp, scene, tileIds.ptr, b.primaryListCapacity, primaryLists.ptr,
                           primaryLengths.ptr);
        hipLaunchKernelGGL(traceLeafListsKernel(), cappedGrid(io.itemBlocks, std::max(multiProcessors, 1u) * 32u), dim3(kBlock), 0, stream, scene, io.ps, countIn, fp.divNumSamples, wide.constOriginX,
                           wide.constOriginY, wide.constOriginZ, primaryLists.ptr, primaryLengths.ptr, b.primaryListCapacity, io.out, io.words.primaryFallbackCount(), counters.ptr, kTMax);
        WideScene     w = wide;
        TraversalPlan rest = t;
        w.rayList = io.out;
        rest.flags |= kFlagNoRayCount;
        launchWide(rest, w, WideArgs{io.ps, io.in, io.words.primaryFallbackCount(), io.words.cursorClosest(io.bounce), kTMax, io.persistentGrid, io.blocks});
    }
    // The same with generation and shading in the list walk's kernel (BatchPlan::primaryFused): kPixelLeafLists, kPrimaryFused -- which fills the queue's count word,
    // appends its hits to the bounce's output queue, its misses to the miss lists and, with the batch's bounce-1 shade flags, the shadow rays still to trace to the
    // shadow list --, then kTraceWide over the positions it handed on.  That list lives in the bounce's INPUT throughput stream (12 B per path, nothing in it at
    // bounce 1: kShade and kSky take throughput 1 there); kShade<false, false, true> works through it in the bounce's shade group (enqueueShadeAndSky).
    static uint32_t* primaryFusedFallback(const BounceIo& io) { return reinterpret_cast<uint32_t*>(io.ps.thr); }
    void enqueuePrimaryFused(const BatchPlan& b, const FrameParams& fp, const BouncePlan& p, const BounceIo& io)
    {
        hipLaunchKernelGGL(pixelLeafListsKernel(), dim3((fp.pixelsPadded + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, fp, scene, tileIds.ptr, b.primaryListCapacity, primaryLists.ptr,
                           primaryLengths.ptr);
        hipLaunchKernelGGL(primaryFusedKernel(), dim3(io.itemBlocks), dim3(kBlock), 0, stream, fp, scene, sky, sunBasis, tileIds.ptr, io.ps, io.in, io.words.queueCount(0), primaryLists.ptr,
                           primaryLengths.ptr, b.primaryListCapacity, io.out, io.words.queueCount(1), missQueue.ptr, missSlots.ptr, io.words.missCount(1), shadowList.ptr,
                           io.words.shadowListCount(1), primaryFusedFallback(io), io.words.primaryFallbackCount(), counters.ptr, p.shadeFlags, kTMax);
        WideScene     w = wide;
        TraversalPlan rest = p.closest;
        w.rayList = primaryFusedFallback(io);
        rest.flags |= kFlagNoRayCount;
        launchWide(rest, w, WideArgs{io.ps, io.in, io.words.primaryFallbackCount(), io.words.cursorClosest(io.bounce), kTMax, io.persistentGrid, io.blocks});
    }
    void enqueueClosest(const TraversalPlan& t, const BounceIo& io)
    {
        uint32_t* const countIn = io.words.queueCount(io.bounce - 1);
        if (t.kernel == kKernelScalar)
            hipLaunchKernelGGL(traceClosestKernel(t.count), dim3(io.blocks), dim3(kBlock), 0, stream, scene, io.ps, io.in, countIn, counters.ptr);
#if defined(RF_EXP_LEGACY_LAYOUTS)
        else if (t.kernel == kKernelPacket)
            hipLaunchKernelGGL(tracePacketKernel(false), io.persistentGrid, dim3(kBlock), 0, stream, scene, wide, sky, sunBasis, io.ps, io.in, countIn, counters.ptr, kTMax, t.flags);
#endif
        else
            launchWide(t, wide, WideArgs{io.ps, io.in, countIn, io.words.cursorClosest(io.bounce), kTMax, io.persistentGrid, io.blocks});
    }
    void enqueueShadeAndSky(const BouncePlan& p, const BounceIo& io, bool fused = false)
    {
        uint32_t* const missCount = io.words.missCount(io.bounce);
        // (behind kPrimaryFused only the rays it handed on are left to shade: the unsorted kernel over their list, on a grid sized for a list that is short)
        if (fused)
            hipLaunchKernelGGL(shadeListedKernel(), cappedGrid(io.itemBlocks, std::max(multiProcessors, 1u) * 32u), dim3(kBlock), 0, stream, scene, sky, sunBasis, io.ps, io.in,
                               io.words.primaryFallbackCount(), io.out, io.words.queueCount(io.bounce), missQueue.ptr, missSlots.ptr, missCount, shadowList.ptr,
                               io.words.shadowListCount(io.bounce), p.shadeFlags, p.sortScale, nullptr, primaryFusedFallback(io));
        else
        hipLaunchKernelGGL(shadeKernel(p.shadeSorted, p.shadeAov), cappedGrid(io.itemBlocks, p.itemGridCap), dim3(kBlock), 0, stream, scene, sky, sunBasis, io.ps, io.in,
                           io.words.queueCount(io.bounce - 1), io.out, io.words.queueCount(io.bounce), missQueue.ptr, missSlots.ptr, missCount, shadowList.ptr,
                           io.words.shadowListCount(io.bounce), p.shadeFlags, p.sortScale, p.shadeAov ? sAov.ptr : nullptr, nullptr);
        // the paths that left the scene at this bounce, while its direction / throughput arrays are intact
        // (its slot comes with the miss list: kSky reads nothing of the bounce's queue -- round 5: reading the slot through the queue position was a third
        // dependent gather, and kShade + kSky went from 19.7 to 15.8 ms per 64 spp without it)
        hipLaunchKernelGGL(skyKernel(options.optTranscendentalsF32), dim3(std::min(io.blocks, skyBlocks)), dim3(kBlock), 0, stream, sky, io.ps, missSlots.ptr, missQueue.ptr, missCount, p.skyFirstBounce);
    }
    void enqueueShadow(const BouncePlan& p, const BounceIo& io)
    {
        uint32_t* const countOut = io.words.queueCount(io.bounce);
        WideScene       wide = this->wide; // (the launches below name `wide`)
        if (p.firstLook)
        {
            // (the bounce's input queue is free by now -- kShade and kSky have consumed it -- and holds the list)
            hipLaunchKernelGGL(shadowFirstLookKernel(), cappedGrid(io.itemBlocks, p.itemGridCap), dim3(kBlock), 0, stream, scene, wide, sky, sunBasis, io.ps, io.out,
                               p.selfShadow ? shadowList.ptr : nullptr, io.words.shadowCount(io.bounce, p.selfShadow ? kFromShadeList : kFromQueue), io.in, io.words.listCount(io.bounce),
                               counters.ptr, kTMax, p.lookFlags);
            wide.rayList = io.in;
        }
        else if (p.selfShadow) wide.rayList = shadowList.ptr; // (positions only: bit 31 clear, the traversal kernel takes its own first look)
        const TraversalPlan& t = p.shadow;
        if (t.kernel == kKernelScalar)
            hipLaunchKernelGGL(traceShadowKernel(t.count), dim3(io.blocks), dim3(kBlock), 0, stream, scene, sky, sunBasis, io.ps, io.out, countOut, counters.ptr, t.flags);
#if defined(RF_EXP_LEGACY_LAYOUTS)
        else if (t.kernel == kKernelPacket)
            hipLaunchKernelGGL(tracePacketKernel(true), io.persistentGrid, dim3(kBlock), 0, stream, scene, wide, sky, sunBasis, io.ps, io.out, countOut, counters.ptr, kTMax, t.flags);
#endif
        else
            launchWide(t, wide, WideArgs{io.ps, io.out, io.words.shadowCount(io.bounce, p.shadowSource), io.words.cursorShadow(io.bounce), kTMax, io.persistentGrid, io.blocks});
    }
    // the batch's sums in sample order: the image, then the first-hit AOV sums and the radiance second moments (timed with the accumulation: rf_stats has no entry of
    // their own for them) -- or, under a tile list, the image and the moments from one launch, then the AOV sums --, then the bucket sums (their own argument list)
    void enqueueSums(const BatchPlan& b, const FrameParams& fp, const PathStreams& ps)
    {
        struct SumLaunch
        {
            SumKernel     kernel;
            uint32_t      pixels; // per workgroup
            bool          runs;   // an LDS-staged kernel: a 64-lane workgroup; else one lane per pixel, kBlock of them
            const float4* src;
            float4 *      dst0, *dst1;
        };
        const auto sumGrid = [&](uint32_t pixelsPerGroup) { return dim3((fp.pixelsPadded + pixelsPerGroup - 1) / pixelsPerGroup); };
        SumLaunch  launches[3];
        uint32_t   n = 0;
        const SumAddressing listAddressing = b.shardList ? SumAddressing::ShardList : SumAddressing::TileList;
        // (the headline image kernel, the whole runs in dynamic LDS, keeps its own argument list: rf_sums.hip)
        if (b.accumulateKernel == kAccumulateRuns)
            hipLaunchKernelGGL(accumulateRunsKernel(b.accumulatePixels), sumGrid(b.accumulatePixels), dim3(64), b.accumulatePixels * 3u * (b.numSamples + 1u) * sizeof(float), stream, fp,
                               tileIds.ptr, ps, image);
        else if (b.accumulateKernel == kAccumulateTiles) launches[n++] = {sumKernel(Sum::RadianceMoments, b.runs, listAddressing), b.accumulatePixels, b.runs, ps.rad, image, moments()};
        else launches[n++] = {sumKernel(Sum::Radiance, false, SumAddressing::Compact), b.accumulatePixels, false, ps.rad, image, nullptr};
        if (b.aovPixels != 0u) launches[n++] = {sumKernel(Sum::Aov, b.runs, b.tileList ? listAddressing : SumAddressing::Compact), b.aovPixels, b.runs, sAov.ptr, aovAlbedoCoverage(), aovNormalDepth()};
        if (b.momentPixels != 0u) launches[n++] = {sumKernel(Sum::Moments, b.runs, SumAddressing::Compact), b.momentPixels, b.runs, ps.rad, moments(), nullptr};
        for (uint32_t i = 0; i < n; ++i)
        {
            const SumLaunch& l = launches[i];
            hipLaunchKernelGGL(l.kernel, sumGrid(l.pixels), dim3(l.runs ? 64u : static_cast<uint32_t>(kBlock)), 0, stream, fp, tileIds.ptr, l.src, l.dst0, l.dst1);
        }
        if (b.bucketPixels != 0u)
            hipLaunchKernelGGL(bucketKernel(b.runs, b.tileList ? listAddressing : SumAddressing::Compact), sumGrid(b.bucketPixels), dim3(b.runs ? 64u : static_cast<uint32_t>(kBlock)), 0, stream, fp, tileIds.ptr, ps.rad, bucketPlanes(),
                               bucketStride(), b.buckets, b.bucketPhase);
    }

    // The direct sums (rf_renderer_set_direct), enqueued right behind bounce 1's launch groups: ps.rad then holds each sample's direct light, and D gets it through the
    // accumulate kernel the plan chose for the batch's image -- the same ordered chain, whatever the batch depth or slot order.  Under a tile list (render_adaptive
    // with kDirectTileCounts; checkAdaptive refuses the call without the bit) the list-addressed radiance sum, staged or one lane per pixel as the batch's other sums are.
    void enqueueDirect(const BatchPlan& b, const FrameParams& fp, const PathStreams& ps)
    {
        const auto sumGrid = [&](uint32_t pixelsPerGroup) { return dim3((fp.pixelsPadded + pixelsPerGroup - 1) / pixelsPerGroup); };
        if (b.accumulateKernel == kAccumulateRuns)
            hipLaunchKernelGGL(accumulateRunsKernel(b.accumulatePixels), sumGrid(b.accumulatePixels), dim3(64), b.accumulatePixels * 3u * (b.numSamples + 1u) * sizeof(float), stream, fp,
                               tileIds.ptr, ps, direct());
        else if (b.accumulateKernel == kAccumulatePixels)
            hipLaunchKernelGGL(sumKernel(Sum::Radiance, false, SumAddressing::Compact), sumGrid(b.accumulatePixels), dim3(static_cast<uint32_t>(kBlock)), 0, stream, fp, tileIds.ptr,
                               static_cast<const float4*>(ps.rad), direct(), static_cast<float4*>(nullptr));
        else
            hipLaunchKernelGGL(sumKernel(Sum::Radiance, b.runs, b.shardList ? SumAddressing::ShardList : SumAddressing::TileList), sumGrid(b.accumulatePixels),
                               dim3(b.runs ? 64u : static_cast<uint32_t>(kBlock)), 0, stream, fp, tileIds.ptr, static_cast<const float4*>(ps.rad), direct(), static_cast<float4*>(nullptr));
    }

    // Trace `numSamples` consecutive samples (sample indices start at frame `firstFrame`) of the shard's tiles -- or, active != nullptr, of the tile list that
    // tileIds / tileValidBefore hold then: the radiance and its squares are added by the tile-list kernel, at the listed tiles' own places.
    // The enqueue loop: frame parameters, planBatch, the counters, raygen, per bounce planBounce and its three launch groups, the totals, the sums.
    void traceBatch(uint32_t firstFrame, uint32_t numSamples, const ActiveTiles* active = nullptr)
    {
        const uint64_t validPixels = active ? active->validPixels : this->validPixels;
        const PolicyInputs in = policyInputs(active);
        BatchPlan      batch = planBatch(options, in, numSamples);
        FrameParams    fp{};
        fp.width = params.width;
        fp.height = params.height;
        fp.camera = params.camera;
        fp.samplesPerPixel = params.samplingParams.numSamplesPerPixel;
        fp.numBounces = batch.numBounces;
        fp.firstFrame = firstFrame;
        fp.numSamples = numSamples;
        fp.numTiles = batch.numTiles;
        fp.pixelsPadded = batch.pixelsPadded;
        fp.slotGroupShift = options.optSlotGroupShift;
        fp.samplePerm = fp.sampleInvPerm = nullptr;
        if (batch.samplePerm)
        {
            if (samplePerm.count < 2ull * numSamples) samplePerm.alloc(2ull * numSamples); // (the stream is idle the first time; later batches are no larger)
            fp.samplePerm = samplePerm.ptr;
            fp.sampleInvPerm = samplePerm.ptr + numSamples;
        }
        fp.tilesX = grid().tilesX;
        if (fp.numTiles == 0) return;
        fp.divNumSamples = FastDiv::make(fp.numSamples), fp.divPixelsPadded = FastDiv::make(fp.pixelsPadded), fp.divTilesX = FastDiv::make(fp.tilesX);
        fp.divSamplesPerPixel = FastDiv::make(fp.samplesPerPixel);
        fp.skipOrigins = batch.constOrigin ? 1u : 0u;
        fp.tileValidBefore = batch.denseRaygen ? tileValidBefore.ptr : nullptr;
        fp.validPixels = static_cast<uint32_t>(validPixels);
        wide.constOriginX = params.camera.origin.x, wide.constOriginY = params.camera.origin.y, wide.constOriginZ = params.camera.origin.z;

        const uint64_t paths = static_cast<uint64_t>(numSamples) * fp.pixelsPadded;
        const uint32_t blocks = static_cast<uint32_t>((paths + kBlock - 1) / kBlock);
        primaryRaysHost += static_cast<unsigned long long>(numSamples) * validPixels;
        // bounce b reads direction / throughput from buffer (b - 1) & 1 and kShade writes the next bounce's into the other one
        PathStreams    ps{sRayO.ptr, sRayD.ptr, sThr.ptr, sRad.ptr, sHit.ptr, sPending.ptr, sNoise.ptr, sRayD2.ptr, sThr2.ptr, sNoise2.ptr};
        const uint32_t numBounces = fp.numBounces;

        // the books a batch keeps (allocation on first use, the grid's warmth, the first-look hold-off): the plan takes them as facts
        wide.occGrid = nullptr;
        wide.rayList = nullptr;
        if (batch.occluderGrid)
        {
            if (occluderGrid.count != batch.occluderGridEntries)
            {
                occluderGrid.alloc(batch.occluderGridEntries);
                occluderGridWarm = false;
                RF_HIP(hipMemsetAsync(occluderGrid.ptr, 0, batch.occluderGridEntries * sizeof(uint32_t), stream));
            }
            wide.occGrid = occluderGrid.ptr;
            wide.occScale = batch.occScale;
            wide.occMask = batch.occMask;
        }
        if (lookBatch.count == 0)
        {
            lookBatch.alloc(2);
            RF_HIP(hipHostMalloc(reinterpret_cast<void**>(&lookBatchHost), 2 * sizeof(unsigned long long)));
            RF_HIP(hipEventCreateWithFlags(&lookEvent, hipEventDisableTiming));
        }
        if (lookPending && hipEventQuery(lookEvent) == hipSuccess)
        {
            lookPending = false;
            if (lookBatchHost[1] != 0ull && lookBatchHost[0] * 4ull < lookBatchHost[1]) firstLookHoldOff = 16u;
        }
        else if (firstLookHoldOff != 0u) --firstLookHoldOff;
        batch.firstLookReady = occluderGridWarm && firstLookHoldOff == 0u;
        if (batch.primaryLists)
        {
            // (grown, never shrunk; a batch that cannot have them keeps the kTraceWide launch -- same image)
            const uint64_t entries = validPixels * batch.primaryListCapacity;
            if (primaryLists.count < entries || primaryLengths.count < validPixels)
            {
                RF_HIP(hipStreamSynchronize(stream)); // an earlier batch may still read the old ones
                primaryLists.release(), primaryLengths.release();
                void *pl = nullptr, *pn = nullptr;
                if (hipMalloc(&pl, std::max<uint64_t>(entries, 1) * sizeof(uint32_t)) == hipSuccess && hipMalloc(&pn, std::max<uint64_t>(validPixels, 1) * sizeof(uint32_t)) == hipSuccess)
                {
                    primaryLists.ptr = static_cast<uint32_t*>(pl), primaryLists.count = std::max<uint64_t>(entries, 1);
                    primaryLengths.ptr = static_cast<uint32_t*>(pn), primaryLengths.count = std::max<uint64_t>(validPixels, 1);
                }
                else
                {
                    (void)hipGetLastError(); // out of device memory: clear the sticky error
                    if (pl != nullptr) (void)hipFree(pl);
                    batch.primaryLists = false;
                }
            }
        }
        RF_HIP(hipMemsetAsync(lookBatch.ptr, 0, 2 * sizeof(unsigned long long), stream));
        BatchTiming bt{getEvent(), getEvent(), numSamples};
        RF_HIP(hipEventRecord(bt.start, stream));

        const uint32_t countWords = BatchCounters{nullptr, numBounces}.words();
        if (queueCounts.count < countWords) queueCounts.alloc(countWords);
        const BatchCounters words{queueCounts.ptr, numBounces};
        unsigned long long  lookMask = 0ull, selfMask = 0ull;
        const uint32_t      itemBlocks = static_cast<uint32_t>((paths + kBlock * kItems - 1) / (kBlock * kItems));
        RF_HIP(hipMemsetAsync(queueCounts.ptr, 0, queueCounts.count * sizeof(uint32_t), stream));

        BounceIo io{0u, ps, queueA.ptr, queueB.ptr, words, blocks, itemBlocks, dim3(std::min(blocks, wideBlocks))};
        if (fp.samplePerm)
            hipLaunchKernelGGL(samplePermutationKernel(), dim3((numSamples + 255) / 256), dim3(256), 0, stream, firstFrame, fp.samplesPerPixel, numSamples,
                               const_cast<uint32_t*>(fp.samplePerm), const_cast<uint32_t*>(fp.sampleInvPerm));
        // (bounce 1 fused: the plan's flag, a bounce-1 launch that takes the lists, and a shade launch that is the plain unsorted kernel)
        bool fused = false;
        if (batch.primaryLists && batch.primaryFused && numBounces != 0u)
        {
            const BouncePlan first = planBounce(options, in, 1u, batch);
            fused = first.closest.kernel == kKernelWide && !first.closest.count && !first.shadeSorted && !first.shadeAov;
        }
        // (fused: kPrimaryFused generates the rays inside bounce 1's closest-hit group; nothing runs here and ms_raygen stays 0)
        if (!fused)
            launchTimed(0, [&] {
                hipLaunchKernelGGL(raygenKernel(options.optTranscendentalsF32), dim3(itemBlocks), dim3(kBlock), 0, stream, fp, scene, tileIds.ptr, io.ps, io.in, words.queueCount(0), counters.ptr);
            });
        for (io.bounce = 1; io.bounce <= numBounces; ++io.bounce)
        {
            const BouncePlan plan = planBounce(options, in, io.bounce, batch);
            if (plan.selfShadow) selfMask |= 1ull << (io.bounce - 1);
            if (plan.firstLook) lookMask |= 1ull << (io.bounce - 1);
            // (the list launches run inside the timing group of the bounce's closest-hit launch: ms_closest, launches_closest and the per-bounce figures keep their meaning)
            const bool lists = io.bounce == 1u && batch.primaryLists && plan.closest.kernel == kKernelWide && !plan.closest.count;
            const bool fusedNow = fused && io.bounce == 1u;
            launchTimed(1, [&] {
                if (fusedNow) enqueuePrimaryFused(batch, fp, plan, io);
                else if (lists) enqueuePrimaryLists(batch, fp, plan.closest, io);
                else enqueueClosest(plan.closest, io);
            }, io.bounce - 1);
            launchTimed(2, [&] { enqueueShadeAndSky(plan, io, fusedNow); });
            launchTimed(3, [&] { enqueueShadow(plan, io); }, io.bounce - 1);
            if (io.bounce == 1u && books.on(Books::kDirect)) launchTimed(4, [&] { enqueueDirect(batch, fp, io.ps); });
            std::swap(io.in, io.out);
            std::swap(io.ps.rayD, io.ps.rayDOut);
            std::swap(io.ps.thr, io.ps.thrOut);
            std::swap(io.ps.noise, io.ps.noiseOut);
        }
        hipLaunchKernelGGL(bounceTotalsKernel(), dim3(1), dim3(64), 0, stream, words.base, std::min(numBounces, 64u), bounceTotals.ptr, words.listCount(1), lookMask, lookBatch.ptr, words.shadowListCount(1), selfMask, counters.ptr);
        if (lookMask != 0ull && lookBatchHost != nullptr)
        {
            RF_HIP(hipMemcpyAsync(lookBatchHost, lookBatch.ptr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            RF_HIP(hipEventRecord(lookEvent, stream));
            lookPending = true;
        }
        if (wide.occGrid != nullptr) occluderGridWarm = true;
        // RF_DEBUG_PRIMARY_LISTS: the batch's list lengths as a histogram on stderr (waits for the batch: a measurement aid, profiles/primary_lists)
        if (batch.primaryLists && numBounces != 0u && std::getenv("RF_DEBUG_PRIMARY_LISTS") != nullptr)
        {
            std::vector<uint32_t> len(validPixels);
            RF_HIP(hipStreamSynchronize(stream));
            RF_HIP(hipMemcpy(len.data(), primaryLengths.ptr, len.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::vector<uint64_t> histogram(kPrimaryListMaxCapacity + 1u, 0);
            uint64_t              none = 0, sum = 0, why[8] = {};
            for (const uint32_t w : len)
                if ((w & kNoPrimaryList) != 0u) ++none, ++why[w & 7u];
                else ++histogram[w & 0xFFu], sum += w & 0xFFu;
            std::fprintf(stderr, "[rf-primary-lists] pixels %zu, without a list %llu (%.4f %%), mean length %.3f, capacity %u, samples %u | length:count", len.size(),
                         static_cast<unsigned long long>(none), len.empty() ? 0.0 : 100.0 * static_cast<double>(none) / static_cast<double>(len.size()),
                         len.size() > none ? static_cast<double>(sum) / static_cast<double>(len.size() - none) : 0.0, batch.primaryListCapacity, numSamples);
            for (size_t l = 0; l < histogram.size(); ++l)
                if (histogram[l] != 0) std::fprintf(stderr, " %zu:%llu", l, static_cast<unsigned long long>(histogram[l]));
            std::fprintf(stderr, " | no list: signs %llu, overflow %llu, big leaf %llu, stack %llu\n", static_cast<unsigned long long>(why[kNoListSigns]),
                         static_cast<unsigned long long>(why[kNoListOverflow]), static_cast<unsigned long long>(why[kNoListBigLeaf]), static_cast<unsigned long long>(why[kNoListStack]));
        }
        launchTimed(4, [&] { enqueueSums(batch, fp, io.ps); });
        RF_HIP(hipGetLastError());
        RF_HIP(hipEventRecord(bt.stop, stream));
        pendingBatches.push_back(bt);
        if (timing) collectTimings();
        if (pendingBatches.size() > 64) collectBatchTimings();
    }
};

Renderer::Renderer(const RendererDescriptor& desc, const SceneView& sceneView) : mImpl(std::make_unique<Impl>())
{
    Impl& m = *mImpl;
    requireAnyDevice();
    m.device = desc.deviceOrdinal;
    RF_HIP(hipSetDevice(m.device)); // (not requireDevice: an ordinal that names no device has always been reported here as the HIP error it is)
    RF_HIP(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));

    if (sceneView.bvhNodes.empty()) throw std::runtime_error("scene has no BVH nodes");
    if (sceneView.positionAttributes.size() != sceneView.vertexAttributes.size())
        throw std::runtime_error("position and vertex attribute counts differ");
    // child links, leaf ranges and texture indices are followed blindly on the device: check them once here
    validateScene(sceneView.bvhNodes, sceneView.positionAttributes.size(), sceneView.vertexAttributes, sceneView.baseColorTextures.size());
    // the device layouts in host memory and the facts about the scene (rf_scene_pack.cpp); everything below copies
    const PackedScene packed = packScene(sceneView);
    {
        // (an empty array -- a layout this scene does not get -- uploads as nullptr)
        const auto up = [](auto& buffer, const auto& host) { buffer.upload(host.data(), host.size()); return buffer.ptr; };
        const WideBuild& wb = packed.wide;
        m.wide.nodes = up(m.wideNodes, wb.nodes);
#if defined(RF_EXP_LEGACY_LAYOUTS)
        m.wide.compact = up(m.wideCompact, wb.compact);
        m.wide.hot = up(m.wideHot, wb.hot);
        m.wide.own = up(m.wideOwn, wb.own);
#endif
        m.wide.quad = up(m.wideQuad, wb.quad);
        m.wide.quadHalf = up(m.wideQuadHalf, wb.quadHalf);
        m.wide.originBound = wb.originBound;
        m.wide.quadLocal = up(m.wideQuadLocal, wb.quadLocal);
        m.wide.oct = up(m.wideOct, wb.oct);
        m.wide.bigLeaves = up(m.bigLeaves, wb.bigLeaves);
        m.wide.rootLo = wb.rootLo;
        m.wide.rootHi = wb.rootHi;
        m.wide.rootLeaf = wb.rootLeaf;
        m.wide.numRecords = static_cast<uint32_t>(wb.nodes.size() / 4);
        m.scene.nodes = up(m.nodes, packed.nodes);
        m.scene.triangles = up(m.triangles, packed.triangles);
        m.scene.attributes = up(m.attributes, packed.attributes);
        m.scene.shadeRecords = up(m.shadeRecords, packed.shadeRecords);
        m.scene.textureDescriptors = up(m.textureDescriptors, packed.textureDescriptors);
        m.scene.texels = up(m.texels, packed.texels);
        m.scene.numTexels = m.texels.count;
        m.blueNoise.upload(blueNoiseTable(), 128 * 128 * 2);
        m.scene.blueNoise = m.blueNoise.ptr;
        m.scene.albedoLut = up(m.albedoLut, packed.albedoLut);
    }
    m.facts = packed.facts;
    m.options.applySceneDefaults(m.facts);

    DeviceCounters zero{};
    m.counters.upload(&zero, 1);
    {
        const std::vector<unsigned long long> z(4 * RenderStats::kMaxBounceStats, 0ull);
        m.bounceTotals.upload(z.data(), z.size());
    }
    {
        hipDeviceProp_t prop{};
        RF_HIP(hipGetDeviceProperties(&prop, m.device));
        int perCu = 0;
        RF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, reinterpret_cast<const void*>(traceWideKernel(false, false, false, 0, false)), kBlock, 0));
        m.wideBlocks = static_cast<uint32_t>(std::max(perCu, 1)) * static_cast<uint32_t>(prop.multiProcessorCount);
        m.multiProcessors = static_cast<uint32_t>(prop.multiProcessorCount);
        m.skyBlocks = 8u * static_cast<uint32_t>(prop.multiProcessorCount);
        m.options.applyEnvironment(m.facts.wideUsable);
    }

    m.maxWidth = desc.maxWidth ? desc.maxWidth : desc.renderParams.width;
    m.maxHeight = desc.maxHeight ? desc.maxHeight : desc.renderParams.height;
    const TileGrid maxGrid(m.maxWidth, m.maxHeight);
    const uint64_t maxTiles = static_cast<uint64_t>(maxGrid.tilesX) * maxGrid.tilesY;
    // 1 Gi paths per batch by default (133 GB of path state + queues out of 288 GB; allocated on demand, so a render only ever
    // takes samples x pixels x 124 B): later bounces of a batch keep ~15 % of
    // the paths, a traversal launch needs millions of rays to fill 6144 persistent waves and to amortise its tail, and the
    // more samples of a pixel a batch holds, the closer the directions of the 64 direction-sorted samples that share a
    // wave (FrameParams::samplePerm).  Measured on the atrium, 1080p, Mrays/s: 64 Mi 5125, 128 Mi 5171, 256 Mi 5224 (before
    // the sample sort); 256 Mi 5692, 512 Mi 5826 / 5796, 1 Gi 5983 (with it).
    const uint64_t want = desc.maxPathsInFlight ? desc.maxPathsInFlight : (1024ull << 20);
    // path slots and queue indices are 32-bit: at most 2^31 paths per batch, and one sample of the whole
    // (padded) frame must fit in a batch
    constexpr uint64_t kMaxPathsPerBatch = 1ull << 31;
    if (maxTiles * 1024 > kMaxPathsPerBatch) throw std::runtime_error("framebuffer too large: more than 2^31 pixels per rank");
    m.maxPaths = std::min(std::max<uint64_t>(want, maxTiles * 1024), kMaxPathsPerBatch);

    m.params = desc.renderParams;
    if (alignedSkyState(m.params.sky, m.sky) != SkyResult::Success) throw std::runtime_error("sky parameters out of range");
    m.updateSunBasis();
    m.books.setSampleCap(m.params.samplingParams.numSamplesPerPixel);
    m.configureShard();
}

Renderer::~Renderer()
{
    if (!mImpl) return;
    (void)hipSetDevice(mImpl->device);
    (void)hipStreamSynchronize(mImpl->stream);
    for (auto& t : mImpl->timed)
    {
        (void)hipEventDestroy(t.start);
        (void)hipEventDestroy(t.stop);
    }
    for (auto& b : mImpl->pendingBatches)
    {
        (void)hipEventDestroy(b.start);
        (void)hipEventDestroy(b.stop);
    }
    for (auto e : mImpl->eventPool) (void)hipEventDestroy(e);
    if (mImpl->lookEvent) (void)hipEventDestroy(mImpl->lookEvent);
    if (mImpl->lookBatchHost) (void)hipHostFree(mImpl->lookBatchHost);
    (void)hipStreamDestroy(mImpl->stream);
}

void Renderer::setRenderParameters(const RenderParameters& p)
{
    Impl& m = *mImpl;
    if (m.params == p) return; // reference_path_tracer.cpp:556-563
    if (p.width > m.maxWidth || p.height > m.maxHeight) throw std::runtime_error("framebuffer size exceeds maxFramebufferSize");
    SkyStateGpu sky;
    if (alignedSkyState(p.sky, sky) != SkyResult::Success) throw std::runtime_error("sky parameters out of range");
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipStreamSynchronize(m.stream));
    const bool resized = p.width != m.params.width || p.height != m.params.height;
    m.params = p;
    m.sky = sky;
    m.updateSunBasis();
    m.books.setSampleCap(p.samplingParams.numSamplesPerPixel);
    m.books.restartAccumulation();
    if (resized) m.books.frameResized(), m.configureShard(); // (the temporal history is of the old size: gone)
}

void Renderer::setTileShard(uint32_t rank, uint32_t worldSize)
{
    Impl& m = *mImpl;
    m.books.refuseSetTileShard(rank, worldSize);
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipStreamSynchronize(m.stream));
    m.books.setShard(rank, worldSize);
    m.configureShard();
}

std::span<const uint32_t> Renderer::shardTiles() const { return mImpl->tiles; }

void Renderer::render(uint32_t numFrames)
{
    Impl& m = *mImpl;
    m.books.refuseRender();
    RF_HIP(hipSetDevice(m.device));
    const uint64_t pixelsPadded = static_cast<uint64_t>(m.tiles.size()) * 1024;
    // Each reference render() call: frame = frameCount++, then one sample if accumulated < spp
    // (reference_path_tracer.cpp:577-591, wgsl:47-57).  Calls past spp only advance frameCount (AccumulationBooks::framesToTrace).
    uint32_t remaining = numFrames;
    while (const uint32_t todo = m.books.framesToTrace(remaining))
    {
        m.clearStaleSums(pixelsPadded);
        remaining -= m.step(todo, pixelsPadded, nullptr);
    }
}

float Renderer::averageRenderpassDurationMs() const
{
    Impl& m = *mImpl;
    (void)hipSetDevice(m.device);
    m.collectBatchTimings();
    if (m.passDurationsMs.empty()) return 0.0f;
    float sum = 0.0f;
    for (float v : m.passDurationsMs) sum += v;
    return sum / static_cast<float>(m.passDurationsMs.size());
}

float Renderer::renderProgressPercentage() const
{
    return 100.0f * static_cast<float>(mImpl->books.accumulated()) / static_cast<float>(mImpl->params.samplingParams.numSamplesPerPixel);
}

uint32_t Renderer::accumulatedSampleCount() const { return mImpl->books.accumulated(); }
uint32_t Renderer::width() const { return mImpl->params.width; }
uint32_t Renderer::height() const { return mImpl->params.height; }
uint32_t Renderer::shardRank() const { return mImpl->books.rank(); }
uint32_t Renderer::shardWorldSize() const { return mImpl->books.worldSize(); }
int      Renderer::deviceOrdinal() const { return mImpl->device; }
float    Renderer::exposure() const { return mImpl->params.exposure; }
void*    Renderer::streamHandle() const { return mImpl->stream; }
uint32_t Renderer::numBounces() const { return mImpl->params.samplingParams.numBounces; }

void Renderer::synchronize()
{
    RF_HIP(hipSetDevice(mImpl->device));
    RF_HIP(hipStreamSynchronize(mImpl->stream));
}

void Renderer::readAccumulation(float* dst)
{
    Impl& m = *mImpl;
    synchronize();
    m.readCompact(m.books.stale(Books::kImage) ? nullptr : m.image, dst);
}

void Renderer::setAovs(uint32_t flags)
{
    Impl& m = *mImpl;
    // any change of the value restarts the sums, kAovFirstHit <-> kAovFirstHit | kAovTileCounts included (the buffers stay: they are the same two either way)
    const Books::Change change = m.books.setAovs(flags);
    if (change == Books::Change::Unchanged) return;
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipStreamSynchronize(m.stream)); // (a batch in flight may still write the records or the sums)
    if (change == Books::Change::RestartedOff)
    {
        // off: nothing of the AOVs stays allocated (the path state keeps its depth; the next batch that needs the records allocates them again)
        m.sAov.release();
        m.storage[Books::kAovs].release();
    }
}

uint32_t Renderer::aovFlags() const { return mImpl->books.sums(Books::kAovs).word; }

void Renderer::readAovs(float* albedoCoverage, float* normalDepth, uint32_t* sampleCount)
{
    Impl& m = *mImpl;
    synchronize();
    const bool empty = m.books.empty(Books::kAovs);
    if (albedoCoverage) m.readCompact(empty ? nullptr : m.aovAlbedoCoverage(), albedoCoverage);
    if (normalDepth) m.readCompact(empty ? nullptr : m.aovNormalDepth(), normalDepth);
    if (sampleCount) *sampleCount = m.books.readCount(Books::kAovs);
}

void Renderer::denoise(const DenoiseParameters& params)
{
    Impl& m = *mImpl;
    m.books.refuseDenoise();
    RF_HIP(hipSetDevice(m.device));
    // (the non-uniform state: prep divides each pixel by its tile's own count)
    enqueueDenoise(m.stream, m.denoiseWork, m.frameSums(m.nonUniformTileSamples()), params, m.params.exposure);
    m.books.noteDenoised();
}

void Renderer::readDenoised(float* rgba, uint32_t* bgra8, uint32_t* sampleCount)
{
    Impl& m = *mImpl;
    m.books.refuseReadDenoised();
    synchronize();
    const size_t n = static_cast<size_t>(m.params.width) * m.params.height;
    if (rgba) RF_HIP(hipMemcpy(rgba, m.denoiseWork.out.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (bgra8) RF_HIP(hipMemcpy(bgra8, m.denoiseWork.bgra.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (sampleCount) *sampleCount = m.books.denoisedSamples();
}

void Renderer::setMoments(bool enabled)
{
    Impl& m = *mImpl;
    const Books::Change change = m.books.setMoments(enabled);
    if (change == Books::Change::Unchanged) return;
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipStreamSynchronize(m.stream)); // (a batch in flight may still write the sums)
    if (change == Books::Change::RestartedOff)
    {
        // off: nothing of the moments stays allocated
        m.storage[Books::kMoments].release();
        m.noiseWork.release();
    }
}

bool Renderer::momentsEnabled() const { return mImpl->books.on(Books::kMoments); }

void Renderer::readMoments(float* sumSq, uint32_t* sampleCount)
{
    Impl& m = *mImpl;
    synchronize();
    if (sumSq) m.readCompact(m.books.empty(Books::kMoments) ? nullptr : m.moments(), sumSq);
    if (sampleCount) *sampleCount = m.books.readCount(Books::kMoments);
}

void Renderer::setDirect(uint32_t flags)
{
    Impl& m = *mImpl;
    // any change of the value restarts the sums, kDirectOn <-> kDirectOn | kDirectTileCounts included (the buffer stays: it is the same one either way)
    const Books::Change change = m.books.setDirect(flags);
    if (change == Books::Change::Unchanged) return;
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipStreamSynchronize(m.stream)); // (a batch in flight may still write the sums)
    // off: nothing of the direct sums stays allocated
    if (change == Books::Change::RestartedOff) m.storage[Books::kDirect].release();
}

bool     Renderer::directEnabled() const { return mImpl->books.on(Books::kDirect); }
uint32_t Renderer::directFlags() const { return mImpl->books.sums(Books::kDirect).word; }

void Renderer::readDirect(float* directSum, uint32_t* sampleCount)
{
    Impl& m = *mImpl;
    synchronize();
    if (directSum) m.readCompact(m.books.empty(Books::kDirect) ? nullptr : m.direct(), directSum);
    if (sampleCount) *sampleCount = m.books.readCount(Books::kDirect);
}

void Renderer::denoiseSplit(const DenoiseParameters& direct, const DenoiseParameters& indirect)
{
    Impl& m = *mImpl;
    m.books.refuseDenoiseSplit();
    RF_HIP(hipSetDevice(m.device));
    enqueueDenoiseSplit(m.stream, m.denoiseWork, m.frameSums(m.nonUniformTileSamples()), direct, indirect, m.params.exposure);
    m.books.noteDenoised();
}

uint32_t Renderer::exportFeatures(const FeatureRequest& request, void* dstDevice, uint64_t dstBytes)
{
    Impl&          m = *mImpl;
    const uint32_t reads = featureReads(request.channels);
    requireFeatureDestination(dstDevice, dstBytes, featureBytes(m.params.width, m.params.height, request), m.device, "rf_renderer_export_features");
    m.books.refuseExportFeatures(reads, featureNeedsTwoSamples(request.channels));
    RF_HIP(hipSetDevice(m.device));
    enqueueExportFeatures(m.stream, m.frameSums(m.nonUniformTileSamples()), request, dstDevice);
    RF_HIP(hipStreamSynchronize(m.stream)); // the buffer may be used from any stream once the call returns
    return m.books.accumulated();
}

void Renderer::setBuckets(uint32_t word)
{
    Impl& m = *mImpl;
    const Books::Change change = m.books.setBuckets(word);
    if (change == Books::Change::Unchanged) return;
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipStreamSynchronize(m.stream)); // (a batch in flight may still write the sums)
    // another K is another allocation (sized before the next sample); off: nothing of the buckets stays allocated
    m.storage[Books::kBuckets].release();
    m.robustShard.release();
    if (change == Books::Change::RestartedOff) m.robustWork.release();
}

uint32_t Renderer::buckets() const { return mImpl->books.buckets(); }

void Renderer::readBuckets(float* planes, uint32_t* K, uint32_t* sampleCount)
{
    Impl& m = *mImpl;
    synchronize();
    const bool   empty = m.books.empty(Books::kBuckets);
    const size_t plane = static_cast<size_t>(m.params.width) * m.params.height * 4;
    if (planes)
        for (uint32_t b = 0; b < buckets(); ++b) m.readCompact(empty ? nullptr : m.bucketPlanes() + b * m.bucketStride(), planes + b * plane);
    if (K) *K = buckets();
    if (sampleCount) *sampleCount = m.books.readCount(Books::kBuckets);
}

bool Renderer::bucketsPerTile() const { return mImpl->books.bucketsPerTile(); }

void Renderer::robustMean()
{
    Impl& m = *mImpl;
    m.books.refuseRobustMean();
    RF_HIP(hipSetDevice(m.device));
    // (per tile -- the buckets' own bit, not the non-uniform state: the call first waits for the stream and copies the counts to the device, as the other per-tile reads do)
    enqueueRobustMean(m.stream, m.robustWork, m.bucketPlanes(), m.bucketStride(), buckets(), m.frameSums(bucketsPerTile() ? m.uploadTileSamples() : nullptr), m.params.exposure);
    m.books.noteRobustMean();
}

void Renderer::readRobustMean(float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* sampleCount)
{
    Impl& m = *mImpl;
    m.books.refuseReadRobustMean();
    synchronize();
    const size_t n = static_cast<size_t>(m.params.width) * m.params.height;
    if (rgba) RF_HIP(hipMemcpy(rgba, m.robustWork.mean.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (bgra8) RF_HIP(hipMemcpy(bgra8, m.robustWork.bgra.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (trim) RF_HIP(hipMemcpy(trim, m.robustWork.trim.ptr, n * sizeof(uint8_t), hipMemcpyDeviceToHost));
    if (sampleCount) *sampleCount = m.books.robustSamples();
}

void Renderer::denoiseRobust(const DenoiseParameters& params)
{
    Impl& m = *mImpl;
    m.books.refuseDenoiseRobust();
    robustMean();
    // (per tile: the counts robustMean uploaded are still on the device, and nothing but this stream reads them)
    enqueueDenoise(m.stream, m.denoiseWork, m.frameSums(m.books.nonUniform() ? m.tileSamplesDevice.ptr : nullptr), params, m.params.exposure, m.robustWork.mean.ptr);
    m.books.noteDenoised();
}

void Renderer::temporalAccumulate(const TemporalParameters& params)
{
    Impl& m = *mImpl;
    m.books.refuseTemporalAccumulate();
    RF_HIP(hipSetDevice(m.device));
    TemporalWork& w = m.temporalWork;
    w.reserve(static_cast<uint64_t>(m.params.width) * m.params.height, m.stream);
    const bool     history = m.books.temporalHistory();
    const uint32_t out = w.result, in = w.history();
    enqueueTemporal(m.stream, m.frameSums(nullptr), m.params.camera, history ? w.color[in].ptr : nullptr, history ? w.geometry[in].ptr : nullptr,
                    history ? &w.camera[in] : nullptr, params, m.params.exposure, w.color[out].ptr, w.geometry[out].ptr, w.bgra.ptr);
    w.camera[out] = m.params.camera;
    m.books.noteTemporal();
}

void Renderer::temporalCommit()
{
    Impl& m = *mImpl;
    m.books.refuseTemporalCommit();
    m.temporalWork.commit(); // (the next accumulate writes the other pair: on the same stream, behind whatever still reads it)
    m.books.commitTemporal();
}

void Renderer::temporalReset() { mImpl->books.resetTemporal(); }

void Renderer::readTemporal(float* rgba, uint32_t* bgra8, float* geometry, uint32_t* sampleCount)
{
    Impl& m = *mImpl;
    m.books.refuseReadTemporal();
    synchronize();
    const TemporalWork& w = m.temporalWork;
    const size_t        n = static_cast<size_t>(m.params.width) * m.params.height;
    if (rgba) RF_HIP(hipMemcpy(rgba, w.color[w.result].ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (bgra8) RF_HIP(hipMemcpy(bgra8, w.bgra.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (geometry) RF_HIP(hipMemcpy(geometry, w.geometry[w.result].ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (sampleCount) *sampleCount = m.books.temporalSamples();
}

void Renderer::denoiseTemporal(const TemporalParameters& temporal, const DenoiseParameters& params)
{
    Impl& m = *mImpl;
    m.books.refuseTemporalAccumulate(true);
    temporalAccumulate(temporal);
    enqueueDenoise(m.stream, m.denoiseWork, m.frameSums(nullptr), params, m.params.exposure, m.temporalWork.color[m.temporalWork.result].ptr); // (one count: no tile counts)
    m.books.noteDenoised();
}

NoiseEstimate Renderer::noiseEstimate(float* errorMap, float* tileSum, float* tileMax)
{
    Impl& m = *mImpl;
    m.books.refuseNoiseEstimate();
    RF_HIP(hipSetDevice(m.device));
    // (the non-uniform state: every tile with its own count -- each >= 2: a tile stops at an estimate --; `samples` reports the leading count)
    return runNoiseEstimate(m.stream, m.noiseWork, m.frameSums(m.nonUniformTileSamples()), errorMap, tileSum, tileMax);
}

// What rf_renderer_render_adaptive and rf_comm_render_adaptive check alike before anything is traced (or exchanged)
void Renderer::checkAdaptive(const AdaptiveParameters& p, bool sharded) const
{
    mImpl->books.refuseAdaptive(p.checkEvery, p.targetTileError, sharded);
}

AdaptiveResult Renderer::renderAdaptive(const AdaptiveParameters& p)
{
    mImpl->books.refuseRenderAdaptive(p.checkEvery, p.targetTileError);
    return renderAdaptiveFrom(p, mImpl->books.accumulated(), false);
}

// The loop of rf_renderer_render_adaptive over the handle's own tiles -- the whole frame, or a tile shard -- with `leading` the frame's leading count: the handle's
// accumulated count, or under a shard the largest over all ranks.  A tile is numbered twice here: its SLOT k in the shard (where its sums and its count
// live) and its frame id m.tiles[k] (coordinates, the estimate's per-tile outputs); without a shard the two are equal, and shardSlots == false keeps the kernels that
// take the id for the slot (rf_renderer_render_adaptive's, as ever).  rf_comm_render_adaptive passes true at every world size, 1 included.
AdaptiveResult Renderer::renderAdaptiveFrom(const AdaptiveParameters& p, uint32_t leading, bool shardSlots)
{
    Impl& m = *mImpl;
    m.books.requireSlotAddressing(shardSlots);
    RF_HIP(hipSetDevice(m.device));
    const uint32_t spp = m.params.samplingParams.numSamplesPerPixel;
    const uint32_t cap = p.maxSamples == 0u ? spp : std::min(p.maxSamples, spp);
    const uint32_t numTiles = static_cast<uint32_t>(m.tiles.size()), frameTiles = m.grid().count();
    const uint32_t firstCheck = std::max(2u, p.minSamples);
    const auto     pixelSamples = [&](const std::vector<uint32_t>& counts) {
        uint64_t n = 0;
        for (uint32_t k = 0; k < numTiles; ++k) n += static_cast<uint64_t>(m.grid().pixelsInFrame(m.tiles[k])) * counts[k];
        return n;
    };

    // the counts (by slot) as a vector for the length of the call (the uniform state: every tile at the accumulated count); the tiles at the leading count are the
    // active ones -- none on a rank whose tiles all stopped below the frame's leading count
    std::vector<uint32_t> counts = m.books.tileCounts();
    std::vector<uint32_t> active, activeIds; // slots; their frame ids
    for (uint32_t k = 0; k < numTiles; ++k)
        if (counts[k] == leading) active.push_back(k);
    const uint64_t pixelSamplesBefore = pixelSamples(counts);
    const uint32_t frameCountBefore = m.books.frameCount();

    AdaptiveResult        out;
    std::vector<float>    sums(frameTiles);
    std::vector<uint32_t> pixels(frameTiles);
    // tileIds / tileValidBefore hold the active list while it is shorter than the shard's; whatever happens, they hold the shard's list again afterwards
    struct Restore
    {
        Impl& m;
        bool  armed = false;
        ~Restore()
        {
            if (!armed) return;
            (void)hipStreamSynchronize(m.stream);
            try { m.uploadTileList(m.tiles, nullptr); } catch (...) {}
        }
    } restore{m};
    ActiveTiles list{numTiles, m.validPixels, shardSlots};
    bool              listStale = active.size() != numTiles;
    const auto        idsOf = [&](const std::vector<uint32_t>& slots) {
        std::vector<uint32_t> ids;
        for (const uint32_t k : slots) ids.push_back(m.tiles[k]);
        return ids;
    };
    activeIds = idsOf(active);
    while (!active.empty() && m.books.accumulated() < cap)
    {
        const uint64_t pixelsPadded = static_cast<uint64_t>(active.size()) * 1024;
        if (listStale)
        {
            RF_HIP(hipStreamSynchronize(m.stream));
            restore.armed = true;
            list = ActiveTiles{static_cast<uint32_t>(active.size()), m.uploadTileList(activeIds, &active), shardSlots};
            listStale = false;
        }
        m.clearStaleSums(static_cast<uint64_t>(numTiles) * 1024);
        uint32_t remaining = std::min(p.checkEvery, cap - m.books.accumulated());
        while (remaining > 0) remaining -= m.step(remaining, pixelsPadded, &list);
        for (const uint32_t k : active) counts[k] = m.books.accumulated();
        m.books.setTileSamples(counts); // (non-uniform from here on, should an estimate throw; settled below)
        if (m.books.accumulated() < firstCheck) continue;
        // the active tiles' estimate, Nf = float(L) for all of them; tileIds holds the list (the shard's own while every tile is active)
        TileSelection sel;
        sel.listDevice = m.tileIds.ptr, sel.listHost = activeIds.data(), sel.listCount = static_cast<uint32_t>(active.size());
        sel.slotsBehindList = shardSlots;
        out.last = runNoiseEstimateTiles(m.stream, m.noiseWork, m.frameSums(nullptr), sel, nullptr, sums.data(), nullptr, pixels.data());
        ++out.estimatePasses;
        std::vector<uint32_t> still;
        for (const uint32_t k : active)
            if (!(sums[m.tiles[k]] / static_cast<float>(pixels[m.tiles[k]]) <= p.targetTileError)) still.push_back(k); // (NaN: never <=, the tile goes on)
        if (still.size() != active.size()) listStale = true;
        active.swap(still);
        activeIds = idsOf(active);
    }
    RF_HIP(hipStreamSynchronize(m.stream)); // (waits for the work it enqueued, as render_until does)

    out.tiles = numTiles;
    out.minTileSamples = out.maxTileSamples = numTiles ? counts[0] : 0u;
    for (uint32_t k = 0; k < numTiles; ++k) out.minTileSamples = std::min(out.minTileSamples, counts[k]), out.maxTileSamples = std::max(out.maxTileSamples, counts[k]);
    out.pixelSamples = pixelSamples(counts);
    out.tracedPixelSamples = out.pixelSamples - pixelSamplesBefore;
    out.framesTraced = m.books.frameCount() - frameCountBefore;
    out.stoppedTiles = m.books.settleTileSamples(counts);
    return out;
}

uint32_t Renderer::settleFrameTileSamples(uint32_t leading, uint32_t minimum, uint32_t skipFrames)
{
    return mImpl->books.settleFrameTileSamples(leading, minimum, skipFrames);
}

const uint32_t* Renderer::shardTileSamplesDevice()
{
    Impl& m = *mImpl;
    RF_HIP(hipSetDevice(m.device));
    if (m.books.nonUniform()) return m.uploadTileSamples();
    // the ordinary form: every tile of the shard at the accumulated count
    const std::vector<uint32_t> counts = m.books.tileCounts();
    RF_HIP(hipStreamSynchronize(m.stream));
    if (m.tileSamplesDevice.count < counts.size()) m.tileSamplesDevice.alloc(counts.size());
    if (!counts.empty()) RF_HIP(hipMemcpy(m.tileSamplesDevice.ptr, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return m.tileSamplesDevice.ptr;
}

bool Renderer::tileSamplesUniform() const { return !mImpl->books.nonUniform() && !mImpl->books.frameNonUniform(); }
void Renderer::requireUniformTileSamples(const char* what) const { mImpl->books.requireUniform(what); }

uint32_t Renderer::readTileSamples(uint32_t* tileSamples) const
{
    const Impl&    m = *mImpl;
    const uint32_t frameTiles = m.grid().count();
    if (tileSamples)
    {
        std::fill(tileSamples, tileSamples + frameTiles, 0u);
        for (size_t i = 0; i < m.tiles.size(); ++i) tileSamples[m.tiles[i]] = m.books.tileCount(i); // (0 after a restart)
    }
    return frameTiles;
}

void Renderer::readMean(float* rgba)
{
    Impl& m = *mImpl;
    synchronize();
    m.readCompact(m.tiles.empty() ? nullptr : m.meanOnDevice(), rgba);
}

uint32_t Renderer::renderUntil(float targetMeanError, uint32_t checkEvery, uint32_t maxFrames, NoiseEstimate* last)
{
    Impl& m = *mImpl;
    m.books.refuseRenderUntil(checkEvery);
    const uint32_t spp = m.params.samplingParams.numSamplesPerPixel;
    NoiseEstimate  estimate;
    uint32_t       frames = 0;
    while (frames < maxFrames && m.books.accumulated() < spp)
    {
        const uint32_t n = std::min({checkEvery, maxFrames - frames, spp - m.books.accumulated()});
        render(n);
        frames += n;
        if (m.books.accumulated() < 2u) continue;
        estimate = noiseEstimate(nullptr, nullptr, nullptr);
        if (estimate.meanError <= static_cast<double>(targetMeanError)) break;
    }
    if (last) *last = estimate;
    return frames;
}

void*    Renderer::accumulationDevicePointer() const { return mImpl->image; }

Renderer::ShardSums Renderer::shardSums() const
{
    const Impl& m = *mImpl;
    const Books& b = m.books;
    return ShardSums{{m.image, m.aovAlbedoCoverage(), m.aovNormalDepth(), m.moments()}, b.shardChannel(Books::kAovs), b.shardChannel(Books::kMoments), b.accumulated(), !m.tiles.empty(),
                     b.shardChannel(Books::kBuckets), buckets(), b.shardTileCounts(Books::kBuckets), b.minTileSamples(), b.shardChannel(Books::kDirect), b.tileCounts(Books::kDirect), m.direct()};
}

const void* Renderer::enqueueShardRobustMean(const uint32_t* slotCounts)
{
    Impl& m = *mImpl;
    if (m.tiles.empty()) return nullptr;
    m.books.requireShardRobustMean();
    RF_HIP(hipSetDevice(m.device));
    if (m.robustShard.count < m.bucketStride())
    {
        RF_HIP(hipStreamSynchronize(m.stream)); // (the last gather may still read the smaller one)
        m.robustShard.alloc(m.bucketStride());
    }
    enqueueRobustMeanShard(m.stream, m.bucketPlanes(), m.bucketStride(), static_cast<uint32_t>(m.tiles.size()), buckets(), m.books.accumulated(), m.robustShard.ptr, slotCounts);
    return m.robustShard.ptr;
}

void* Renderer::checkpointScratch(uint64_t bytes)
{
    Impl& m = *mImpl;
    if (m.checkpointWork.count * sizeof(uint64_t) < bytes)
    {
        synchronize(); // (an earlier digest may still use the smaller one)
        m.checkpointWork.alloc((bytes + sizeof(uint64_t) - 1) / sizeof(uint64_t));
    }
    return m.checkpointWork.ptr;
}

Renderer::CheckpointBooks Renderer::checkpointBooks(bool prepare)
{
    Impl& m = *mImpl;
    const uint64_t pixelsPadded = prepare ? static_cast<uint64_t>(m.tiles.size()) * 1024 : 0u;
    if (prepare) synchronize();
    if (pixelsPadded != 0u) m.clearStaleSums(pixelsPadded);
    CheckpointBooks b;
    const Books::Checkpoint c = m.books.checkpoint();
    b.frameCount = c.frameCount, b.accumulated = c.accumulated, b.frameLeadingSamples = c.frameLeadingSamples, b.frameMinTileSamples = c.frameMinTileSamples;
    b.aovFlags = c.word[Books::kAovs], b.moments = c.word[Books::kMoments], b.directWord = c.word[Books::kDirect], b.bucketsWord = c.word[Books::kBuckets];
    std::copy(c.family, c.family + Books::kFamilies, b.family);
    b.tileSamples = c.tileSamples;
    if (pixelsPadded != 0u)
    {
        b.planes[0] = m.image;
        if (c.family[Books::kAovs].on) b.planes[1] = m.aovAlbedoCoverage(), b.planes[2] = m.aovNormalDepth();
        if (c.family[Books::kMoments].on) b.planes[3] = m.moments();
        if (c.family[Books::kDirect].on) b.planes[4] = m.direct();
        for (uint32_t k = 0; k < buckets(); ++k) b.planes[5 + k] = m.bucketPlanes() + k * m.bucketStride();
    }
    static_assert(sizeof(Camera) == sizeof b.camera && sizeof(float) * 6 == sizeof b.sky);
    std::memcpy(b.camera, &m.params.camera, sizeof b.camera);
    const float sky[6] = {m.params.sky.turbidity, m.params.sky.albedo[0], m.params.sky.albedo[1], m.params.sky.albedo[2], m.params.sky.sunZenithDegrees, m.params.sky.sunAzimuthDegrees};
    std::memcpy(b.sky, sky, sizeof sky);
    b.numBounces = m.params.samplingParams.numBounces, b.samplesPerPixel = m.params.samplingParams.numSamplesPerPixel;
    std::memcpy(b.sceneCounts, m.facts.sceneCounts, sizeof b.sceneCounts);
    std::memcpy(b.rootBounds, m.facts.sceneRootBounds, sizeof b.rootBounds);
    return b;
}

void Renderer::checkpointRestart(bool zeroNow)
{
    Impl& m = *mImpl;
    synchronize();
    m.books.restartAccumulation();
    const uint64_t pixelsPadded = static_cast<uint64_t>(m.tiles.size()) * 1024;
    if (zeroNow && pixelsPadded != 0u) m.clearStaleSums(pixelsPadded);
}

void Renderer::checkpointAdopt(const CheckpointBooks& b)
{
    Books::Checkpoint c;
    c.frameCount = b.frameCount, c.accumulated = b.accumulated, c.frameLeadingSamples = b.frameLeadingSamples, c.frameMinTileSamples = b.frameMinTileSamples;
    std::copy(b.family, b.family + Books::kFamilies, c.family);
    c.tileSamples = b.tileSamples;
    mImpl->books.adopt(c);
}

void Renderer::clearAccumulationIfStale()
{
    Impl& m = *mImpl;
    if (!m.books.stale(Books::kImage) || m.image == nullptr) return;
    RF_HIP(hipSetDevice(m.device));
    m.zeroImageIfStale(std::min<uint64_t>(accumulationBytes(), m.imageBytes));
}

void Renderer::layoutInfo(uint32_t (&layouts)[48], uint32_t (&misc)[4], float& quadHalfAreaRatio, uint64_t& treeBytes) const
{
    writeLayoutInfo(mImpl->options, mImpl->policyInputs(), layouts, misc, quadHalfAreaRatio, treeBytes);
}

void Renderer::launchPlan(uint32_t bounce, uint32_t numSamples, rf_launch_plan& out) const
{
    const Impl& m = *mImpl;
    if (bounce == 0u || bounce > m.params.samplingParams.numBounces || numSamples == 0u) throw std::invalid_argument("launch plan: bounce must be 1 .. the bounce count, num_samples >= 1");
    (void)hipSetDevice(m.device);
    const PolicyInputs in = m.policyInputs();
    BatchPlan          batch = planBatch(m.options, in, numSamples);
    batch.firstLookReady = m.nextBatchFirstLookReady(batch);
    writeLaunchPlan(batch, planBounce(m.options, in, bounce, batch), bounce, out);
}

void Renderer::memoryInfo(uint64_t& pathStateBytes, uint64_t& pathsAllocated, uint64_t& maxPathsPerBatch, uint64_t& sceneBytes) const
{
    const Impl& m = *mImpl;
    pathsAllocated = m.allocatedPaths;
    pathStateBytes = m.pathStateBytes() + m.storage[Books::kDirect].buffers[0].count * sizeof(float4) + m.primaryListBytes() + m.temporalWork.bytes(); // (the direct sums, while they are on: 16 B per pixel of the shard's tiles; the leaf lists of bounce 1; the temporal planes once they exist: 68 B per pixel)
    maxPathsPerBatch = m.effectivePaths ? std::min(m.effectivePaths, m.maxPaths) : m.maxPaths;
    sceneBytes = (m.nodes.count + m.triangles.count + m.wideNodes.count + m.wideCompact.count + m.wideHot.count + m.wideOwn.count + m.wideQuad.count + m.wideQuadHalf.count + m.wideQuadLocal.count + m.wideOct.count + m.attributes.count + m.shadeRecords.count) * sizeof(float4) +
                 m.texels.count * sizeof(uint32_t) + m.bigLeaves.count * sizeof(uint2) + m.occluderGrid.count * sizeof(uint32_t); // (the occluder grid: allocated by the first batch)
}
uint64_t Renderer::accumulationBytes() const { return static_cast<uint64_t>(mImpl->tiles.size()) * 1024 * sizeof(float4); }

void Renderer::bindAccumulationBuffer(void* devicePtr, uint64_t bytes)
{
    Impl& m = *mImpl;
    synchronize();
    // The caller's buffer was produced on streams this library does not know (e.g. torch's current stream filling
    // it with zeros), and the handle's stream is non-blocking: wait for the whole device once, here, so that the
    // first memset / sum kernel into the buffer cannot overtake the caller's own writes.  After this call the buffer
    // belongs to the handle's stream until rf_renderer_synchronize() returns ("Streams").
    RF_HIP(hipDeviceSynchronize());
    if (devicePtr == nullptr)
    {
        m.image = nullptr;
        m.configureShard();
        return;
    }
    if (bytes < accumulationBytes()) throw std::runtime_error("accumulation buffer too small");
    m.image = static_cast<float4*>(devicePtr);
    m.imageBytes = bytes;
    m.books.restartAccumulation();
}

void Renderer::readTonemapped(uint32_t* dst)
{
    Impl& m = *mImpl;
    synchronize();
    const uint32_t         n = static_cast<uint32_t>(m.tiles.size() * 1024);
    DeviceBuffer<uint32_t> out;
    out.alloc(std::max<uint32_t>(n, 1));
    m.zeroImageIfStale(static_cast<size_t>(n) * sizeof(float4));
    // (non-uniform tile counts: kTonemap over the per-tile mean with accumulatedSamples = 1, the denoiser's display path; x / 1 is exact, so the uniform state's texels are
    // the ones the direct launch gives)
    if (n && m.books.nonUniform()) hipLaunchKernelGGL(tonemapKernel(), dim3((n + 255) / 256), dim3(256), 0, m.stream, m.meanOnDevice(), n, 1u, m.params.exposure, out.ptr);
    else if (n) hipLaunchKernelGGL(tonemapKernel(), dim3((n + 255) / 256), dim3(256), 0, m.stream, m.image, n, m.books.accumulated(), m.params.exposure, out.ptr);
    RF_HIP(hipStreamSynchronize(m.stream));
    std::vector<uint32_t> compact(n);
    if (n) RF_HIP(hipMemcpy(compact.data(), out.ptr, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
    std::memset(dst, 0, static_cast<size_t>(m.params.width) * m.params.height * 4);
    untileHostTexels(compact.data(), m.tiles.data(), static_cast<uint32_t>(m.tiles.size()), m.params.width, m.params.height, sizeof(uint32_t), dst);
}

void Renderer::tonemapDeviceImage(const void* imageDevice, uint64_t numPixels, uint32_t samples, uint32_t* dst)
{
    Impl& m = *mImpl;
    if (numPixels == 0) return;
    if (numPixels > 0xFFFFFFFFull) throw std::runtime_error("image too large");
    RF_HIP(hipSetDevice(m.device));
    const uint32_t         n = static_cast<uint32_t>(numPixels);
    DeviceBuffer<uint32_t> out;
    out.alloc(n);
    hipLaunchKernelGGL(tonemapKernel(), dim3((n + 255) / 256), dim3(256), 0, m.stream, static_cast<const float4*>(imageDevice), n, samples, m.params.exposure, out.ptr);
    RF_HIP(hipGetLastError());
    RF_HIP(hipMemcpyAsync(dst, out.ptr, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, m.stream));
    RF_HIP(hipStreamSynchronize(m.stream));
}

void Renderer::renderDeferred(uint32_t numFrames)
{
    Impl& m = *mImpl;
    RF_HIP(hipSetDevice(m.device));
    const uint32_t W = m.params.width, H = m.params.height;
    const size_t   n = static_cast<size_t>(W) * H;
    if (m.deferredSample.count != 3 * n)
    {
        RF_HIP(hipStreamSynchronize(m.stream));
        m.deferredSample.alloc(3 * n);
        m.deferredAccum.alloc(3 * n);
        m.deferredBgra.alloc(n);
        m.deferredFrameCount = 0;
    }
    const uint32_t waves = ((W + 7) / 8) * ((H + 7) / 8);
    for (uint32_t f = 0; f < numFrames; ++f)
    {
        // r2Sequence(frameCount, 1 << 20), src/common/r_sequence.hpp:9-21 (the host-side variant: + 0.5, 1/G constants)
        constexpr float G = 1.32471795f;
        constexpr float A1 = 1.0f / G, A2 = 1.0f / (G * G);
        const float     i = static_cast<float>(m.deferredFrameCount % (1u << 20));
        const float     a = 0.5f + A1 * i, b = 0.5f + A2 * i;
        const float     jx = a - std::floor(a), jy = b - std::floor(b);
        hipLaunchKernelGGL(deferredLightingKernel(), dim3((waves * 64 + kBlock - 1) / kBlock), dim3(kBlock), 0, m.stream, m.scene, m.sky, m.sunBasis, m.params.camera, W, H,
                           m.deferredFrameCount, jx, jy, m.params.exposure, m.deferredSample.ptr, m.deferredAccum.ptr, m.deferredBgra.ptr, m.counters.ptr);
        ++m.deferredFrameCount;
    }
    RF_HIP(hipGetLastError());
}

void Renderer::resetDeferred() { mImpl->deferredFrameCount = 0; }
uint32_t Renderer::deferredFrameCount() const { return mImpl->deferredFrameCount; }

void Renderer::readDeferred(float* sampleRgb, float* accumulationRgb, uint32_t* bgra8)
{
    Impl& m = *mImpl;
    synchronize();
    const size_t n = static_cast<size_t>(m.params.width) * m.params.height;
    if (m.deferredSample.count != 3 * n) throw std::runtime_error("no deferred frame has been rendered at this framebuffer size");
    if (sampleRgb) RF_HIP(hipMemcpy(sampleRgb, m.deferredSample.ptr, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (accumulationRgb) RF_HIP(hipMemcpy(accumulationRgb, m.deferredAccum.ptr, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (bgra8) RF_HIP(hipMemcpy(bgra8, m.deferredBgra.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

void Renderer::setCounting(bool enabled) { mImpl->options.counting = enabled; }

// The names that need the device are handled here; every other one is a knob of the launch policy (LaunchOptions::set)
void Renderer::setOption(const std::string& name, int64_t value)
{
    Impl& m = *mImpl;
    if (name == "reserve_samples")
    {
        // allocate path state for batches of up to `value` samples now (otherwise it grows on first use)
        const uint64_t pixelsPadded = static_cast<uint64_t>(m.tiles.size()) * 1024;
        RF_HIP(hipSetDevice(m.device));
        if (pixelsPadded)
        {
            uint64_t samples = std::min<uint64_t>(std::max<uint64_t>(static_cast<uint64_t>(value), 1), std::max(m.maxPaths / pixelsPadded, uint64_t{1}));
            samples = std::max<uint64_t>(std::min(samples, m.pathsThatFit() / pixelsPadded), 1);
            (void)m.ensurePathState(samples * pixelsPadded); // best effort: render() falls back to smaller batches
        }
    }
    else if (name == "persistent_blocks")
    {
        // > 0: every persistent launch takes that grid; 0: back to what the device holds of the kernel launched (residentBlocks)
        m.wideBlocksForced = value > 0;
        m.wideBlocks = value > 0 ? static_cast<uint32_t>(value) : m.residentBlocks(traceWideKernel(false, false, false, 0, false), m.options.optExtraLds);
    }
    else if (!m.options.set(name, value, m.facts.wideUsable)) throw std::invalid_argument("unknown option " + name);
    else if (name == "extra_lds")
    {
        // (the persistent grid, sized again for the occupancy that is left)
        hipDeviceProp_t prop{};
        RF_HIP(hipGetDeviceProperties(&prop, m.device));
        int perCu = 0;
        RF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, reinterpret_cast<const void*>(traceWideKernel(false, false, false, 0, false)), kBlock, m.options.optExtraLds));
        m.wideBlocks = static_cast<uint32_t>(std::max(perCu, 1)) * static_cast<uint32_t>(prop.multiProcessorCount);
    }
}
void Renderer::setTiming(bool enabled) { mImpl->timing = enabled; }

void Renderer::resetStats()
{
    Impl& m = *mImpl;
    synchronize();
    m.collectTimings();
    DeviceCounters zero{};
    RF_HIP(hipMemcpy(m.counters.ptr, &zero, sizeof zero, hipMemcpyHostToDevice));
    RF_HIP(hipMemset(m.bounceTotals.ptr, 0, 4 * RenderStats::kMaxBounceStats * sizeof(unsigned long long)));
    m.hostStats = RenderStats{};
    m.primaryRaysHost = 0;
}

RenderStats Renderer::stats()
{
    Impl& m = *mImpl;
    synchronize();
    m.collectTimings();
    DeviceCounters c{};
    RF_HIP(hipMemcpy(&c, m.counters.ptr, sizeof c, hipMemcpyDeviceToHost));
    RenderStats s = m.hostStats;
    s.primaryRays = m.primaryRaysHost;
    s.closestRays = c.closestRays;
    s.shadowRays = c.shadowRays;
    s.closestNodeVisits = c.closestNodeVisits;
    s.closestTriangleTests = c.closestTriangleTests;
    s.shadowNodeVisits = c.shadowNodeVisits;
    s.shadowTriangleTests = c.shadowTriangleTests;
    s.stackHighWater = c.stackHigh;
    s.closestRecordFetches = c.closestRecordFetches;
    s.shadowRecordFetches = c.shadowRecordFetches;
    s.paths = m.primaryRaysHost;
    s.abandonedRays = c.abandonedRays;
    s.scalarRedoRays = c.scalarRedo[0] + c.scalarRedo[1];
    s.primaryListRays = c.primaryListRays, s.primaryFallbackRays = c.primaryFallbackRays, s.primaryFusedRays = c.primaryFusedRays;
    if (std::getenv("RF_DEBUG_COUNTERS"))
        std::fprintf(stderr, "[rf] rays redone by the scalar traversal: closest %llu of %llu, shadow %llu of %llu\n", c.scalarRedo[0], c.closestRays, c.scalarRedo[1], c.shadowRays);
#if defined(RF_EXP_PHASE)
    if (std::getenv("RF_DEBUG_COUNTERS") && !m.options.counting)
    {
        for (int k = 0; k < 2; ++k)
        {
            const double rays = static_cast<double>(k ? c.shadowRays : c.closestRays), steps = static_cast<double>(k ? c.shadowRecordFetches : c.closestRecordFetches);
            std::fprintf(stderr,
                         "[rf-phase] %s: rays %.0f | per ray: steps %.2f leaf visits %.2f triangle tests %.2f | wave trips per 64 rays: outer %.2f descend %.2f leaf phase %.2f refill %.2f"
                         " | lanes busy: descend %.3f leaf phase %.3f\n",
                         k ? "shadow " : "closest", rays, steps / rays, c.leafTrips[k] / rays, c.popLaneTrips[k] / rays, c.outerTrips[k] * 64.0 / rays,
                         c.descendTrips[k] * 64.0 / rays, c.leafPhases[k] * 64.0 / rays, c.refillTrips[k] * 64.0 / rays, steps / (64.0 * c.descendTrips[k]),
                         c.leafTrips[k] / (64.0 * c.leafPhases[k]));
            std::fprintf(stderr, "[rf-phase] %s: lanes of a descend trip: stepping %.3f, parked at a leaf %.3f, without a ray %.3f | lanes of a leaf pass: at a leaf %.3f, at an interior node %.3f, without a ray %.3f\n",
                         k ? "shadow " : "closest", steps / (64.0 * c.descendTrips[k]), c.descendParked[k] / (64.0 * c.descendTrips[k]), c.descendIdle[k] / (64.0 * c.descendTrips[k]),
                         c.leafTrips[k] / (64.0 * c.leafPhases[k]), c.leafInterior[k] / (64.0 * c.leafPhases[k]), c.leafIdle[k] / (64.0 * c.leafPhases[k]));
        }
        std::fprintf(stderr, "[rf-phase] occluder cache: shadow rays %llu, occluded %llu, cache tried %llu, answered at the cached leaf %llu\n", c.shadowRays, c.occludedRays, c.occluderTried, c.occluderHit);
    }
#endif
    if (std::getenv("RF_DEBUG_COUNTERS") && m.options.counting)
    {
        for (int k = 0; k < 2; ++k)
        {
            const double rays = static_cast<double>(k ? c.shadowRays : c.closestRays), steps = static_cast<double>(k ? c.shadowRecordFetches : c.closestRecordFetches);
            const double tris = static_cast<double>(k ? c.shadowTriangleTests : c.closestTriangleTests);
            std::fprintf(stderr,
                         "[rf] %s: rays %.0f | per ray: steps %.2f tris %.2f pops %.2f | wave trips per 64 rays: outer %.2f descend %.2f leafphase %.2f leaf %.2f refill %.2f"
                         " | lane utilisation: descend %.3f leaf %.3f\n",
                         k ? "shadow " : "closest", rays, steps / rays, tris / rays, c.popLaneTrips[k] / rays, c.outerTrips[k] * 64.0 / rays,
                         c.descendTrips[k] * 64.0 / rays, c.leafPhases[k] * 64.0 / rays, c.leafTrips[k] * 64.0 / rays, c.refillTrips[k] * 64.0 / rays,
                         steps / (64.0 * c.descendTrips[k]), tris / (64.0 * c.leafTrips[k]));
        }
    }
    unsigned long long totals[4 * RenderStats::kMaxBounceStats];
    RF_HIP(hipMemcpy(totals, m.bounceTotals.ptr, sizeof totals, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < RenderStats::kMaxBounceStats; ++b)
    {
        s.closestRaysByBounce[b] = totals[b];
        s.shadowRaysByBounce[b] = totals[RenderStats::kMaxBounceStats + b];
        s.shadowRaysHintAnswered += totals[2 * RenderStats::kMaxBounceStats + b];
        s.shadowRaysSelfAnswered += totals[3 * RenderStats::kMaxBounceStats + b];
    }
    return s;
}

void Renderer::tracePrimaryStats(const Camera& camera, uint32_t width, uint32_t height, uint32_t* nodesVisitedOut, uint8_t* hitOut,
                                 float* tOut, uint32_t* triangleTestsOut)
{
    Impl& m = *mImpl;
    synchronize();
    const size_t           n = static_cast<size_t>(width) * height;
    DeviceBuffer<uint32_t> nv, tt;
    DeviceBuffer<uint8_t>  hit;
    DeviceBuffer<float>    t;
    nv.alloc(n);
    tt.alloc(n);
    hit.alloc(n);
    t.alloc(n);
    const uint32_t waves = ((width + 7) / 8) * ((height + 7) / 8);
    hipLaunchKernelGGL(primaryStatsKernel(), dim3((waves * 64 + kBlock - 1) / kBlock), dim3(kBlock), 0, m.stream, m.scene, camera, width, height,
                       nv.ptr, hit.ptr, t.ptr, tt.ptr, m.counters.ptr);
    RF_HIP(hipGetLastError());
    RF_HIP(hipStreamSynchronize(m.stream));
    RF_HIP(hipMemcpy(nodesVisitedOut, nv.ptr, n * 4, hipMemcpyDeviceToHost));
    if (hitOut) RF_HIP(hipMemcpy(hitOut, hit.ptr, n, hipMemcpyDeviceToHost));
    if (tOut) RF_HIP(hipMemcpy(tOut, t.ptr, n * 4, hipMemcpyDeviceToHost));
    if (triangleTestsOut) RF_HIP(hipMemcpy(triangleTestsOut, tt.ptr, n * 4, hipMemcpyDeviceToHost));
}

void Renderer::intersectRays(const float* rays6, uint64_t numRays, float tMax, uint32_t* triangleOut, float* tOut, float* uvOut, float* pOut,
                             uint32_t* nodesVisitedOut, uint32_t* triangleTestsOut)
{
    Impl& m = *mImpl;
    synchronize();
    if (numRays == 0) return;
    if (m.options.queryVariant == 2)
    {
        std::vector<float4> hit, p4;
        m.queryWide(rays6, numRays, tMax, false, hit, p4);
        for (uint64_t i = 0; i < numRays; ++i)
        {
            const uint32_t tri = floatBits(hit[i].x);
            const bool     found = tri != kMiss;
            triangleOut[i] = tri;
            if (tOut) tOut[i] = found ? hit[i].w : 0.0f;
            if (uvOut) uvOut[2 * i] = found ? hit[i].y : 0.0f, uvOut[2 * i + 1] = found ? hit[i].z : 0.0f;
            if (pOut) pOut[3 * i] = found ? p4[i].x : 0.0f, pOut[3 * i + 1] = found ? p4[i].y : 0.0f, pOut[3 * i + 2] = found ? p4[i].z : 0.0f;
            if (nodesVisitedOut) nodesVisitedOut[i] = 0;
            if (triangleTestsOut) triangleTestsOut[i] = 0;
        }
        return;
    }
    DeviceBuffer<float>    rays, t, uv, p;
    DeviceBuffer<uint32_t> tri, nv, tt;
    rays.upload(rays6, 6 * numRays);
    tri.alloc(numRays);
    t.alloc(numRays);
    uv.alloc(2 * numRays);
    p.alloc(3 * numRays);
    nv.alloc(numRays);
    tt.alloc(numRays);
    hipLaunchKernelGGL(intersectRaysKernel(), dim3(static_cast<uint32_t>((numRays + kBlock - 1) / kBlock)), dim3(kBlock), 0, m.stream, m.scene, rays.ptr,
                       numRays, tMax, tri.ptr, t.ptr, uv.ptr, p.ptr, nv.ptr, tt.ptr, m.counters.ptr);
    RF_HIP(hipGetLastError());
    RF_HIP(hipStreamSynchronize(m.stream));
    RF_HIP(hipMemcpy(triangleOut, tri.ptr, numRays * 4, hipMemcpyDeviceToHost));
    if (tOut) RF_HIP(hipMemcpy(tOut, t.ptr, numRays * 4, hipMemcpyDeviceToHost));
    if (uvOut) RF_HIP(hipMemcpy(uvOut, uv.ptr, numRays * 8, hipMemcpyDeviceToHost));
    if (pOut) RF_HIP(hipMemcpy(pOut, p.ptr, numRays * 12, hipMemcpyDeviceToHost));
    if (nodesVisitedOut) RF_HIP(hipMemcpy(nodesVisitedOut, nv.ptr, numRays * 4, hipMemcpyDeviceToHost));
    if (triangleTestsOut) RF_HIP(hipMemcpy(triangleTestsOut, tt.ptr, numRays * 4, hipMemcpyDeviceToHost));
}

void Renderer::occludedRays(const float* rays6, uint64_t numRays, float tMax, float* visibilityOut)
{
    Impl& m = *mImpl;
    synchronize();
    if (numRays == 0) return;
    if (m.options.queryVariant == 2)
    {
        std::vector<float4> rad, unused;
        m.queryWide(rays6, numRays, tMax, true, rad, unused);
        for (uint64_t i = 0; i < numRays; ++i) visibilityOut[i] = rad[i].x != 0.0f ? 1.0f : 0.0f;
        return;
    }
    DeviceBuffer<float> rays, vis;
    rays.upload(rays6, 6 * numRays);
    vis.alloc(numRays);
    hipLaunchKernelGGL(occludedRaysKernel(), dim3(static_cast<uint32_t>((numRays + kBlock - 1) / kBlock)), dim3(kBlock), 0, m.stream, m.scene, rays.ptr,
                       numRays, tMax, vis.ptr, m.counters.ptr);
    RF_HIP(hipGetLastError());
    RF_HIP(hipStreamSynchronize(m.stream));
    RF_HIP(hipMemcpy(visibilityOut, vis.ptr, numRays * 4, hipMemcpyDeviceToHost));
}

void Renderer::castRays(const RayQueryRequest& q)
{
    Impl& m = *mImpl;
    if (q.numRays == 0) return; // nothing is read, checked or touched
    checkRayQueryRequest(q);
    checkRayQueryOverlaps(q); // (every range's arithmetic first: it refuses what does not fit 64 bits)
    RF_HIP(hipSetDevice(m.device));
    const ByteRange origins = inputRange(q.origins, q.numRays, q.originStride, "origins"), directions = inputRange(q.directions, q.numRays, q.directionStride, "directions");
    requireDeviceRange(reinterpret_cast<const void*>(q.origins), origins.end - origins.begin, m.device, "rf_renderer_cast_rays", "origins", "the rays", "the scene");
    requireDeviceRange(reinterpret_cast<const void*>(q.directions), directions.end - directions.begin, m.device, "rf_renderer_cast_rays", "directions", "the rays", "the scene");
    for (uint32_t i = 0; i < kCastOutputs; ++i)
    {
        if (q.outputs[i] == 0u) continue;
        const ByteRange r = outputRange(q, i);
        requireDeviceRange(reinterpret_cast<const void*>(q.outputs[i]), r.end - r.begin, m.device, "rf_renderer_cast_rays", kCastOutputName[i], "the rays' values", "the scene");
    }
    m.castRays(q, planChunks(q.numRays, m.maxPaths, m.pathsThatFit(), m.options.optCastChunk));
}
} // namespace rf
