// rf_comm.hip -- the frame exchange (rf_comm.hpp): the gather plans, TileComm (one gather as its steps, the device un-tile, the root-side calls) and RcclTransport,
// the RCCL side of the transport seam (rf_transport.hpp).  The local test transport: rf_comm_local.cpp; the sharded calls over a handle: rf_comm_sharded.cpp.
#include "rf_comm.hpp"

#include "rf_denoise.hpp"
#include "rf_features.hpp"
#include "rf_hip_host.hpp"
#include "rf_noise.hpp"
#include "rf_renderer.hpp" // tilesForRank, TileGrid
#include "rf_robust.hpp"
#include "rf_transport.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <future>
#include <stdexcept>
#include <string>
#include <thread>

namespace rf
{
namespace
{
#define RF_NCCL(expr)                                                                                         \
    do                                                                                                        \
    {                                                                                                         \
        const ncclResult_t _r = (expr);                                                                       \
        if (_r != ncclSuccess)                                                                                \
            throw std::runtime_error(std::string("RCCL error: ") + ncclGetErrorString(_r) + " in " #expr);    \
    } while (0)

constexpr uint32_t kTilePixels = kTileSize * kTileSize; // 1024

// One workgroup per tile of the frame: tile-major (8x8-pixel blocks, one wave each) -> row-major.  Reads are 1-KiB contiguous per wave, writes 128-byte row segments.
// `own`: the root's shard of the plane, read in place; every other tile comes from the staging area, at its slot.  store(row-major index, the pixel) writes it out.
template<class Store>
__device__ __forceinline__ void untileTileTo(const float4* __restrict__ staging, const float4* __restrict__ own, uint32_t ownRank, uint32_t ownFirstTile,
                                             const uint32_t* __restrict__ tileSlot, const uint32_t* __restrict__ tileOwner, uint32_t width, uint32_t height, uint32_t tilesX, Store store)
{
    const uint32_t tile = blockIdx.x;
    const uint32_t slot = tileSlot[tile];
    const float4* __restrict__ src = tileOwner[tile] == ownRank ? own + static_cast<size_t>(slot - ownFirstTile) * kTilePixels : staging + static_cast<size_t>(slot) * kTilePixels;
    const uint32_t x0 = (tile % tilesX) * kTileSize, y0 = (tile / tilesX) * kTileSize;
#pragma unroll
    for (uint32_t k = 0; k < kTilePixels / 256; ++k)
    {
        const uint32_t w = k * 256 + threadIdx.x;
        const uint32_t block = w >> 6, lane = w & 63u;
        const uint32_t x = x0 + (block & 3u) * 8u + (lane & 7u), y = y0 + (block >> 2) * 8u + (lane >> 3);
        if (x < width && y < height) store(static_cast<size_t>(y) * width + x, src[w]);
    }
}
__device__ __forceinline__ void untileTile(const float4* __restrict__ staging, const float4* __restrict__ own, float4* __restrict__ image, uint32_t ownRank, uint32_t ownFirstTile,
                                           const uint32_t* __restrict__ tileSlot, const uint32_t* __restrict__ tileOwner, uint32_t width, uint32_t height, uint32_t tilesX)
{
    untileTileTo(staging, own, ownRank, ownFirstTile, tileSlot, tileOwner, width, height, tilesX, [=](size_t at, const float4& v) { image[at] = v; });
}

__global__ __launch_bounds__(256) void kUntile(const float4* __restrict__ staging, const float4* __restrict__ own, uint32_t ownRank, uint32_t ownFirstTile,
                                               const uint32_t* __restrict__ tileSlot, const uint32_t* __restrict__ tileOwner, uint32_t width, uint32_t height,
                                               uint32_t tilesX, float4* __restrict__ image)
{
    untileTile(staging, own, image, ownRank, ownFirstTile, tileSlot, tileOwner, width, height, tilesX);
}

// The same for every carried plane of a multi-plane gather in ONE launch: grid (tiles of the frame, carried planes); blockIdx.y picks the plane's pointers from the
// by-value argument struct (kernel arguments: no device-side table, no upload).
struct UntilePlane
{
    const float4* staging; // this plane's staging area
    const float4* own;     // the root's shard of this plane, read in place
    float4*       image;   // this plane's row-major image
};
struct UntilePlaneArgs
{
    UntilePlane plane[kSumPlanes]; // [blockIdx.y]: the carried sum planes in plane order
};
__global__ __launch_bounds__(256) void kUntilePlanes(UntilePlaneArgs args, uint32_t ownRank, uint32_t ownFirstTile, const uint32_t* __restrict__ tileSlot,
                                                     const uint32_t* __restrict__ tileOwner, uint32_t width, uint32_t height, uint32_t tilesX)
{
    const UntilePlane pl = args.plane[blockIdx.y];
    untileTile(pl.staging, pl.own, pl.image, ownRank, ownFirstTile, tileSlot, tileOwner, width, height, tilesX);
}

// The un-tile of plane 4, the ranks' {M.rgb, float(c)}: the same walk, and every pixel is split on its way out -- mean = {M.rgb, 1} and trim = uint8(c), both
// row-major.  A launch of its own behind the sum planes' (their kernels, arguments and grids stay what they are without the plane).  Reads 1 KiB contiguous per wave;
// writes 128-byte row segments of the mean and 8-byte ones of the trim image.
__global__ __launch_bounds__(256) void kUntileRobust(const float4* __restrict__ staging, const float4* __restrict__ own, uint32_t ownRank, uint32_t ownFirstTile,
                                                     const uint32_t* __restrict__ tileSlot, const uint32_t* __restrict__ tileOwner, uint32_t width, uint32_t height,
                                                     uint32_t tilesX, float4* __restrict__ mean, uint8_t* __restrict__ trim)
{
    untileTileTo(staging, own, ownRank, ownFirstTile, tileSlot, tileOwner, width, height, tilesX, [=](size_t at, const float4& v) {
        mean[at] = make_float4(v.x, v.y, v.z, 1.0f);
        trim[at] = static_cast<uint8_t>(v.w);
    });
}

// The gathered per-tile sample counts, one lane per tile of the frame: frameCounts[tile] = the count its owner sent (staged rank after rank, in slot order: tileSlot) or,
// for the root's own tiles without loop-back, the root's counts read in place.
__global__ __launch_bounds__(256) void kUntileCounts(const uint32_t* __restrict__ staged, const uint32_t* __restrict__ own, uint32_t ownRank, uint32_t ownFirstTile,
                                                     const uint32_t* __restrict__ tileSlot, const uint32_t* __restrict__ tileOwner, uint32_t numTiles, uint32_t* __restrict__ frameCounts)
{
    const uint32_t tile = blockIdx.x * 256u + threadIdx.x;
    if (tile >= numTiles) return;
    const uint32_t slot = tileSlot[tile];
    frameCounts[tile] = tileOwner[tile] == ownRank ? own[slot - ownFirstTile] : staged[slot];
}
} // namespace

GatherLayout gatherLayout(uint32_t width, uint32_t height, uint32_t worldSize)
{
    GatherLayout g;
    const TileGrid grid(width, height);
    g.tilesX = grid.tilesX;
    g.tilesY = grid.tilesY;
    const uint32_t n = grid.count();
    g.tileSlot.assign(n, 0);
    g.tileOwner.assign(n, 0);
    g.rankFirstTile.assign(worldSize + 1, 0);
    uint32_t at = 0;
    for (uint32_t r = 0; r < worldSize; ++r)
    {
        g.rankFirstTile[r] = at;
        const std::vector<uint32_t> tiles = tilesForRank(width, height, r, worldSize);
        for (uint32_t i = 0; i < tiles.size(); ++i)
        {
            g.tileSlot[tiles[i]] = at + i;
            g.tileOwner[tiles[i]] = r;
        }
        at += static_cast<uint32_t>(tiles.size());
    }
    g.rankFirstTile[worldSize] = at;
    return g;
}

std::vector<GatherOp> gatherPlan(const GatherLayout& g, uint32_t worldSize, uint32_t rank, uint32_t root, bool loopback)
{
    std::vector<GatherOp> ops;
    const auto            tilesOf = [&](uint32_t r) { return g.rankFirstTile[r + 1] - g.rankFirstTile[r]; };
    // the root posts every receive at once (one group), so all of its xGMI ingress links carry data concurrently
    if (rank == root)
        for (uint32_t p = 0; p < worldSize; ++p)
        {
            if (tilesOf(p) == 0 || (p == root && !loopback)) continue;
            ops.push_back(GatherOp{0u, p, g.rankFirstTile[p], tilesOf(p)});
        }
    if (tilesOf(rank) > 0 && (rank != root || loopback)) ops.push_back(GatherOp{1u, root, 0u, tilesOf(rank)});
    return ops;
}

std::vector<GatherPlaneOp> gatherPlanPlanes(const GatherLayout& g, uint32_t worldSize, uint32_t rank, uint32_t root, bool loopback, uint32_t planeMask)
{
    // the one-plane plan once per carried plane: its receives (rank order), then its send, keep their places within the plane; receives of all planes come first
    const std::vector<GatherOp> one = gatherPlan(g, worldSize, rank, root, loopback);
    std::vector<GatherPlaneOp>  ops;
    for (const uint32_t sends : {0u, 1u})
        for (uint32_t p = 0; p < kPlaneDirect; ++p)
        {
            if (((planeMask | kPlaneMaskImage) >> p & 1u) == 0u) continue;
            for (const GatherOp& op : one)
                if (op.isSend == sends) ops.push_back(GatherPlaneOp{op.isSend, op.peer, p, op.offsetTiles, op.countTiles});
        }
    // plane 5 follows as a whole, its receives and then its send: the list is the one without it plus the one-plane plan (per pair the k-th send still meets the k-th
    // receive: the sends among themselves and the receives among themselves stay in plane order)
    if (planeMask & kPlaneMaskDirect)
        for (const GatherOp& op : one) ops.push_back(GatherPlaneOp{op.isSend, op.peer, kPlaneDirect, op.offsetTiles, op.countTiles});
    return ops;
}

std::vector<GatherOp> gatherPlanCounts(const GatherLayout& g, uint32_t worldSize, uint32_t rank, uint32_t root, bool loopback)
{
    return gatherPlan(g, worldSize, rank, root, loopback); // (one word per tile: the offsets and counts in words are the one-plane plan's in tiles)
}

double commTimeoutSeconds()
{
    if (const char* v = std::getenv("RF_COMM_TIMEOUT_S")) return std::atof(v);
    return 180.0;
}

namespace
{
// The RCCL transport: the transfers as ncclSend / ncclRecv in one group (all of the root's xGMI ingress links carry data concurrently)
class RcclTransport final : public Transport
{
    ncclComm_t           mComm = nullptr; // nullptr again once the first exchange's watchdog has aborted it
    uint32_t             mRank;
    int                  mDevice;
    bool                 mFirstExchangeDone = false;
    DeviceBuffer<double> mScalar;

    RcclTransport(uint32_t rank, int device) : mRank(rank), mDevice(device) {}
    void abort()
    {
        (void)ncclCommAbort(mComm);
        mComm = nullptr;
    }
    void watchFirstExchange(hipStream_t stream, hipEvent_t queuedBefore);

public:
    static std::unique_ptr<Transport> create(const uint8_t idBytes[kCommIdBytes], uint32_t rank, uint32_t worldSize, int device);
    ~RcclTransport() override
    {
        if (!mComm) return;
        (void)hipSetDevice(mDevice);
        (void)ncclCommDestroy(mComm);
    }

    bool isLocal() const override { return false; }
    void info(uint32_t& count, uint32_t& userRank, int& device) const override
    {
        int c = 0, r = 0, d = 0;
        RF_NCCL(ncclCommCount(mComm, &c));
        RF_NCCL(ncclCommUserRank(mComm, &r));
        RF_NCCL(ncclCommCuDevice(mComm, &d));
        count = static_cast<uint32_t>(c), userRank = static_cast<uint32_t>(r), device = d;
    }
    void requireAlive() const override
    {
        if (mComm == nullptr) throw std::runtime_error("the RCCL communicator was aborted");
    }

    void exchange(const std::vector<Transfer>& transfers, hipStream_t stream) override
    {
        // (first exchange only) marks the end of what was queued on the stream BEFORE the exchange -- this rank's frame kernels: the watchdog measures the exchange,
        // not the render in front of it
        hipEvent_t queuedBefore = nullptr;
        struct EventGuard
        {
            hipEvent_t& e;
            ~EventGuard()
            {
                if (e) (void)hipEventDestroy(e);
            }
        } eventGuard{queuedBefore};
        if (!mFirstExchangeDone)
        {
            RF_HIP(hipEventCreateWithFlags(&queuedBefore, hipEventDisableTiming));
            RF_HIP(hipEventRecord(queuedBefore, stream));
        }
        RF_NCCL(ncclGroupStart());
        try
        {
            for (const Transfer& op : transfers)
            {
                const ncclDataType_t type = op.kind == Transfer::Kind::F32 ? ncclFloat : ncclUint32;
                if (op.isSend) RF_NCCL(ncclSend(op.from, op.words, type, static_cast<int>(op.peer), mComm, stream));
                else RF_NCCL(ncclRecv(op.to, op.words, type, static_cast<int>(op.peer), mComm, stream));
            }
        }
        catch (...)
        {
            (void)ncclGroupEnd(); // never leave the thread inside an open group
            throw;
        }
        RF_NCCL(ncclGroupEnd());
        if (mFirstExchangeDone) return; // (later exchanges stay fully asynchronous)
        watchFirstExchange(stream, queuedBefore);
        mFirstExchangeDone = true;
    }

    double allReduceMax(double value, hipStream_t stream) override
    {
        mScalar.ensure(2);
        RF_HIP(hipMemcpyAsync(mScalar.ptr, &value, sizeof value, hipMemcpyHostToDevice, stream));
        RF_NCCL(ncclAllReduce(mScalar.ptr, mScalar.ptr + 1, 1, ncclDouble, ncclMax, mComm, stream));
        double out = 0.0;
        RF_HIP(hipMemcpyAsync(&out, mScalar.ptr + 1, sizeof out, hipMemcpyDeviceToHost, stream));
        RF_HIP(hipStreamSynchronize(stream));
        return out;
    }
};

std::unique_ptr<Transport> RcclTransport::create(const uint8_t idBytes[kCommIdBytes], uint32_t rank, uint32_t worldSize, int device)
{
    std::unique_ptr<RcclTransport> t(new RcclTransport(rank, device));
    ncclUniqueId                   id;
    std::memcpy(&id, idBytes, kCommIdBytes);
    // ncclCommInitRank blocks until every rank of the world has called it.  It runs on a helper thread so that a rank whose
    // peers never arrive reports that after RF_COMM_TIMEOUT_S instead of hanging the job (the helper is abandoned then: the
    // caller is expected to exit).
    const double timeout = commTimeoutSeconds();
    auto         task = std::make_shared<std::packaged_task<ncclResult_t()>>([device, worldSize, rank, id, comm = &t->mComm]() -> ncclResult_t {
        if (hipSetDevice(device) != hipSuccess) return ncclUnhandledCudaError;
        return ncclCommInitRank(comm, static_cast<int>(worldSize), id, static_cast<int>(rank));
    });
    std::future<ncclResult_t> done = task->get_future();
    std::thread([task] { (*task)(); }).detach();
    if (timeout > 0.0 && done.wait_for(std::chrono::duration<double>(timeout)) != std::future_status::ready)
    {
        (void)t.release(); // the helper still writes into it: leaked on purpose
        throw std::runtime_error("RCCL: ncclCommInitRank did not complete within " + std::to_string(static_cast<int>(timeout)) + " s on rank " + std::to_string(rank) + " of " +
                                 std::to_string(worldSize) + " (a rank is missing, or the ranks do not share one unique id); RF_COMM_TIMEOUT_S changes the limit");
    }
    RF_NCCL(done.get());
    int count = 0;
    RF_NCCL(ncclCommCount(t->mComm, &count));
    if (static_cast<uint32_t>(count) != worldSize) throw std::runtime_error("RCCL communicator spans " + std::to_string(count) + " ranks, expected " + std::to_string(worldSize));
    return t;
}

// The first exchange of a communicator also sets up its peer connections; a peer that never posts its side (it died, it
// disagrees about the frame size or the root) would leave this stream stuck forever.  Watch this one exchange: past the
// time limit the communicator is aborted and the caller gets an error instead of a hang.  NOTE: an exception thrown on
// one rank leaves its peers waiting in their own gather until THEIR limit expires.  The clock starts when the work queued
// on this stream before the exchange (Renderer::render() is asynchronous: the whole frame may still be in front of it) has
// drained, so a long first frame does not abort a healthy job; what remains inside the limit is the connection set-up, the
// transfer, and the wait for the slowest peer to finish ITS frame -- ranks own equal tile counts (+-1), so that wait is a
// fraction of a frame.
// A second, much larger cap (kDrainFactor x the limit, from loop entry) covers the case the first clock never starts in: this rank's OWN queued kernels
// never drain (a hung or faulted kernel keeps the event at hipErrorNotReady forever) -- the loop would otherwise spin without any limit.
void RcclTransport::watchFirstExchange(hipStream_t stream, hipEvent_t queuedBefore)
{
    constexpr double kDrainFactor = 20.0;
    const double     timeout = commTimeoutSeconds();
    const auto       entered = std::chrono::steady_clock::now();
    auto             t0 = entered;
    bool             drained = false;
    for (;;)
    {
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) RF_HIP(q);
        if (!drained)
        {
            const hipError_t e = hipEventQuery(queuedBefore);
            if (e == hipSuccess)
            {
                drained = true;
                t0 = std::chrono::steady_clock::now();
            }
            else if (e != hipErrorNotReady) RF_HIP(e);
        }
        ncclResult_t async = ncclSuccess;
        RF_NCCL(ncclCommGetAsyncError(mComm, &async));
        if (async != ncclSuccess && async != ncclInProgress) throw std::runtime_error(std::string("RCCL error during the first frame exchange: ") + ncclGetErrorString(async));
        if (drained && timeout > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout)
        {
            abort();
            throw std::runtime_error("RCCL: the first frame exchange did not complete within " + std::to_string(static_cast<int>(timeout)) + " s on rank " +
                                     std::to_string(mRank) + " (a peer is missing or disagrees about frame size / root); communicator aborted");
        }
        if (!drained && timeout > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - entered).count() > kDrainFactor * timeout)
        {
            abort();
            throw std::runtime_error("RCCL: the work queued in front of the first frame exchange did not drain within " + std::to_string(static_cast<int>(kDrainFactor * timeout)) +
                                     " s on rank " + std::to_string(mRank) + " (a kernel of this rank's own frame hangs); communicator aborted");
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}
} // namespace

void makeUniqueId(uint8_t out[kCommIdBytes])
{
    static_assert(sizeof(ncclUniqueId) == kCommIdBytes);
    if (makeLocalUniqueId(out)) return;
    ncclUniqueId id;
    RF_NCCL(ncclGetUniqueId(&id));
    std::memcpy(out, &id, kCommIdBytes);
}

std::unique_ptr<Transport> makeTransport(const uint8_t id[kCommIdBytes], uint32_t rank, uint32_t worldSize, int device)
{
    if (std::unique_ptr<Transport> local = makeLocalTransport(id, rank, worldSize, device)) return local;
    return RcclTransport::create(id, rank, worldSize, device);
}

struct TileComm::Impl
{
    std::unique_ptr<Transport> transport;
    uint32_t   rank = 0, world = 1;
    int        device = 0;

    uint32_t         layoutW = 0, layoutH = 0;
    GatherLayout     layout;
    DeviceBuffer<uint32_t> dTileSlot, dTileOwner;
    DeviceBuffer<float4>   staging;               // one GatherLayout area per carried plane, one after another
    DeviceBuffer<float4>   images[kGatherPlanes]; // per plane: the row-major image the root un-tiles into (allocated when first carried)
    // the per-tile sample counts of a gather with kGatherMaskTileCounts: staged rank after rank as they arrive, then per tile of the frame (kUntileCounts), and that on the host
    DeviceBuffer<uint32_t> countStaging, frameCounts;
    std::vector<uint32_t>  frameCountsHost;
    DeviceBuffer<float4>   meanImage; // readMean's, allocated by the first call
    DeviceBuffer<float4>   splitImages; // readSplit's: the direct component, then the indirect one; allocated by the first call
    // plane 4's un-tile leaves images[kPlaneRobustMean] = {M.rgb, 1} and this, one trim byte per pixel; readRobustMean's texels, allocated by the first call that asks for them
    DeviceBuffer<uint8_t>  trimImage;
    DeviceBuffer<uint32_t> robustBgra;
    uint32_t         imageW = 0, imageH = 0;
    // What the last gather left here (replaced as a whole by the next one): whether one was made, its root, and on the root the carried planes (0: none valid) and
    // the sample count the caller gave.  A plain gather drops the extra planes' validity, not their buffers.
    bool             gatherMade = false;
    uint32_t         lastRoot = 0, gatheredMask = 0, gatheredSamples = 0, gatheredRobustK = 0;
    // the root-side denoiser and estimate over the gathered planes: their work buffers, allocated by the first call; the snapshot is dropped by the next gather
    DenoiseWork      denoiseWork;
    bool             denoisedValid = false;
    NoiseWork        noiseWork;
    // HIP events around the last exchange on the caller's stream (sends / receives + the root's un-tile): what the frame-end gather costs THIS rank
    // once its own frame kernels have drained (lastExchangeMs())
    hipEvent_t       exchangeStart = nullptr, exchangeStop = nullptr;
    bool             exchangeTimed = false;

    // A new frame size: the previous gather's kUntile (on the caller's non-blocking stream) may still be reading the tables and
    // the staging / image buffers that are about to be replaced -- wait for it, then upload on that same stream.
    void ensureLayout(uint32_t w, uint32_t h, hipStream_t stream)
    {
        if (w == layoutW && h == layoutH) return;
        RF_HIP(hipStreamSynchronize(stream));
        layout = gatherLayout(w, h, world);
        dTileSlot.ensure(layout.tileSlot.size());
        dTileOwner.ensure(layout.tileOwner.size());
        RF_HIP(hipMemcpyAsync(dTileSlot.ptr, layout.tileSlot.data(), layout.tileSlot.size() * 4, hipMemcpyHostToDevice, stream));
        RF_HIP(hipMemcpyAsync(dTileOwner.ptr, layout.tileOwner.data(), layout.tileOwner.size() * 4, hipMemcpyHostToDevice, stream));
        RF_HIP(hipStreamSynchronize(stream)); // (`layout` outlives the copy anyway; this keeps pageable-copy semantics out of the picture)
        layoutW = w;
        layoutH = h;
    }

    // the root-side calls: this rank was the root of the last gather and that gather carried `need`
    void requireGathered(const char* what, uint32_t need, const char* needName) const
    {
        if (!gatherMade) throw std::invalid_argument(std::string(what) + ": no gather has been made on this communicator (call rf_renderer_gather_frame first)");
        if (rank != lastRoot)
            throw std::invalid_argument(std::string(what) + ": rank " + std::to_string(rank) + " was not the root of the last gather (rank " + std::to_string(lastRoot) +
                                        " was): the gathered planes exist on the root only");
        if ((gatheredMask & need) != need)
            throw std::invalid_argument(std::string(what) + ": the last gather did not carry " + needName);
    }

    // What the root-side passes read (rf_frame_sums.hpp): the gathered planes where they lie, row-major, at the recorded N -- gathered with the counts, each tile its
    // own.  (A plane the last gather did not carry is whatever an earlier one left: requireGathered is the caller's check.)
    bool      perTile() const { return (gatheredMask & kGatherMaskTileCounts) != 0u; }
    FrameSums gathered() const
    {
        return FrameSums{images[kPlaneImage].ptr, images[kPlaneMoments].ptr, images[kPlaneAlbedoCoverage].ptr, images[kPlaneNormalDepth].ptr, images[kPlaneDirect].ptr, imageW, imageH, 0u,
                         gatheredSamples, perTile() ? frameCounts.ptr : nullptr};
    }
    // ... and what they check behind their planes, in this order: `minimum` samples (1, or a variance's 2), a frame the kernels can index and, gathered with the
    // counts, `minimum` samples in every tile
    void requireSamples(const char* what, uint32_t minimum) const
    {
        const std::string name(what);
        const bool        variance = minimum >= 2u;
        if (gatheredSamples < minimum) throw std::invalid_argument(name + (variance ? ": a variance needs at least 2 accumulated samples" : ": the gathered sums hold no sample"));
        if (static_cast<uint64_t>(imageW) * imageH >= (1ull << 31)) throw std::invalid_argument(name + ": image too large");
        if (perTile() && *std::min_element(frameCountsHost.begin(), frameCountsHost.end()) < minimum)
            throw std::invalid_argument(name + (variance ? ": a variance needs at least 2 samples in every tile of the gathered frame" : ": a tile of the gathered frame holds no sample"));
    }

    // ---- one gather, step by step (TileComm::gatherPlanes).  What the steps share:
    struct Gather
    {
        const void* const* compact; // [plane]: this rank's tile-major buffers
        const uint32_t*    tileCounts;
        uint32_t           planeMask, width, height, root;
        bool               loopback, withCounts, isRoot;
        hipStream_t        stream;
        uint32_t           robustK; // the K of plane 4's combine
        uint32_t           carried[kGatherPlanes] = {}, carriedIndex[kGatherPlanes] = {}, numPlanes = 0; // the carried planes in plane order; carriedIndex[p]: plane p's staging area
        size_t             planeStagingPixels = 0;                                                       // one plane's staging area
        uint32_t           ownRank() const { return loopback ? 0xFFFFFFFFu : root; }                      // (the root's un-tile: no tile is read in place under loop-back)
    };
    uint32_t tilesOf(uint32_t r) const { return layout.rankFirstTile[r + 1] - layout.rankFirstTile[r]; }

    // 1. the arguments; the device current and the layout of this frame size in place
    void checkGather(Gather& g)
    {
        transport->requireAlive();
        if (g.root >= world) throw std::invalid_argument("gather root out of range");
        if (g.width == 0 || g.height == 0) throw std::invalid_argument("empty frame");
        g.withCounts = (g.planeMask & kGatherMaskTileCounts) != 0u;
        if ((g.planeMask & kPlaneMaskImage) == 0u || ((g.planeMask & ~kGatherMaskTileCounts) >> kGatherPlanes) != 0u)
            throw std::invalid_argument("gather plane mask: plane 0 always travels, planes 0 .. 5 exist");
        for (uint32_t p = 0; p < kGatherPlanes; ++p)
            if (g.planeMask >> p & 1u) g.carriedIndex[p] = g.numPlanes, g.carried[g.numPlanes++] = p;
        g.isRoot = rank == g.root;
        RF_HIP(hipSetDevice(device));
        ensureLayout(g.width, g.height, g.stream);
        for (uint32_t k = 0; k < g.numPlanes; ++k)
            if (tilesOf(rank) > 0 && g.compact[g.carried[k]] == nullptr) throw std::invalid_argument("null tile buffer");
        if (g.withCounts && tilesOf(rank) > 0 && g.tileCounts == nullptr) throw std::invalid_argument("null tile count buffer");
        g.planeStagingPixels = static_cast<size_t>(layout.rankFirstTile[world]) * kTilePixels;
    }

    // 2. the record of the last gather goes now: whatever happens afterwards, nothing stale is read through the root-side calls
    void dropLastGather(uint32_t root)
    {
        gatherMade = true;
        lastRoot = root;
        gatheredMask = 0;
        gatheredSamples = 0;
        denoisedValid = false;
    }

    // 3. (root) room for the staged shards and the row-major images
    void sizeRootBuffers(const Gather& g)
    {
        const size_t stagingWant = g.planeStagingPixels * g.numPlanes, imageWant = static_cast<size_t>(g.width) * g.height;
        bool         grows = stagingWant > staging.count;
        for (uint32_t k = 0; k < g.numPlanes; ++k) grows = grows || imageWant > images[g.carried[k]].count;
        const size_t frameTiles = static_cast<size_t>(layout.tilesX) * layout.tilesY;
        if (g.withCounts) grows = grows || layout.rankFirstTile[world] > countStaging.count || frameTiles > frameCounts.count;
        const bool robust = (g.planeMask & kPlaneMaskRobustMean) != 0u;
        if (robust) grows = grows || imageWant > trimImage.count;
        if (grows) RF_HIP(hipStreamSynchronize(g.stream)); // a consumer of the old buffers may still run
        if (g.withCounts) countStaging.ensure(layout.rankFirstTile[world]), frameCounts.ensure(frameTiles);
        staging.ensure(stagingWant);
        for (uint32_t k = 0; k < g.numPlanes; ++k) images[g.carried[k]].ensure(imageWant);
        if (robust) trimImage.ensure(imageWant);
        imageW = g.width;
        imageH = g.height;
    }

    // 4. one group: exactly the operations of gatherPlanPlanes() -- with the image alone, gatherPlan()'s (the lists the CPU tests check for every rank of a world) -- and
    // behind them, with the counts, those of gatherPlanCounts(): per (source, destination) pair the counts are the last send and the last receive
    std::vector<Transfer> transferList(const Gather& g) const
    {
        const size_t floatsPerTile = static_cast<size_t>(kTilePixels) * 4;
        const auto   stagingOf = [&](const GatherPlaneOp& op) { return staging.ptr + g.carriedIndex[op.plane] * g.planeStagingPixels + static_cast<size_t>(op.offsetTiles) * kTilePixels; };
        const auto   compactOf = [&](const GatherPlaneOp& op) { return static_cast<const float*>(g.compact[op.plane]) + op.offsetTiles * floatsPerTile; };
        std::vector<Transfer> list;
        for (const GatherPlaneOp& op : gatherPlanPlanes(layout, world, rank, g.root, g.loopback, g.planeMask & ~kGatherMaskTileCounts))
            list.push_back(Transfer{op.isSend != 0u, op.peer, op.isSend ? compactOf(op) : nullptr, op.isSend ? nullptr : stagingOf(op), op.countTiles * floatsPerTile, Transfer::Kind::F32});
        if (g.withCounts)
            for (const GatherOp& op : gatherPlanCounts(layout, world, rank, g.root, g.loopback))
                list.push_back(Transfer{op.isSend != 0u, op.peer, op.isSend ? g.tileCounts + op.offsetTiles : nullptr, op.isSend ? nullptr : countStaging.ptr + op.offsetTiles, op.countTiles,
                                        Transfer::Kind::U32});
        return list;
    }

    // 5. the exchange between its two events: exchangeStop follows the un-tile on the root, the exchange elsewhere
    void startExchangeClock(hipStream_t stream)
    {
        if (exchangeStart == nullptr)
        {
            RF_HIP(hipEventCreate(&exchangeStart));
            RF_HIP(hipEventCreate(&exchangeStop));
        }
        exchangeTimed = false;
        RF_HIP(hipEventRecord(exchangeStart, stream));
    }
    void stopExchangeClock(hipStream_t stream)
    {
        RF_HIP(hipEventRecord(exchangeStop, stream));
        exchangeTimed = true;
    }

    // 6. (root) staged shards + the root's own -> row-major images, and one count per tile of the frame
    void untile(const Gather& g)
    {
        const uint32_t numTiles = layout.tilesX * layout.tilesY;
        // (plane 4 has a launch of its own: the sum planes go as they go without it, each from its own staging area -- D's lies behind plane 4's)
        const bool      robust = (g.planeMask & kPlaneMaskRobustMean) != 0u;
        UntilePlaneArgs args{};
        uint32_t        sumPlanes = 0;
        for (uint32_t k = 0; k < g.numPlanes; ++k)
        {
            const uint32_t p = g.carried[k];
            if (isSumPlane(p)) args.plane[sumPlanes++] = UntilePlane{staging.ptr + k * g.planeStagingPixels, static_cast<const float4*>(g.compact[p]), images[p].ptr};
        }
        if (sumPlanes == 1)
            hipLaunchKernelGGL(kUntile, dim3(numTiles), dim3(256), 0, g.stream, staging.ptr, static_cast<const float4*>(g.compact[kPlaneImage]), g.ownRank(), layout.rankFirstTile[rank],
                               dTileSlot.ptr, dTileOwner.ptr, g.width, g.height, layout.tilesX, images[kPlaneImage].ptr);
        else
            hipLaunchKernelGGL(kUntilePlanes, dim3(numTiles, sumPlanes), dim3(256), 0, g.stream, args, g.ownRank(), layout.rankFirstTile[rank], dTileSlot.ptr, dTileOwner.ptr, g.width,
                               g.height, layout.tilesX);
        if (robust)
            hipLaunchKernelGGL(kUntileRobust, dim3(numTiles), dim3(256), 0, g.stream, staging.ptr + g.carriedIndex[kPlaneRobustMean] * g.planeStagingPixels,
                               static_cast<const float4*>(g.compact[kPlaneRobustMean]), g.ownRank(), layout.rankFirstTile[rank], dTileSlot.ptr, dTileOwner.ptr, g.width, g.height,
                               layout.tilesX, images[kPlaneRobustMean].ptr, trimImage.ptr);
        if (g.withCounts)
            hipLaunchKernelGGL(kUntileCounts, dim3((numTiles + 255u) / 256u), dim3(256), 0, g.stream, countStaging.ptr, g.tileCounts, g.ownRank(), layout.rankFirstTile[rank], dTileSlot.ptr,
                               dTileOwner.ptr, numTiles, frameCounts.ptr);
        RF_HIP(hipGetLastError());
    }

    // 7. (root) what this gather left.  With the counts: they come to the host as well (the root-side calls check them) and N is the largest -- the one wait of such a
    // gather, on the root alone
    void recordGather(const Gather& g, uint32_t samples)
    {
        if (g.withCounts)
        {
            frameCountsHost.assign(layout.tilesX * layout.tilesY, 0u);
            RF_HIP(hipMemcpyAsync(frameCountsHost.data(), frameCounts.ptr, frameCountsHost.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
            RF_HIP(hipStreamSynchronize(g.stream));
            samples = *std::max_element(frameCountsHost.begin(), frameCountsHost.end());
        }
        gatheredMask = g.planeMask;
        gatheredSamples = samples;
        gatheredRobustK = g.robustK;
    }
};

int deviceCount()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
    {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

void TileComm::uniqueId(uint8_t out[kCommIdBytes]) { makeUniqueId(out); }

TileComm::TileComm(const uint8_t idBytes[kCommIdBytes], uint32_t rank, uint32_t worldSize, int deviceOrdinal) : mImpl(std::make_unique<Impl>())
{
    if (worldSize == 0 || rank >= worldSize) throw std::invalid_argument("invalid rank / world size");
    int deviceCount = 0;
    if (hipGetDeviceCount(&deviceCount) != hipSuccess || deviceCount == 0)
        throw std::runtime_error("rayfinder_amd: no HIP device available (the RCCL frame exchange needs one GPU per rank)");
    mImpl->rank = rank;
    mImpl->world = worldSize;
    mImpl->device = deviceOrdinal;
    RF_HIP(hipSetDevice(deviceOrdinal));
    mImpl->transport = makeTransport(idBytes, rank, worldSize, deviceOrdinal);
}

TileComm::~TileComm()
{
    mImpl->transport.reset(); // (first: the communicator goes before the events and the buffers)
    if (mImpl->exchangeStart)
    {
        (void)hipEventDestroy(mImpl->exchangeStart);
        (void)hipEventDestroy(mImpl->exchangeStop);
    }
}

uint32_t TileComm::rank() const { return mImpl->rank; }
uint32_t TileComm::worldSize() const { return mImpl->world; }
int      TileComm::deviceOrdinal() const { return mImpl->device; }

bool TileComm::localTransport() const { return mImpl->transport->isLocal(); }
void TileComm::rcclInfo(uint32_t& count, uint32_t& userRank, int& device) const { mImpl->transport->info(count, userRank, device); }

const void* TileComm::gatherFrame(const void* compactDevice, uint32_t width, uint32_t height, uint32_t root, void* streamHandle, bool loopback)
{
    const void* const planes[kGatherPlanes] = {compactDevice}; // (the other planes: nullptr)
    return gatherPlanes(planes, kPlaneMaskImage, 0u, width, height, root, streamHandle, loopback);
}

const void* TileComm::gatherPlanes(const void* const compactDevice[kGatherPlanes], uint32_t planeMask, uint32_t samples, uint32_t width, uint32_t height, uint32_t root,
                                   void* streamHandle, bool loopback, const uint32_t* tileCountsDevice, uint32_t robustK)
{
    Impl&        m = *mImpl;
    Impl::Gather g{compactDevice, tileCountsDevice, planeMask, width, height, root, loopback, false, false, static_cast<hipStream_t>(streamHandle), robustK};
    m.checkGather(g);
    m.dropLastGather(root);
    if (g.isRoot) m.sizeRootBuffers(g);
    const std::vector<Transfer> transfers = m.transferList(g);
    m.startExchangeClock(g.stream);
    m.transport->exchange(transfers, g.stream);
    if (g.isRoot) m.untile(g);
    m.stopExchangeClock(g.stream);
    if (!g.isRoot) return nullptr;
    m.recordGather(g, samples);
    return m.images[kPlaneImage].ptr;
}

double TileComm::lastExchangeMs()
{
    Impl& m = *mImpl;
    if (!m.exchangeTimed) return -1.0;
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipEventSynchronize(m.exchangeStop));
    float ms = 0.0f;
    RF_HIP(hipEventElapsedTime(&ms, m.exchangeStart, m.exchangeStop));
    return static_cast<double>(ms);
}

void TileComm::readFrame(float* dstHost, void* streamHandle)
{
    Impl& m = *mImpl;
    if (m.images[kPlaneImage].ptr == nullptr || m.imageW == 0) throw std::runtime_error("no gathered frame on this rank (only the gather root has one)");
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipMemcpyAsync(dstHost, m.images[kPlaneImage].ptr, static_cast<size_t>(m.imageW) * m.imageH * sizeof(float4), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
}

namespace
{
// [plane]; plane 4 is no sum plane (rf_comm.hpp: isSumPlane) and is not served by readPlane / planeDevice
const char* const kPlaneNames[kGatherPlanes] = {"the image (plane 0)",
                                                "the first-hit AOVs (plane 1, AC: gather with RF_GATHER_AOVS)",
                                                "the first-hit AOVs (plane 2, ND: gather with RF_GATHER_AOVS)",
                                                "the radiance second moments (plane 3, Q: gather with RF_GATHER_MOMENTS)",
                                                "the robust mean (plane 4: gather with RF_GATHER_ROBUST_MEAN)",
                                                "the direct sums (plane 5, D: gather with RF_GATHER_DIRECT)"};
void requireSumPlane(uint32_t plane)
{
    if (!isSumPlane(plane))
        throw std::invalid_argument("plane out of range: 0 = S, 1 = AC, 2 = ND, 3 = Q, 5 = D (plane 4, the robust mean, is read through rf_comm_read_robust_mean)");
}
}

void TileComm::gatheredPlanes(uint32_t& planeMask, uint32_t& width, uint32_t& height, uint32_t& samples) const
{
    const Impl& m = *mImpl;
    m.requireGathered("rf_comm_gathered_planes", kPlaneMaskImage, kPlaneNames[kPlaneImage]); // (no image: the last gather threw on this rank)
    planeMask = m.gatheredMask, width = m.imageW, height = m.imageH, samples = m.gatheredSamples;
}

const void* TileComm::planeDevice(uint32_t plane) const
{
    const Impl& m = *mImpl;
    requireSumPlane(plane);
    m.requireGathered("rf_comm_plane_device", 1u << plane, kPlaneNames[plane]);
    return m.images[plane].ptr;
}

void TileComm::readPlane(uint32_t plane, float* dstHost, void* streamHandle)
{
    Impl& m = *mImpl;
    requireSumPlane(plane);
    m.requireGathered("rf_comm_read_plane", 1u << plane, kPlaneNames[plane]);
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    RF_HIP(hipMemcpyAsync(dstHost, m.images[plane].ptr, static_cast<size_t>(m.imageW) * m.imageH * sizeof(float4), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
}

void TileComm::denoise(const DenoiseParameters& params, float exposure, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_denoise", kPlaneMaskImage | kPlaneMaskAovs, "the first-hit AOVs (gather with RF_GATHER_AOVS)");
    m.requireSamples("rf_comm_denoise", 1u);
    RF_HIP(hipSetDevice(m.device));
    // the gathered planes are row-major (tilesX = 0) and hold one count N: the filter rf_denoise_images runs, without the sums leaving the device -- or, gathered with
    // the counts, each tile its own: rf_denoise_tiles'
    enqueueDenoise(static_cast<hipStream_t>(streamHandle), m.denoiseWork, m.gathered(), params, exposure);
    m.denoisedValid = true;
}

void TileComm::readDenoised(float* rgba, uint32_t* bgra8, uint32_t* sampleCount, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_read_denoised", kPlaneMaskImage | kPlaneMaskAovs, "the first-hit AOVs (gather with RF_GATHER_AOVS)");
    if (!m.denoisedValid) throw std::invalid_argument("no denoised image: call rf_comm_denoise first (the image is dropped by the next gather)");
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    const size_t n = static_cast<size_t>(m.imageW) * m.imageH;
    if (rgba) RF_HIP(hipMemcpyAsync(rgba, m.denoiseWork.out.ptr, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
    if (bgra8) RF_HIP(hipMemcpyAsync(bgra8, m.denoiseWork.bgra.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
    if (sampleCount) *sampleCount = m.gatheredSamples;
}

NoiseEstimate TileComm::noiseEstimate(float* errorMap, float* tileSum, float* tileMax, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_noise_estimate", kPlaneMaskImage | kPlaneMaskMoments, "the radiance second moments (gather with RF_GATHER_MOMENTS)");
    m.requireSamples("rf_comm_noise_estimate", 2u);
    RF_HIP(hipSetDevice(m.device));
    // (gathered with the counts: every tile with its own count; `samples` reports the largest)
    return runNoiseEstimate(static_cast<hipStream_t>(streamHandle), m.noiseWork, m.gathered(), errorMap, tileSum, tileMax);
}

uint32_t TileComm::readTileSamples(uint32_t* tileSamples) const
{
    const Impl& m = *mImpl;
    m.requireGathered("rf_comm_read_tile_samples", kPlaneMaskImage | kGatherMaskTileCounts, "the per-tile sample counts (gather with RF_GATHER_TILE_COUNTS)");
    if (tileSamples) std::copy(m.frameCountsHost.begin(), m.frameCountsHost.end(), tileSamples);
    return static_cast<uint32_t>(m.frameCountsHost.size());
}

void TileComm::readMean(float* rgba, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_read_mean", kPlaneMaskImage | kGatherMaskTileCounts, "the per-tile sample counts (gather with RF_GATHER_TILE_COUNTS)");
    const size_t n = static_cast<size_t>(m.imageW) * m.imageH;
    if (n >= (1ull << 31)) throw std::invalid_argument("rf_comm_read_mean: image too large");
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    if (m.meanImage.count < n)
    {
        RF_HIP(hipStreamSynchronize(stream)); // (an earlier read may still use the smaller one)
        m.meanImage.alloc(n);
    }
    enqueueTileMeanRows(stream, m.images[kPlaneImage].ptr, m.frameCounts.ptr, m.imageW, m.imageH, m.meanImage.ptr);
    RF_HIP(hipMemcpyAsync(rgba, m.meanImage.ptr, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
}

void TileComm::readRobustMean(float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* K, uint32_t* sampleCount, float exposure, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_read_robust_mean", kPlaneMaskImage | kPlaneMaskRobustMean, "the robust mean (plane 4: gather with RF_GATHER_ROBUST_MEAN)");
    const size_t n = static_cast<size_t>(m.imageW) * m.imageH;
    if (n >= (1ull << 31)) throw std::invalid_argument("rf_comm_read_robust_mean: image too large");
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    if (rgba) RF_HIP(hipMemcpyAsync(rgba, m.images[kPlaneRobustMean].ptr, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
    if (trim) RF_HIP(hipMemcpyAsync(trim, m.trimImage.ptr, n * sizeof(uint8_t), hipMemcpyDeviceToHost, stream));
    if (bgra8)
    {
        if (m.robustBgra.count < n)
        {
            RF_HIP(hipStreamSynchronize(stream)); // (an earlier read may still use the smaller one)
            m.robustBgra.alloc(n);
        }
        enqueueRobustTexels(stream, m.images[kPlaneRobustMean].ptr, static_cast<uint32_t>(n), exposure, m.robustBgra.ptr);
        RF_HIP(hipMemcpyAsync(bgra8, m.robustBgra.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    RF_HIP(hipStreamSynchronize(stream));
    if (K) *K = m.gatheredRobustK;
    if (sampleCount) *sampleCount = m.gatheredSamples;
}

void TileComm::denoiseRobust(const DenoiseParameters& params, float exposure, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_denoise_robust", kPlaneMaskImage | kPlaneMaskAovs, "the first-hit AOVs (gather with RF_GATHER_AOVS | RF_GATHER_ROBUST_MEAN)");
    m.requireGathered("rf_comm_denoise_robust", kPlaneMaskRobustMean, "the robust mean (plane 4: gather with RF_GATHER_AOVS | RF_GATHER_ROBUST_MEAN)");
    m.requireSamples("rf_comm_denoise_robust", 1u);
    RF_HIP(hipSetDevice(m.device));
    // denoise()'s call with prep's colour = the gathered M (rf_denoise.hpp: plane 0 is then not read)
    enqueueDenoise(static_cast<hipStream_t>(streamHandle), m.denoiseWork, m.gathered(), params, exposure, m.images[kPlaneRobustMean].ptr);
    m.denoisedValid = true;
}

void TileComm::denoiseSplit(const DenoiseParameters& direct, const DenoiseParameters& indirect, float exposure, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_denoise_split", kPlaneMaskImage | kPlaneMaskAovs, "the first-hit AOVs (gather with RF_GATHER_AOVS | RF_GATHER_DIRECT)");
    m.requireGathered("rf_comm_denoise_split", kPlaneMaskDirect, "the direct sums (plane 5, D: gather with RF_GATHER_AOVS | RF_GATHER_DIRECT)");
    m.requireSamples("rf_comm_denoise_split", 1u);
    RF_HIP(hipSetDevice(m.device));
    // the filter rf_denoise_split_images runs over row-major sums (tilesX = 0), without the sums leaving the device -- or, gathered with the counts, rf_denoise_split_tiles'
    enqueueDenoiseSplit(static_cast<hipStream_t>(streamHandle), m.denoiseWork, m.gathered(), direct, indirect, exposure);
    m.denoisedValid = true;
}

void TileComm::readSplit(float* directRgba, float* indirectRgba, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_read_split", kPlaneMaskImage | kPlaneMaskDirect, kPlaneNames[kPlaneDirect]);
    const bool perTile = m.perTile();
    if (!perTile && m.gatheredSamples == 0u) throw std::invalid_argument("rf_comm_read_split: the gathered sums hold no sample");
    const size_t n = static_cast<size_t>(m.imageW) * m.imageH;
    if (n >= (1ull << 31)) throw std::invalid_argument("rf_comm_read_split: image too large");
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    if (m.splitImages.count < 2 * n)
    {
        RF_HIP(hipStreamSynchronize(stream)); // (an earlier read may still use the smaller one)
        m.splitImages.alloc(2 * n);
    }
    float4* const direct = m.splitImages.ptr;
    float4* const indirect = m.splitImages.ptr + n;
    enqueueSplitMeanRows(stream, m.images[kPlaneImage].ptr, m.images[kPlaneDirect].ptr, perTile ? m.frameCounts.ptr : nullptr, m.gatheredSamples, m.imageW, m.imageH, direct, indirect);
    if (directRgba) RF_HIP(hipMemcpyAsync(directRgba, direct, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
    if (indirectRgba) RF_HIP(hipMemcpyAsync(indirectRgba, indirect, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
}

uint32_t TileComm::exportFeatures(const FeatureRequest& request, void* dstDevice, uint64_t dstBytes, void* streamHandle)
{
    Impl& m = *mImpl;
    m.requireGathered("rf_comm_export_features", kPlaneMaskImage, kPlaneNames[kPlaneImage]);
    const uint32_t reads = featureReads(request.channels);
    if (reads & kFeatureReadsAovs) m.requireGathered("rf_comm_export_features", kPlaneMaskAovs, "the first-hit AOVs (gather with RF_GATHER_AOVS)");
    if (reads & kFeatureReadsQ) m.requireGathered("rf_comm_export_features", kPlaneMaskMoments, "the radiance second moments (gather with RF_GATHER_MOMENTS)");
    if (reads & kFeatureReadsD) m.requireGathered("rf_comm_export_features", kPlaneMaskDirect, "the direct sums (plane 5, D: gather with RF_GATHER_DIRECT)");
    if (static_cast<uint64_t>(m.imageW) * m.imageH >= (1ull << 31)) throw std::invalid_argument("rf_comm_export_features: image too large");
    requireFeatureDestination(dstDevice, dstBytes, featureBytes(m.imageW, m.imageH, request), m.device, "rf_comm_export_features");
    if (m.gatheredSamples == 0u) throw std::invalid_argument("rf_comm_export_features: the gathered sums hold no sample");
    if (featureNeedsTwoSamples(request.channels) &&
        (m.gatheredSamples < 2u || (m.perTile() && *std::min_element(m.frameCountsHost.begin(), m.frameCountsHost.end()) < 2u)))
        throw std::invalid_argument("rf_comm_export_features: RF_FEATURE_VARIANCE / RF_FEATURE_ERROR need at least 2 samples in every tile of the gathered frame");
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    // the gathered planes are row-major and hold one count N -- or, gathered with the counts, each tile its own (a tile without a sample: +0 in every channel)
    enqueueExportFeatures(stream, m.gathered(), request, dstDevice);
    RF_HIP(hipStreamSynchronize(stream));
    return m.gatheredSamples;
}

double TileComm::allReduceMax(double value, void* streamHandle)
{
    RF_HIP(hipSetDevice(mImpl->device));
    return mImpl->transport->allReduceMax(value, static_cast<hipStream_t>(streamHandle));
}
} // namespace rf
