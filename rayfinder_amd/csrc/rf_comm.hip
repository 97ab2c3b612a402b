// rf_comm.hip -- RCCL gather of tile shards + device un-tile (see rf_comm.hpp).
#include "rf_comm.hpp"

#include "rf_denoise.hpp"
#include "rf_hip_host.hpp"
#include "rf_noise.hpp"
#include "rf_renderer.hpp" // tilesForRank, TileGrid

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <map>
#include <mutex>
#include <random>
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

// One workgroup per tile of the frame: tile-major (8x8-pixel blocks, one wave each) -> row-major.  Reads are
// 1-KiB contiguous per wave, writes 128-byte row segments.  `own`: the root's shard, read in place.
__global__ __launch_bounds__(256) void kUntile(const float4* __restrict__ staging, const float4* __restrict__ own, uint32_t ownRank, uint32_t ownFirstTile,
                                               const uint32_t* __restrict__ tileSlot, const uint32_t* __restrict__ tileOwner, uint32_t width, uint32_t height,
                                               uint32_t tilesX, float4* __restrict__ image)
{
    const uint32_t tile = blockIdx.x;
    const uint32_t slot = tileSlot[tile];
    const float4*  src = tileOwner[tile] == ownRank ? own + static_cast<size_t>(slot - ownFirstTile) * kTilePixels : staging + static_cast<size_t>(slot) * kTilePixels;
    const uint32_t x0 = (tile % tilesX) * kTileSize, y0 = (tile / tilesX) * kTileSize;
#pragma unroll
    for (uint32_t k = 0; k < kTilePixels / 256; ++k)
    {
        const uint32_t w = k * 256 + threadIdx.x;
        const uint32_t block = w >> 6, lane = w & 63u;
        const uint32_t x = x0 + (block & 3u) * 8u + (lane & 7u), y = y0 + (block >> 2) * 8u + (lane >> 3);
        if (x < width && y < height) image[static_cast<size_t>(y) * width + x] = src[w];
    }
}

// The same for every carried plane of a multi-plane gather in ONE launch: grid (tiles of the frame, carried planes); blockIdx.y picks the plane's pointers from the
// by-value argument struct (kernel arguments: no device-side table, no upload), everything else is kUntile -- wave k of a workgroup moves the tile's 8x8 blocks with
// 1-KiB contiguous reads and 128-byte row-segment writes; own / staging per tile from the same tileSlot / tileOwner tables.
struct UntilePlane
{
    const float4* staging; // this plane's staging area
    const float4* own;     // the root's shard of this plane, read in place
    float4*       image;   // this plane's row-major image
};
struct UntilePlaneArgs
{
    UntilePlane plane[kGatherPlanes]; // [blockIdx.y]: the carried planes in plane order
};
__global__ __launch_bounds__(256) void kUntilePlanes(UntilePlaneArgs args, uint32_t ownRank, uint32_t ownFirstTile, const uint32_t* __restrict__ tileSlot,
                                                     const uint32_t* __restrict__ tileOwner, uint32_t width, uint32_t height, uint32_t tilesX)
{
    const UntilePlane             pl = args.plane[blockIdx.y];
    const uint32_t                tile = blockIdx.x;
    const uint32_t                slot = tileSlot[tile];
    const float4* __restrict__    src = tileOwner[tile] == ownRank ? pl.own + static_cast<size_t>(slot - ownFirstTile) * kTilePixels : pl.staging + static_cast<size_t>(slot) * kTilePixels;
    float4* __restrict__          image = pl.image;
    const uint32_t                x0 = (tile % tilesX) * kTileSize, y0 = (tile / tilesX) * kTileSize;
#pragma unroll
    for (uint32_t k = 0; k < kTilePixels / 256; ++k)
    {
        const uint32_t w = k * 256 + threadIdx.x;
        const uint32_t block = w >> 6, lane = w & 63u;
        const uint32_t x = x0 + (block & 3u) * 8u + (lane & 7u), y = y0 + (block >> 2) * 8u + (lane >> 3);
        if (x < width && y < height) image[static_cast<size_t>(y) * width + x] = src[w];
    }
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
        for (uint32_t p = 0; p < kGatherPlanes; ++p)
        {
            if (((planeMask | kPlaneMaskImage) >> p & 1u) == 0u) continue;
            for (const GatherOp& op : one)
                if (op.isSend == sends) ops.push_back(GatherPlaneOp{op.isSend, op.peer, p, op.offsetTiles, op.countTiles});
        }
    return ops;
}

std::vector<GatherOp> gatherPlanCounts(const GatherLayout& g, uint32_t worldSize, uint32_t rank, uint32_t root, bool loopback)
{
    return gatherPlan(g, worldSize, rank, root, loopback); // (one word per tile: the offsets and counts in words are the one-plane plan's in tiles)
}

namespace
{
// ------------------------------------------------------------------------------------------------
// The LOCAL transport (round 6; a TEST transport, RF_COMM_TRANSPORT=local): the same exchange -- the same gatherPlan(), the same staging offsets, the same
// kUntile -- with every ncclSend / ncclRecv pair replaced by a device-to-device copy between the buffers of N communicators that live in ONE process, one host
// thread per rank.  RCCL refuses two ranks on one device, and the boxes this is developed on have one GPU: without this, TileComm::gatherFrame() and kUntile
// had only ever executed with one owner (world 1: every tile `own`, or every tile staging in loop-back).  With it, worlds 2 / 3 / 4 / 8 run on one GPU: the
// root's receives land at rankFirstTile[peer] of its staging area, kUntile picks own / staging per tile from tileOwner / tileSlot, and the image must equal
// the single-rank one bit for bit (tests/test_gpu_parity.py: test_local_transport_gather_*).  What it does NOT exercise: RCCL itself and xGMI.
//
// Semantics mirror a group of point-to-point operations: a send is matched with the receive the peer posts for it, in posting order per (source,
// destination); the receiver's stream waits for the sender's stream (an event recorded behind the sender's frame kernels), copies, and the sender's stream
// waits for the copy before anything queued behind the exchange may touch the buffer again.  Host side a rank posts all its sends, then performs its
// receives (each waits for its send to be posted), then waits until its sends have been taken -- dead-lock free for the gather (and for loop-back).  A
// peer that never arrives is an error after RF_COMM_TIMEOUT_S, as with RCCL.
// ------------------------------------------------------------------------------------------------
constexpr char kLocalMagic[8] = {'R', 'F', 'L', 'O', 'C', 'A', 'L', '1'};

struct LocalPost
{
    const void* src = nullptr;
    size_t      bytes = 0;
    int         srcDevice = 0;
    hipEvent_t  ready = nullptr;    // recorded on the sender's stream behind everything queued before the exchange
    hipEvent_t  consumed = nullptr; // recorded on the receiver's stream behind its copy (set when `taken`)
    bool        taken = false;
};

struct LocalFabric
{
    uint32_t                world = 0;
    std::mutex              mutex;
    std::condition_variable cv;
    std::map<std::pair<uint32_t, uint32_t>, std::deque<std::shared_ptr<LocalPost>>> mail; // (source, destination) -> sends not yet received, oldest first
    std::vector<hipEvent_t> freeEvents, allEvents;
    // allReduceMax: a generation barrier
    uint64_t generation = 0;
    uint32_t arrived = 0;
    double   running = 0.0, result = 0.0;
    uint32_t attached = 0;

    hipEvent_t takeEvent() // (mutex held)
    {
        if (!freeEvents.empty())
        {
            hipEvent_t e = freeEvents.back();
            freeEvents.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        RF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        allEvents.push_back(e);
        return e;
    }
    ~LocalFabric()
    {
        for (hipEvent_t e : allEvents) (void)hipEventDestroy(e);
    }
};

std::mutex                                                                    gFabricMutex;
std::map<std::array<uint8_t, kCommIdBytes>, std::weak_ptr<LocalFabric>>        gFabrics;

bool localTransportRequested()
{
    const char* v = std::getenv("RF_COMM_TRANSPORT");
    return v != nullptr && std::strcmp(v, "local") == 0;
}
bool isLocalId(const uint8_t id[kCommIdBytes]) { return std::memcmp(id, kLocalMagic, sizeof kLocalMagic) == 0; }

std::shared_ptr<LocalFabric> attachFabric(const uint8_t id[kCommIdBytes], uint32_t world)
{
    std::array<uint8_t, kCommIdBytes> key;
    std::memcpy(key.data(), id, kCommIdBytes);
    std::lock_guard<std::mutex> lock(gFabricMutex);
    std::shared_ptr<LocalFabric> f = gFabrics[key].lock();
    if (!f)
    {
        f = std::make_shared<LocalFabric>();
        f->world = world;
        gFabrics[key] = f;
    }
    if (f->world != world) throw std::runtime_error("local transport: the ranks of one id disagree about the world size");
    for (auto it = gFabrics.begin(); it != gFabrics.end();) it = it->second.expired() ? gFabrics.erase(it) : std::next(it);
    return f;
}
} // namespace

namespace
{
// seconds a rank waits for its peers in ncclCommInitRank and in its FIRST gather before it gives up with an error
// instead of hanging (a missing rank, a wrong id, a dead xGMI link); RF_COMM_TIMEOUT_S overrides, 0 = wait forever
double commTimeoutSeconds()
{
    if (const char* v = std::getenv("RF_COMM_TIMEOUT_S")) return std::atof(v);
    return 180.0;
}
} // namespace

struct TileComm::Impl
{
    ncclComm_t comm = nullptr;
    std::shared_ptr<LocalFabric> fabric; // the local (test) transport instead of RCCL: see LocalFabric
    uint32_t   rank = 0, world = 1;
    int        device = 0;

    uint32_t         layoutW = 0, layoutH = 0;
    GatherLayout     layout;
    DeviceBuffer<uint32_t> dTileSlot, dTileOwner;
    DeviceBuffer<float4>   staging;               // one GatherLayout area per carried plane, one after another
    DeviceBuffer<float4>   images[kGatherPlanes]; // per plane: the row-major image the root un-tiles into (allocated when first carried)
    DeviceBuffer<double>   scalar;
    // the per-tile sample counts of a gather with kGatherMaskTileCounts: staged rank after rank as they arrive, then per tile of the frame (kUntileCounts), and that on the host
    DeviceBuffer<uint32_t> countStaging, frameCounts;
    std::vector<uint32_t>  frameCountsHost;
    DeviceBuffer<float4>   meanImage; // readMean's, allocated by the first call
    uint32_t         imageW = 0, imageH = 0;
    // What the last gather left here (replaced as a whole by the next one): whether one was made, its root, and on the root the carried planes (0: none valid) and
    // the sample count the caller gave.  A plain gather drops the extra planes' validity, not their buffers.
    bool             gatherMade = false;
    uint32_t         lastRoot = 0, gatheredMask = 0, gatheredSamples = 0;
    // the root-side denoiser and estimate over the gathered planes: their work buffers, allocated by the first call; the snapshot is dropped by the next gather
    DenoiseWork      denoiseWork;
    bool             denoisedValid = false;
    NoiseWork        noiseWork;
    bool             firstGatherDone = false;
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

void TileComm::uniqueId(uint8_t out[kCommIdBytes])
{
    static_assert(sizeof(ncclUniqueId) == kCommIdBytes);
    if (localTransportRequested())
    {
        // the local transport's ids carry a magic prefix (TileComm's constructor recognises them whatever the environment says by then) + 120 random bytes
        std::memcpy(out, kLocalMagic, sizeof kLocalMagic);
        std::random_device rd;
        for (uint32_t i = sizeof kLocalMagic; i < kCommIdBytes; ++i) out[i] = static_cast<uint8_t>(rd());
        return;
    }
    ncclUniqueId id;
    RF_NCCL(ncclGetUniqueId(&id));
    std::memcpy(out, &id, kCommIdBytes);
}

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
    if (isLocalId(idBytes))
    {
        mImpl->fabric = attachFabric(idBytes, worldSize); // (not collective: a rank's peers are waited for in the exchange itself)
        return;
    }
    ncclUniqueId id;
    std::memcpy(&id, idBytes, kCommIdBytes);
    // ncclCommInitRank blocks until every rank of the world has called it.  It runs on a helper thread so that a rank whose
    // peers never arrive reports that after RF_COMM_TIMEOUT_S instead of hanging the job (the helper is abandoned then: the
    // caller is expected to exit).
    const double timeout = commTimeoutSeconds();
    auto         task = std::make_shared<std::packaged_task<ncclResult_t()>>([deviceOrdinal, worldSize, rank, id, comm = &mImpl->comm]() -> ncclResult_t {
        if (hipSetDevice(deviceOrdinal) != hipSuccess) return ncclUnhandledCudaError;
        return ncclCommInitRank(comm, static_cast<int>(worldSize), id, static_cast<int>(rank));
    });
    std::future<ncclResult_t> done = task->get_future();
    std::thread([task] { (*task)(); }).detach();
    if (timeout > 0.0 && done.wait_for(std::chrono::duration<double>(timeout)) != std::future_status::ready)
    {
        mImpl.release(); // the helper still writes into it: leaked on purpose
        throw std::runtime_error("RCCL: ncclCommInitRank did not complete within " + std::to_string(static_cast<int>(timeout)) + " s on rank " + std::to_string(rank) + " of " +
                                 std::to_string(worldSize) + " (a rank is missing, or the ranks do not share one unique id); RF_COMM_TIMEOUT_S changes the limit");
    }
    RF_NCCL(done.get());
    int count = 0;
    RF_NCCL(ncclCommCount(mImpl->comm, &count));
    if (static_cast<uint32_t>(count) != worldSize) throw std::runtime_error("RCCL communicator spans " + std::to_string(count) + " ranks, expected " + std::to_string(worldSize));
}

TileComm::~TileComm()
{
    if (mImpl && mImpl->comm)
    {
        (void)hipSetDevice(mImpl->device);
        (void)ncclCommDestroy(mImpl->comm);
    }
    if (mImpl && mImpl->exchangeStart)
    {
        (void)hipEventDestroy(mImpl->exchangeStart);
        (void)hipEventDestroy(mImpl->exchangeStop);
    }
}

uint32_t TileComm::rank() const { return mImpl->rank; }
uint32_t TileComm::worldSize() const { return mImpl->world; }
int      TileComm::deviceOrdinal() const { return mImpl->device; }

bool TileComm::localTransport() const { return mImpl->fabric != nullptr; }

void TileComm::rcclInfo(uint32_t& count, uint32_t& userRank, int& device) const
{
    if (mImpl->fabric)
    {
        count = mImpl->world, userRank = mImpl->rank, device = mImpl->device; // (no RCCL communicator behind it: localTransport() says so)
        return;
    }
    int c = 0, r = 0, d = 0;
    RF_NCCL(ncclCommCount(mImpl->comm, &c));
    RF_NCCL(ncclCommUserRank(mImpl->comm, &r));
    RF_NCCL(ncclCommCuDevice(mImpl->comm, &d));
    count = static_cast<uint32_t>(c), userRank = static_cast<uint32_t>(r), device = d;
}

const void* TileComm::gatherFrame(const void* compactDevice, uint32_t width, uint32_t height, uint32_t root, void* streamHandle, bool loopback)
{
    const void* const planes[kGatherPlanes] = {compactDevice, nullptr, nullptr, nullptr};
    return gatherPlanes(planes, kPlaneMaskImage, 0u, width, height, root, streamHandle, loopback);
}

const void* TileComm::gatherPlanes(const void* const compactDevice[kGatherPlanes], uint32_t planeMask, uint32_t samples, uint32_t width, uint32_t height, uint32_t root,
                                   void* streamHandle, bool loopback, const uint32_t* tileCountsDevice)
{
    Impl& m = *mImpl;
    if (m.comm == nullptr && !m.fabric) throw std::runtime_error("the RCCL communicator was aborted");
    if (root >= m.world) throw std::invalid_argument("gather root out of range");
    if (width == 0 || height == 0) throw std::invalid_argument("empty frame");
    const bool withCounts = (planeMask & kGatherMaskTileCounts) != 0u;
    if ((planeMask & kPlaneMaskImage) == 0u || ((planeMask & ~kGatherMaskTileCounts) >> kGatherPlanes) != 0u)
        throw std::invalid_argument("gather plane mask: plane 0 always travels, planes 0 .. 3 exist");
    // the carried planes in plane order; carriedIndex[p]: which staging area plane p has
    uint32_t carried[kGatherPlanes] = {}, carriedIndex[kGatherPlanes] = {}, numPlanes = 0;
    for (uint32_t p = 0; p < kGatherPlanes; ++p)
        if (planeMask >> p & 1u) carriedIndex[p] = numPlanes, carried[numPlanes++] = p;
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    m.ensureLayout(width, height, stream);
    const GatherLayout& g = m.layout;
    const auto          tilesOf = [&](uint32_t r) { return g.rankFirstTile[r + 1] - g.rankFirstTile[r]; };
    const size_t        floatsPerTile = static_cast<size_t>(kTilePixels) * 4;
    const bool          isRoot = m.rank == root;
    for (uint32_t k = 0; k < numPlanes; ++k)
        if (tilesOf(m.rank) > 0 && compactDevice[carried[k]] == nullptr) throw std::invalid_argument("null tile buffer");
    if (withCounts && tilesOf(m.rank) > 0 && tileCountsDevice == nullptr) throw std::invalid_argument("null tile count buffer");
    // the record of the last gather goes now: whatever happens below, nothing stale is read through the root-side calls
    m.gatherMade = true;
    m.lastRoot = root;
    m.gatheredMask = 0;
    m.gatheredSamples = 0;
    m.denoisedValid = false;
    const size_t planeStagingPixels = static_cast<size_t>(g.rankFirstTile[m.world]) * kTilePixels; // one plane's staging area
    if (isRoot)
    {
        const size_t stagingWant = planeStagingPixels * numPlanes, imageWant = static_cast<size_t>(width) * height;
        bool         grows = stagingWant > m.staging.count;
        for (uint32_t k = 0; k < numPlanes; ++k) grows = grows || imageWant > m.images[carried[k]].count;
        const size_t frameTiles = static_cast<size_t>(g.tilesX) * g.tilesY;
        if (withCounts) grows = grows || g.rankFirstTile[m.world] > m.countStaging.count || frameTiles > m.frameCounts.count;
        if (grows) RF_HIP(hipStreamSynchronize(stream)); // a consumer of the old buffers may still run
        if (withCounts) m.countStaging.ensure(g.rankFirstTile[m.world]), m.frameCounts.ensure(frameTiles);
        m.staging.ensure(stagingWant);
        for (uint32_t k = 0; k < numPlanes; ++k) m.images[carried[k]].ensure(imageWant);
        m.imageW = width;
        m.imageH = height;
    }
    const auto stagingOf = [&](const GatherPlaneOp& op) { return m.staging.ptr + carriedIndex[op.plane] * planeStagingPixels + static_cast<size_t>(op.offsetTiles) * kTilePixels; };
    const auto compactOf = [&](const GatherPlaneOp& op) { return static_cast<const float*>(compactDevice[op.plane]) + op.offsetTiles * floatsPerTile; };

    // one group: exactly the operations of gatherPlanPlanes() -- with the image alone, gatherPlan()'s (the lists the CPU tests check for every rank of a world) -- and
    // behind them, with the counts, those of gatherPlanCounts(): per (source, destination) pair the counts are the last send and the last receive
    struct Transfer
    {
        bool           isSend;
        uint32_t       peer;
        const void*    from; // a send's source
        void*          to;   // a receive's destination
        size_t         words; // 4-byte elements
        ncclDataType_t type;
    };
    std::vector<Transfer> plan;
    for (const GatherPlaneOp& op : gatherPlanPlanes(g, m.world, m.rank, root, loopback, planeMask & ~kGatherMaskTileCounts))
        plan.push_back(Transfer{op.isSend != 0u, op.peer, op.isSend ? compactOf(op) : nullptr, op.isSend ? nullptr : stagingOf(op), op.countTiles * floatsPerTile, ncclFloat});
    if (withCounts)
        for (const GatherOp& op : gatherPlanCounts(g, m.world, m.rank, root, loopback))
            plan.push_back(Transfer{op.isSend != 0u, op.peer, op.isSend ? tileCountsDevice + op.offsetTiles : nullptr, op.isSend ? nullptr : m.countStaging.ptr + op.offsetTiles,
                                    op.countTiles, ncclUint32});
    // (first exchange only) marks the end of what was queued on the stream BEFORE the exchange -- this rank's frame kernels: the
    // watchdog below measures the exchange, not the render in front of it
    hipEvent_t queuedBefore = nullptr;
    if (!m.firstGatherDone)
    {
        RF_HIP(hipEventCreateWithFlags(&queuedBefore, hipEventDisableTiming));
        RF_HIP(hipEventRecord(queuedBefore, stream));
    }
    struct EventGuard
    {
        hipEvent_t& e;
        ~EventGuard()
        {
            if (e) (void)hipEventDestroy(e);
        }
    } eventGuard{queuedBefore};
    if (m.exchangeStart == nullptr)
    {
        RF_HIP(hipEventCreate(&m.exchangeStart));
        RF_HIP(hipEventCreate(&m.exchangeStop));
    }
    m.exchangeTimed = false;
    RF_HIP(hipEventRecord(m.exchangeStart, stream));
    if (m.fabric)
    {
        // ---- the local transport: the plan's operations as device-to-device copies between the ranks' buffers (see LocalFabric)
        LocalFabric&  f = *m.fabric;
        const double  timeout = commTimeoutSeconds();
        const auto    waitFor = [&](std::unique_lock<std::mutex>& lock, auto&& ready, const char* what) {
            if (timeout > 0.0)
            {
                if (!f.cv.wait_for(lock, std::chrono::duration<double>(timeout), ready))
                    throw std::runtime_error(std::string("local transport: ") + what + " did not happen within " + std::to_string(static_cast<int>(timeout)) + " s on rank " +
                                             std::to_string(m.rank) + " (a peer is missing or disagrees about frame size / root)");
            }
            else f.cv.wait(lock, ready);
        };
        std::vector<std::shared_ptr<LocalPost>> mine;
        for (const Transfer& op : plan) // 1. post every send
        {
            if (!op.isSend) continue;
            auto post = std::make_shared<LocalPost>();
            post->src = op.from;
            post->bytes = op.words * sizeof(uint32_t);
            post->srcDevice = m.device;
            {
                std::lock_guard<std::mutex> lock(f.mutex);
                post->ready = f.takeEvent();
            }
            RF_HIP(hipEventRecord(post->ready, stream));
            {
                std::lock_guard<std::mutex> lock(f.mutex);
                f.mail[{m.rank, op.peer}].push_back(post);
            }
            f.cv.notify_all();
            mine.push_back(post);
        }
        for (const Transfer& op : plan) // 2. every receive: wait for the peer's send, copy behind it
        {
            if (op.isSend) continue;
            std::shared_ptr<LocalPost> post;
            {
                std::unique_lock<std::mutex> lock(f.mutex);
                auto&                        box = f.mail[{op.peer, m.rank}];
                waitFor(lock, [&] { return !box.empty(); }, "a peer's send");
                post = box.front();
                box.pop_front();
                post->consumed = f.takeEvent();
            }
            if (post->bytes != op.words * sizeof(uint32_t)) // (a plane's tiles or a shard's counts: each operation has its own size)
                throw std::runtime_error("local transport: rank " + std::to_string(op.peer) + " sends " + std::to_string(post->bytes) + " bytes, rank " + std::to_string(m.rank) + " expects " +
                                         std::to_string(op.words * sizeof(uint32_t)) + " (the ranks disagree about the frame)");
            RF_HIP(hipStreamWaitEvent(stream, post->ready, 0));
            RF_HIP(hipMemcpyAsync(op.to, post->src, post->bytes, hipMemcpyDeviceToDevice, stream));
            RF_HIP(hipEventRecord(post->consumed, stream));
            {
                std::lock_guard<std::mutex> lock(f.mutex);
                post->taken = true;
            }
            f.cv.notify_all();
        }
        for (const std::shared_ptr<LocalPost>& post : mine) // 3. my sends: the buffer is mine again once the receiver's copy has run
        {
            {
                std::unique_lock<std::mutex> lock(f.mutex);
                waitFor(lock, [&] { return post->taken; }, "the root's receive");
            }
            RF_HIP(hipStreamWaitEvent(stream, post->consumed, 0));
            std::lock_guard<std::mutex> lock(f.mutex);
            f.freeEvents.push_back(post->ready);
            f.freeEvents.push_back(post->consumed);
        }
        m.firstGatherDone = true;
    }
    else
    {
    RF_NCCL(ncclGroupStart());
    try
    {
        for (const Transfer& op : plan)
        {
            if (op.isSend) RF_NCCL(ncclSend(op.from, op.words, op.type, static_cast<int>(op.peer), m.comm, stream));
            else RF_NCCL(ncclRecv(op.to, op.words, op.type, static_cast<int>(op.peer), m.comm, stream));
        }
    }
    catch (...)
    {
        (void)ncclGroupEnd(); // never leave the thread inside an open group
        throw;
    }
    RF_NCCL(ncclGroupEnd());
    if (!m.firstGatherDone)
    {
        // The first exchange of a communicator also sets up its peer connections; a peer that never posts its side (it died, it
        // disagrees about the frame size or the root) would leave this stream stuck forever.  Watch this one exchange: past the
        // time limit the communicator is aborted and the caller gets an error instead of a hang.  Later gathers are not watched
        // (they stay fully asynchronous).  NOTE: an exception thrown on one rank leaves its peers waiting in their own gather
        // until THEIR limit expires.  The clock starts when the work queued on this stream before the exchange (Renderer::render()
        // is asynchronous: the whole frame may still be in front of it) has drained, so a long first frame does not abort a healthy
        // job; what remains inside the limit is the connection set-up, the transfer, and the wait for the slowest peer to finish ITS
        // frame -- ranks own equal tile counts (+-1), so that wait is a fraction of a frame.
        // A second, much larger cap (kDrainFactor x the limit, from loop entry) covers the case the first clock never starts in: this rank's OWN queued kernels
        // never drain (a hung or faulted kernel keeps the event at hipErrorNotReady forever) -- the loop would otherwise spin without any limit.
        constexpr double kDrainFactor = 20.0;
        const double timeout = commTimeoutSeconds();
        const auto   entered = std::chrono::steady_clock::now();
        auto         t0 = entered;
        bool         drained = false;
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
            RF_NCCL(ncclCommGetAsyncError(m.comm, &async));
            if (async != ncclSuccess && async != ncclInProgress) throw std::runtime_error(std::string("RCCL error during the first frame exchange: ") + ncclGetErrorString(async));
            if (drained && timeout > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout)
            {
                (void)ncclCommAbort(m.comm);
                m.comm = nullptr;
                throw std::runtime_error("RCCL: the first frame exchange did not complete within " + std::to_string(static_cast<int>(timeout)) + " s on rank " +
                                         std::to_string(m.rank) + " (a peer is missing or disagrees about frame size / root); communicator aborted");
            }
            if (!drained && timeout > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - entered).count() > kDrainFactor * timeout)
            {
                (void)ncclCommAbort(m.comm);
                m.comm = nullptr;
                throw std::runtime_error("RCCL: the work queued in front of the first frame exchange did not drain within " + std::to_string(static_cast<int>(kDrainFactor * timeout)) +
                                         " s on rank " + std::to_string(m.rank) + " (a kernel of this rank's own frame hangs); communicator aborted");
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        m.firstGatherDone = true;
    }
    } // (RCCL transport)
    if (!isRoot)
    {
        RF_HIP(hipEventRecord(m.exchangeStop, stream));
        m.exchangeTimed = true;
        return nullptr;
    }

    const uint32_t numTiles = g.tilesX * g.tilesY;
    if (numPlanes == 1)
        hipLaunchKernelGGL(kUntile, dim3(numTiles), dim3(256), 0, stream, m.staging.ptr, static_cast<const float4*>(compactDevice[kPlaneImage]), loopback ? 0xFFFFFFFFu : m.rank,
                           g.rankFirstTile[m.rank], m.dTileSlot.ptr, m.dTileOwner.ptr, width, height, g.tilesX, m.images[kPlaneImage].ptr);
    else
    {
        UntilePlaneArgs args{};
        for (uint32_t k = 0; k < numPlanes; ++k)
            args.plane[k] = UntilePlane{m.staging.ptr + k * planeStagingPixels, static_cast<const float4*>(compactDevice[carried[k]]), m.images[carried[k]].ptr};
        hipLaunchKernelGGL(kUntilePlanes, dim3(numTiles, numPlanes), dim3(256), 0, stream, args, loopback ? 0xFFFFFFFFu : m.rank, g.rankFirstTile[m.rank], m.dTileSlot.ptr,
                           m.dTileOwner.ptr, width, height, g.tilesX);
    }
    if (withCounts)
        hipLaunchKernelGGL(kUntileCounts, dim3((numTiles + 255u) / 256u), dim3(256), 0, stream, m.countStaging.ptr, tileCountsDevice, loopback ? 0xFFFFFFFFu : m.rank,
                           g.rankFirstTile[m.rank], m.dTileSlot.ptr, m.dTileOwner.ptr, numTiles, m.frameCounts.ptr);
    RF_HIP(hipGetLastError());
    RF_HIP(hipEventRecord(m.exchangeStop, stream));
    m.exchangeTimed = true;
    if (withCounts)
    {
        // the counts on the host as well (the root-side calls check them, N is the largest): the one wait of such a gather, on the root alone
        m.frameCountsHost.assign(numTiles, 0u);
        RF_HIP(hipMemcpyAsync(m.frameCountsHost.data(), m.frameCounts.ptr, numTiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        RF_HIP(hipStreamSynchronize(stream));
        samples = *std::max_element(m.frameCountsHost.begin(), m.frameCountsHost.end());
    }
    m.gatheredMask = planeMask;
    m.gatheredSamples = samples;
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
const char* const kPlaneNames[kGatherPlanes] = {"the image (plane 0)", "the first-hit AOVs (plane 1, AC: gather with RF_GATHER_AOVS)", "the first-hit AOVs (plane 2, ND: gather with RF_GATHER_AOVS)",
                                                "the radiance second moments (plane 3, Q: gather with RF_GATHER_MOMENTS)"};
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
    if (plane >= kGatherPlanes) throw std::invalid_argument("plane out of range: 0 = S, 1 = AC, 2 = ND, 3 = Q");
    m.requireGathered("rf_comm_plane_device", 1u << plane, kPlaneNames[plane]);
    return m.images[plane].ptr;
}

void TileComm::readPlane(uint32_t plane, float* dstHost, void* streamHandle)
{
    Impl& m = *mImpl;
    if (plane >= kGatherPlanes) throw std::invalid_argument("plane out of range: 0 = S, 1 = AC, 2 = ND, 3 = Q");
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
    if (m.gatheredSamples == 0u) throw std::invalid_argument("rf_comm_denoise: the gathered sums hold no sample");
    if (static_cast<uint64_t>(m.imageW) * m.imageH >= (1ull << 31)) throw std::invalid_argument("rf_comm_denoise: image too large");
    const bool perTile = (m.gatheredMask & kGatherMaskTileCounts) != 0u;
    if (perTile && *std::min_element(m.frameCountsHost.begin(), m.frameCountsHost.end()) == 0u) throw std::invalid_argument("rf_comm_denoise: a tile of the gathered frame holds no sample");
    RF_HIP(hipSetDevice(m.device));
    // the gathered planes are row-major (tilesX = 0) and hold one count N: the filter rf_denoise_images runs, without the sums leaving the device -- or, gathered with
    // the counts, each tile its own: rf_denoise_tiles'
    enqueueDenoise(static_cast<hipStream_t>(streamHandle), m.denoiseWork, m.images[kPlaneImage].ptr, m.images[kPlaneAlbedoCoverage].ptr, m.images[kPlaneNormalDepth].ptr, m.imageW,
                   m.imageH, 0u, m.gatheredSamples, params, exposure, perTile ? m.frameCounts.ptr : nullptr);
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
    if (m.gatheredSamples < 2u) throw std::invalid_argument("rf_comm_noise_estimate: a variance needs at least 2 accumulated samples");
    if (static_cast<uint64_t>(m.imageW) * m.imageH >= (1ull << 31)) throw std::invalid_argument("rf_comm_noise_estimate: image too large");
    RF_HIP(hipSetDevice(m.device));
    if (m.gatheredMask & kGatherMaskTileCounts)
    {
        // every tile with its own count; `samples` reports the largest
        if (*std::min_element(m.frameCountsHost.begin(), m.frameCountsHost.end()) < 2u)
            throw std::invalid_argument("rf_comm_noise_estimate: a variance needs at least 2 samples in every tile of the gathered frame");
        TileSelection sel;
        sel.tileSamplesDevice = m.frameCounts.ptr;
        return runNoiseEstimateTiles(static_cast<hipStream_t>(streamHandle), m.noiseWork, m.images[kPlaneImage].ptr, m.images[kPlaneMoments].ptr, m.imageW, m.imageH, false, sel,
                                     m.gatheredSamples, errorMap, tileSum, tileMax, nullptr);
    }
    return runNoiseEstimate(static_cast<hipStream_t>(streamHandle), m.noiseWork, m.images[kPlaneImage].ptr, m.images[kPlaneMoments].ptr, m.imageW, m.imageH, false,
                            m.gatheredSamples, errorMap, tileSum, tileMax);
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

double TileComm::allReduceMax(double value, void* streamHandle)
{
    Impl&       m = *mImpl;
    hipStream_t stream = static_cast<hipStream_t>(streamHandle);
    RF_HIP(hipSetDevice(m.device));
    if (m.fabric)
    {
        // local transport: a generation barrier over the fabric's ranks (host side; the caller's stream is drained first, as the RCCL path's read-back does)
        RF_HIP(hipStreamSynchronize(stream));
        LocalFabric&                 f = *m.fabric;
        std::unique_lock<std::mutex> lock(f.mutex);
        const uint64_t               gen = f.generation;
        f.running = f.arrived == 0 ? value : std::max(f.running, value);
        if (++f.arrived == f.world)
        {
            f.result = f.running;
            f.arrived = 0;
            ++f.generation;
            f.cv.notify_all();
            return f.result;
        }
        const double timeout = commTimeoutSeconds();
        const auto   released = [&] { return f.generation != gen; };
        if (timeout > 0.0)
        {
            if (!f.cv.wait_for(lock, std::chrono::duration<double>(timeout), released)) throw std::runtime_error("local transport: all-reduce timed out on rank " + std::to_string(m.rank));
        }
        else f.cv.wait(lock, released);
        return f.result;
    }
    m.scalar.ensure(2);
    RF_HIP(hipMemcpyAsync(m.scalar.ptr, &value, sizeof value, hipMemcpyHostToDevice, stream));
    RF_NCCL(ncclAllReduce(m.scalar.ptr, m.scalar.ptr + 1, 1, ncclDouble, ncclMax, m.comm, stream));
    double out = 0.0;
    RF_HIP(hipMemcpyAsync(&out, m.scalar.ptr + 1, sizeof out, hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
    return out;
}
} // namespace rf
