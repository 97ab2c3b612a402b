// rf_checkpoint.hip -- the state digest of a handle's sums and the checkpoint built on it (the definition and the calls: include/rayfinder_amd.h; the blob: INTEGRATION.md 3).
//   kDigestTiles   grid (tiles in the list, planes): one 256-lane workgroup per (tile, plane), 4 pixels per lane, each pixel one coalesced 16-byte load of the compact
//                  tile-major texel; the terms are summed mod 2^64 -- a wave reduction by __shfl_down on the two halves, the four waves through LDS -- and lane 0 stores one
//                  word per (plane, tile).  No atomics, no floating point: a sum mod 2^64 has no order, so the word is the same however the lanes are scheduled.
// The host adds the tile words into plane digests, and a checkpoint carries them tile by tile: a load verifies what lies in device memory after its copies.
#include "rf_checkpoint.hpp"

#include "rf_hip_host.hpp"
#include "rf_renderer.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>

namespace rf
{
namespace
{
using namespace ckpt;

struct DigestPlaneArgs
{
    const uint4* plane[kMaxPlanes]; // [blockIdx.y]: the plane's compact tile-major texels
    uint32_t     id[kMaxPlanes];    // ... and its id in the digest's numbering
};

__device__ __forceinline__ uint64_t mix64Device(uint64_t z)
{
    z ^= z >> 30, z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27, z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// tileTable: the list's tile ids, and behind them each tile's slot in the buffers (numTiles words each); out[plane * numTiles + t]
__global__ __launch_bounds__(256) void kDigestTiles(DigestPlaneArgs args, const uint32_t* __restrict__ tileTable, uint32_t numTiles, uint32_t width, uint32_t height,
                                                    uint32_t tilesX, uint64_t* __restrict__ out)
{
    const uint32_t t = blockIdx.x, p = blockIdx.y;
    const uint32_t tile = tileTable[t], slot = tileTable[numTiles + t];
    const uint4* __restrict__ src = args.plane[p] + static_cast<size_t>(slot) * kTileTexels;
    const uint64_t planeKey = static_cast<uint64_t>(args.id[p]) << 32;
    const uint32_t x0 = (tile % tilesX) * 32u, y0 = (tile / tilesX) * 32u;
    uint64_t       sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTileTexels / 256u; ++k)
    {
        const uint32_t w = k * 256u + threadIdx.x;
        const uint32_t block = w >> 6, lane = w & 63u;
        const uint32_t x = x0 + (block & 3u) * 8u + (lane & 7u), y = y0 + (block >> 2) * 8u + (lane >> 3);
        if (x < width && y < height) // (the padding texels of a ragged tile are never read)
        {
            const uint4    v = src[w];
            const uint64_t key = mix64Device(planeKey | (static_cast<uint64_t>(y) * width + x));
            sum += mix64Device(key ^ ((static_cast<uint64_t>(v.y) << 32) | v.x)) + mix64Device((key + 0x9E3779B97F4A7C15ull) ^ ((static_cast<uint64_t>(v.w) << 32) | v.z));
        }
    }
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1)
    {
        const uint32_t lo = __shfl_down(static_cast<uint32_t>(sum), offset), hi = __shfl_down(static_cast<uint32_t>(sum >> 32), offset);
        sum += (static_cast<uint64_t>(hi) << 32) | lo;
    }
    __shared__ uint64_t waveSum[4];
    if ((threadIdx.x & 63u) == 0u) waveSum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) out[static_cast<size_t>(p) * numTiles + t] = waveSum[0] + waveSum[1] + waveSum[2] + waveSum[3];
}

// storage index (Renderer::CheckpointBooks::planes) of a digest plane id
uint32_t storageIndex(uint32_t id) { return id == kPlaneD ? 4u : (id >= kPlaneBucket0 ? 5u + (id - kPlaneBucket0) : id); }

// The tile words of `numPlanes` planes over the handle's own tiles, slot k of every buffer holding tile tiles[k]: [plane][tile], waited for
// (kernelMs != nullptr: the launch's own time between two events on the stream)
std::vector<uint64_t> digestTiles(Renderer& r, const void* const* planes, const uint32_t* ids, uint32_t numPlanes, float* kernelMs = nullptr)
{
    if (kernelMs) *kernelMs = 0.0f;
    const std::span<const uint32_t> tiles = r.shardTiles();
    const uint32_t                  n = static_cast<uint32_t>(tiles.size());
    std::vector<uint64_t>           words(static_cast<size_t>(numPlanes) * n);
    if (words.empty()) return words;
    if (numPlanes > kMaxPlanes) throw std::logic_error("digestTiles: more planes than a handle holds");
    DigestPlaneArgs args{};
    for (uint32_t p = 0; p < numPlanes; ++p)
    {
        if (planes[p] == nullptr) throw std::logic_error("digestTiles: a plane without a buffer");
        args.plane[p] = static_cast<const uint4*>(planes[p]), args.id[p] = ids[p];
    }
    std::vector<uint32_t> table(tiles.begin(), tiles.end());
    for (uint32_t k = 0; k < n; ++k) table.push_back(k);
    // the words and, behind them, the table: one buffer the handle keeps (no allocation per call once it has grown)
    const hipStream_t stream = static_cast<hipStream_t>(r.streamHandle());
    const size_t      wordBytes = words.size() * sizeof(uint64_t), tableBytes = table.size() * sizeof(uint32_t);
    auto* const       wordsDevice = static_cast<uint64_t*>(r.checkpointScratch(wordBytes + tableBytes));
    auto* const       tableDevice = reinterpret_cast<uint32_t*>(wordsDevice + words.size());
    RF_HIP(hipMemcpyAsync(tableDevice, table.data(), tableBytes, hipMemcpyHostToDevice, stream)); // (pageable memory: staged before the call returns)
    struct Events
    {
        hipEvent_t start = nullptr, stop = nullptr;
        ~Events()
        {
            if (start) (void)hipEventDestroy(start);
            if (stop) (void)hipEventDestroy(stop);
        }
    } events;
    if (kernelMs)
    {
        RF_HIP(hipEventCreate(&events.start));
        RF_HIP(hipEventCreate(&events.stop));
        RF_HIP(hipEventRecord(events.start, stream));
    }
    hipLaunchKernelGGL(kDigestTiles, dim3(n, numPlanes), dim3(256), 0, stream, args, tableDevice, n, r.width(), r.height(), TileGrid(r.width(), r.height()).tilesX, wordsDevice);
    RF_HIP(hipGetLastError());
    if (kernelMs) RF_HIP(hipEventRecord(events.stop, stream));
    RF_HIP(hipMemcpyAsync(words.data(), wordsDevice, wordBytes, hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
    if (kernelMs) RF_HIP(hipEventElapsedTime(kernelMs, events.start, events.stop));
    return words;
}

Header headerOf(const Renderer::CheckpointBooks& b, Renderer& r)
{
    Header h{};
    std::memcpy(h.magic, kMagic, sizeof kMagic);
    h.version = kVersion, h.headerBytes = kHeaderBytes;
    h.width = r.width(), h.height = r.height(), h.numTiles = static_cast<uint32_t>(r.shardTiles().size());
    h.frameCount = b.frameCount, h.accumulated = b.accumulated, h.frameLeadingSamples = b.frameLeadingSamples, h.frameMinTileSamples = b.frameMinTileSamples;
    h.aovFlags = b.aovFlags, h.moments = b.moments, h.directWord = b.directWord, h.bucketsWord = b.bucketsWord;
    for (uint32_t f = 0; f < kFamilies; ++f) h.family[f] = Family{b.family[f].samples, b.family[f].samples == 0u ? 1u : 0u};
    std::memcpy(h.camera, b.camera, sizeof h.camera);
    std::memcpy(h.sky, b.sky, sizeof h.sky);
    h.numBounces = b.numBounces;
    std::memcpy(h.sceneCounts, b.sceneCounts, sizeof h.sceneCounts);
    std::memcpy(h.rootBounds, b.rootBounds, sizeof h.rootBounds);
    h.totalBytes = blobBytes(h);
    return h;
}

[[noreturn]] void refuse(const std::string& what) { throw std::invalid_argument("load_checkpoint: " + what); }
} // namespace

StateDigest stateDigest(Renderer& r)
{
    RF_HIP(hipSetDevice(r.deviceOrdinal()));
    const Renderer::CheckpointBooks b = r.checkpointBooks();
    StateDigest                     d;
    d.frameCount = b.frameCount, d.accumulated = b.accumulated, d.numTiles = static_cast<uint32_t>(r.shardTiles().size());
    d.aovFlags = b.aovFlags, d.moments = b.moments, d.directWord = b.directWord, d.bucketsWord = b.bucketsWord;
    for (uint32_t f = 0; f < kFamilies; ++f) d.familyOn[f] = b.family[f].on ? 1u : 0u, d.familySamples[f] = b.family[f].samples;
    // every plane of a family that is on (a restarted one lies there as zeros)
    const void* planes[kMaxPlanes];
    uint32_t    ids[kMaxPlanes], storage[kMaxPlanes], numPlanes = 0;
    for (uint32_t s = 0; s < kMaxPlanes; ++s)
        if (b.planes[s] != nullptr) planes[numPlanes] = b.planes[s], storage[numPlanes] = s, ids[numPlanes++] = s == 4u ? kPlaneD : (s >= 5u ? kPlaneBucket0 + (s - 5u) : s);
    const std::vector<uint64_t> words = digestTiles(r, planes, ids, numPlanes, &d.kernelMs);
    for (uint32_t p = 0; p < numPlanes; ++p)
        for (uint32_t k = 0; k < d.numTiles; ++k) d.plane[storage[p]] += words[static_cast<size_t>(p) * d.numTiles + k];
    const std::span<const uint32_t> tiles = r.shardTiles();
    for (uint32_t k = 0; k < d.numTiles; ++k) d.counts += countTerm(tiles[k], b.tileSamples[k]);
    return d;
}

void saveCheckpoint(Renderer& r, void* dst, uint64_t* bytes)
{
    RF_HIP(hipSetDevice(r.deviceOrdinal()));
    const Renderer::CheckpointBooks b = r.checkpointBooks();
    const Header                    h = headerOf(b, r);
    if (dst == nullptr)
    {
        *bytes = h.totalBytes;
        return;
    }
    if (*bytes < h.totalBytes) throw std::invalid_argument("save_checkpoint: the buffer holds " + std::to_string(*bytes) + " bytes and the checkpoint needs " + std::to_string(h.totalBytes));
    uint32_t       ids[kMaxPlanes];
    const uint32_t numPlanes = storedPlanes(h, ids), n = h.numTiles;
    const void*    planes[kMaxPlanes];
    for (uint32_t p = 0; p < numPlanes; ++p) planes[p] = b.planes[storageIndex(ids[p])];
    const std::vector<uint64_t>     words = digestTiles(r, planes, ids, numPlanes);
    const std::span<const uint32_t> tiles = r.shardTiles();
    auto*                           at = static_cast<unsigned char*>(dst);
    std::memcpy(at, &h, kHeaderBytes), at += kHeaderBytes;
    if (n != 0u)
    {
        std::memcpy(at, tiles.data(), 4ull * n), at += 4ull * n;
        std::memcpy(at, b.tileSamples.data(), 4ull * n), at += 4ull * n;
    }
    if (!words.empty()) std::memcpy(at, words.data(), words.size() * sizeof(uint64_t)), at += words.size() * sizeof(uint64_t);
    // the compact buffers lie in slot order already: every plane leaves as it is
    const uint64_t planeBytes = static_cast<uint64_t>(n) * kTileTexels * kTexelBytes;
    // (the caller's memory is pinned for the length of the copies where the runtime allows it: the planes then travel by DMA straight into it, not through a staging buffer)
    const uint64_t payload = planeBytes * numPlanes;
    const bool     pinned = payload != 0u && hipHostRegister(at, payload, hipHostRegisterDefault) == hipSuccess;
    if (payload != 0u && !pinned) (void)hipGetLastError();
    struct Unpin
    {
        void* ptr;
        ~Unpin()
        {
            if (ptr) (void)hipHostUnregister(ptr);
        }
    } unpin{pinned ? at : nullptr};
    for (uint32_t p = 0; p < numPlanes && planeBytes != 0u; ++p, at += planeBytes) RF_HIP(hipMemcpy(at, planes[p], planeBytes, hipMemcpyDeviceToHost));
    *bytes = h.totalBytes;
}

void loadCheckpoint(Renderer& r, const void* const* blobs, const uint64_t* sizes, uint32_t count)
{
    if (blobs == nullptr || sizes == nullptr || count == 0u) refuse("no blob");
    std::vector<View> views;
    for (uint32_t i = 0; i < count; ++i) views.push_back(parse(blobs[i], sizes[i]));
    for (uint32_t i = 1; i < count; ++i) requireSameFrame(views[0], views[i]);
    // the handle's books as they stand: no device call is made before the last refusal below
    const Renderer::CheckpointBooks mine = r.checkpointBooks(false);
    const Header&                   h = views[0].header;
    if (h.width != r.width() || h.height != r.height())
        refuse("the checkpoint's frame is " + std::to_string(h.width) + " x " + std::to_string(h.height) + " and the handle's size is " + std::to_string(r.width()) + " x " + std::to_string(r.height()));
    if (std::memcmp(h.camera, mine.camera, sizeof h.camera) != 0) refuse("the checkpoint was rendered with another camera than the handle's");
    if (std::memcmp(h.sky, mine.sky, sizeof h.sky) != 0) refuse("the checkpoint was rendered with another sky than the handle's");
    if (h.numBounces != mine.numBounces) refuse("the checkpoint was rendered with numBounces " + std::to_string(h.numBounces) + " and the handle's is " + std::to_string(mine.numBounces));
    if (std::memcmp(h.sceneCounts, mine.sceneCounts, sizeof h.sceneCounts) != 0 || std::memcmp(h.rootBounds, mine.rootBounds, sizeof h.rootBounds) != 0)
        refuse("the checkpoint is of another scene than the handle's (the counts of BVH nodes, triangles, textures or texels, or the root box, differ)");
    if (h.aovFlags != mine.aovFlags || h.moments != mine.moments || h.directWord != mine.directWord || h.bucketsWord != mine.bucketsWord)
        refuse("the checkpoint's switch words (AOV flags " + std::to_string(h.aovFlags) + ", moments " + std::to_string(h.moments) + ", direct " + std::to_string(h.directWord) + ", buckets " +
               std::to_string(h.bucketsWord) + ") differ from the handle's (" + std::to_string(mine.aovFlags) + ", " + std::to_string(mine.moments) + ", " + std::to_string(mine.directWord) + ", " +
               std::to_string(mine.bucketsWord) + "): set them first (rf_checkpoint_info)");
    uint32_t lead = 0; // the blob that holds the most samples: the families' books are read from it
    for (uint32_t i = 0; i < count; ++i)
    {
        if (views[i].header.accumulated > mine.samplesPerPixel)
            refuse("the checkpoint's accumulated count " + std::to_string(views[i].header.accumulated) + " is above the handle's numSamplesPerPixel " + std::to_string(mine.samplesPerPixel));
        if (views[i].header.accumulated > views[lead].header.accumulated) lead = i;
    }
    // every tile of the handle's shard exactly once
    const std::span<const uint32_t>                       tiles = r.shardTiles();
    const uint32_t                                        n = static_cast<uint32_t>(tiles.size());
    std::map<uint32_t, std::pair<uint32_t, uint32_t>>     where; // tile -> (blob, its index there)
    uint32_t                                              frameMost = 0, frameLeast = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < count; ++i)
        for (uint32_t k = 0; k < views[i].header.numTiles; ++k)
        {
            const uint32_t tile = views[i].tileId(k);
            frameMost = std::max(frameMost, views[i].tileSamples(k)), frameLeast = std::min(frameLeast, views[i].tileSamples(k));
            if (!std::binary_search(tiles.begin(), tiles.end(), tile)) continue; // (not the handle's: ignored)
            if (!where.emplace(tile, std::make_pair(i, k)).second) refuse("tile " + std::to_string(tile) + " of the handle's shard appears twice among the blobs");
        }
    for (const uint32_t tile : tiles)
        if (where.find(tile) == where.end()) refuse("tile " + std::to_string(tile) + " of the handle's shard is missing from the blobs");

    // ---- from here the handle changes
    Renderer::CheckpointBooks next = mine;
    next.frameCount = h.frameCount;
    next.tileSamples.assign(n, 0u);
    next.accumulated = 0;
    for (uint32_t k = 0; k < n; ++k)
    {
        const auto [blob, at] = where[tiles[k]];
        next.tileSamples[k] = views[blob].tileSamples(at);
        next.accumulated = std::max(next.accumulated, next.tileSamples[k]);
    }
    const Header& books = views[lead].header;
    for (uint32_t f = 0; f < kFamilies; ++f)
    {
        // a family follows the accumulation at the distance it had where it was saved (0: on from the first sample)
        const uint32_t behind = books.accumulated - books.family[f].samples;
        next.family[f].samples = (books.family[f].restarted || next.accumulated <= behind) ? 0u : next.accumulated - behind;
    }
    if (h.frameLeadingSamples != 0u) next.frameLeadingSamples = h.frameLeadingSamples, next.frameMinTileSamples = h.frameMinTileSamples;
    else if (r.shardWorldSize() > 1u && frameMost != frameLeast && frameLeast != 0xFFFFFFFFu) next.frameLeadingSamples = frameMost, next.frameMinTileSamples = frameLeast;
    else next.frameLeadingSamples = next.frameMinTileSamples = 0u;
    if (r.shardWorldSize() == 1u) next.frameLeadingSamples = next.frameMinTileSamples = 0u; // (a whole-frame handle keeps its own counts alone)

    RF_HIP(hipSetDevice(r.deviceOrdinal()));
    r.checkpointRestart(true);
    if (n == 0u || next.accumulated == 0u)
    {
        // nothing to copy: a shard without a tile, or tiles without a sample
        next.accumulated = 0;
        for (auto& f : next.family) f.samples = 0u;
        r.checkpointAdopt(next);
        return;
    }
    const Renderer::CheckpointBooks fresh = r.checkpointBooks(); // the buffers as they are now (sized for the shard, zeroed)
    const hipStream_t               stream = static_cast<hipStream_t>(r.streamHandle());
    const uint64_t                  tileBytes = static_cast<uint64_t>(kTileTexels) * kTexelBytes, planeBytes = tileBytes * n;
    struct Pinned
    {
        void* ptr = nullptr;
        ~Pinned()
        {
            if (ptr) (void)hipHostFree(ptr);
        }
    } staging;
    RF_HIP(hipHostMalloc(&staging.ptr, planeBytes, hipHostMallocDefault));
    // the planes every blob stores (they agree on the switches and on which families are restarted -- but for a rank of a settled frame that never traced a sample: its
    // tiles hold zeros, which is what the zeroed buffers already are)
    uint32_t       ids[kMaxPlanes];
    const uint32_t numPlanes = storedPlanes(books, ids);
    const void*    planes[kMaxPlanes];
    const auto     planeIn = [](const View& v, uint32_t id) -> int {
        for (uint32_t p = 0; p < v.numPlanes; ++p)
            if (v.planeIds[p] == id) return static_cast<int>(p);
        return -1;
    };
    for (uint32_t p = 0; p < numPlanes; ++p)
    {
        void* const device = const_cast<void*>(fresh.planes[storageIndex(ids[p])]);
        if (device == nullptr) throw std::logic_error("load_checkpoint: a stored plane without a buffer");
        planes[p] = device;
        for (uint32_t k = 0; k < n; ++k)
        {
            const auto [blob, at] = where[tiles[k]];
            const int  stored = planeIn(views[blob], ids[p]);
            auto*      to = static_cast<unsigned char*>(staging.ptr) + tileBytes * k;
            if (stored < 0) std::memset(to, 0, tileBytes);
            else std::memcpy(to, views[blob].planeTile(static_cast<uint32_t>(stored), at), tileBytes);
        }
        RF_HIP(hipMemcpyAsync(device, staging.ptr, planeBytes, hipMemcpyHostToDevice, stream));
        RF_HIP(hipStreamSynchronize(stream)); // (the staging buffer is packed again for the next plane)
    }
    // what now lies in device memory against what the blobs say of it, tile by tile
    const std::vector<uint64_t> words = digestTiles(r, planes, ids, numPlanes);
    for (uint32_t p = 0; p < numPlanes; ++p)
        for (uint32_t k = 0; k < n; ++k)
        {
            const auto [blob, at] = where[tiles[k]];
            const int  stored = planeIn(views[blob], ids[p]);
            if (stored < 0) continue;
            if (words[static_cast<size_t>(p) * n + k] != views[blob].tileDigest(static_cast<uint32_t>(stored), at))
            {
                r.checkpointRestart(false);
                throw CheckpointCorrupt("load_checkpoint: the digest of plane " + std::to_string(ids[p]) + ", tile " + std::to_string(tiles[k]) +
                                        " differs from the one the checkpoint stores: the blob is corrupt; the accumulation was restarted");
            }
        }
    r.checkpointAdopt(next);
}
} // namespace rf
