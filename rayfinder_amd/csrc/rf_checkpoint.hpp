// rf_checkpoint.hpp -- the checkpoint blob (the byte layout: INTEGRATION.md 3) and the state digest's host side (the definition: include/rayfinder_amd.h).
// Host only: rf_checkpoint.cpp parses and sizes blobs without a device and without the HIP runtime; rf_checkpoint.hip owns the digest kernel and the copies.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace rf
{
class Renderer;

namespace ckpt
{
constexpr char     kMagic[8] = {'R', 'F', 'C', 'K', 'P', 'T', '1', '\0'};
constexpr uint32_t kVersion = 1, kHeaderBytes = 288, kFamilies = 5, kMaxBucketPlanes = 15, kMaxPlanes = 5 + kMaxBucketPlanes;
constexpr uint32_t kTileTexels = 1024, kTexelBytes = 16, kMaxFrameEdge = 1u << 16;
enum : uint32_t { kFamilyImage = 0, kFamilyAovs = 1, kFamilyMoments = 2, kFamilyDirect = 3, kFamilyBuckets = 4 };
// the digest's plane ids: the gather's numbering
enum : uint32_t { kPlaneS = 0, kPlaneAC = 1, kPlaneND = 2, kPlaneQ = 3, kPlaneD = 5, kPlaneBucket0 = 16, kCountsId = 0xC0 };

constexpr uint64_t mix64(uint64_t z)
{
    z ^= z >> 30, z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27, z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t countTerm(uint32_t tile, uint32_t samples) { return mix64(mix64((uint64_t{kCountsId} << 32) | tile) ^ uint64_t{samples}); }

struct Family
{
    uint32_t samples, restarted;
};
// The fixed header, field for field as it lies in the blob (little-endian; the library runs on little-endian hosts only)
struct Header
{
    char     magic[8];
    uint32_t version, headerBytes;
    uint64_t totalBytes;
    uint32_t width, height, numTiles, frameCount, accumulated, frameLeadingSamples, frameMinTileSamples;
    uint32_t aovFlags, moments, directWord, bucketsWord;
    Family   family[kFamilies]; // S, the AOVs, Q, D, the buckets
    uint32_t camera[19], sky[6], numBounces; // the render-parameter guard (with width and height above)
    uint32_t pad0;
    uint64_t sceneCounts[4]; // the scene guard: BVH nodes, triangles, textures, texels ...
    uint32_t rootBounds[6];  // ... and the root node's box, as bit patterns
    uint32_t reserved[4];
};
static_assert(sizeof(Header) == kHeaderBytes && offsetof(Header, sceneCounts) == 216);

// A parsed blob: the header by value, the arrays as offsets into the caller's memory (unaligned: read through the accessors)
struct View
{
    Header               header{};
    const unsigned char* base = nullptr;
    uint64_t             bytes = 0;
    uint32_t             numPlanes = 0;          // stored planes
    uint32_t             planeIds[kMaxPlanes]{}; // their digest ids, in blob order
    uint64_t             tileIdsAt = 0, tileSamplesAt = 0, tileDigestsAt = 0, planesAt = 0;

    uint32_t             tileId(uint32_t k) const;
    uint32_t             tileSamples(uint32_t k) const;
    uint64_t             tileDigest(uint32_t plane, uint32_t k) const;
    const unsigned char* planeTile(uint32_t plane, uint32_t k) const { return base + planesAt + (static_cast<uint64_t>(plane) * header.numTiles + k) * kTileTexels * kTexelBytes; }
};

// the stored planes of a header's switch words and family books, in blob order (-> their number); std::invalid_argument for a word the setters would refuse
uint32_t storedPlanes(const Header& h, uint32_t (&ids)[kMaxPlanes]);
// the blob's size for a header whose switches, families and tile count are filled in
uint64_t blobBytes(const Header& h);
// Every length and count against `bytes`, before any array is touched: std::invalid_argument naming the cause
View parse(const void* blob, uint64_t bytes);
// do two blobs of one load agree on everything but their tile lists (and, in a frame settled by rf_comm_render_adaptive, the ranks' own leading counts)?
void requireSameFrame(const View& a, const View& b);
} // namespace ckpt

// The state digest (rf_renderer_state_digest) of a handle
struct StateDigest
{
    uint64_t plane[ckpt::kMaxPlanes]{}; // S, AC, ND, Q, D, bucket 0 .. 14 (off or absent: 0)
    uint64_t counts = 0;
    uint32_t familyOn[ckpt::kFamilies]{}, familySamples[ckpt::kFamilies]{};
    uint32_t frameCount = 0, accumulated = 0, numTiles = 0;
    uint32_t aovFlags = 0, moments = 0, directWord = 0, bucketsWord = 0;
    float    kernelMs = 0.0f; // kDigestTiles' own time in this call, between two events on the handle's stream (no tile: 0)
};
StateDigest stateDigest(Renderer& r);
// rf_renderer_save_checkpoint: dst == nullptr: the size only
void saveCheckpoint(Renderer& r, void* dst, uint64_t* bytes);
// rf_renderer_load_checkpoint: std::invalid_argument (nothing touched) or CheckpointCorrupt (the handle restarted, its frame counter kept)
struct CheckpointCorrupt : std::runtime_error
{
    using std::runtime_error::runtime_error;
};
void loadCheckpoint(Renderer& r, const void* const* blobs, const uint64_t* sizes, uint32_t count);
} // namespace rf
