// rf_checkpoint.cpp -- the checkpoint blob's parser: every length and count of a blob is checked against its size here, on the host, before anything copies from it.
// No HIP dependency: rf_checkpoint_info works without a device, and tests/checkpoint_parse_main.cpp links this file alone.
#include "rf_checkpoint.hpp"

#include <cstring>

namespace rf::ckpt
{
namespace
{
[[noreturn]] void refuse(const std::string& what) { throw std::invalid_argument("checkpoint: " + what); }

uint32_t gridTiles(uint32_t width, uint32_t height) { return ((width + 31u) / 32u) * ((height + 31u) / 32u); }

template<typename T>
T readAt(const unsigned char* base, uint64_t at)
{
    T v;
    std::memcpy(&v, base + at, sizeof v);
    return v;
}
} // namespace

uint32_t View::tileId(uint32_t k) const { return readAt<uint32_t>(base, tileIdsAt + 4ull * k); }
uint32_t View::tileSamples(uint32_t k) const { return readAt<uint32_t>(base, tileSamplesAt + 4ull * k); }
uint64_t View::tileDigest(uint32_t plane, uint32_t k) const { return readAt<uint64_t>(base, tileDigestsAt + 8ull * (static_cast<uint64_t>(plane) * header.numTiles + k)); }

uint32_t storedPlanes(const Header& h, uint32_t (&ids)[kMaxPlanes])
{
    if (h.aovFlags != 0u && h.aovFlags != 1u && h.aovFlags != 0x101u) refuse("the AOV flags word is none the library sets");
    if (h.moments > 1u) refuse("the moments word is neither 0 nor 1");
    if (h.directWord != 0u && h.directWord != 1u && h.directWord != 0x101u) refuse("the direct word is none the library sets");
    const uint32_t K = h.bucketsWord & 0xFFu;
    const bool     tileCounts = (h.bucketsWord & 0x100u) != 0u, shardTileCounts = (h.bucketsWord & 0x400u) != 0u;
    if ((h.bucketsWord & ~0x5FFu) != 0u || (K == 0u && (tileCounts || shardTileCounts)) || (K != 0u && (K % 2u == 0u || K < 3u || K > kMaxBucketPlanes)) || (shardTileCounts && !tileCounts))
        refuse("the buckets word is none the library sets");
    const bool on[kFamilies] = {true, (h.aovFlags & 1u) != 0u, h.moments != 0u, (h.directWord & 1u) != 0u, K != 0u};
    for (uint32_t f = 0; f < kFamilies; ++f)
    {
        const Family& fam = h.family[f];
        if (fam.restarted > 1u) refuse("a family's restarted word is neither 0 nor 1");
        if ((fam.restarted != 0u) != (fam.samples == 0u)) refuse("a family is restarted exactly when it holds no sample");
        if (!on[f] && fam.restarted == 0u) refuse("a family that is off holds samples");
        if (fam.samples > h.accumulated) refuse("a family holds more samples than the accumulation");
    }
    if (h.family[kFamilyImage].samples != h.accumulated) refuse("the accumulation's sample count differs from the accumulated count");
    uint32_t n = 0;
    if (!h.family[kFamilyImage].restarted) ids[n++] = kPlaneS;
    if (on[kFamilyAovs] && !h.family[kFamilyAovs].restarted) ids[n++] = kPlaneAC, ids[n++] = kPlaneND;
    if (on[kFamilyMoments] && !h.family[kFamilyMoments].restarted) ids[n++] = kPlaneQ;
    if (on[kFamilyDirect] && !h.family[kFamilyDirect].restarted) ids[n++] = kPlaneD;
    if (on[kFamilyBuckets] && !h.family[kFamilyBuckets].restarted)
        for (uint32_t b = 0; b < K; ++b) ids[n++] = kPlaneBucket0 + b;
    return n;
}

uint64_t blobBytes(const Header& h)
{
    uint32_t       ids[kMaxPlanes];
    const uint64_t planes = storedPlanes(h, ids), n = h.numTiles;
    // (n <= 2^22 tiles and <= 20 planes: far inside 64 bits)
    return kHeaderBytes + n * 8u + planes * n * 8u + planes * n * kTileTexels * kTexelBytes;
}

View parse(const void* blob, uint64_t bytes)
{
    if (blob == nullptr) refuse("null blob");
    if (bytes < sizeof kMagic) refuse("truncated: " + std::to_string(bytes) + " bytes hold no magic");
    View v;
    v.base = static_cast<const unsigned char*>(blob);
    v.bytes = bytes;
    if (std::memcmp(v.base, kMagic, sizeof kMagic) != 0) refuse("bad magic (not a rayfinder checkpoint)");
    if (bytes < kHeaderBytes) refuse("truncated: " + std::to_string(bytes) + " bytes are shorter than the " + std::to_string(kHeaderBytes) + "-byte header");
    std::memcpy(&v.header, v.base, kHeaderBytes);
    const Header& h = v.header;
    if (h.version != kVersion) refuse("unsupported version " + std::to_string(h.version) + " (this library reads version " + std::to_string(kVersion) + ")");
    if (h.headerBytes != kHeaderBytes) refuse("the header length " + std::to_string(h.headerBytes) + " is not version 1's " + std::to_string(kHeaderBytes));
    if (h.totalBytes != bytes) refuse("the blob says " + std::to_string(h.totalBytes) + " bytes and " + std::to_string(bytes) + " were given (truncated or padded)");
    if (h.width == 0u || h.height == 0u || h.width > kMaxFrameEdge || h.height > kMaxFrameEdge) refuse("frame size out of range");
    if (h.numTiles > gridTiles(h.width, h.height)) refuse("more tiles than the frame's grid holds");
    v.numPlanes = storedPlanes(h, v.planeIds);
    const uint64_t want = blobBytes(h);
    if (want != bytes)
        refuse("the tile count and the stored planes need " + std::to_string(want) + " bytes and the blob holds " + std::to_string(bytes) + " (tile count inconsistent with length)");
    if (h.frameLeadingSamples < h.frameMinTileSamples) refuse("the frame's leading count is below its smallest");
    if (h.frameLeadingSamples != 0u && h.accumulated > h.frameLeadingSamples) refuse("the accumulated count is above the frame's leading count");
    v.tileIdsAt = kHeaderBytes;
    v.tileSamplesAt = v.tileIdsAt + 4ull * h.numTiles;
    v.tileDigestsAt = v.tileSamplesAt + 4ull * h.numTiles;
    v.planesAt = v.tileDigestsAt + 8ull * v.numPlanes * h.numTiles;
    const uint32_t frameTiles = gridTiles(h.width, h.height), top = h.frameLeadingSamples != 0u ? h.frameLeadingSamples : h.accumulated;
    for (uint32_t k = 0; k < h.numTiles; ++k)
    {
        if (v.tileId(k) >= frameTiles) refuse("a tile id lies outside the frame's grid");
        if (k != 0u && v.tileId(k) <= v.tileId(k - 1)) refuse("the tile ids are not ascending");
        if (v.tileSamples(k) > top) refuse("a tile holds more samples than the leading count");
        if (v.tileSamples(k) > h.accumulated) refuse("a tile holds more samples than the accumulated count");
    }
    return v;
}

void requireSameFrame(const View& a, const View& b)
{
    const Header &x = a.header, &y = b.header;
    if (x.width != y.width || x.height != y.height) refuse("the blobs are of different frame sizes");
    if (x.frameCount != y.frameCount) refuse("the blobs were saved at different frame counters");
    if (x.aovFlags != y.aovFlags || x.moments != y.moments || x.directWord != y.directWord || x.bucketsWord != y.bucketsWord) refuse("the blobs' switch words differ");
    if (std::memcmp(x.camera, y.camera, sizeof x.camera) != 0 || std::memcmp(x.sky, y.sky, sizeof x.sky) != 0 || x.numBounces != y.numBounces) refuse("the blobs' render parameters differ");
    if (std::memcmp(x.sceneCounts, y.sceneCounts, sizeof x.sceneCounts) != 0 || std::memcmp(x.rootBounds, y.rootBounds, sizeof x.rootBounds) != 0) refuse("the blobs are of different scenes");
    if (x.frameLeadingSamples != y.frameLeadingSamples || x.frameMinTileSamples != y.frameMinTileSamples) refuse("the blobs' frame-level tile counts differ");
    // The accumulated counts may differ: a checkpoint is keyed by tile, and the shards of one frame keep their own leading counts -- after rf_comm_render_adaptive, or
    // after each ran rf_renderer_render_adaptive by itself.  What must agree is how far every family lies behind its blob's accumulation (0: on from the first sample).
    for (uint32_t f = 0; f < kFamilies; ++f)
    {
        const bool xRestarted = x.family[f].restarted != 0u, yRestarted = y.family[f].restarted != 0u;
        // (a shard without a sample of its own: nothing to compare)
        if (x.accumulated == 0u || y.accumulated == 0u) continue;
        if (xRestarted != yRestarted) refuse("a family holds samples in one blob and none in another");
        if (!xRestarted && (x.accumulated - x.family[f].samples) != (y.accumulated - y.family[f].samples)) refuse("the blobs' sample counts per family differ");
    }
}
} // namespace rf::ckpt
