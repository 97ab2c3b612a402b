// rf_ray_query_request.hpp -- a ray batch (include/rayfinder_amd.h, rf_renderer_cast_rays) as the host sees it: which outputs, what is refused without a device, the
// byte range of every buffer, whether two ranges overlap, and how the rays are cut into chunks of one path-state allocation.  Host only, no HIP: the C ABI's checks are
// these functions, and tests/ray_query_request_main.cpp runs them under the sanitizers without a device.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace rf
{
constexpr uint32_t kRaysClosest = 0u, kRaysAny = 1u;

// the outputs in the struct's order, as mask bits; floats (or words) per ray of each
constexpr uint32_t kCastTriangle = 0x001u, kCastT = 0x002u, kCastBary = 0x004u, kCastPosition = 0x008u, kCastGeometricNormal = 0x010u, kCastNormal = 0x020u,
                   kCastTexcoord = 0x040u, kCastAlbedo = 0x080u, kCastTexture = 0x100u, kCastVisibility = 0x200u;
constexpr uint32_t kCastOutputs = 10;
constexpr uint32_t kCastOutputWidth[kCastOutputs] = {1, 1, 2, 3, 3, 3, 2, 3, 1, 1};
constexpr const char* kCastOutputName[kCastOutputs] = {"triangle", "t", "bary", "position", "geometric_normal", "normal", "texcoord", "albedo", "texture", "visibility"};
constexpr uint32_t kCastClosestMask = 0x1FFu, kCastAnyMask = kCastVisibility;
// the outputs that read the triangle's shading record (the others come from the hit stream alone)
constexpr uint32_t kCastNeedsRecord = kCastPosition | kCastGeometricNormal | kCastNormal | kCastTexcoord | kCastAlbedo | kCastTexture;

// The batch without its types: addresses as integers, so that the arithmetic below is plain integer arithmetic
struct RayQueryRequest
{
    uint64_t origins = 0, directions = 0;
    uint32_t originStride = 3, directionStride = 3;
    uint64_t numRays = 0;
    float    tMax = 0.0f;
    uint32_t kind = kRaysClosest;
    uint32_t reserved[2] = {0u, 0u};
    uint64_t outputs[kCastOutputs] = {}; // 0: not wanted
    uint32_t mask() const
    {
        uint32_t m = 0;
        for (uint32_t i = 0; i < kCastOutputs; ++i)
            if (outputs[i] != 0u) m |= 1u << i;
        return m;
    }
};

// [begin, end) in bytes; empty when begin == end
struct ByteRange
{
    uint64_t begin = 0, end = 0;
    bool     empty() const { return begin == end; }
};

inline bool rangesOverlap(const ByteRange& a, const ByteRange& b) { return !a.empty() && !b.empty() && a.begin < b.end && b.begin < a.end; }

// count * width * 4 bytes behind `address`; std::invalid_argument where the product or the end does not fit 64 bits
inline ByteRange checkedRange(uint64_t address, uint64_t count, uint64_t width, const char* what)
{
    const uint64_t kMax = ~uint64_t{0};
    const uint64_t perItem = width * 4u; // (width is a 32-bit value: no overflow)
    if (count != 0u && perItem > kMax / count) throw std::invalid_argument(std::string("ray batch: the size of ") + what + " overflows 64 bits");
    const uint64_t bytes = count * perItem;
    if (bytes > kMax - address) throw std::invalid_argument(std::string("ray batch: ") + what + " ends past the address space");
    return ByteRange{address, address + bytes};
}

// A strided input of n rays: ray i at address + i * stride * 4, 3 floats.  The range ends behind the LAST ray's third float, not behind a full stride: the second
// half of an (N, 6) tensor has no floats behind its last row.
inline ByteRange inputRange(uint64_t address, uint64_t numRays, uint32_t stride, const char* what)
{
    if (numRays == 0u) return ByteRange{address, address};
    const ByteRange body = checkedRange(address, numRays - 1u, stride, what);
    return ByteRange{address, checkedRange(body.end, 1u, 3u, what).end};
}

inline ByteRange outputRange(const RayQueryRequest& q, uint32_t output) { return checkedRange(q.outputs[output], q.numRays, kCastOutputWidth[output], kCastOutputName[output]); }

// What is refused without a device, in the order the header lists it (the NULL batch is the C entry point's)
inline void checkRayQueryRequest(const RayQueryRequest& q)
{
    if (q.origins == 0u || q.directions == 0u) throw std::invalid_argument("ray batch: origins and directions must be given");
    if (q.originStride < 3u || q.directionStride < 3u) throw std::invalid_argument("ray batch: a stride below 3 floats");
    if (q.kind != kRaysClosest && q.kind != kRaysAny) throw std::invalid_argument("ray batch: the kind is RF_RAYS_CLOSEST or RF_RAYS_ANY");
    if (q.reserved[0] != 0u || q.reserved[1] != 0u) throw std::invalid_argument("ray batch: the reserved words must be 0");
    const uint32_t mask = q.mask();
    if (mask == 0u) throw std::invalid_argument("ray batch: no output is given");
    if (q.kind == kRaysAny && (mask & ~kCastAnyMask) != 0u) throw std::invalid_argument("ray batch: RF_RAYS_ANY writes visibility only");
    if (q.kind == kRaysClosest && (mask & ~kCastClosestMask) != 0u) throw std::invalid_argument("ray batch: visibility is RF_RAYS_ANY's output");
    if (std::isnan(q.tMax)) throw std::invalid_argument("ray batch: t_max is NaN");
}

// Every buffer's range, then: no output overlaps another output or an input (the inputs may overlap each other: they are only read)
inline void checkRayQueryOverlaps(const RayQueryRequest& q)
{
    const ByteRange in[2] = {inputRange(q.origins, q.numRays, q.originStride, "origins"), inputRange(q.directions, q.numRays, q.directionStride, "directions")};
    ByteRange       out[kCastOutputs];
    for (uint32_t i = 0; i < kCastOutputs; ++i) out[i] = q.outputs[i] != 0u ? outputRange(q, i) : ByteRange{};
    for (uint32_t i = 0; i < kCastOutputs; ++i)
    {
        for (uint32_t k = 0; k < 2; ++k)
            if (rangesOverlap(out[i], in[k])) throw std::invalid_argument(std::string("ray batch: ") + kCastOutputName[i] + " overlaps " + (k == 0 ? "origins" : "directions"));
        for (uint32_t j = i + 1; j < kCastOutputs; ++j)
            if (rangesOverlap(out[i], out[j])) throw std::invalid_argument(std::string("ray batch: ") + kCastOutputName[i] + " overlaps " + kCastOutputName[j]);
    }
}

// The chunk plan: chunk c covers rays [c * C, min((c + 1) * C, N)).  C = min(the configured path depth, what fits the device now, the option cast_chunk where it is
// not 0, 2^32 - 1: the queues hold 32-bit positions), and never 0.
struct ChunkPlan
{
    uint64_t numRays = 0, chunk = 1;
    uint64_t count() const { return (numRays + chunk - 1u) / chunk; } // (numRays + chunk - 1 < 2^64: chunk < 2^32, and a numRays near 2^64 is refused by its ranges)
    uint64_t first(uint64_t c) const { return c * chunk; }
    uint64_t size(uint64_t c) const
    {
        const uint64_t begin = first(c);
        return begin >= numRays ? 0u : (numRays - begin < chunk ? numRays - begin : chunk);
    }
    // the path state one call allocates: the largest chunk
    uint64_t depth() const { return numRays < chunk ? numRays : chunk; }
};

inline ChunkPlan planChunks(uint64_t numRays, uint64_t configuredDepth, uint64_t fits, uint64_t castChunk)
{
    uint64_t c = configuredDepth < fits ? configuredDepth : fits;
    if (castChunk != 0u && castChunk < c) c = castChunk;
    if (c > 0xFFFFFFFFull) c = 0xFFFFFFFFull;
    if (c == 0u) c = 1u;
    return ChunkPlan{numRays, c};
}
} // namespace rf
