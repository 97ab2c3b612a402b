// rf_feature_request.hpp -- a feature request (include/rayfinder_amd.h, "Feature export") as the host sees it: which channels, how many, which sums they read, how many
// bytes the frame needs and whether the 16-byte store path applies.  Host only, no HIP: the C ABI's checks are these functions, and tests/features_request_main.cpp
// runs them under the sanitizers without a device.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>

namespace rf
{
// channel bits, in output order (ascending bit order), and each group's channel count
constexpr uint32_t kFeatureColor = 0x001u, kFeatureAlbedo = 0x002u, kFeatureNormal = 0x004u, kFeatureDepth = 0x008u, kFeatureCoverage = 0x010u, kFeatureDirect = 0x020u,
                   kFeatureIndirect = 0x040u, kFeatureVariance = 0x080u, kFeatureError = 0x100u, kFeatureSamples = 0x200u, kFeatureAll = 0x3FFu;
constexpr uint32_t kFeatureGroups = 10;
constexpr uint32_t kFeatureGroupChannels[kFeatureGroups] = {3, 3, 3, 1, 1, 3, 3, 3, 1, 1};
constexpr uint32_t kFeatureMaxChannels = 22;
constexpr uint32_t kFeaturesChw = 0u, kFeaturesHwc = 1u;
constexpr uint32_t kFeaturesF32 = 0u, kFeaturesF16 = 1u;

// the sums a channel mask reads, as a mask of families
constexpr uint32_t kFeatureReadsS = 1u, kFeatureReadsQ = 2u, kFeatureReadsAovs = 4u, kFeatureReadsD = 8u;

struct FeatureRequest
{
    uint32_t channels = 0, layout = kFeaturesChw, dtype = kFeaturesF32;
};

inline uint32_t featureChannelCount(uint32_t channels)
{
    uint32_t c = 0;
    for (uint32_t g = 0; g < kFeatureGroups; ++g)
        if (channels & (1u << g)) c += kFeatureGroupChannels[g];
    return c;
}

inline uint32_t featureReads(uint32_t channels)
{
    uint32_t reads = 0;
    if (channels & (kFeatureColor | kFeatureIndirect | kFeatureVariance | kFeatureError)) reads |= kFeatureReadsS;
    if (channels & (kFeatureVariance | kFeatureError)) reads |= kFeatureReadsQ;
    if (channels & (kFeatureAlbedo | kFeatureNormal | kFeatureDepth | kFeatureCoverage)) reads |= kFeatureReadsAovs;
    if (channels & (kFeatureDirect | kFeatureIndirect)) reads |= kFeatureReadsD;
    return reads;
}

// VARIANCE / ERROR divide by Nf - 1: every count they see must be >= 2
inline bool featureNeedsTwoSamples(uint32_t channels) { return (channels & (kFeatureVariance | kFeatureError)) != 0u; }

inline uint32_t featureElementBytes(uint32_t dtype) { return dtype == kFeaturesF16 ? 2u : 4u; }

// std::invalid_argument for an empty mask, unknown channel, layout or dtype bits, or a reserved word that is not 0
inline FeatureRequest checkedFeatureRequest(uint32_t channels, uint32_t layout, uint32_t dtype, uint32_t reserved)
{
    if (channels == 0u) throw std::invalid_argument("feature request: the channel mask is empty");
    if (channels & ~kFeatureAll) throw std::invalid_argument("feature request: unknown channel bits (the mask is a combination of RF_FEATURE_*)");
    if (layout != kFeaturesChw && layout != kFeaturesHwc) throw std::invalid_argument("feature request: the layout is RF_FEATURES_CHW or RF_FEATURES_HWC");
    if (dtype != kFeaturesF32 && dtype != kFeaturesF16) throw std::invalid_argument("feature request: the element type is RF_FEATURES_F32 or RF_FEATURES_F16");
    if (reserved != 0u) throw std::invalid_argument("feature request: the reserved word must be 0");
    return FeatureRequest{channels, layout, dtype};
}

// bytes of the frame's features: width * height * C elements (the callers have checked width * height < 2^31: with C <= 22 and 4 bytes at most the product is below 2^38)
inline uint64_t featureBytes(uint32_t width, uint32_t height, const FeatureRequest& req)
{
    return static_cast<uint64_t>(width) * height * featureChannelCount(req.channels) * featureElementBytes(req.dtype);
}

// The 16-byte store path: every row start of the destination is 16-byte aligned -- the pointer is, and the width is a multiple of the elements in 16 bytes (4 f32,
// 8 f16).  Otherwise the kernel stores element by element.
inline bool featureStoresVectorised(uint32_t width, uint64_t dstAddress, uint32_t dtype)
{
    const uint32_t perVector = 16u / featureElementBytes(dtype);
    return (dstAddress & 15u) == 0u && width % perVector == 0u;
}

// What rf_export_features_images refuses before any device call.  haveMask: bit kFeatureReads* is set when that family's input pointer (S, Q, both AOV sums, D) was given.
inline void checkFeatureImages(uint32_t width, uint32_t height, uint32_t samples, const uint32_t* tileSamples, uint32_t haveMask, const FeatureRequest& req, const void* out)
{
    if (!out) throw std::invalid_argument("null argument");
    if (width == 0u || height == 0u) throw std::invalid_argument("image size must be non-zero");
    if (static_cast<uint64_t>(width) * height >= (1ull << 31)) throw std::invalid_argument("image too large");
    const uint32_t reads = featureReads(req.channels);
    if (reads & ~haveMask) throw std::invalid_argument("null argument: a selected channel reads a sum that was not given");
    const uint32_t least = featureNeedsTwoSamples(req.channels) ? 2u : 1u;
    const char*    what = least == 2u ? "RF_FEATURE_VARIANCE / RF_FEATURE_ERROR need at least 2 samples in every count" : "the sample count of every tile must be > 0";
    if (tileSamples)
    {
        const uint64_t tiles = static_cast<uint64_t>((width + 31u) / 32u) * ((height + 31u) / 32u);
        for (uint64_t t = 0; t < tiles; ++t)
            if (tileSamples[t] < least) throw std::invalid_argument(what);
    }
    else if (samples < least)
        throw std::invalid_argument(least == 2u ? what : "sample count must be > 0");
}
} // namespace rf
