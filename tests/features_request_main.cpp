// features_request_main.cpp -- a stand-alone driver of the feature request's host arithmetic (rayfinder_amd/csrc/rf_feature_request.hpp), built by
// tests/test_features_api.py with -fsanitize=address,undefined and run as a plain executable.  It walks every channel mask, layout and element type through the
// checks the C ABI makes before it touches a device, the byte count at the largest frame the ABI admits, the store-path predicate, and checkFeatureImages over
// exact-size heap arrays of tile counts (one word past the end is the sanitizer's).  Exit 0: every expectation held.
#include "rf_feature_request.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

namespace
{
int failures = 0;
void expect(bool ok, const char* what)
{
    if (!ok) std::fprintf(stderr, "FAILED: %s\n", what), ++failures;
}
template<typename F>
bool refused(F&& f)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument&)
    {
        return true;
    }
    return false;
}
} // namespace

int main()
{
    using namespace rf;
    // every mask of the ten groups: the count is the sum of the groups', at most kFeatureMaxChannels; every other word is refused
    uint32_t checked = 0;
    for (uint32_t mask = 0; mask < 0x1000u; ++mask)
    {
        const bool valid = mask != 0u && (mask & ~kFeatureAll) == 0u;
        expect(refused([&] { checkedFeatureRequest(mask, kFeaturesChw, kFeaturesF32, 0u); }) == !valid, "mask validity");
        if (!valid) continue;
        uint32_t c = 0;
        for (uint32_t g = 0; g < kFeatureGroups; ++g) c += (mask >> g & 1u) * kFeatureGroupChannels[g];
        expect(featureChannelCount(mask) == c && c >= 1u && c <= kFeatureMaxChannels, "channel count");
        expect((featureReads(mask) != 0u) == ((mask & ~kFeatureSamples) != 0u), "only SAMPLES reads no sum");
        ++checked;
    }
    expect(checked == 1023u && featureChannelCount(kFeatureAll) == kFeatureMaxChannels, "1023 valid masks, 22 channels in all");
    for (const uint32_t bad : {0x400u, 0x80000000u, 0xFFFFFFFFu}) expect(refused([&] { checkedFeatureRequest(bad, 0u, 0u, 0u); }), "unknown channel bits");
    for (const uint32_t word : {2u, 3u, 0xFFFFFFFFu})
    {
        expect(refused([&] { checkedFeatureRequest(1u, word, 0u, 0u); }), "unknown layout");
        expect(refused([&] { checkedFeatureRequest(1u, 0u, word, 0u); }), "unknown dtype");
        expect(refused([&] { checkedFeatureRequest(1u, 0u, 0u, word); }), "reserved word");
    }
    // the byte count at the ABI's largest frame (width * height < 2^31) fits 64 bits with room to spare
    const FeatureRequest all32{kFeatureAll, kFeaturesHwc, kFeaturesF32}, all16{kFeatureAll, kFeaturesChw, kFeaturesF16};
    expect(featureBytes(46340u, 46340u, all32) == 46340ull * 46340ull * 22ull * 4ull, "bytes, f32");
    expect(featureBytes(0x7FFFFFFFu, 1u, all16) == 0x7FFFFFFFull * 22ull * 2ull, "bytes, f16");
    expect(featureBytes(3u, 5u, FeatureRequest{kFeatureDepth, kFeaturesChw, kFeaturesF16}) == 30u, "bytes, one channel");
    // the 16-byte store path: pointer and width
    expect(featureStoresVectorised(64u, 0x1000u, kFeaturesF32) && !featureStoresVectorised(64u, 0x1004u, kFeaturesF32) && !featureStoresVectorised(66u, 0x1000u, kFeaturesF32),
           "vector path, f32");
    expect(featureStoresVectorised(64u, 0x1000u, kFeaturesF16) && !featureStoresVectorised(68u, 0x1000u, kFeaturesF16) && !featureStoresVectorised(64u, 0x1002u, kFeaturesF16) &&
               featureStoresVectorised(68u, 0x1000u, kFeaturesF32),
           "vector path, f16");
    // checkFeatureImages over exact-size count arrays: 33 x 65 is 2 x 3 tiles
    int            dummy = 0;
    const uint32_t everything = kFeatureReadsS | kFeatureReadsQ | kFeatureReadsAovs | kFeatureReadsD;
    const FeatureRequest color{kFeatureColor, 0u, 0u}, variance{kFeatureVariance, 0u, 0u}, guides{kFeatureNormal | kFeatureDepth, 0u, 0u}, split{kFeatureIndirect, 0u, 0u};
    for (uint32_t zeroAt = 0; zeroAt <= 6u; ++zeroAt)
    {
        std::unique_ptr<uint32_t[]> counts(new uint32_t[6]);
        for (uint32_t t = 0; t < 6u; ++t) counts[t] = t == zeroAt ? 0u : 2u;
        expect(refused([&] { checkFeatureImages(33u, 65u, 0u, counts.get(), everything, color, &dummy); }) == (zeroAt < 6u), "a tile count of 0");
        for (uint32_t t = 0; t < 6u; ++t) counts[t] = t == zeroAt ? 1u : 2u;
        expect(!refused([&] { checkFeatureImages(33u, 65u, 0u, counts.get(), everything, color, &dummy); }), "counts of 1 serve COLOR");
        expect(refused([&] { checkFeatureImages(33u, 65u, 0u, counts.get(), everything, variance, &dummy); }) == (zeroAt < 6u), "VARIANCE needs 2 everywhere");
    }
    expect(refused([&] { checkFeatureImages(8u, 8u, 0u, nullptr, everything, color, &dummy); }), "samples == 0");
    expect(refused([&] { checkFeatureImages(8u, 8u, 1u, nullptr, everything, variance, &dummy); }) && !refused([&] { checkFeatureImages(8u, 8u, 2u, nullptr, everything, variance, &dummy); }),
           "VARIANCE with one count");
    expect(refused([&] { checkFeatureImages(0u, 8u, 4u, nullptr, everything, color, &dummy); }) && refused([&] { checkFeatureImages(8u, 0u, 4u, nullptr, everything, color, &dummy); }),
           "a zero size");
    expect(refused([&] { checkFeatureImages(65536u, 32768u, 4u, nullptr, everything, color, &dummy); }), "image too large");
    expect(refused([&] { checkFeatureImages(8u, 8u, 4u, nullptr, everything, color, nullptr); }), "no output");
    expect(refused([&] { checkFeatureImages(8u, 8u, 4u, nullptr, kFeatureReadsQ | kFeatureReadsAovs | kFeatureReadsD, color, &dummy); }), "COLOR without S");
    expect(refused([&] { checkFeatureImages(8u, 8u, 4u, nullptr, kFeatureReadsS, variance, &dummy); }), "VARIANCE without Q");
    expect(refused([&] { checkFeatureImages(8u, 8u, 4u, nullptr, kFeatureReadsS | kFeatureReadsQ | kFeatureReadsD, guides, &dummy); }), "guides without the AOVs");
    expect(refused([&] { checkFeatureImages(8u, 8u, 4u, nullptr, kFeatureReadsS, split, &dummy); }) && refused([&] { checkFeatureImages(8u, 8u, 4u, nullptr, kFeatureReadsD, split, &dummy); }),
           "INDIRECT needs S and D");
    expect(!refused([&] { checkFeatureImages(8u, 8u, 4u, nullptr, 0u, FeatureRequest{kFeatureSamples, 0u, 0u}, &dummy); }), "SAMPLES reads nothing");
    std::printf("%u masks checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
