// rf_features.hip -- the feature export: the per-pixel feature channels of a frame's sums as one CHW / HWC tensor of f32 or f16 in caller-owned device memory.  The
// arithmetic is the one include/rayfinder_amd.h writes out ("Feature export"), one IEEE f32 operation at a time in that order (-ffp-contract=off, correctly rounded
// divide and sqrt, no denormal flushing), written as prepPixel (rf_denoise.hip), estimateTile, kTileMean and kSplitMeanRows (rf_noise.hip) write theirs:
// tests/features_restatement.py reproduces it bit for bit.  No atomics: every output is one lane's fixed sequence of operations.
//   kExportFeatures<TILE_MAJOR, F16, VEC>  one 256-lane workgroup per 32 x 32 tile, in four strips of 8 rows x 32 pixels.  Per strip every lane reads one pixel of
//                   each plane the request needs in the SOURCE's order -- tile-major: entry j of tile t at plane[t * 1024 + j], consecutive lanes consecutive float4,
//                   1 KiB per wave instruction; row-major: lanes along x --, forms the pixel's channels in registers and stages them in LDS in the DESTINATION's order
//                   (about C KiB per workgroup: 256 pixels x C channels -- 25 KiB for all 22, 6 workgroups per CU; no limit up to 19); then the workgroup stores
//                   the strip along x.  VEC: 16 bytes per lane (4 f32 / 8 f16, two halves packed per dword: nothing narrower than a dword is stored); else element
//                   by element, the same values.
#include "rf_features.hpp"

#include "rf_math.hpp"
#include "rf_renderer.hpp" // TileGrid

#include <cfloat>

namespace rf
{
namespace
{
constexpr float    kEpsLum = 0.00390625f; // 2^-8 (the estimate's)
constexpr uint32_t kChwRunStride = 36;    // floats between two CHW runs of 32 in the stage (16-byte aligned)

struct FeatureArgs
{
    const float4 *  colorSum, *sumSq, *albedoCoverage, *normalDepth, *directSum;
    const uint32_t* tileSamples;
    uint32_t        samples, width, height, tilesX, channels, numChannels, hwc, reads;
};

// The channels of one pixel from its sums and its sample count, in ascending bit order, each handed to put().  `channels` is uniform over the launch.
template<typename Put>
__device__ __forceinline__ void featurePixel(uint32_t channels, uint32_t numChannels, const float4& S, const float4& Q, const float4& AC, const float4& ND, const float4& D,
                                             uint32_t count, Put&& put)
{
    if (count == 0u) // no sample: +0 in every channel
    {
        for (uint32_t c = 0; c < numChannels; ++c) put(0.0f);
        return;
    }
    const float nf = static_cast<float>(count);
    if (channels & kFeatureColor) put(S.x / nf), put(S.y / nf), put(S.z / nf); // (kTonemap's / kTileMean's division)
    if (channels & kFeatureAlbedo) put(AC.x / nf), put(AC.y / nf), put(AC.z / nf);
    if (channels & (kFeatureNormal | kFeatureDepth))
    {
        // the denoiser's guide, exactly as prepPixel forms it
        const float z = ND.w / AC.w;
        const bool  background = AC.w == 0.0f || !(z > 0.0f);
        if (channels & kFeatureNormal)
        {
            Vec3 n = splat(0.0f);
            if (!background)
            {
                const Vec3  m = vec3(ND.x / nf, ND.y / nf, ND.z / nf);
                const float d = dot(m, m);
                n = (d != 0.0f && fabsf(d) <= FLT_MAX) ? normalize(m) : splat(0.0f);
            }
            put(n.x), put(n.y), put(n.z);
        }
        if (channels & kFeatureDepth) put(background ? 0.0f : z);
    }
    if (channels & kFeatureCoverage) put(AC.w / nf);
    if (channels & kFeatureDirect) put(D.x / nf), put(D.y / nf), put(D.z / nf);
    if (channels & kFeatureIndirect) put((S.x - D.x) / nf), put((S.y - D.y) / nf), put((S.z - D.z) / nf); // (one subtraction, one division: kSplitMeanRows)
    if (channels & (kFeatureVariance | kFeatureError))
    {
        // mu and v exactly as estimateTile forms them
        const float nf1 = nf - 1.0f;
        const float s[3] = {S.x, S.y, S.z}, q[3] = {Q.x, Q.y, Q.z};
        float       mu[3], v[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
        {
            mu[ch] = s[ch] / nf;
            const float sm = s[ch] * mu[ch];
            const float d = q[ch] - sm;
            const float vv = d / nf1;
            v[ch] = vv > 0.0f ? vv : 0.0f; // (NaN: 0)
        }
        if (channels & kFeatureVariance) put(v[0] / nf), put(v[1] / nf), put(v[2] / nf); // the variance of the mean
        if (channels & kFeatureError)
        {
            const float s2 = ((v[0] + v[1]) + v[2]) / nf;
            const float l = (mu[0] + mu[1]) + mu[2];
            float       e = rf_sqrt(s2) / (l + kEpsLum);
            if (!(e <= FLT_MAX)) e = 0.0f;
            put(e);
        }
    }
    if (channels & kFeatureSamples) put(nf);
}

// f32 -> f16, one round-to-nearest-even conversion (v_cvt_f16_f32, for a pair v_cvt_pk_f16_f32, under the kernel's default rounding mode; half subnormals kept, overflow
// to inf, NaN stays NaN)
__device__ __forceinline__ uint32_t halfBits(float f) { return static_cast<uint32_t>(__builtin_bit_cast(uint16_t, static_cast<_Float16>(f))); }
__device__ __forceinline__ uint32_t halfPair(float lo, float hi) { return halfBits(lo) | (halfBits(hi) << 16); }

// one float4 of a sum plane as ONE 16-byte load (the planes are read once: non-temporal)
typedef float Float4V __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 loadSum(const float4* p)
{
    const Float4V v = __builtin_nontemporal_load(reinterpret_cast<const Float4V*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

template<bool TILE_MAJOR, bool F16, bool VEC>
__global__ __launch_bounds__(256) void kExportFeatures(FeatureArgs a, void* dst)
{
    extern __shared__ __attribute__((aligned(16))) float stage[]; // 256 pixels x C channels of one strip, in the destination's order
    const uint32_t t = threadIdx.x, tile = blockIdx.x, tileY = tile / a.tilesX, tileX = tile - tileY * a.tilesX;
    const uint32_t C = a.numChannels, x0 = tileX * kTileSize, y0 = tileY * kTileSize;
    const uint32_t count = a.tileSamples ? a.tileSamples[tile] : a.samples;
    const uint32_t inRow = a.width - x0 < kTileSize ? a.width - x0 : kTileSize; // in-frame pixels of a row of the tile
    // the strip as the destination sees it: runs of runLen contiguous elements -- CHW: run c * 8 + row holds 32 pixels of channel c; HWC: run `row` holds 32 x C
    // (in the stage a CHW run takes kChwRunStride floats: with the 4 floats of padding the lanes of a tile-major wave, 8 pixels of 8 rows, spread over the banks)
    const uint32_t runLen = a.hwc ? kTileSize * C : kTileSize, validLen = a.hwc ? inRow * C : inRow, total = 256u * C;
    const uint32_t runStride = a.hwc ? runLen : kChwRunStride;
    for (uint32_t k = 0; k < 4u; ++k)
    {
        const uint32_t ys = y0 + 8u * k; // the strip's first row
        if (ys >= a.height) break;       // (uniform over the workgroup)
        {
            const uint32_t j = k * 256u + t; // tile-major: blocks 4k .. 4k + 3, the tile's rows 8k .. 8k + 7; row-major: the same rows
            const uint32_t tx = TILE_MAJOR ? ((j >> 6) & 3u) * 8u + (j & 7u) : (j & 31u), row = TILE_MAJOR ? ((j & 63u) >> 3) : ((j >> 5) & 7u);
            const uint32_t x = x0 + tx, y = ys + row;
            if (x < a.width && y < a.height)
            {
                const size_t src = TILE_MAJOR ? static_cast<size_t>(tile) * 1024u + j : static_cast<size_t>(y) * a.width + x;
                // (whole 16-byte loads, read once: a struct load of which the arithmetic uses three members would be split into dword loads)
                const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float4 S = (a.reads & kFeatureReadsS) ? loadSum(a.colorSum + src) : none;
                const float4 Q = (a.reads & kFeatureReadsQ) ? loadSum(a.sumSq + src) : none;
                const float4 AC = (a.reads & kFeatureReadsAovs) ? loadSum(a.albedoCoverage + src) : none;
                const float4 ND = (a.reads & kFeatureReadsAovs) ? loadSum(a.normalDepth + src) : none;
                const float4 D = (a.reads & kFeatureReadsD) ? loadSum(a.directSum + src) : none;
                uint32_t       at = a.hwc ? (row * kTileSize + tx) * C : row * kChwRunStride + tx;
                const uint32_t step = a.hwc ? 1u : 8u * kChwRunStride;
                featurePixel(a.channels, C, S, Q, AC, ND, D, count, [&](float v) {
                    stage[at] = v;
                    at += step;
                });
            }
        }
        __syncthreads();
        constexpr uint32_t V = VEC ? (F16 ? 8u : 4u) : 1u; // elements per store
        for (uint32_t e0 = t * V; e0 < total; e0 += 256u * V)
        {
            const uint32_t run = e0 / runLen, e = e0 - run * runLen;
            const uint32_t c = a.hwc ? 0u : run >> 3, row = a.hwc ? run : run & 7u;
            const uint32_t y = ys + row;
            if (y >= a.height || e >= validLen) continue; // (VEC: validLen and e are multiples of V -- the width is --, so a vector lies wholly inside the frame or outside)
            const float* const staged = stage + run * runStride + e;
            const size_t       g = a.hwc ? (static_cast<size_t>(y) * a.width + x0) * C + e : (static_cast<size_t>(c) * a.height + y) * a.width + x0 + e;
            if (VEC)
            {
                const float4 lo = *reinterpret_cast<const float4*>(staged);
                if (F16)
                {
                    const float4 hi = *reinterpret_cast<const float4*>(staged + 4);
                    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(dst) + g) = make_uint4(halfPair(lo.x, lo.y), halfPair(lo.z, lo.w), halfPair(hi.x, hi.y), halfPair(hi.z, hi.w));
                }
                else
                    *reinterpret_cast<float4*>(static_cast<float*>(dst) + g) = lo;
            }
            else if (F16)
                static_cast<uint16_t*>(dst)[g] = static_cast<uint16_t>(halfBits(*staged));
            else
                static_cast<float*>(dst)[g] = *staged;
        }
        __syncthreads(); // (the next strip overwrites the stage)
    }
}

template<bool TILE_MAJOR>
auto exportKernel(bool f16, bool vec)
{
    return f16 ? (vec ? kExportFeatures<TILE_MAJOR, true, true> : kExportFeatures<TILE_MAJOR, true, false>)
               : (vec ? kExportFeatures<TILE_MAJOR, false, true> : kExportFeatures<TILE_MAJOR, false, false>);
}
} // namespace

void requireFeatureDestination(const void* dst, uint64_t bytes, uint64_t needed, int deviceOrdinal, const char* what)
{
    const std::string name(what);
    if (!dst) throw std::invalid_argument("null argument");
    if (bytes < needed)
        throw std::invalid_argument(name + ": the destination holds " + std::to_string(bytes) + " bytes, the frame's features need " + std::to_string(needed));
    requireDeviceRange(dst, needed, deviceOrdinal, what, "the destination", "the frame's features", "the sums");
}

void requireDeviceRange(const void* p, uint64_t bytes, int deviceOrdinal, const char* what, const char* noun, const char* content, const char* owner)
{
    const std::string name(what), buffer(noun);
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess)
    {
        (void)hipGetLastError(); // (the failed lookup must not show up as the next call's error)
        throw std::invalid_argument(name + ": " + buffer + " is not device memory (hipPointerGetAttributes does not know the pointer)");
    }
    if (attr.type != hipMemoryTypeDevice) throw std::invalid_argument(name + ": " + buffer + " is not device memory (host, registered or managed memory is refused)");
    if (attr.device != deviceOrdinal)
        throw std::invalid_argument(name + ": " + buffer + " lies on device " + std::to_string(attr.device) + ", " + owner + " on device " + std::to_string(deviceOrdinal));
    // the allocation the pointer lies in, where the runtime can tell: the bytes must fit behind the pointer
    hipDeviceptr_t base = nullptr;
    size_t         size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) (void)hipGetLastError();
    else if (static_cast<const char*>(p) + bytes > static_cast<const char*>(base) + size)
        throw std::invalid_argument(name + ": " + content + " do not fit into the allocation " + buffer + " points into");
}

void enqueueExportFeatures(hipStream_t stream, const FrameSums& s, const FeatureRequest& request, void* dst)
{
    const uint32_t    width = s.width, height = s.height;
    const TileGrid    grid(width, height);
    const uint32_t    C = featureChannelCount(request.channels);
    const bool        f16 = request.dtype == kFeaturesF16;
    const bool        vec = featureStoresVectorised(width, reinterpret_cast<uint64_t>(dst), request.dtype);
    const FeatureArgs args{s.colorSum, s.sumSq,        s.albedoCoverage, s.normalDepth,     s.directSum, s.tileSamples, s.samples, width, height, grid.tilesX,
                           request.channels, C, request.layout == kFeaturesHwc ? 1u : 0u, featureReads(request.channels)};
    const auto        kernel = s.tilesX != 0u ? exportKernel<true>(f16, vec) : exportKernel<false>(f16, vec);
    const uint32_t    ldsBytes = C * 8u * (args.hwc ? kTileSize : kChwRunStride) * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3(grid.count()), dim3(256), ldsBytes, stream, args, dst);
    RF_HIP(hipGetLastError());
}

void exportFeaturesImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const uint32_t* tileSamples, const float* colorSum, const float* sumSq,
                          const float* albedoCoverage, const float* normalDepth, const float* directSum, const FeatureRequest& request, void* outHost)
{
    const uint64_t bytes = featureBytes(width, height, request);
    // only the planes a selected channel reads travel (the others may be NULL)
    const uint32_t reads = featureReads(request.channels);
    const auto     read = [&](uint32_t family, const float* plane) { return reads & family ? plane : nullptr; };
    DeviceBuffer<uint8_t> out; // (before the stage: freed after it has drained its stream)
    StagedFrame           f(deviceOrdinal, width, height, samples, tileSamples, read(kFeatureReadsS, colorSum), read(kFeatureReadsQ, sumSq), read(kFeatureReadsAovs, albedoCoverage),
                            read(kFeatureReadsAovs, normalDepth), read(kFeatureReadsD, directSum));
    out.alloc(bytes);
    enqueueExportFeatures(f.stream.handle, f.sums, request, out.ptr);
    f.download(outHost, out.ptr, bytes);
    f.wait();
}
} // namespace rf
