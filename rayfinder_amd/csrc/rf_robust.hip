// rf_robust.hip -- the firefly-robust mean of an accumulation: a median-of-means over the K bucket sums (rf_sums.hip) whose trim count follows the Gini coefficient of
// the buckets' levels (after Buisine et al. 2021, "Firefly removal in Monte Carlo rendering with adaptive Median of meaNs").  The arithmetic is the one
// include/rayfinder_amd.h writes out ("Bucket sums and the robust mean"), one IEEE f32 operation at a time in that order (-ffp-contract=off, correctly rounded
// divide, no denormal flushing): tests/robust_restatement.py reproduces it bit for bit.  No atomics: every output is one lane's fixed sequence of operations.
//   kRobustMean<K>       one lane per pixel; K is a compile-time constant, so the K bucket means and keys live in registers and the sort is a fixed network
//   kRobustMeanTiles<K>  the same with the sample count of the pixel's 32x32 tile (a frame of rf_renderer_render_adaptive, rf_robust_mean_tiles)
//   kRobustMeanShard<K>  a tile shard's own pixels in place, {M.rgb, float(c)} per pixel: what the frame gather carries as plane 4 (RF_GATHER_ROBUST_MEAN)
//   kRobustMeanShardTiles<K>  the same with one count per slot of the shard (a frame of rf_comm_render_adaptive with RF_BUCKETS_SHARD_TILE_COUNTS)
// The display image is the existing kTonemap over the mean with accumulatedSamples = 1.
#include "rf_robust.hpp"

#include "rf_kernels.hpp"
#include "rf_math.hpp"

#include <cfloat>

namespace rf
{
namespace
{
// index of pixel (x, y) in a compact tile-major buffer that holds every tile of the frame in tile order (localPixelToXY's layout)
__device__ __forceinline__ uint32_t tileMajorIndex(uint32_t x, uint32_t y, uint32_t tilesX)
{
    const uint32_t tile = (y >> 5) * tilesX + (x >> 5);
    const uint32_t block = ((y & 31u) >> 3) * 4u + ((x & 31u) >> 3);
    return tile * 1024u + block * 64u + (y & 7u) * 8u + (x & 7u);
}

// The body every kernel shares: one lane's pixel i = (x, y) over its sample count >= K -- samplesAll (kRobustMean: one count for the frame) or, TILES, the count of the
// pixel's tile, tileSamples[(y / 32) frameTilesX + (x / 32)] (kRobustMeanTiles); nothing else differs.  SHARD (kRobustMeanShard): pixel i of a shard-compact tile-major
// buffer of `width` pixels, read and written in place -- no coordinates, no tile table --, the count samplesAll, and the output {M.rgb, float(c)} in `mean` alone;
// SHARD and TILES (kRobustMeanShardTiles): the count of the pixel's slot, tileSamples[i / 1024] -- one count per 256-lane workgroup, so it stays a scalar
template<uint32_t K, bool TILES, bool SHARD = false>
__device__ __forceinline__ void robustPixel(const float4* planes, size_t planeStride, uint32_t width, uint32_t height, uint32_t tilesX, uint32_t samplesAll,
                                            const uint32_t* tileSamples, uint32_t frameTilesX, float4* mean, uint8_t* trim)
{
    static_assert(K % 2u == 1u && K >= 3u && K <= 15u, "K odd, 3 .. 15");
    constexpr uint32_t HALF = (K - 1u) / 2u;
    const uint32_t     i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (SHARD ? width : width * height)) return;
    const uint32_t y = SHARD ? 0u : i / width, x = i - y * width;
    const uint32_t src = !SHARD && tilesX ? tileMajorIndex(x, y, tilesX) : i;
    // (SHARD: i >> 10 from the workgroup's first pixel -- 256 lanes never straddle a slot of 1 024 --, which the compiler can see is uniform)
    const uint32_t samples = TILES ? tileSamples[SHARD ? (blockIdx.x * blockDim.x) >> 10 : (y >> 5) * frameTilesX + (x >> 5)] : samplesAll;
    const uint32_t each = samples / K, more = samples - each * K; // buckets 0 .. more - 1 hold one sample more
    float          mr[K], mg[K], mb[K], key[K];
#pragma unroll
    for (uint32_t b = 0; b < K; ++b)
    {
        const float  nf = static_cast<float>(each + (b < more ? 1u : 0u));
        const float4 B = planes[b * planeStride + src];
        mr[b] = B.x / nf, mg[b] = B.y / nf, mb[b] = B.z / nf;
        const float l = (mr[b] + mg[b]) + mb[b];
        key[b] = l <= FLT_MAX ? l : __builtin_inff(); // (NaN: +inf)
    }
    // ascending by key, ties by bucket index: an odd-even transposition network (K rounds) that exchanges two NEIGHBOURS only when the left key is strictly greater,
    // so equal keys never pass each other
#pragma unroll
    for (uint32_t round = 0; round < K; ++round)
#pragma unroll
        for (uint32_t j = round & 1u; j + 1u < K; j += 2u)
        {
            const bool  swap = key[j] > key[j + 1u];
            const float k0 = key[j], k1 = key[j + 1u], r0 = mr[j], r1 = mr[j + 1u], g0 = mg[j], g1 = mg[j + 1u], b0 = mb[j], b1 = mb[j + 1u];
            key[j] = swap ? k1 : k0, key[j + 1u] = swap ? k0 : k1;
            mr[j] = swap ? r1 : r0, mr[j + 1u] = swap ? r0 : r1;
            mg[j] = swap ? g1 : g0, mg[j + 1u] = swap ? g0 : g1;
            mb[j] = swap ? b1 : b0, mb[j + 1u] = swap ? b0 : b1;
        }
    float num = 0.0f, sum = 0.0f;
#pragma unroll
    for (uint32_t r = 0; r < K; ++r)
    {
        num += static_cast<float>(2 * static_cast<int>(r) - static_cast<int>(K - 1u)) * key[r];
        sum += key[r];
    }
    const float    den = static_cast<float>(K) * sum;
    const float    G = den > 0.0f ? num / den : 0.0f;
    const float    t = G * (static_cast<float>(K) * 0.5f);
    // min(uint(floor(t)), HALF), the comparison taken in f32 first (a huge t never reaches the conversion); NaN: every comparison false, the median
    const uint32_t c = t >= 0.0f ? (t >= static_cast<float>(HALF) ? HALF : static_cast<uint32_t>(floorf(t))) : HALF;
    float          sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (uint32_t r = 0; r < K; ++r)
    {
        const bool kept = r >= c && r + c <= K - 1u;
        sr = kept ? sr + mr[r] : sr, sg = kept ? sg + mg[r] : sg, sb = kept ? sb + mb[r] : sb;
    }
    const float nk = static_cast<float>(K - 2u * c);
    mean[i] = make_float4(sr / nk, sg / nk, sb / nk, SHARD ? static_cast<float>(c) : 1.0f);
    if (!SHARD) trim[i] = static_cast<uint8_t>(c);
}

template<uint32_t K>
__global__ __launch_bounds__(256) void kRobustMean(const float4* planes, size_t planeStride, uint32_t width, uint32_t height, uint32_t tilesX, uint32_t samples, float4* mean,
                                                   uint8_t* trim)
{
    robustPixel<K, false>(planes, planeStride, width, height, tilesX, samples, nullptr, 0u, mean, trim);
}

// The same with one count per 32x32 tile: tileSamples[tile_y * frameTilesX + tile_x] >= K, frameTilesX = ceil(width / 32) (the estimate's tile numbering; the planes
// may still be row-major, tilesX == 0)
template<uint32_t K>
__global__ __launch_bounds__(256) void kRobustMeanTiles(const float4* planes, size_t planeStride, uint32_t width, uint32_t height, uint32_t tilesX, const uint32_t* tileSamples,
                                                        uint32_t frameTilesX, float4* mean, uint8_t* trim)
{
    robustPixel<K, true>(planes, planeStride, width, height, tilesX, 0u, tileSamples, frameTilesX, mean, trim);
}

using RobustKernel = void (*)(const float4*, size_t, uint32_t, uint32_t, uint32_t, uint32_t, float4*, uint8_t*);
RobustKernel robustKernel(uint32_t K)
{
    switch (K)
    {
    case 3: return kRobustMean<3>;
    case 5: return kRobustMean<5>;
    case 7: return kRobustMean<7>;
    case 9: return kRobustMean<9>;
    case 11: return kRobustMean<11>;
    case 13: return kRobustMean<13>;
    case 15: return kRobustMean<15>;
    default: throw std::logic_error("robustKernel: no such kernel is compiled");
    }
}
using RobustTilesKernel = void (*)(const float4*, size_t, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t, float4*, uint8_t*);
RobustTilesKernel robustTilesKernel(uint32_t K)
{
    switch (K)
    {
    case 3: return kRobustMeanTiles<3>;
    case 5: return kRobustMeanTiles<5>;
    case 7: return kRobustMeanTiles<7>;
    case 9: return kRobustMeanTiles<9>;
    case 11: return kRobustMeanTiles<11>;
    case 13: return kRobustMeanTiles<13>;
    case 15: return kRobustMeanTiles<15>;
    default: throw std::logic_error("robustTilesKernel: no such kernel is compiled");
    }
}

// A tile shard's own combine, ahead of the frame gather (RF_GATHER_ROBUST_MEAN): one lane per pixel of the shard-compact tile-major planes, the output in the same
// place of a buffer laid out the same way -- source index = destination index = i, no coordinates, no tile table.  out[i] = {M.rgb, float(c)}: c <= 7 is exact in an
// f32 and M.a is the constant 1, so the trim count travels in .w and the root's un-tile splits it off again.  The padding pixels of ragged tiles hold zero sums: M = 0,
// c = 0 (0 / n = 0, den = 0 so G = 0), and the un-tile never reads them.
template<uint32_t K>
__global__ __launch_bounds__(256) void kRobustMeanShard(const float4* __restrict__ planes, size_t planeStride, uint32_t pixels, uint32_t samples, float4* __restrict__ out)
{
    // SHARD: `width` is the pixel count; height, tilesX, tileSamples, frameTilesX and trim are not used
    robustPixel<K, false, true>(planes, planeStride, /* width = */ pixels, /* height */ 1u, /* tilesX */ 0u, samples, /* tileSamples */ nullptr, /* frameTilesX */ 0u, out, /* trim */ nullptr);
}

// The same with one count per slot of the shard: slotCounts[i >> 10] >= K, the shard's per-tile counts in slot order (Renderer::shardTileSamplesDevice: what the
// gather sends as counts).  A tile shard after rf_comm_render_adaptive, its own tiles at different counts or all at one count below the frame's leading count.
template<uint32_t K>
__global__ __launch_bounds__(256) void kRobustMeanShardTiles(const float4* __restrict__ planes, size_t planeStride, uint32_t pixels, const uint32_t* __restrict__ slotCounts,
                                                             float4* __restrict__ out)
{
    robustPixel<K, true, true>(planes, planeStride, /* width = */ pixels, /* height */ 1u, /* tilesX */ 0u, /* samplesAll */ 0u, slotCounts, /* frameTilesX */ 0u, out, /* trim */ nullptr);
}

using RobustShardKernel = void (*)(const float4*, size_t, uint32_t, uint32_t, float4*);
RobustShardKernel robustShardKernel(uint32_t K)
{
    switch (K)
    {
    case 3: return kRobustMeanShard<3>;
    case 5: return kRobustMeanShard<5>;
    case 7: return kRobustMeanShard<7>;
    case 9: return kRobustMeanShard<9>;
    case 11: return kRobustMeanShard<11>;
    case 13: return kRobustMeanShard<13>;
    case 15: return kRobustMeanShard<15>;
    default: throw std::logic_error("robustShardKernel: no such kernel is compiled");
    }
}
using RobustShardTilesKernel = void (*)(const float4*, size_t, uint32_t, const uint32_t*, float4*);
RobustShardTilesKernel robustShardTilesKernel(uint32_t K)
{
    switch (K)
    {
    case 3: return kRobustMeanShardTiles<3>;
    case 5: return kRobustMeanShardTiles<5>;
    case 7: return kRobustMeanShardTiles<7>;
    case 9: return kRobustMeanShardTiles<9>;
    case 11: return kRobustMeanShardTiles<11>;
    case 13: return kRobustMeanShardTiles<13>;
    case 15: return kRobustMeanShardTiles<15>;
    default: throw std::logic_error("robustShardTilesKernel: no such kernel is compiled");
    }
}
} // namespace

void RobustWork::reserve(uint64_t n, hipStream_t stream)
{
    if (n <= bgra.count) return; // (allocated last: it has room only when every buffer has)
    RF_HIP(hipStreamSynchronize(stream)); // (a smaller set may still be in use by the last run)
    release();
    mean.alloc(n);
    trim.alloc(n);
    bgra.alloc(n);
}

void RobustWork::release()
{
    mean.release();
    trim.release();
    bgra.release();
}

void enqueueRobustMean(hipStream_t stream, RobustWork& w, const float4* planes, size_t planeStride, uint32_t K, const FrameSums& f, float exposure)
{
    const uint32_t width = f.width, height = f.height, n = width * height;
    w.reserve(n, stream);
    if (f.tileSamples)
        hipLaunchKernelGGL(robustTilesKernel(K), dim3((n + 255) / 256), dim3(256), 0, stream, planes, planeStride, width, height, f.tilesX, f.tileSamples,
                           TileGrid(width, height).tilesX, w.mean.ptr, w.trim.ptr);
    else
        hipLaunchKernelGGL(robustKernel(K), dim3((n + 255) / 256), dim3(256), 0, stream, planes, planeStride, width, height, f.tilesX, f.samples, w.mean.ptr, w.trim.ptr);
    hipLaunchKernelGGL(tonemapKernel(), dim3((n + 255) / 256), dim3(256), 0, stream, static_cast<const float4*>(w.mean.ptr), n, 1u, exposure, w.bgra.ptr);
    RF_HIP(hipGetLastError());
}

void enqueueRobustMeanShard(hipStream_t stream, const float4* planes, size_t planeStride, uint32_t shardTiles, uint32_t K, uint32_t samples, float4* out,
                            const uint32_t* slotCounts)
{
    const uint32_t n = shardTiles * 1024u;
    if (n == 0u) return;
    if (slotCounts) hipLaunchKernelGGL(robustShardTilesKernel(K), dim3((n + 255) / 256), dim3(256), 0, stream, planes, planeStride, n, slotCounts, out);
    else hipLaunchKernelGGL(robustShardKernel(K), dim3((n + 255) / 256), dim3(256), 0, stream, planes, planeStride, n, samples, out);
    RF_HIP(hipGetLastError());
}

void enqueueRobustTexels(hipStream_t stream, const float4* mean, uint32_t pixels, float exposure, uint32_t* bgra)
{
    hipLaunchKernelGGL(tonemapKernel(), dim3((pixels + 255) / 256), dim3(256), 0, stream, mean, pixels, 1u, exposure, bgra);
    RF_HIP(hipGetLastError());
}

// rf_robust_mean_images (tileSamples == nullptr) and rf_robust_mean_tiles (one count per tile of the frame's grid, host memory)
static void robustMeanHost(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t K, uint32_t samples, const uint32_t* tileSamples, const float* buckets, float exposure,
                           float* outRgba, uint32_t* outBgra8, uint8_t* outTrim)
{
    DeviceBuffer<float4> in; // (the two before the stage: freed after it has drained its stream)
    RobustWork           work;
    StagedFrame          f(deviceOrdinal, width, height, samples, tileSamples, nullptr, nullptr, nullptr, nullptr, nullptr);
    f.upload(in, reinterpret_cast<const float4*>(buckets), K * f.pixels());
    enqueueRobustMean(f.stream.handle, work, in.ptr, f.pixels(), K, f.sums, exposure);
    f.download(outRgba, work.mean.ptr, f.pixels() * sizeof(float4));
    f.download(outBgra8, work.bgra.ptr, f.pixels() * sizeof(uint32_t));
    f.download(outTrim, work.trim.ptr, f.pixels() * sizeof(uint8_t));
    f.wait();
}

void robustMeanImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t K, uint32_t samples, const float* buckets, float exposure, float* outRgba,
                      uint32_t* outBgra8, uint8_t* outTrim)
{
    robustMeanHost(deviceOrdinal, width, height, K, samples, nullptr, buckets, exposure, outRgba, outBgra8, outTrim);
}

void robustMeanTiles(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t K, const uint32_t* tileSamples, const float* buckets, float exposure, float* outRgba,
                     uint32_t* outBgra8, uint8_t* outTrim)
{
    robustMeanHost(deviceOrdinal, width, height, K, 0u, tileSamples, buckets, exposure, outRgba, outBgra8, outTrim);
}
} // namespace rf
