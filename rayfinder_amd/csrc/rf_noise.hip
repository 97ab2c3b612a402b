// rf_noise.hip -- the noise estimate over the radiance sum S and its second moments Q (the sums themselves: rf_sums.hip).  The arithmetic is the one
// include/rayfinder_amd.h writes out ("Radiance second moments and the noise estimate"), one IEEE f32 operation at a time in that order (-ffp-contract=off, correctly
// rounded divide and sqrt, no denormal flushing): tests/noise_restatement.py reproduces it bit for bit.  No floating-point atomics: every output is one lane's fixed
// sequence of operations.
//   kNoiseEstimate          one 256-lane workgroup per 32x32 tile: the per-pixel relative standard error, the tile's halving-tree sum, maximum and counts
//   kNoiseEstimateTiles     kNoiseEstimate's body (estimateTile) for a list of tiles and / or one sample count per tile
//   kNoiseEstimateSlots     the same for a list of tiles of a tile shard: the tile's sums sit at its SLOT of the shard's compact buffers
//   kTileMean               {S.rgb / float(tile's sample count), 1} per pixel
//   kTileMeanRows           the same over a row-major frame
//   kSplitMeanRows          {D.rgb / float(n), 1} and {(S.rgb - D.rgb) / float(n), 1} per pixel of a row-major frame (the gathered frame's two components)
#include "rf_noise.hpp"

#include "rf_math.hpp"

#include <vector>

namespace rf
{
namespace
{
constexpr float kEpsLum = 0.00390625f; // 2^-8

// One workgroup per tile of the 32x32 grid.  tileMajor: entry j of the tile sits at S[tile * 1024 + j] (8x8 blocks, localPixelToXY's layout: the workgroup reads
// two contiguous 16 KB runs); else the sums are row-major.  nf = float(N), nf1 = nf - 1.  errorMap (row-major) may be nullptr.  srcTile: where the tile's sums sit in
// a tile-major buffer (`tile` itself, or its slot in a shard's compact buffer); the coordinates and every output belong to `tile`.
// (estimateTile: the work of one 256-lane workgroup for tile `tile`, shared by kNoiseEstimate and kNoiseEstimateTiles)
__device__ __forceinline__ void estimateTile(const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, uint32_t tilesX, uint32_t tileMajor, uint32_t tile, uint32_t srcTile,
                                             float nf, float nf1, float* errorMap, float* tileSum, float* tileMax, uint32_t* tilePixels, uint32_t* tileNonfinite)
{
    __shared__ float    a[1024]; // a[ty * 32 + tx]
    __shared__ float    sMax[256];
    __shared__ uint32_t sCount[2];
    const uint32_t t = threadIdx.x, tileY = tile / tilesX, tileX = tile - tileY * tilesX;
    if (t < 2u) sCount[t] = 0u;
    __syncthreads();
    float    m = -__builtin_inff();
    uint32_t pixels = 0, bad = 0;
    for (uint32_t j = t; j < 1024u; j += 256u)
    {
        const uint32_t block = j >> 6, lane = j & 63u;
        const uint32_t tx = tileMajor ? (block & 3u) * 8u + (lane & 7u) : (j & 31u), ty = tileMajor ? (block >> 2) * 8u + (lane >> 3) : (j >> 5);
        const uint32_t x = tileX * kTileSize + tx, y = tileY * kTileSize + ty;
        float          e = 0.0f;
        if (x < width && y < height)
        {
            const size_t src = tileMajor ? static_cast<size_t>(srcTile) * 1024u + j : static_cast<size_t>(y) * width + x;
            const float4 s4 = colorSum[src], q4 = sumSq[src];
            const float  s[3] = {s4.x, s4.y, s4.z}, q[3] = {q4.x, q4.y, q4.z};
            float        mu[3], v[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
            {
                mu[ch] = s[ch] / nf;
                const float sm = s[ch] * mu[ch];
                const float d = q[ch] - sm;
                const float vv = d / nf1;
                v[ch] = vv > 0.0f ? vv : 0.0f; // (NaN: 0)
            }
            const float s2 = ((v[0] + v[1]) + v[2]) / nf;
            const float l = (mu[0] + mu[1]) + mu[2];
            e = rf_sqrt(s2) / (l + kEpsLum);
            ++pixels;
            if (!(e <= FLT_MAX))
            {
                ++bad;
                e = 0.0f;
            }
            m = e > m ? e : m;
            if (errorMap) errorMap[static_cast<size_t>(y) * width + x] = e;
        }
        a[ty * 32u + tx] = e;
    }
    sMax[t] = m;
    atomicAdd(&sCount[0], pixels);
    if (bad) atomicAdd(&sCount[1], bad);
    __syncthreads();
    for (uint32_t h = 512u; h >= 1u; h >>= 1)
    {
        for (uint32_t i = t; i < h; i += 256u) a[i] = a[i] + a[i + h];
        if (h <= 128u && t < h)
        {
            const float o = sMax[t + h];
            if (o > sMax[t]) sMax[t] = o;
        }
        __syncthreads();
    }
    if (t == 0u)
    {
        tileSum[tile] = a[0];
        tileMax[tile] = sMax[0] + 0.0f; // (a maximum of -0 is returned as +0: which zero a maximum keeps is not an IEEE operation)
        tilePixels[tile] = sCount[0];
        tileNonfinite[tile] = sCount[1];
    }
}

__global__ __launch_bounds__(256) void kNoiseEstimate(const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, uint32_t tilesX, uint32_t tileMajor, float nf,
                                                      float nf1, float* errorMap, float* tileSum, float* tileMax, uint32_t* tilePixels, uint32_t* tileNonfinite)
{
    estimateTile(colorSum, sumSq, width, height, tilesX, tileMajor, blockIdx.x, blockIdx.x, nf, nf1, errorMap, tileSum, tileMax, tilePixels, tileNonfinite);
}

// One workgroup per LISTED tile (tileList == nullptr: tile blockIdx.x), with the tile's own sample count (tileSamples[tile]; nullptr: nf for all).  Nf = float(count),
// Nf - 1 one f32 subtraction, as the host computes them for kNoiseEstimate.  Every per-tile output is written at the tile's own index: entries of unlisted tiles stay.
__global__ __launch_bounds__(256) void kNoiseEstimateTiles(const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, uint32_t tilesX, uint32_t tileMajor,
                                                           const uint32_t* tileList, const uint32_t* tileSamples, float nf, float* errorMap, float* tileSum, float* tileMax,
                                                           uint32_t* tilePixels, uint32_t* tileNonfinite)
{
    const uint32_t tile = tileList ? tileList[blockIdx.x] : blockIdx.x;
    const float    n = tileSamples ? static_cast<float>(tileSamples[tile]) : nf;
    estimateTile(colorSum, sumSq, width, height, tilesX, tileMajor, tile, tile, n, n - 1.0f, errorMap, tileSum, tileMax, tilePixels, tileNonfinite);
}

// One workgroup per listed tile of a tile SHARD (rf_comm_render_adaptive): tileList holds the `listed` frame tile ids and, behind them, the tiles' slots in the shard's
// compact tile-major sums.  Nf = nf for all; the per-tile outputs at the tile's frame id, as above.
__global__ __launch_bounds__(256) void kNoiseEstimateSlots(const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, uint32_t tilesX, const uint32_t* tileList,
                                                           uint32_t listed, float nf, float* errorMap, float* tileSum, float* tileMax, uint32_t* tilePixels, uint32_t* tileNonfinite)
{
    estimateTile(colorSum, sumSq, width, height, tilesX, 1u, tileList[blockIdx.x], tileList[listed + blockIdx.x], nf, nf - 1.0f, errorMap, tileSum, tileMax, tilePixels, tileNonfinite);
}

// mean[i] = {S.rgb / float(n), 1}, n = the sample count of the pixel's tile (tileSamples[i >> 10]; nullptr: `samples` for all); n = 0: {0, 0, 0, 1}.  Compact tile-major.
__global__ __launch_bounds__(256) void kTileMean(const float4* image, const uint32_t* tileSamples, uint32_t samples, uint32_t n, float4* mean)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t count = tileSamples ? tileSamples[i >> 10] : samples;
    const float4   s = image[i];
    const float    nf = static_cast<float>(count);
    mean[i] = count ? make_float4(s.x / nf, s.y / nf, s.z / nf, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}

// The same over a row-major width x height frame (the gathered image on the root): n = tileSamples[tile of the pixel], tile = (y / 32) * tilesX + x / 32
__global__ __launch_bounds__(256) void kTileMeanRows(const float4* image, const uint32_t* tileSamples, uint32_t width, uint32_t height, uint32_t tilesX, float4* mean)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    const uint32_t count = tileSamples[(y / kTileSize) * tilesX + x / kTileSize];
    const float4   s = image[i];
    const float    nf = static_cast<float>(count);
    mean[i] = count ? make_float4(s.x / nf, s.y / nf, s.z / nf, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}

// The two components of a row-major width x height frame (the gathered S and D on the root), one lane per pixel, S and D read once each:
// direct[i] = {D.rgb / float(n), 1}, indirect[i] = {(S.rgb - D.rgb) / float(n), 1} -- one f32 subtraction, then one IEEE division, per channel.  n = the count of the
// pixel's tile (tileSamples, as kTileMeanRows) or, tileSamples == nullptr, `samples` for all; n = 0: {0, 0, 0, 1} for both.  No LDS; 32 bytes in and out per pixel.
__global__ __launch_bounds__(256) void kSplitMeanRows(const float4* __restrict__ image, const float4* __restrict__ directSum, const uint32_t* __restrict__ tileSamples, uint32_t samples,
                                                      uint32_t width, uint32_t height, uint32_t tilesX, float4* __restrict__ direct, float4* __restrict__ indirect)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    uint32_t count = samples;
    if (tileSamples)
    {
        const uint32_t y = i / width, x = i - y * width;
        count = tileSamples[(y / kTileSize) * tilesX + x / kTileSize];
    }
    const float4 s = image[i], d = directSum[i];
    const float  nf = static_cast<float>(count);
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    direct[i] = count ? make_float4(d.x / nf, d.y / nf, d.z / nf, 1.0f) : none;
    indirect[i] = count ? make_float4((s.x - d.x) / nf, (s.y - d.y) / nf, (s.z - d.z) / nf, 1.0f) : none;
}
} // namespace

TileMeanKernel tileMeanKernel() { return kTileMean; }

void enqueueTileMeanRows(hipStream_t stream, const float4* image, const uint32_t* tileSamples, uint32_t width, uint32_t height, float4* mean)
{
    const uint32_t n = width * height; // (< 2^31: the callers check)
    hipLaunchKernelGGL(kTileMeanRows, dim3((n + 255u) / 256u), dim3(256), 0, stream, image, tileSamples, width, height, TileGrid(width, height).tilesX, mean);
    RF_HIP(hipGetLastError());
}

void enqueueSplitMeanRows(hipStream_t stream, const float4* image, const float4* directSum, const uint32_t* tileSamples, uint32_t samples, uint32_t width, uint32_t height,
                          float4* direct, float4* indirect)
{
    const uint32_t n = width * height; // (< 2^31: the callers check)
    hipLaunchKernelGGL(kSplitMeanRows, dim3((n + 255u) / 256u), dim3(256), 0, stream, image, directSum, tileSamples, samples, width, height, TileGrid(width, height).tilesX, direct,
                       indirect);
    RF_HIP(hipGetLastError());
}

void NoiseWork::reserve(uint64_t nTiles, uint64_t nMap, hipStream_t stream)
{
    if (nTiles <= tiles && nMap <= errorMap.count) return;
    RF_HIP(hipStreamSynchronize(stream)); // (a smaller set may still be in use by the last run)
    nTiles = std::max(nTiles, tiles), nMap = std::max<uint64_t>(nMap, errorMap.count);
    release(); // (the whole set goes before any of the new one comes)
    tileSumMax.alloc(2 * nTiles);
    tileCounts.alloc(2 * nTiles);
    errorMap.alloc(nMap);
    tiles = nTiles;
}

void NoiseWork::release()
{
    tileSumMax.release(), tileCounts.release(), errorMap.release();
    tiles = 0;
}

NoiseEstimate runNoiseEstimate(hipStream_t stream, NoiseWork& w, const FrameSums& sums, float* errorMap, float* tileSum, float* tileMax)
{
    return runNoiseEstimateTiles(stream, w, sums, TileSelection{}, errorMap, tileSum, tileMax, nullptr);
}

NoiseEstimate runNoiseEstimateTiles(hipStream_t stream, NoiseWork& w, const FrameSums& s, const TileSelection& sel, float* errorMap, float* tileSum, float* tileMax,
                                    uint32_t* tilePixels)
{
    const uint32_t width = s.width, height = s.height, tilesX = TileGrid(width, height).tilesX, tiles = TileGrid(width, height).count();
    const uint32_t tileMajor = s.tilesX != 0u ? 1u : 0u; // (the kernels take a flag and the grid's own tilesX)
    const uint32_t listed = sel.listDevice ? sel.listCount : tiles;
    const uint64_t n = static_cast<uint64_t>(width) * height;
    NoiseEstimate  out;
    out.samples = s.samples;
    if (listed == 0) return out;
    w.reserve(tiles, errorMap ? n : 0, stream);
    const float nf = static_cast<float>(s.samples), nf1 = nf - 1.0f;
    float* const map = errorMap ? w.errorMap.ptr : static_cast<float*>(nullptr);
    if (sel.slotsBehindList)
    {
        if (!tileMajor || sel.listDevice == nullptr || s.tileSamples != nullptr) throw std::logic_error("a shard's slot list: tile-major sums, a list, one count");
        hipLaunchKernelGGL(kNoiseEstimateSlots, dim3(listed), dim3(256), 0, stream, s.colorSum, s.sumSq, width, height, tilesX, sel.listDevice, listed, nf, map, w.tileSumMax.ptr,
                           w.tileSumMax.ptr + w.tiles, w.tileCounts.ptr, w.tileCounts.ptr + w.tiles);
    }
    else if (sel.listDevice == nullptr && s.tileSamples == nullptr)
        hipLaunchKernelGGL(kNoiseEstimate, dim3(tiles), dim3(256), 0, stream, s.colorSum, s.sumSq, width, height, tilesX, tileMajor, nf, nf1, map, w.tileSumMax.ptr,
                           w.tileSumMax.ptr + w.tiles, w.tileCounts.ptr, w.tileCounts.ptr + w.tiles);
    else
        hipLaunchKernelGGL(kNoiseEstimateTiles, dim3(listed), dim3(256), 0, stream, s.colorSum, s.sumSq, width, height, tilesX, tileMajor, sel.listDevice, s.tileSamples,
                           nf, map, w.tileSumMax.ptr, w.tileSumMax.ptr + w.tiles, w.tileCounts.ptr, w.tileCounts.ptr + w.tiles);
    RF_HIP(hipGetLastError());
    std::vector<float>    sums(tiles), maxima(tiles);
    std::vector<uint32_t> pixels(tiles), nonfinite(tiles);
    RF_HIP(hipMemcpyAsync(sums.data(), w.tileSumMax.ptr, tiles * sizeof(float), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipMemcpyAsync(maxima.data(), w.tileSumMax.ptr + w.tiles, tiles * sizeof(float), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipMemcpyAsync(pixels.data(), w.tileCounts.ptr, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipMemcpyAsync(nonfinite.data(), w.tileCounts.ptr + w.tiles, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (errorMap) RF_HIP(hipMemcpyAsync(errorMap, w.errorMap.ptr, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    RF_HIP(hipStreamSynchronize(stream));
    // the frame (or the listed tiles), on the host: tile sums added in f64 in ascending tile order; the first tile that attains the maximum
    const auto tileAt = [&](uint32_t i) { return sel.listDevice ? sel.listHost[i] : i; };
    double total = 0.0;
    out.maxError = maxima[tileAt(0)];
    out.worstTile = tileAt(0);
    for (uint32_t i = 0; i < listed; ++i)
    {
        const uint32_t t = tileAt(i);
        total += static_cast<double>(sums[t]);
        if (maxima[t] > out.maxError) out.maxError = maxima[t], out.worstTile = t;
        out.pixels += pixels[t];
        out.nonfinitePixels += nonfinite[t];
    }
    out.meanError = total / static_cast<double>(out.pixels);
    // (with a list, the entries of unlisted tiles are whatever an earlier run left: the caller reads the listed ones)
    if (tileSum) std::memcpy(tileSum, sums.data(), tiles * sizeof(float));
    if (tileMax) std::memcpy(tileMax, maxima.data(), tiles * sizeof(float));
    if (tilePixels) std::memcpy(tilePixels, pixels.data(), tiles * sizeof(uint32_t));
    return out;
}

NoiseEstimate noiseEstimateImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* sumSq, float* errorMap, float* tileSum,
                                  float* tileMax)
{
    return noiseEstimateTiles(deviceOrdinal, width, height, nullptr, samples, colorSum, sumSq, errorMap, tileSum, tileMax);
}

NoiseEstimate noiseEstimateTiles(int deviceOrdinal, uint32_t width, uint32_t height, const uint32_t* tileSamples, uint32_t samples, const float* colorSum, const float* sumSq,
                                 float* errorMap, float* tileSum, float* tileMax)
{
    NoiseWork   work; // (before the stage: freed after it has drained its stream)
    StagedFrame f(deviceOrdinal, width, height, samples, tileSamples, colorSum, sumSq, nullptr, nullptr, nullptr);
    return runNoiseEstimate(f.stream.handle, work, f.sums, errorMap, tileSum, tileMax);
}
} // namespace rf
