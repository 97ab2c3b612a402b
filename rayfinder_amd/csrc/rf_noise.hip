// rf_noise.hip -- per-pixel radiance second moments and the noise estimate over them.  The arithmetic is the one include/rayfinder_amd.h writes out ("Radiance
// second moments and the noise estimate"), one IEEE f32 operation at a time in that order (-ffp-contract=off, correctly rounded divide and sqrt, no denormal
// flushing): tests/noise_restatement.py reproduces it bit for bit.  No floating-point atomics: every output is one lane's fixed sequence of operations.
//   kAccumulateMoments      one lane per pixel, any slot order (kAccumulate's addressing): Q += r r per channel, samples in index order
//   kAccumulateMomentsRuns  the same sums for the pixel-major slot order, the runs staged (squared) in LDS in fixed-size chunks (kAccumulateAovRuns' shape)
//   kNoiseEstimate          one 256-lane workgroup per 32x32 tile: the per-pixel relative standard error, the tile's halving-tree sum, maximum and counts
//   kAccumulateTiles        tile-adaptive sampling: S += r AND Q += r r in one pass, for a LIST of tiles of the whole frame, written at the listed tiles' own places
//   kAccumulateTilesRuns    the same sums for the pixel-major slot order, the runs staged in LDS (kAccumulateMomentsRuns' shape)
//   kAccumulateTilesAov     the first-hit AOV sums of a tile-list batch (kAccumulateAov's chains), written at the listed tiles' own places; any slot order
//   kAccumulateTilesAovRuns the same sums for the pixel-major slot order, the records staged in LDS (kAccumulateAovRuns' shape)
//   kNoiseEstimateTiles     kNoiseEstimate's body (estimateTile) for a list of tiles and / or one sample count per tile
//   kTileMean               {S.rgb / float(tile's sample count), 1} per pixel
// The radiance kernels read the per-slot radiance stream the image is accumulated from (ps.rad) and nothing else of the path state, the two AOV kernels the per-slot
// records kShade<false, true> wrote at bounce 1: the trace and shading kernels do not know about them.
#include "rf_noise.hpp"

#include "rf_math.hpp"

#include <vector>

namespace rf
{
namespace
{
constexpr float kEpsLum = 0.00390625f; // 2^-8

__global__ __launch_bounds__(kBlock) void kAccumulateMoments(FrameParams fp, const uint32_t* tileIds, const float4* rad, float4* moments)
{
    const uint32_t lp = blockIdx.x * kBlock + threadIdx.x;
    if (lp >= fp.pixelsPadded) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    float4 q = moments[lp];
    for (uint32_t k = 0; k < fp.numSamples; ++k)
    {
        const Vec3 r = load3(rad + samplePixelToSlot(fp, fp.sampleInvPerm ? fp.sampleInvPerm[k] : k, lp));
        q.x += r.x * r.x;
        q.y += r.y * r.y;
        q.z += r.z * r.z;
    }
    moments[lp] = q;
}

// Pixel-major slot order (slotGroupShift = 0): a pixel's samples are one run of numSamples float4.  One 64-lane workgroup takes kMomentPixels pixels; per chunk of
// kMomentChunk samples it reads their radiance (two pixels' chunks = 1 KiB per load round, coalesced when the samples are not permuted), squares it -- in parallel,
// one multiply per channel -- and stores the squares in LDS at the sample's index; then each of the 48 summing lanes -- one (pixel, channel) -- adds the chunk in
// sample order onto its running sum.  6.3 KB of LDS per workgroup at any batch depth (<= ~8 KB keeps twenty workgroups resident per CU, profiles/r06_raygen).
__global__ __launch_bounds__(64) void kAccumulateMomentsRuns(FrameParams fp, const uint32_t* tileIds, const float4* rad, float4* moments)
{
    constexpr uint32_t R = kMomentChunk + 1u; // rows padded by one float: the summing lanes walk different banks
    __shared__ float   sRun[kMomentPixels * 3u * R]; // [pixel][channel][sample of the chunk]
    static_assert(kMomentPixels * 3u <= 64u && kMomentChunk * 2u == 64u && kMomentPixels % 2u == 0u, "one summing lane per (pixel, channel); two pixels' chunks per load round");
    const uint32_t S = fp.numSamples, lane = threadIdx.x, lp0 = blockIdx.x * kMomentPixels;
    const uint32_t px = lane / 3u, c = lane - 3u * px, lp = lp0 + px;
    const bool     sums = lane < kMomentPixels * 3u && lp < fp.pixelsPadded;
    float          acc = sums ? reinterpret_cast<const float*>(moments + lp)[c] : 0.0f;
    for (uint32_t k0 = 0; k0 < S; k0 += kMomentChunk)
    {
        const uint32_t n = min(kMomentChunk, S - k0), kk = lane & (kMomentChunk - 1u), half = lane >> 5;
        if (kk < n)
        {
            const uint32_t k = k0 + kk, p = fp.sampleInvPerm ? fp.sampleInvPerm[k] : k; // sample k sits at position p of the pixel's run
            // load round i: pixels 2 i and 2 i + 1 of the workgroup, lane = (pixel of the pair, sample of the chunk)
#pragma unroll
            for (uint32_t i = 0; i < kMomentPixels / 2u; ++i)
            {
                const uint32_t pi = 2u * i + half, lpi = lp0 + pi;
                if (lpi >= fp.pixelsPadded) continue;
                const Vec3 v = load3(rad + static_cast<size_t>(lpi) * S + p);
                float*     dst = sRun + pi * 3u * R + kk;
                dst[0] = v.x * v.x, dst[R] = v.y * v.y, dst[2u * R] = v.z * v.z;
            }
        }
        __syncthreads();
        if (sums)
        {
            const float* src = sRun + lane * R; // (row lane = pixel px, channel c)
            for (uint32_t j = 0; j < n; ++j) acc += src[j]; // sample order: one dependent chain of f32 additions per channel
        }
        __syncthreads(); // the next chunk overwrites the rows
    }
    if (!sums) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    reinterpret_cast<float*>(moments + lp)[c] = acc;
}

// One workgroup per tile of the 32x32 grid.  tileMajor: entry j of the tile sits at S[tile * 1024 + j] (8x8 blocks, localPixelToXY's layout: the workgroup reads
// two contiguous 16 KB runs); else the sums are row-major.  nf = float(N), nf1 = nf - 1.  errorMap (row-major) may be nullptr.
// (estimateTile: the work of one 256-lane workgroup for tile `tile`, shared by kNoiseEstimate and kNoiseEstimateTiles)
__device__ __forceinline__ void estimateTile(const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, uint32_t tilesX, uint32_t tileMajor, uint32_t tile, float nf,
                                             float nf1, float* errorMap, float* tileSum, float* tileMax, uint32_t* tilePixels, uint32_t* tileNonfinite)
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
            const size_t src = tileMajor ? static_cast<size_t>(tile) * 1024u + j : static_cast<size_t>(y) * width + x;
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
    estimateTile(colorSum, sumSq, width, height, tilesX, tileMajor, blockIdx.x, nf, nf1, errorMap, tileSum, tileMax, tilePixels, tileNonfinite);
}

// One workgroup per LISTED tile (tileList == nullptr: tile blockIdx.x), with the tile's own sample count (tileSamples[tile]; nullptr: nf for all).  Nf = float(count),
// Nf - 1 one f32 subtraction, as the host computes them for kNoiseEstimate.  Every per-tile output is written at the tile's own index: entries of unlisted tiles stay.
__global__ __launch_bounds__(256) void kNoiseEstimateTiles(const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, uint32_t tilesX, uint32_t tileMajor,
                                                           const uint32_t* tileList, const uint32_t* tileSamples, float nf, float* errorMap, float* tileSum, float* tileMax,
                                                           uint32_t* tilePixels, uint32_t* tileNonfinite)
{
    const uint32_t tile = tileList ? tileList[blockIdx.x] : blockIdx.x;
    const float    n = tileSamples ? static_cast<float>(tileSamples[tile]) : nf;
    estimateTile(colorSum, sumSq, width, height, tilesX, tileMajor, tile, n, n - 1.0f, errorMap, tileSum, tileMax, tilePixels, tileNonfinite);
}

// Tile-adaptive sampling: the batch's path slots belong to the fp.numTiles tiles tileIds lists (local pixel lp = list position * 1024 + pixel of the tile), and the
// handle's sums hold the WHOLE frame, compact slot == tile id: the sums of lp sit at tileIds[lp >> 10] * 1024 + (lp & 1023).  S += r and Q += r r per channel, samples
// in index order: kAccumulate's and kAccumulateMoments' chains (one add; one multiply and one add), from one read of the radiance.  Any slot order.
__global__ __launch_bounds__(kBlock) void kAccumulateTiles(FrameParams fp, const uint32_t* tileIds, const float4* rad, float4* image, float4* moments)
{
    const uint32_t lp = blockIdx.x * kBlock + threadIdx.x;
    if (lp >= fp.pixelsPadded) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    const size_t at = static_cast<size_t>(tileIds[lp >> 10]) * 1024u + (lp & 1023u);
    float4       s = image[at], q = moments[at];
    for (uint32_t k = 0; k < fp.numSamples; ++k)
    {
        const Vec3 r = load3(rad + samplePixelToSlot(fp, fp.sampleInvPerm ? fp.sampleInvPerm[k] : k, lp));
        s.x += r.x;
        s.y += r.y;
        s.z += r.z;
        q.x += r.x * r.x;
        q.y += r.y * r.y;
        q.z += r.z * r.z;
    }
    image[at] = s;
    moments[at] = q;
}

// The same sums for the pixel-major slot order (slotGroupShift = 0), in kAccumulateMomentsRuns' shape: one 64-lane workgroup takes kMomentPixels pixels, stages their
// runs' radiance in LDS in chunks of kMomentChunk samples (at the sample's index), and each of the 48 summing lanes -- one (pixel, channel) -- walks its row in sample
// order with TWO running sums: S += r, Q += r r.  The row holds r, not r r: the square is the same one f32 multiply wherever it is taken, and one row serves both
// sums -- 6.3 KB of LDS per workgroup, kAccumulateMomentsRuns' figure, for one read of the radiance instead of kAccumulateRuns' and kAccumulateMomentsRuns' two.
__global__ __launch_bounds__(64) void kAccumulateTilesRuns(FrameParams fp, const uint32_t* tileIds, const float4* rad, float4* image, float4* moments)
{
    constexpr uint32_t R = kMomentChunk + 1u; // rows padded by one float: the summing lanes walk different banks
    __shared__ float   sRun[kMomentPixels * 3u * R]; // [pixel][channel][sample of the chunk]
    const uint32_t S = fp.numSamples, lane = threadIdx.x, lp0 = blockIdx.x * kMomentPixels;
    const uint32_t px = lane / 3u, c = lane - 3u * px, lp = lp0 + px;
    uint32_t       x, y;
    const bool     sums = lane < kMomentPixels * 3u && lp < fp.pixelsPadded && localPixelToXY(fp, tileIds, lp, x, y); // (pixels outside the frame: read, never summed)
    const size_t   at = sums ? static_cast<size_t>(tileIds[lp >> 10]) * 1024u + (lp & 1023u) : 0u;
    float          accS = sums ? reinterpret_cast<const float*>(image + at)[c] : 0.0f;
    float          accQ = sums ? reinterpret_cast<const float*>(moments + at)[c] : 0.0f;
    for (uint32_t k0 = 0; k0 < S; k0 += kMomentChunk)
    {
        const uint32_t n = min(kMomentChunk, S - k0), kk = lane & (kMomentChunk - 1u), half = lane >> 5;
        if (kk < n)
        {
            const uint32_t k = k0 + kk, p = fp.sampleInvPerm ? fp.sampleInvPerm[k] : k; // sample k sits at position p of the pixel's run
#pragma unroll
            for (uint32_t i = 0; i < kMomentPixels / 2u; ++i)
            {
                const uint32_t pi = 2u * i + half, lpi = lp0 + pi;
                if (lpi >= fp.pixelsPadded) continue;
                const Vec3 v = load3(rad + static_cast<size_t>(lpi) * S + p);
                float*     dst = sRun + pi * 3u * R + kk;
                dst[0] = v.x, dst[R] = v.y, dst[2u * R] = v.z;
            }
        }
        __syncthreads();
        if (sums)
        {
            const float* src = sRun + lane * R; // (row lane = pixel px, channel c)
            for (uint32_t j = 0; j < n; ++j)
            {
                const float r = src[j];
                accS += r; // sample order: one dependent chain of f32 additions per channel and sum
                accQ += r * r;
            }
        }
        __syncthreads(); // the next chunk overwrites the rows
    }
    if (!sums) return;
    reinterpret_cast<float*>(image + at)[c] = accS;
    reinterpret_cast<float*>(moments + at)[c] = accQ;
}

// The first-hit AOV sums of a tile-list batch (rf_renderer_render_adaptive with RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS): the records are the batch's own, at the batch's
// slots (kShade<false, true> numbers them along the active list), the sums the WHOLE frame's: those of lp sit at tileIds[lp >> 10] * 1024 + (lp & 1023), as for S and Q
// above.  kAccumulateAov's chains: eight running sums per pixel, one f32 add per sample in sample-index order.  Any slot order.
__global__ __launch_bounds__(kBlock) void kAccumulateTilesAov(FrameParams fp, const uint32_t* tileIds, const float4* aov, float4* albedoCoverage, float4* normalDepth)
{
    const uint32_t lp = blockIdx.x * kBlock + threadIdx.x;
    if (lp >= fp.pixelsPadded) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    const size_t at = static_cast<size_t>(tileIds[lp >> 10]) * 1024u + (lp & 1023u);
    float4       a = albedoCoverage[at], b = normalDepth[at];
    for (uint32_t k = 0; k < fp.numSamples; ++k)
    {
        const size_t slot = samplePixelToSlot(fp, fp.sampleInvPerm ? fp.sampleInvPerm[k] : k, lp);
        const float4 ra = aov[2 * slot], rb = aov[2 * slot + 1];
        a.x += ra.x, a.y += ra.y, a.z += ra.z, a.w += ra.w;
        b.x += rb.x, b.y += rb.y, b.z += rb.z, b.w += rb.w;
    }
    albedoCoverage[at] = a;
    normalDepth[at] = b;
}

// The same sums for the pixel-major slot order (slotGroupShift = 0), in kAccumulateAovRuns' shape: one 64-lane workgroup takes kAovPixels pixels, stages their runs'
// 32-byte records in LDS in chunks of kAovChunk samples (at the sample's index), and each lane -- one (pixel, channel) -- adds the chunk in sample order onto its
// running sum.  8 x 8 x (32 + 1) floats = 8.4 KB of LDS per workgroup at any step length.
__global__ __launch_bounds__(64) void kAccumulateTilesAovRuns(FrameParams fp, const uint32_t* tileIds, const float4* aov, float4* albedoCoverage, float4* normalDepth)
{
    constexpr uint32_t R = kAovChunk + 1u; // rows padded by one float: the summing lanes walk different banks
    __shared__ float   sRun[kAovPixels * 8u * R]; // [pixel][channel][sample of the chunk]
    static_assert(kAovPixels * 8u == 64u && kAovPixels * kAovChunk * 2u % 64u == 0u, "one summing lane per (pixel, channel); whole load rounds");
    const uint32_t S = fp.numSamples, lane = threadIdx.x, lp0 = blockIdx.x * kAovPixels;
    const uint32_t px = lane / 8u, c = lane % 8u, lp = lp0 + px;
    uint32_t       x, y;
    const bool     sums = lp < fp.pixelsPadded && localPixelToXY(fp, tileIds, lp, x, y); // (pixels outside the frame: read, never summed)
    const size_t   at = sums ? static_cast<size_t>(tileIds[lp >> 10]) * 1024u + (lp & 1023u) : 0u;
    float* const   sum = reinterpret_cast<float*>(c < 4u ? albedoCoverage + at : normalDepth + at) + (c & 3u);
    float          acc = sums ? *sum : 0.0f;
    for (uint32_t k0 = 0; k0 < S; k0 += kAovChunk)
    {
        const uint32_t n = min(kAovChunk, S - k0);
        // load round i: pixel i of the workgroup, lane = (sample of the chunk, half of the record)
        for (uint32_t i = 0; i < kAovPixels; ++i)
        {
            const uint32_t kk = lane >> 1, half = lane & 1u, lpi = lp0 + i;
            if (kk >= n || lpi >= fp.pixelsPadded) continue;
            const uint32_t k = k0 + kk, p = fp.sampleInvPerm ? fp.sampleInvPerm[k] : k; // sample k sits at position p of the pixel's run
            const float4   v = aov[2 * (static_cast<size_t>(lpi) * S + p) + half];
            float*         dst = sRun + (i * 8u + half * 4u) * R + kk;
            dst[0] = v.x, dst[R] = v.y, dst[2u * R] = v.z, dst[3u * R] = v.w;
        }
        __syncthreads();
        if (sums)
        {
            const float* src = sRun + lane * R; // (row lane = pixel px, channel c)
            for (uint32_t kk = 0; kk < n; ++kk) acc += src[kk]; // sample order: one dependent chain of f32 additions per channel
        }
        __syncthreads(); // the next chunk overwrites the rows
    }
    if (sums) *sum = acc;
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
} // namespace

AccumulateTilesKernel accumulateTilesKernel(bool runs) { return runs ? kAccumulateTilesRuns : kAccumulateTiles; }
AccumulateAovKernel   accumulateTilesAovKernel(bool runs) { return runs ? kAccumulateTilesAovRuns : kAccumulateTilesAov; }
TileMeanKernel        tileMeanKernel() { return kTileMean; }

AccumulateMomentsKernel accumulateMomentsKernel(bool runs) { return runs ? kAccumulateMomentsRuns : kAccumulateMoments; }

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

NoiseEstimate runNoiseEstimate(hipStream_t stream, NoiseWork& w, const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, bool tileMajor, uint32_t samples,
                               float* errorMap, float* tileSum, float* tileMax)
{
    return runNoiseEstimateTiles(stream, w, colorSum, sumSq, width, height, tileMajor, TileSelection{}, samples, errorMap, tileSum, tileMax, nullptr);
}

NoiseEstimate runNoiseEstimateTiles(hipStream_t stream, NoiseWork& w, const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, bool tileMajor,
                                    const TileSelection& sel, uint32_t samples, float* errorMap, float* tileSum, float* tileMax, uint32_t* tilePixels)
{
    const uint32_t tilesX = TileGrid(width, height).tilesX, tiles = TileGrid(width, height).count();
    const uint32_t listed = sel.listDevice ? sel.listCount : tiles;
    const uint64_t n = static_cast<uint64_t>(width) * height;
    NoiseEstimate  out;
    out.samples = samples;
    if (listed == 0) return out;
    w.reserve(tiles, errorMap ? n : 0, stream);
    const float nf = static_cast<float>(samples), nf1 = nf - 1.0f;
    float* const map = errorMap ? w.errorMap.ptr : static_cast<float*>(nullptr);
    if (sel.listDevice == nullptr && sel.tileSamplesDevice == nullptr)
        hipLaunchKernelGGL(kNoiseEstimate, dim3(tiles), dim3(256), 0, stream, colorSum, sumSq, width, height, tilesX, tileMajor ? 1u : 0u, nf, nf1, map, w.tileSumMax.ptr,
                           w.tileSumMax.ptr + w.tiles, w.tileCounts.ptr, w.tileCounts.ptr + w.tiles);
    else
        hipLaunchKernelGGL(kNoiseEstimateTiles, dim3(listed), dim3(256), 0, stream, colorSum, sumSq, width, height, tilesX, tileMajor ? 1u : 0u, sel.listDevice, sel.tileSamplesDevice,
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
    requireDevice(deviceOrdinal);
    const uint64_t n = static_cast<uint64_t>(width) * height;
    const uint32_t tiles = TileGrid(width, height).count();
    // (leaving the scope: the stream is synchronised, the buffers are freed, the stream is destroyed -- ScopedStream)
    ScopedStream           stream;
    DeviceBuffer<float4>   in[2];
    DeviceBuffer<uint32_t> counts;
    NoiseWork              work;
    ScopedStream::Drain    drain{stream};
    const float*           src[2] = {colorSum, sumSq};
    for (int b = 0; b < 2; ++b)
    {
        in[b].alloc(n);
        RF_HIP(hipMemcpyAsync(in[b].ptr, src[b], n * sizeof(float4), hipMemcpyHostToDevice, stream.handle));
    }
    TileSelection sel;
    if (tileSamples)
    {
        counts.alloc(tiles);
        RF_HIP(hipMemcpyAsync(counts.ptr, tileSamples, tiles * sizeof(uint32_t), hipMemcpyHostToDevice, stream.handle));
        sel.tileSamplesDevice = counts.ptr;
    }
    return runNoiseEstimateTiles(stream.handle, work, in[0].ptr, in[1].ptr, width, height, false, sel, samples, errorMap, tileSum, tileMax, nullptr);
}
} // namespace rf
