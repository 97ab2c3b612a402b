// rf_sums.hip -- the per-pixel sums in sample order (rf_sums.hpp): the image S, the radiance second moments Q and the two first-hit AOV sums, from the per-slot
// records a batch leaves (the radiance stream ps.rad; kShade<false, true>'s AOV records of bounce 1).  The trace and shading kernels do not know about them.
//   kSumPixels<Sum, TILE_LIST>   one lane per pixel, any slot order                         (Sum = ShardList<...>: the tile list of a tile shard, see sumIndex)
//   kSumRuns<Sum, TILE_LIST>     pixel-major slot order: a 64-lane workgroup stages its pixels' runs in LDS in 32-sample chunks, one summing lane per (pixel, channel)
//   kAccumulateRuns<PIXELS>      pixel-major slot order, the image alone: the WHOLE runs of PIXELS pixels in dynamic LDS (the headline path, profiles/r06_raygen)
//   kBucketSumPixels<TILE_LIST, Sum> / kBucketSumRuns<TILE_LIST, Sum>  the K bucket planes (rf_renderer_set_buckets): sample k of the batch goes to plane
//                                (phase + k) mod K; the same two forms, every plane addressed through sumIndex (Sum = ShardList<RadianceSum>: a tile shard's slot list)
// What is summed is a policy struct (below); where a pixel's sums live is sumIndex.  The contract all three keep: each channel of each sum is one dependent chain of
// f32 additions in sample-index order (Q's term: one f32 multiply of the loaded value with itself), no atomics, no contraction (-ffp-contract=off).
// To add a sum: one policy struct, one enumerator of Sum, its instantiations in sumKernel's table, one entry in Impl::enqueueSums' list.
#include "rf_sums.hpp"

namespace rf
{
namespace
{
// ShardList<SUM>: the sum SUM under a tile list of a handle WITH a tile shard (rf_comm_render_adaptive).  The handle's sums are then compact over the shard, so a listed
// tile has two numbers: its frame tile id tileIds[k], which the pixel coordinates come from, and its SLOT in the shard, tileIds[numTiles + k] -- the host uploads the
// slots behind the ids.  A wrapper of the policy and not a third template parameter of the kernels, so that the kernels compiled before it keep their names.
template<class SUM>
struct ShardList : SUM
{
};
template<class SUM>
constexpr bool kShardList = false;
template<class SUM>
constexpr bool kShardList<ShardList<SUM>> = true;

// Where the sums of local pixel lp live: the ONLY place that knows.  Shard-compact: at lp.  TILE_LIST: the batch's path slots belong to the numTiles tiles that
// tileIds lists (lp = list position * 1024 + pixel of the tile); the sums hold the whole frame, compact slot == tile id -- or, SUM = ShardList<...>, the shard, at the
// slots listed behind the ids.
template<class SUM, bool TILE_LIST>
__device__ __forceinline__ size_t sumIndex(const uint32_t* tileIds, uint32_t numTiles, uint32_t lp)
{
    static_assert(TILE_LIST || !kShardList<SUM>, "a shard's slot list is a tile list");
    return TILE_LIST ? static_cast<size_t>(tileIds[(kShardList<SUM> ? numTiles : 0u) + (lp >> 10)]) * 1024u + (lp & 1023u) : lp;
}
// A pixel's running sums are the eight floats {dst0[at].xyzw, dst1[at].xyzw}: term i of channel c is float c + 4 i of them
__device__ __forceinline__ float* sumFloat(float4* dst0, float4* dst1, size_t at, uint32_t f) { return reinterpret_cast<float*>((f < 4u ? dst0 : dst1) + at) + (f & 3u); }

// ---- The sums.  A slot holds kRecords float4 records of kChannels / kRecords channels each; values() loads one record and hands out its channels' values -- what
// kSumRuns' loading lanes stage in LDS --; term(v, i) is what a value adds to the channel's running sum i < kTerms; kRunPixels x kChannels <= 64 summing lanes.
// kTestPerRound: kSumRuns takes the sample-in-chunk test and the permutation entry in every load round (true) or once per chunk (false): each sum keeps the form it was
// measured with.
struct RadianceSum // S += r.  Shard-compact: one lane per pixel only (its staged kernel there is kAccumulateRuns); under a tile list (the direct sums D of
{                  // rf_renderer_set_direct with RF_DIRECT_TILE_COUNTS) both forms, the staged one with MomentSum's constants
    static constexpr uint32_t kChannels = 3, kRecords = 1, kTerms = 1, kRunPixels = kMomentPixels, kChunk = kMomentChunk;
#if defined(RF_EXP_DIRECT_TEST_PER_ROUND) // (the A/B of profiles/direct_adaptive: the test and the permutation entry in every load round measured 122 us against 90)
    static constexpr bool     kTestPerRound = true;
#else
    static constexpr bool     kTestPerRound = false;
#endif
    __device__ static __forceinline__ void values(const float4* rec, float (&v)[4])
    {
        const float4 r = *rec;
        v[0] = r.x, v[1] = r.y, v[2] = r.z;
    }
    __device__ static __forceinline__ float term(float v, uint32_t) { return v; }
};
struct MomentSum // Q += r r: squared where it is loaded (in kSumRuns: by the 64 loading lanes in parallel, not by the 48 that sum)
{
    static constexpr uint32_t kChannels = 3, kRecords = 1, kTerms = 1, kRunPixels = kMomentPixels, kChunk = kMomentChunk;
    static constexpr bool     kTestPerRound = false;
    __device__ static __forceinline__ void values(const float4* rec, float (&v)[4])
    {
        const Vec3 r = load3(rec);
        v[0] = r.x * r.x, v[1] = r.y * r.y, v[2] = r.z * r.z;
    }
    __device__ static __forceinline__ float term(float v, uint32_t) { return v; }
};
struct RadianceMomentSum // S += r (dst0) and Q += r r (dst1) from one read of the radiance: one staged row serves both, the square is the same one multiply wherever it is taken
{
    static constexpr uint32_t kChannels = 3, kRecords = 1, kTerms = 2, kRunPixels = kMomentPixels, kChunk = kMomentChunk;
    static constexpr bool     kTestPerRound = false;
    __device__ static __forceinline__ void values(const float4* rec, float (&v)[4])
    {
        const Vec3 r = load3(rec);
        v[0] = r.x, v[1] = r.y, v[2] = r.z;
    }
    __device__ static __forceinline__ float term(float v, uint32_t i) { return i == 0u ? v : v * v; }
};
struct AovSum // dst0 += {albedo.rgb, coverage}, dst1 += {normal.xyz, depth}: channels 0 .. 7 of the slot's two records
{
    static constexpr uint32_t kChannels = 8, kRecords = 2, kTerms = 1, kRunPixels = kAovPixels, kChunk = kAovChunk;
    // kSumRuns takes the sample-in-chunk test and the permutation entry in EVERY load round, as the AOV kernels did before they were folded: at 320 samples per
    // batch the kernel is bound by how long a run's lines stay cached between chunks, and the shorter load phase of the once-per-chunk form measured 2 % slower
    // there (profiles/sum_kernels), though 12 % faster at 32
    static constexpr bool     kTestPerRound = true;
    __device__ static __forceinline__ void values(const float4* rec, float (&v)[4])
    {
        const float4 r = *rec;
        v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
    }
    __device__ static __forceinline__ float term(float v, uint32_t) { return v; }
};
template<class SUM>
constexpr uint32_t kSumBuffers = (SUM::kChannels + 4u * (SUM::kTerms - 1u) + 3u) / 4u; // dst0 alone, or dst0 and dst1

// One lane per pixel: the pixel's sums in registers, its samples' records in sample-index order wherever the slot order put them.
template<class SUM, bool TILE_LIST>
__global__ __launch_bounds__(kBlock) void kSumPixels(FrameParams fp, const uint32_t* tileIds, const float4* src, float4* dst0, float4* dst1)
{
    constexpr uint32_t RC = SUM::kChannels / SUM::kRecords; // channels per record
    const uint32_t     lp = blockIdx.x * kBlock + threadIdx.x;
    if (lp >= fp.pixelsPadded) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    const size_t at = sumIndex<SUM, TILE_LIST>(tileIds, fp.numTiles, lp);
    float4       sum[kSumBuffers<SUM>]; // the pixel's running sums: float c + 4 i of them is term i of channel c (sumFloat)
#pragma unroll
    for (uint32_t d = 0; d < kSumBuffers<SUM>; ++d) sum[d] = (d == 0u ? dst0 : dst1)[at];
    for (uint32_t k = 0; k < fp.numSamples; ++k)
    {
        const float4* rec = src + SUM::kRecords * samplePixelToSlot(fp, fp.sampleInvPerm ? fp.sampleInvPerm[k] : k, lp);
        float         v[SUM::kRecords][4];
#pragma unroll
        for (uint32_t r = 0; r < SUM::kRecords; ++r) SUM::values(rec + r, v[r]);
#pragma unroll
        for (uint32_t c = 0; c < SUM::kChannels; ++c)
#pragma unroll
            for (uint32_t i = 0; i < SUM::kTerms; ++i) // sample order: one dependent chain of f32 additions per channel and sum
                reinterpret_cast<float*>(sum)[c + 4u * i] += SUM::term(v[c / RC][c % RC], i);
    }
#pragma unroll
    for (uint32_t d = 0; d < kSumBuffers<SUM>; ++d) (d == 0u ? dst0 : dst1)[at] = sum[d];
}

// Pixel-major slot order (slotGroupShift = 0): a pixel's samples are one run of numSamples slots, where the one-lane-per-pixel reads are a gather at a stride of the run.
// One 64-lane workgroup takes kRunPixels pixels.  Per chunk of kChunk samples the 64 lanes read the pixels' records -- 1 KiB per load round, coalesced when the samples
// are not permuted -- and store their values in LDS at the SAMPLE's index; then each summing lane -- one (pixel, channel) -- adds the chunk in sample order onto its
// running sums.  The order is the result, so the additions stay sequential; only the memory traffic changes.
template<class SUM, bool TILE_LIST>
__global__ __launch_bounds__(64) void kSumRuns(FrameParams fp, const uint32_t* tileIds, const float4* src, float4* dst0, float4* dst1)
{
    constexpr uint32_t C = SUM::kChannels, RC = C / SUM::kRecords, PIXELS = SUM::kRunPixels, CHUNK = SUM::kChunk;
    constexpr uint32_t R = CHUNK + 1u;                          // rows padded by one float: the summing lanes walk different banks
    constexpr uint32_t ROUND = 64u / (SUM::kRecords * CHUNK);   // pixels whose chunks one load round of the 64 lanes reads
    __shared__ float   sRun[PIXELS * C * R];                    // [pixel][channel][sample of the chunk]
    static_assert(PIXELS * C <= 64u && ROUND * SUM::kRecords * CHUNK == 64u && PIXELS % ROUND == 0u, "one summing lane per (pixel, channel); whole load rounds");
    const uint32_t S = fp.numSamples, lane = threadIdx.x, lp0 = blockIdx.x * PIXELS;
    const uint32_t px = lane / C, c = lane - C * px, lp = lp0 + px;
    uint32_t       x, y;
    const bool     sums = lane < PIXELS * C && lp < fp.pixelsPadded && localPixelToXY(fp, tileIds, lp, x, y); // (pixels outside the frame: staged, never summed)
    const size_t   at = sums ? sumIndex<SUM, TILE_LIST>(tileIds, fp.numTiles, lp) : 0u;
    float          acc[SUM::kTerms];
#pragma unroll
    for (uint32_t i = 0; i < SUM::kTerms; ++i) acc[i] = sums ? *sumFloat(dst0, dst1, at, c + 4u * i) : 0.0f;
    // loading lane = (pixel of the round, sample of the chunk, record of the slot)
    const uint32_t rec = lane % SUM::kRecords, kk = (lane / SUM::kRecords) % CHUNK;
    const uint32_t pr = ROUND > 1u ? lane / (SUM::kRecords * CHUNK) : 0u; // (one pixel per round: said outright, so that the round's pixel and run offset stay scalar)
    for (uint32_t k0 = 0; k0 < S; k0 += CHUNK)
    {
        const uint32_t n = min(CHUNK, S - k0);
        const auto stage = [&](uint32_t i, uint32_t p) { // load round i: this lane's record of pixel ROUND i + pr, sample k0 + kk (at position p of the run) -> its rows
            const uint32_t pi = ROUND * i + pr;
            float          v[4];
            SUM::values(src + SUM::kRecords * (static_cast<size_t>(lp0 + pi) * S + p) + rec, v);
            float* row = sRun + (pi * C + rec * RC) * R + kk;
#pragma unroll
            for (uint32_t j = 0; j < RC; ++j) row[j * R] = v[j];
        };
        if constexpr (SUM::kTestPerRound)
        {
            for (uint32_t i = 0; i < PIXELS / ROUND; ++i)
            {
                if (kk >= n || lp0 + ROUND * i + pr >= fp.pixelsPadded) continue;
                const uint32_t k = k0 + kk;
                stage(i, fp.sampleInvPerm ? fp.sampleInvPerm[k] : k);
            }
        }
        else if (kk < n)
        {
            const uint32_t k = k0 + kk, p = fp.sampleInvPerm ? fp.sampleInvPerm[k] : k; // sample k sits at position p of the pixel's run
#pragma unroll
            for (uint32_t i = 0; i < PIXELS / ROUND; ++i)
                if (lp0 + ROUND * i + pr < fp.pixelsPadded) stage(i, p);
        }
        __syncthreads();
        if (sums)
        {
            const float* row = sRun + lane * R; // (row lane = pixel px, channel c)
            for (uint32_t j = 0; j < n; ++j)
            {
                const float v = row[j];
#pragma unroll
                for (uint32_t i = 0; i < SUM::kTerms; ++i) acc[i] += SUM::term(v, i); // sample order: one dependent chain of f32 additions per channel and sum
            }
        }
        __syncthreads(); // the next chunk overwrites the rows
    }
    if (!sums) return;
#pragma unroll
    for (uint32_t i = 0; i < SUM::kTerms; ++i) *sumFloat(dst0, dst1, at, c + 4u * i) = acc[i];
}

// The image for the pixel-major slot order, the whole run at once: one wave takes PIXELS pixels, reads their runs coalesced (1 KiB per load) into LDS, then one lane per
// (pixel, channel) adds its samples in sample-index order.  Dynamic LDS: PIXELS * 3 * (numSamples + 1) floats (rows padded by one float: bank-conflict-free sums), so deep
// batches take fewer pixels per workgroup to keep workgroups resident (round 6: 320 spp per batch: 4 pixels = 15 KB, ten workgroups per CU, 3.36 ms; 2 pixels: 2.24 ms;
// 64 spp: 4 pixels 0.37 ms, 2 pixels 0.43: profiles/r06_raygen).  It keeps the argument list it was tuned with (the path streams by value): with the other kernels'
// list the same body compiles to another scalar prologue and measured 1.5 % slower (profiles/sum_kernels).
template<uint32_t PIXELS>
__global__ __launch_bounds__(64) void kAccumulateRuns(FrameParams fp, const uint32_t* tileIds, PathStreams ps, float4* image)
{
    extern __shared__ float sRun[]; // [pixel][channel][sample], rows of S + 1 floats: the twelve lanes that sum walk twelve different banks
    const uint32_t S = fp.numSamples, R = S + 1u, lane = threadIdx.x;
    const uint32_t lp0 = blockIdx.x * PIXELS;
    for (uint32_t px = 0; px < PIXELS; ++px)
    {
        const uint32_t lp = lp0 + px;
        if (lp >= fp.pixelsPadded) break;
        const float4* run = ps.rad + static_cast<size_t>(lp) * S;
        float*        dst = sRun + px * 3u * R;
        for (uint32_t p = lane; p < S; p += 64u)
        {
            // position p of the run holds sample samplePerm[p]: stored at ITS index, so that the sums below walk LDS in order
            const Vec3     v = load3(run + p);
            const uint32_t k = fp.samplePerm ? fp.samplePerm[p] : p;
            dst[k] = v.x;
            dst[R + k] = v.y;
            dst[2u * R + k] = v.z;
        }
    }
    __syncthreads();
    if (lane >= PIXELS * 3u) return;
    const uint32_t px = lane / 3u, c = lane % 3u, lp = lp0 + px;
    if (lp >= fp.pixelsPadded) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    float*       out = reinterpret_cast<float*>(image + lp) + c;
    float        acc = *out;
    const float* src = sRun + (px * 3u + c) * R;
#pragma unroll 8
    for (uint32_t k = 0; k < S; ++k) acc += src[k]; // sample order (wgsl:56-57): one dependent chain of f32 additions per channel
    *out = acc;
}

// ---- The bucket sums: the radiance of sample k of the batch onto plane (phase + k) mod K, K a launch argument.  No lane keeps K accumulators (an array indexed at run
// time would go to scratch): a summing lane owns ONE bucket at a time and visits that bucket's samples, k = first, first + K, ..., in sample order.
// the first sample of [k0, ...) that belongs to bucket b, as an offset from k0: the smallest f >= 0 with (phase + k0 + f) mod K == b
__device__ __forceinline__ uint32_t firstOfBucket(uint32_t b, uint32_t phaseAtK0, uint32_t K) { return b >= phaseAtK0 ? b - phaseAtK0 : b + K - phaseAtK0; }

// Where a pixel's bucket sums live in every plane: the image's place (sumIndex of the radiance sum SUM: RadianceSum, or ShardList<RadianceSum> under a tile shard's
// slot list -- rf_comm_render_adaptive with RF_BUCKETS_SHARD_TILE_COUNTS)
template<class SUM, bool TILE_LIST>
__device__ __forceinline__ size_t bucketIndex(const uint32_t* tileIds, uint32_t numTiles, uint32_t lp) { return sumIndex<SUM, TILE_LIST>(tileIds, numTiles, lp); }

// One lane per pixel, any slot order: plane after plane, each plane's sums in registers while its samples are added.
template<bool TILE_LIST, class SUM = RadianceSum>
__global__ __launch_bounds__(kBlock) void kBucketSumPixels(FrameParams fp, const uint32_t* tileIds, const float4* src, float4* planes, size_t planeStride, uint32_t K,
                                                              uint32_t phase)
{
    const uint32_t lp = blockIdx.x * kBlock + threadIdx.x;
    if (lp >= fp.pixelsPadded) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    const size_t at = bucketIndex<SUM, TILE_LIST>(tileIds, fp.numTiles, lp);
    for (uint32_t b = 0; b < K; ++b)
    {
        const uint32_t first = firstOfBucket(b, phase, K);
        if (first >= fp.numSamples) continue; // (a batch shorter than K: this plane gets no sample)
        float4* const dst = planes + b * planeStride + at;
        float4        sum = *dst;
        for (uint32_t k = first; k < fp.numSamples; k += K)
        {
            const float4 r = src[samplePixelToSlot(fp, fp.sampleInvPerm ? fp.sampleInvPerm[k] : k, lp)];
            sum.x += r.x, sum.y += r.y, sum.z += r.z; // sample order: one dependent chain of f32 additions per channel and bucket
        }
        *dst = sum;
    }
}

// Pixel-major slot order, patterned on kSumRuns: a 64-lane workgroup takes kBucketPixels pixels, stages their radiance in LDS in chunks of kBucketChunk samples (two
// coalesced load rounds of 1 KiB), then the summing slots -- slot = (pixel, channel) * K + bucket, kBucketPixels * 3 * K <= 180 of them, up to three per lane at fixed
// register positions -- each walk their row from their bucket's first sample of the chunk at stride K.
template<bool TILE_LIST, class SUM = RadianceSum>
__global__ __launch_bounds__(64) void kBucketSumRuns(FrameParams fp, const uint32_t* tileIds, const float4* src, float4* planes, size_t planeStride, uint32_t K, uint32_t phase)
{
    constexpr uint32_t PIXELS = kBucketPixels, CHUNK = kBucketChunk, R = CHUNK + 1u, ROUND = 64u / CHUNK, ROWS = PIXELS * 3u;
    constexpr uint32_t SLOTS = (ROWS * kMaxBuckets + 63u) / 64u; // summing slots per lane
    __shared__ float   sRun[ROWS * R];                           // [pixel][channel][sample of the chunk]
    static_assert(ROUND * CHUNK == 64u && PIXELS % ROUND == 0u, "whole load rounds");
    const uint32_t S = fp.numSamples, lane = threadIdx.x, lp0 = blockIdx.x * PIXELS;
    // slot s of this lane: row = (pixel, channel), bucket, where its running sum lives
    uint32_t row[SLOTS], bucket[SLOTS];
    float*   out[SLOTS];
    float    acc[SLOTS];
#pragma unroll
    for (uint32_t s = 0; s < SLOTS; ++s)
    {
        const uint32_t slot = lane + 64u * s;
        row[s] = slot / K, bucket[s] = slot - row[s] * K;
        const uint32_t px = row[s] / 3u, c = row[s] - 3u * px, lp = lp0 + px;
        uint32_t       x, y;
        const bool     sums = row[s] < ROWS && lp < fp.pixelsPadded && localPixelToXY(fp, tileIds, lp, x, y); // (pixels outside the frame: staged, never summed)
        out[s] = sums ? reinterpret_cast<float*>(planes + bucket[s] * planeStride + bucketIndex<SUM, TILE_LIST>(tileIds, fp.numTiles, lp)) + c : nullptr;
        acc[s] = sums ? *out[s] : 0.0f;
    }
    const uint32_t kk = lane % CHUNK, pr = lane / CHUNK; // loading lane = (pixel of the round, sample of the chunk)
    for (uint32_t k0 = 0; k0 < S; k0 += CHUNK)
    {
        const uint32_t n = min(CHUNK, S - k0);
        if (kk < n)
        {
            const uint32_t k = k0 + kk, p = fp.sampleInvPerm ? fp.sampleInvPerm[k] : k; // sample k sits at position p of the pixel's run
#pragma unroll
            for (uint32_t i = 0; i < PIXELS / ROUND; ++i)
            {
                const uint32_t pi = ROUND * i + pr;
                if (lp0 + pi >= fp.pixelsPadded) continue;
                const float4 r = src[static_cast<size_t>(lp0 + pi) * S + p];
                float*       dst = sRun + pi * 3u * R + kk;
                dst[0] = r.x, dst[R] = r.y, dst[2u * R] = r.z;
            }
        }
        __syncthreads();
        const uint32_t phaseAtK0 = (phase + k0) % K;
#pragma unroll
        for (uint32_t s = 0; s < SLOTS; ++s)
        {
            if (out[s] == nullptr) continue;
            const float* run = sRun + row[s] * R;
            for (uint32_t j = firstOfBucket(bucket[s], phaseAtK0, K); j < n; j += K) acc[s] += run[j]; // sample order: one dependent chain of f32 additions per channel and bucket
        }
        __syncthreads(); // the next chunk overwrites the rows
    }
#pragma unroll
    for (uint32_t s = 0; s < SLOTS; ++s)
        if (out[s] != nullptr) *out[s] = acc[s];
}
} // namespace

SumKernel sumKernel(Sum sum, bool runs, SumAddressing addressing)
{
    const bool tileList = addressing == SumAddressing::TileList;
    if (addressing == SumAddressing::ShardList)
    {
        if (sum == Sum::RadianceMoments) return runs ? kSumRuns<ShardList<RadianceMomentSum>, true> : kSumPixels<ShardList<RadianceMomentSum>, true>;
        if (sum == Sum::Aov) return runs ? kSumRuns<ShardList<AovSum>, true> : kSumPixels<ShardList<AovSum>, true>;
        if (sum == Sum::Radiance) return runs ? kSumRuns<ShardList<RadianceSum>, true> : kSumPixels<ShardList<RadianceSum>, true>;
        throw std::logic_error("sumKernel: no such kernel is compiled");
    }
    if (sum == Sum::Radiance && !runs && !tileList) return kSumPixels<RadianceSum, false>;
    if (sum == Sum::Radiance && tileList) return runs ? kSumRuns<RadianceSum, true> : kSumPixels<RadianceSum, true>;
    if (sum == Sum::Moments && !tileList) return runs ? kSumRuns<MomentSum, false> : kSumPixels<MomentSum, false>;
    if (sum == Sum::RadianceMoments && tileList) return runs ? kSumRuns<RadianceMomentSum, true> : kSumPixels<RadianceMomentSum, true>;
    if (sum == Sum::Aov && tileList) return runs ? kSumRuns<AovSum, true> : kSumPixels<AovSum, true>;
    if (sum == Sum::Aov) return runs ? kSumRuns<AovSum, false> : kSumPixels<AovSum, false>;
    throw std::logic_error("sumKernel: no such kernel is compiled");
}
BucketKernel bucketKernel(bool runs, SumAddressing addressing)
{
    if (addressing == SumAddressing::ShardList) return runs ? kBucketSumRuns<true, ShardList<RadianceSum>> : kBucketSumPixels<true, ShardList<RadianceSum>>;
    if (addressing == SumAddressing::TileList) return runs ? kBucketSumRuns<true> : kBucketSumPixels<true>;
    return runs ? kBucketSumRuns<false> : kBucketSumPixels<false>;
}
AccumulateRunsKernel accumulateRunsKernel(uint32_t pixels) { return pixels == 1u ? kAccumulateRuns<1> : pixels == 2u ? kAccumulateRuns<2> : kAccumulateRuns<kAccPixels>; }
} // namespace rf
