// rf_sums.hpp -- the per-pixel sums in sample order (rf_sums.hip): every kernel that adds a batch's per-slot records onto a running sum of the handle -- the image S,
// the radiance second moments Q, the two first-hit AOV sums, the K bucket sums -- and the constants of their launches.  The host (planBatch, rf_launch_policy.cpp / Impl::enqueueSums) picks a
// kernel by (sum, LDS-staged or one lane per pixel, shard-compact or tile-list addressing) and launches them with one argument list; the headline image kernel and the
// bucket kernels (K planes, a phase) keep their own.
#pragma once

#include "rf_kernels.hpp"
#include "rf_launch_constants.hpp"

namespace rf
{
// What a launch adds.  Each channel of each sum is ONE dependent chain of f32 additions in sample-index order (Q's term: one f32 multiply of the loaded value with
// itself), no atomics, no contraction: the bit-exactness contract of the sums.
enum class Sum : uint32_t
{
    Radiance,        // dst0 = S: += r.rgb of src[slot]
    Moments,         // dst0 = Q: += {r.x r.x, r.y r.y, r.z r.z} of src[slot]
    RadianceMoments, // dst0 = S, dst1 = Q, from one read of src[slot] (tile-adaptive sampling)
    Aov,             // dst0 += {albedo.rgb, coverage} = src[2 slot], dst1 += {normal.xyz, depth} = src[2 slot + 1] (kShade<false, true>'s records of bounce 1)
};
// src: the batch's per-slot records; dst0 / dst1: the handle's sums, compact tile-major (dst1 unused by the sums that have one buffer).  The sums of local pixel lp
// sit at lp -- or, tileList (rf_renderer_render_adaptive: the batch's path slots belong to the fp.numTiles tiles that tileIds lists, the sums hold the WHOLE frame,
// compact slot == tile id), at tileIds[lp >> 10] * 1024 + (lp & 1023) -- or, shardList (rf_comm_render_adaptive: the same under a tile shard, the sums hold the
// SHARD; tileIds holds the fp.numTiles listed tile ids and behind them the tiles' slots in the shard), at tileIds[fp.numTiles + (lp >> 10)] * 1024 + (lp & 1023).
// The sums of pixels outside the frame are neither read nor written.
using SumKernel = void (*)(FrameParams fp, const uint32_t* tileIds, const float4* src, float4* dst0, float4* dst1);

// runs: the LDS-staged kernel for the pixel-major slot order (slotGroupShift 0), a 64-lane workgroup per kMomentPixels (Moments, RadianceMoments) or kAovPixels (Aov)
// pixels, their runs staged in chunks of 32 samples: (pixels x channels) rows of (32 + 1) floats = 6 336 B / 8 448 B of LDS at any batch depth (<= ~8 KB keeps twenty
// workgroups resident per CU, profiles/r06_raygen).  Else one lane per pixel, kBlock pixels per workgroup, any slot order.
// Compiled: Radiance (one lane per pixel; its staged kernel is accumulateRunsKernel) and Moments with shard-compact addressing, RadianceMoments with a tile list, Aov
// with both, RadianceMoments and Aov with a shard's slot list; Radiance with a tile list and with a shard's slot list in both forms (the direct sums D under
// RF_DIRECT_TILE_COUNTS: the staged form takes kMomentPixels pixels in chunks of kMomentChunk, 6 336 B of LDS); anything else throws.
constexpr uint32_t kMomentChunk = 32, kAovChunk = 32; // (kMomentPixels, kAovPixels: rf_launch_constants.hpp)
enum class SumAddressing : uint32_t
{
    Compact,   // the sums of local pixel lp at lp
    TileList,  // a tile list over a whole-frame handle
    ShardList, // a tile list over a tile shard: ids, then slots
};
SumKernel sumKernel(Sum sum, bool runs, SumAddressing addressing);

// Radiance, pixel-major slot order, the WHOLE run in LDS: pixelsPerWorkgroup (1, 2 or kAccPixels) x 3 x (numSamples + 1) floats of dynamic LDS, numSamples <= kAccMaxSamples;
// the image sits at lp (no tile list).  Its source is ps.rad
// (kAccPixels, kAccMaxSamples: rf_launch_constants.hpp)
using AccumulateRunsKernel = void (*)(FrameParams fp, const uint32_t* tileIds, PathStreams ps, float4* image);
AccumulateRunsKernel accumulateRunsKernel(uint32_t pixelsPerWorkgroup);

// The bucket sums (rf_renderer_set_buckets): K planes of `planeStride` float4 each, one after another, every plane laid out like the image (shard-compact, the sums of
// local pixel lp at lp).  Sample k of the batch is added to plane (phase + k) mod K, phase = (the bucket sample count before the batch) mod K < K: plane b holds
// {sum r.x, sum r.y, sum r.z, 0} over the samples of ordinal b mod K, each channel of each plane one dependent chain of f32 additions in sample order -- the contract above.
// 3 <= K <= kMaxBuckets.  runs: the LDS-staged kernel for the pixel-major slot order, a 64-lane workgroup per kBucketPixels pixels, their runs staged in chunks of
// kBucketChunk samples (kBucketPixels x 3 rows of kBucketChunk + 1 floats = 1 584 B of LDS), one summing lane per (pixel, channel, bucket) walking its row at stride K;
// else one lane per pixel (kBlock per workgroup, any slot order), plane after plane.  Its source is ps.rad.
// tileList (rf_renderer_render_adaptive with RF_BUCKETS_TILE_COUNTS): the batch's path slots belong to the fp.numTiles tiles that tileIds lists and every plane holds
// the WHOLE frame: the sums of local pixel lp sit at tileIds[lp >> 10] * 1024 + (lp & 1023) of every plane, as the other sums' do.  All listed tiles share one bucket
// sample count, so one phase serves the launch; a batch shorter than K leaves the planes it does not reach untouched.
// shardList (rf_comm_render_adaptive with RF_BUCKETS_SHARD_TILE_COUNTS): the same under a tile shard, every plane holds the SHARD and the sums of local pixel lp sit at
// tileIds[fp.numTiles + (lp >> 10)] * 1024 + (lp & 1023) of it.  A rank's active tiles all sit at the frame's leading count, which is that rank's bucket sample count:
// one phase serves the launch there too.
constexpr uint32_t kMaxBuckets = 15, kBucketChunk = 32; // (kBucketPixels: rf_launch_constants.hpp)
using BucketKernel = void (*)(FrameParams fp, const uint32_t* tileIds, const float4* src, float4* planes, size_t planeStride, uint32_t K, uint32_t phase);
BucketKernel bucketKernel(bool runs, SumAddressing addressing);
} // namespace rf
