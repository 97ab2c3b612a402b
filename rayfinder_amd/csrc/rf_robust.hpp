// rf_robust.hpp -- the firefly-robust mean over the bucket sums (rf_robust.hip; the definition: include/rayfinder_amd.h, "Bucket sums and the robust mean"): its
// device buffers and its launch sequence, shared by the renderer's rf_renderer_robust_mean (inputs: the handle's own compact tile-major bucket planes) and the
// standalone rf_robust_mean_images (inputs: row-major planes).
#pragma once

#include "rf_frame_sums.hpp"
#include "rf_hip_host.hpp"
#include "rf_renderer.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rf
{
struct RobustWork
{
    DeviceBuffer<float4>   mean; // M = {rgb, 1}, row-major
    DeviceBuffer<uint8_t>  trim; // c of every pixel, row-major
    DeviceBuffer<uint32_t> bgra; // kTonemap of `mean` (accumulatedSamples = 1)

    // room for `pixels` in every buffer (stream-synchronises before it frees a smaller set)
    void reserve(uint64_t pixels, hipStream_t stream);
    void release();
};

// Enqueue kRobustMean<K> and kTonemap on `stream`.  planes: K planes of planeStride float4 each, every one laid out as `frame` says (rf_frame_sums.hpp: its size,
// layout and counts are used, its five planes are not).  K odd, 3 .. 15; frame.samples >= K.
// frame.tileSamples (every count >= K) != nullptr: every pixel is combined with its tile's count (kRobustMeanTiles<K>).
void enqueueRobustMean(hipStream_t stream, RobustWork& work, const float4* planes, size_t planeStride, uint32_t K, const FrameSums& frame, float exposure);

// A tile shard's own combine ahead of the frame gather: enqueue kRobustMeanShard<K> on `stream` over the shard-compact tile-major planes (K planes of planeStride float4
// each, shardTiles * 1024 pixels used, one count `samples` >= K) -> out[i] = {M.rgb, float(c)} in the same layout (shardTiles * 1024 float4).  Nothing is enqueued
// for an empty shard.  slotCounts (device, one count >= K per slot of the shard) != nullptr: every pixel is combined with its slot's count
// (kRobustMeanShardTiles<K>) and `samples` is not used; the buffer must stay as it is until the stream has run the kernel.
void enqueueRobustMeanShard(hipStream_t stream, const float4* planes, size_t planeStride, uint32_t shardTiles, uint32_t K, uint32_t samples, float4* out,
                            const uint32_t* slotCounts = nullptr);
// kTonemap over a row-major mean image M (accumulatedSamples = 1): the robust mean's display texels
void enqueueRobustTexels(hipStream_t stream, const float4* mean, uint32_t pixels, float exposure, uint32_t* bgra);
} // namespace rf
