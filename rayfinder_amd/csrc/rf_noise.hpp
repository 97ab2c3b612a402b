// rf_noise.hpp -- the noise estimate over the radiance sum and its second moments (rf_noise.hip; the sums themselves: rf_sums.hpp): the launch sequence of the
// estimate, shared by rf_renderer_noise_estimate (inputs: the handle's own compact tile-major sums), rf_comm_noise_estimate (the planes gathered on the root) and the
// standalone rf_noise_estimate_images (inputs: row-major sums) -- each hands in its FrameSums --, and the per-tile mean.
#pragma once

#include "rf_frame_sums.hpp"
#include "rf_kernels.hpp"

namespace rf
{
// mean[i] = {S.rgb / float(count), 1} over n compact tile-major pixels; count = tileSamples[i >> 10], or `samples` for all when tileSamples is nullptr; count 0: rgb 0
using TileMeanKernel = void (*)(const float4* image, const uint32_t* tileSamples, uint32_t samples, uint32_t n, float4* mean);
TileMeanKernel tileMeanKernel();
// The same over a row-major width x height frame (width * height < 2^31), enqueued on `stream`: tileSamples has one count per tile of the frame's 32 x 32 grid
void enqueueTileMeanRows(hipStream_t stream, const float4* image, const uint32_t* tileSamples, uint32_t width, uint32_t height, float4* mean);
// The direct and the indirect component of a row-major width x height frame (width * height < 2^31) from its sums S (`image`) and D, one launch of kSplitMeanRows on
// `stream`: direct[i] = {D.rgb / float(n), 1}, indirect[i] = {(S.rgb - D.rgb) / float(n), 1}; n = the pixel's tile's count (tileSamples as above) or, tileSamples ==
// nullptr, `samples`; n = 0: {0, 0, 0, 1} for both
void enqueueSplitMeanRows(hipStream_t stream, const float4* image, const float4* directSum, const uint32_t* tileSamples, uint32_t samples, uint32_t width, uint32_t height,
                          float4* direct, float4* indirect);

// Device buffers of one estimate: per-tile {sum, max} and {pixels, non-finite pixels}, and the row-major error map (only when a caller asks for it)
struct NoiseWork
{
    DeviceBuffer<float>    tileSumMax; // [tiles] sums, then [tiles] maxima
    DeviceBuffer<uint32_t> tileCounts; // [tiles] in-frame pixels, then [tiles] non-finite pixels
    DeviceBuffer<float>    errorMap;   // width * height
    uint64_t               tiles = 0;  // capacity in tiles (the map's: errorMap.count)

    // room for `tiles` tiles and, if wanted, a map of `pixels` (stream-synchronises before it frees a smaller set)
    void reserve(uint64_t tiles, uint64_t mapPixels, hipStream_t stream);
    void release();
};

// Enqueue the estimate over the frame's S and Q (rf_frame_sums.hpp) on `stream`, copy the per-tile results (and the map) back, wait, and reduce them on the host (the
// definition: include/rayfinder_amd.h).  sums.samples >= 2; with sums.tileSamples (kNoiseEstimateTiles; without: kNoiseEstimate) every count >= 2, and the result's
// `samples` still reports sums.samples.  errorMap (width * height), tileSum, tileMax (one entry per tile of the 32 x 32 grid): host pointers, NULL = skip.
NoiseEstimate runNoiseEstimate(hipStream_t stream, NoiseWork& work, const FrameSums& sums, float* errorMap, float* tileSum, float* tileMax);

// Which tiles an estimate covers.  listDevice / listHost: the same ascending list of listCount tile ids (nullptr: every tile of the frame).
// slotsBehindList: the sums are the compact tile-major buffers of a tile SHARD, and listDevice holds, behind the listCount ids, each listed tile's slot in them
// (tile-major, a list and no per-tile counts: rf_comm_render_adaptive's estimate).
struct TileSelection
{
    const uint32_t* listDevice = nullptr;
    const uint32_t* listHost = nullptr;
    uint32_t        listCount = 0;
    bool            slotsBehindList = false;
};
// runNoiseEstimate for a selection: the result's mean, maximum and counts are over the listed tiles (worst_tile in the frame's numbering).  tilePixels (host, one entry
// per tile of the frame, NULL = skip): in-frame pixels.  With a list, only the listed tiles' entries of tileSum / tileMax / tilePixels and of the map are written.
NoiseEstimate runNoiseEstimateTiles(hipStream_t stream, NoiseWork& work, const FrameSums& sums, const TileSelection& selection, float* errorMap, float* tileSum,
                                    float* tileMax, uint32_t* tilePixels);
} // namespace rf
