// rf_noise.hpp -- the noise estimate over the radiance sum and its second moments (rf_noise.hip; the sums themselves: rf_sums.hpp): the launch sequence of the
// estimate, shared by rf_renderer_noise_estimate (inputs: the handle's own compact tile-major sums) and the standalone rf_noise_estimate_images (inputs: row-major
// sums), and the per-tile mean.
#pragma once

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

// Enqueue kNoiseEstimate on `stream`, copy the per-tile results (and the map) back, wait, and reduce them on the host (the definition: include/rayfinder_amd.h).
// tileMajor: the sums are compact tile-major buffers holding every tile of the frame in tile order (a handle without a tile shard); else row-major.
// errorMap (width * height), tileSum, tileMax (one entry per tile of the 32 x 32 grid): host pointers, NULL = skip.  samples >= 2, width * height < 2^31.
NoiseEstimate runNoiseEstimate(hipStream_t stream, NoiseWork& work, const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, bool tileMajor,
                               uint32_t samples, float* errorMap, float* tileSum, float* tileMax);

// Which tiles an estimate covers and with what counts.  listDevice / listHost: the same ascending list of listCount tile ids (nullptr: every tile of the frame);
// tileSamplesDevice: one sample count per tile of the frame, each >= 2 (nullptr: `samples` for all).  Both nullptr: kNoiseEstimate itself.
// slotsBehindList: the sums are the compact tile-major buffers of a tile SHARD, and listDevice holds, behind the listCount ids, each listed tile's slot in them
// (tile-major, a list and no per-tile counts: rf_comm_render_adaptive's estimate).
struct TileSelection
{
    const uint32_t* listDevice = nullptr;
    const uint32_t* listHost = nullptr;
    uint32_t        listCount = 0;
    const uint32_t* tileSamplesDevice = nullptr;
    bool            slotsBehindList = false;
};
// runNoiseEstimate for a selection: the result's mean, maximum and counts are over the listed tiles (worst_tile in the frame's numbering).  tilePixels (host, one entry
// per tile of the frame, NULL = skip): in-frame pixels.  With a list, only the listed tiles' entries of tileSum / tileMax / tilePixels and of the map are written.
NoiseEstimate runNoiseEstimateTiles(hipStream_t stream, NoiseWork& work, const float4* colorSum, const float4* sumSq, uint32_t width, uint32_t height, bool tileMajor,
                                    const TileSelection& selection, uint32_t samples, float* errorMap, float* tileSum, float* tileMax, uint32_t* tilePixels);
} // namespace rf
