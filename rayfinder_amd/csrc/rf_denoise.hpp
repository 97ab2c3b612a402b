// rf_denoise.hpp -- the edge-aware a-trous denoiser's device work buffers and its launch sequence (rf_denoise.hip), shared by the renderer's
// rf_renderer_denoise (inputs: the handle's own compact tile-major sums) and the standalone rf_denoise_images (inputs: row-major sums).
#pragma once

#include "rf_hip_host.hpp"
#include "rf_renderer.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rf
{
struct DenoiseWork
{
    DeviceBuffer<float4>   e[2];   // ping-pong demodulated irradiance {e.rgb, ℓ}
    DeviceBuffer<float4>   guide;  // {n.xyz, z}; z <= 0 (or NaN): background
    DeviceBuffer<float4>   albedo; // {a + εa, 0}
    DeviceBuffer<float4>   out;    // the denoised mean {rgb, 1}
    DeviceBuffer<uint32_t> bgra;   // kTonemap of `out` (accumulatedSamples = 1)
    DeviceBuffer<float4>   eI[2];  // the split-component filter's second ping-pong pair, the indirect component's {e.rgb, ℓ} (e[] then holds the direct one's); empty
                                   // until the first split run

    // room for `pixels` in every buffer (stream-synchronises before it frees a smaller set); split: in eI[] as well.  Whatever has to grow, the whole set is freed
    // and allocated again in one go.
    void reserve(uint64_t pixels, hipStream_t stream, bool split = false);
};

// Enqueue kDenoisePrep, the L kDenoiseAtrous passes and kTonemap on `stream`.  tilesX != 0: the sums are compact tile-major buffers holding every tile of the
// frame in tile order (a handle without a tile shard), tilesX tiles per row; 0: row-major.  width * height < 2^31; the parameters are valid.
// tileSamples (device, one count > 0 per tile of the frame's 32 x 32 grid, tile_y * ceil(width / 32) + tile_x) != nullptr: prep divides each pixel by its tile's
// count (kDenoisePrepTiles) and `samples` is not used; the buffer must stay as it is until the stream has run the prep.
// mean (device, row-major width * height) != nullptr: prep takes c = mean.rgb instead of colorSum.rgb / Nf (kDenoisePrepMean: rf_renderer_denoise_robust hands in
// the robust mean; with tileSamples, kDenoisePrepMeanTiles: the AOV sums are divided by each pixel's tile's count); colorSum is not read.
void enqueueDenoise(hipStream_t stream, DenoiseWork& work, const float4* colorSum, const float4* albedoCoverage, const float4* normalDepth, uint32_t width,
                    uint32_t height, uint32_t tilesX, uint32_t samples, const DenoiseParameters& params, float exposure, const uint32_t* tileSamples = nullptr,
                    const float4* mean = nullptr);

// The split-component filter (rf_renderer_denoise_split): kDenoisePrepSplit, max(L_D, L_I) kDenoiseAtrousSplit passes -- the last one adds the components and
// remodulates -- and kTonemap on `stream`; the result in work.out / work.bgra as enqueueDenoise leaves it.  directSum: D, laid out like colorSum.  tilesX as above.
// tileSamples as above: prep divides S, D and the AOV sums of each pixel by its tile's count (kDenoisePrepSplitTiles) and `samples` is not used.
void enqueueDenoiseSplit(hipStream_t stream, DenoiseWork& work, const float4* colorSum, const float4* directSum, const float4* albedoCoverage, const float4* normalDepth,
                         uint32_t width, uint32_t height, uint32_t tilesX, uint32_t samples, const DenoiseParameters& direct, const DenoiseParameters& indirect,
                         float exposure, const uint32_t* tileSamples = nullptr);
} // namespace rf
