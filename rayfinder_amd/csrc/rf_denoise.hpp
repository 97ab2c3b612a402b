// rf_denoise.hpp -- the edge-aware a-trous denoiser's device work buffers and its launch sequence (rf_denoise.hip), shared by the renderer's
// rf_renderer_denoise (inputs: the handle's own compact tile-major sums) and the standalone rf_denoise_images (inputs: row-major sums).
#pragma once

#include "rf_renderer.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rf
{
struct DenoiseWork
{
    float4*   e[2] = {};          // ping-pong demodulated irradiance {e.rgb, ℓ}
    float4*   guide = nullptr;    // {n.xyz, z}; z <= 0 (or NaN): background
    float4*   albedo = nullptr;   // {a + εa, 0}
    float4*   out = nullptr;      // the denoised mean {rgb, 1}
    uint32_t* bgra = nullptr;     // kTonemap of `out` (accumulatedSamples = 1)
    uint64_t  pixels = 0;         // capacity

    // room for `pixels` (stream-synchronises before it frees a smaller set)
    void reserve(uint64_t pixels, hipStream_t stream);
    void release();
    ~DenoiseWork() { release(); }
};

// Enqueue kDenoisePrep, the L kDenoiseAtrous passes and kTonemap on `stream`.  tilesX != 0: the sums are compact tile-major buffers holding every tile of the
// frame in tile order (a handle without a tile shard), tilesX tiles per row; 0: row-major.  width * height < 2^31; the parameters are valid.
void enqueueDenoise(hipStream_t stream, DenoiseWork& work, const float4* colorSum, const float4* albedoCoverage, const float4* normalDepth, uint32_t width,
                    uint32_t height, uint32_t tilesX, uint32_t samples, const DenoiseParameters& params, float exposure);
} // namespace rf
