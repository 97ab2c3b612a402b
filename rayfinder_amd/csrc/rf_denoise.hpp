// rf_denoise.hpp -- the edge-aware a-trous denoiser's device work buffers and its launch sequence (rf_denoise.hip), shared by the renderer's
// rf_renderer_denoise (inputs: the handle's own compact tile-major sums), rf_comm_denoise (the planes gathered on the root) and the standalone rf_denoise_images
// (inputs: row-major sums) -- each hands in its FrameSums.
#pragma once

#include "rf_frame_sums.hpp"
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

// Enqueue kDenoisePrep, the L kDenoiseAtrous passes and kTonemap on `stream` over the frame's S, AC and ND (rf_frame_sums.hpp); the parameters are valid.
// sums.tileSamples (every count > 0) != nullptr: prep divides each pixel by its tile's count (kDenoisePrepTiles).
// mean (device, row-major width * height) != nullptr: prep takes c = mean.rgb instead of colorSum.rgb / Nf (kDenoisePrepMean: rf_renderer_denoise_robust hands in
// the robust mean; with tileSamples, kDenoisePrepMeanTiles: the AOV sums are divided by each pixel's tile's count); colorSum is not read.
void enqueueDenoise(hipStream_t stream, DenoiseWork& work, const FrameSums& sums, const DenoiseParameters& params, float exposure, const float4* mean = nullptr);

// The split-component filter (rf_renderer_denoise_split) over the frame's S, D, AC and ND: kDenoisePrepSplit, max(L_D, L_I) kDenoiseAtrousSplit passes -- the last
// one adds the components and remodulates -- and kTonemap on `stream`; the result in work.out / work.bgra as enqueueDenoise leaves it.
// sums.tileSamples as above: prep divides S, D and the AOV sums of each pixel by its tile's count (kDenoisePrepSplitTiles).
void enqueueDenoiseSplit(hipStream_t stream, DenoiseWork& work, const FrameSums& sums, const DenoiseParameters& direct, const DenoiseParameters& indirect, float exposure);
} // namespace rf
