// rf_temporal.hpp -- the temporal history (rf_temporal.hip; the definition: include/rayfinder_amd.h, "Temporal history"): the previous view's frame reprojected into
// the current camera and blended behind the current view's samples.  Its device buffers and its one launch, shared by the renderer's rf_renderer_temporal_accumulate
// (inputs: the handle's own compact tile-major sums) and the standalone rf_temporal_images (inputs: row-major planes).
#pragma once

#include "rf_frame_sums.hpp"
#include "rf_hip_host.hpp"
#include "rf_renderer.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rf
{
// Two pairs of row-major planes -- T = {mean colour rgb, effective sample count}, G = {unit normal xyz, depth; 0: background} -- and the result's texels.  Which
// pair holds the result and which the history is an index: a commit swaps the roles, no plane is copied.  Whether either is VALID is the books' business
// (AccumulationBooks::temporalValid / temporalHistory).
struct TemporalWork
{
    DeviceBuffer<float4>   color[2], geometry[2];
    DeviceBuffer<uint32_t> bgra;        // kTonemap's texels of color[result] (accumulatedSamples = 1)
    uint32_t               result = 0;  // the pair the next accumulate writes; the history is the other one
    Camera                 camera[2]{}; // the camera each pair was made with

    uint32_t history() const { return result ^ 1u; }
    void     commit() { result ^= 1u; }
    // room for `pixels` in every buffer.  A set of another size is freed first (the stream is waited for): the caller has dropped whatever it held.
    void     reserve(uint64_t pixels, hipStream_t stream);
    void     release();
    uint64_t bytes() const { return (color[0].count + color[1].count + geometry[0].count + geometry[1].count) * sizeof(float4) + bgra.count * sizeof(uint32_t); }
};

// Enqueue kTemporalReproject on `stream` over the frame's S, AC and ND (rf_frame_sums.hpp; one count, sums.samples > 0: tileSamples is not read): prep, reprojection,
// blend and the texel of every pixel in one pass.  histColor / histGeometry / histCamera: all nullptr (no history) or all given; the outputs are row-major and all
// given.  The parameters are valid.
void enqueueTemporal(hipStream_t stream, const FrameSums& sums, const Camera& camera, const float4* histColor, const float4* histGeometry, const Camera* histCamera,
                     const TemporalParameters& params, float exposure, float4* outColor, float4* outGeometry, uint32_t* outBgra);
} // namespace rf
