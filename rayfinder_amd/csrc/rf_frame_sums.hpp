// rf_frame_sums.hpp -- "the sums of one frame", as every post-process pass reads them (the denoisers, the noise estimate, the robust mean, the feature export, the
// temporal history), and the staging of the stand-alone *Images / *Tiles calls, which bring host-assembled planes to the device for one pass.  Each owner of sums
// describes them once: the renderer handle (Renderer::Impl::frameSums: its own compact tile-major buffers), TileComm (Impl::gathered: the row-major planes on the
// gather's root) and StagedFrame (row-major, uploaded).  Host code only.
#pragma once

#include "rf_hip_host.hpp"
#include "rf_renderer.hpp" // TileGrid

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rf
{
// The sums of one frame in device memory, all in one layout; a plane the pass does not read may be nullptr.
struct FrameSums
{
    const float4 *  colorSum = nullptr, *sumSq = nullptr, *albedoCoverage = nullptr, *normalDepth = nullptr, *directSum = nullptr;
    uint32_t        width = 0, height = 0; // width * height < 2^31
    uint32_t        tilesX = 0;            // != 0: compact tile-major buffers holding every tile of the frame in tile order (a handle without a tile shard), tilesX tiles per row; 0: row-major
    uint32_t        samples = 0;           // the count of every pixel, unless tileSamples says otherwise
    // device, one count per tile of the frame's 32 x 32 grid (tile_y * ceil(width / 32) + tile_x); nullptr: `samples` for every pixel.  A pass that takes it does not
    // use `samples`; the buffer must stay as it is until the stream has run the pass.
    const uint32_t* tileSamples = nullptr;
};

// One stand-alone call's stream and inputs: makes `deviceOrdinal` current, uploads the row-major host planes that are given (a null plane is skipped and stays
// nullptr in `sums`) and the per-tile counts (null: one count, `samples`), all asynchronously on a stream of its own.  The ordering every such call relies on: the
// stream is drained before anything the pass used is freed, however the scope is left.  The members below go in that order (the Drain first); what the CALLER
// owns -- the pass's work struct, further buffers -- is declared BEFORE the StagedFrame, so that it is freed after it.
struct StagedFrame
{
    ScopedStream           stream;
    DeviceBuffer<float4>   planes[5];
    DeviceBuffer<uint32_t> counts;
    ScopedStream::Drain    drain{stream};
    FrameSums              sums;

    StagedFrame(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const uint32_t* tileSamples, const float* colorSum, const float* sumSq,
                const float* albedoCoverage, const float* normalDepth, const float* directSum)
        : stream(deviceOrdinal)
    {
        const float* const src[5] = {colorSum, sumSq, albedoCoverage, normalDepth, directSum};
        for (int b = 0; b < 5; ++b)
            if (src[b]) upload(planes[b], reinterpret_cast<const float4*>(src[b]), static_cast<uint64_t>(width) * height);
        if (tileSamples) upload(counts, tileSamples, TileGrid(width, height).count());
        sums = FrameSums{planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, planes[4].ptr, width, height, 0u, samples, counts.ptr};
    }

    uint64_t pixels() const { return static_cast<uint64_t>(sums.width) * sums.height; }
    // a further input of the call: `count` elements of host memory into a buffer the caller owns (declared before this)
    template<typename T>
    void upload(DeviceBuffer<T>& dst, const T* srcHost, uint64_t count)
    {
        dst.alloc(count);
        RF_HIP(hipMemcpyAsync(dst.ptr, srcHost, count * sizeof(T), hipMemcpyHostToDevice, stream.handle));
    }
    // a result: `bytes` of device memory to dstHost, unless that is null
    void download(void* dstHost, const void* srcDevice, uint64_t bytes)
    {
        if (dstHost) RF_HIP(hipMemcpyAsync(dstHost, srcDevice, bytes, hipMemcpyDeviceToHost, stream.handle));
    }
    void wait() { RF_HIP(hipStreamSynchronize(stream.handle)); }
};
} // namespace rf
