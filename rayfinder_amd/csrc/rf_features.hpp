// rf_features.hpp -- the feature export (rf_features.hip; the definition: include/rayfinder_amd.h, "Feature export"): the per-pixel feature channels of a frame's sums
// -- means, first-hit guides, the variance of the mean, the noise estimate's error, the sample count -- written as one planar (CHW) or interleaved (HWC) f32 / f16
// tensor into caller-owned device memory.  Shared by rf_renderer_export_features (the handle's own compact tile-major sums), rf_comm_export_features (the row-major
// planes gathered on the root) and the standalone rf_export_features_images (host-assembled row-major sums).
#pragma once

#include "rf_feature_request.hpp"
#include "rf_frame_sums.hpp"
#include "rf_hip_host.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rf
{
// std::invalid_argument unless hipPointerGetAttributes reports `dst` as device memory of device `deviceOrdinal` (a host pointer, registered or managed memory and
// another device's memory are all refused), or when `bytes` is smaller than `needed`.  No launch.
void requireFeatureDestination(const void* dst, uint64_t bytes, uint64_t needed, int deviceOrdinal, const char* what);
// The pointer part of it, for any caller-owned buffer (rf_renderer_cast_rays checks every input and output with it): std::invalid_argument unless
// hipPointerGetAttributes reports `p` as device memory of device `deviceOrdinal` and, where the runtime can tell the allocation, `bytes` fit behind it.  `what`: the
// entry point, `noun`: the buffer ("the destination", "origins"), `content`: what must fit ("the frame's features"), `owner`: what lives on deviceOrdinal ("the sums",
// "the scene").  No launch.
void requireDeviceRange(const void* p, uint64_t bytes, int deviceOrdinal, const char* what, const char* noun, const char* content, const char* owner);

// Enqueue the one export kernel on `stream` over the frame's sums (rf_frame_sums.hpp; a plane no selected channel reads may be nullptr): one 256-lane workgroup per
// 32 x 32 tile.  The request is valid; dst holds featureBytes() and is element aligned.
void enqueueExportFeatures(hipStream_t stream, const FrameSums& sums, const FeatureRequest& request, void* dst);

// (the standalone export over host-assembled sums, exportFeaturesImages, is declared with the other *Images calls: rf_renderer.hpp)
} // namespace rf
