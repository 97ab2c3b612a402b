// rf_ray_query.hpp -- the kernels of rf_renderer_cast_rays (rf_ray_query.hip) as the host driver sees them (rf_renderer.hip: Renderer::castRays enqueues them around
// the kTraceWide launch the policy picks).  The request's host arithmetic: rf_ray_query_request.hpp.
#pragma once

#include "rf_kernels.hpp"

namespace rf
{
namespace kern
{
// the caller's output buffers, each already advanced to the chunk's first ray; nullptr: not wanted (the mask says the same: bit i of rf_ray_query_request.hpp's kCast*)
struct CastOutputs
{
    uint32_t* triangle;
    float*    t;
    float*    bary;
    float*    position;
    float*    geometricNormal;
    float*    normal;
    float*    texcoord;
    float*    albedo;
    uint32_t* texture;
    float*    visibility;
};

using CastLoadKernel = void (*)(const float* origins, const float* directions, uint32_t originStride, uint32_t directionStride, uint32_t n, PathStreams ps, uint32_t* queue, uint32_t* count);
using CastScalarKernel = void (*)(DeviceScene scene, PathStreams ps, uint32_t n, float tMax);
using CastResolveKernel = void (*)(DeviceScene scene, const float4* hit, const float4* rad, CastOutputs out, uint32_t n, uint32_t mask);

CastLoadKernel    castLoadKernel(bool anyHit);
CastScalarKernel  castScalarKernel(bool anyHit);
CastResolveKernel castResolveKernel();
constexpr uint32_t kCastBlock = 256;
} // namespace kern
} // namespace rf
