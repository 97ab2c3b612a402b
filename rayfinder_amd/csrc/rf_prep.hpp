// rf_prep.hpp -- the values the denoiser's prep forms of one pixel's sums (include/rayfinder_amd.h, "Edge-aware a-trous denoiser", prep): the mean colour c, the
// background test with the depth z, and the unit normal n.  One IEEE f32 operation at a time in the order written.  For kernels that need prep's values in
// registers: kTemporalReproject (rf_temporal.hip), whose step 1 is defined as "exactly prep's values".  The text is prepPixel's (rf_denoise.hip), operation for
// operation.  prepPixel keeps its own copy for now: rewritten over these functions it compiled to the same arithmetic in another block order, and rf_denoise.hip's
// code object is held byte for byte; tests/test_gpu_temporal.py holds G = {n, z} and c to tests/denoise_restatement.py's prep, bits equal.
#pragma once

#include "rf_math.hpp"

#include <hip/hip_runtime.h>

#include <cfloat>

namespace rf
{
// index of pixel (x, y) in a compact tile-major buffer that holds every tile of the frame in tile order (localPixelToXY's layout)
__device__ __forceinline__ uint32_t prepTileMajorIndex(uint32_t x, uint32_t y, uint32_t tilesX)
{
    const uint32_t tile = (y >> 5) * tilesX + (x >> 5);
    const uint32_t block = ((y & 31u) >> 3) * 4u + ((x & 31u) >> 3);
    return tile * 1024u + block * 64u + (y & 7u) * 8u + (x & 7u);
}

// c = S.rgb / Nf (kTonemap's division)
__device__ __forceinline__ Vec3 prepColor(const float4& S, float nf) { return vec3(S.x / nf, S.y / nf, S.z / nf); }

// z = ND.w / AC.w; background (passes through, never a neighbour): no coverage, or a depth that is not > 0 (NaN included)
__device__ __forceinline__ bool prepBackground(const float4& AC, const float4& ND, float& z)
{
    z = ND.w / AC.w;
    return AC.w == 0.0f || !(z > 0.0f);
}

// n = normalize(ND.xyz / Nf), or 0 where the mean normal's squared length is 0, infinite or NaN
__device__ __forceinline__ Vec3 prepNormal(const float4& ND, float nf)
{
    const Vec3  m = vec3(ND.x / nf, ND.y / nf, ND.z / nf);
    const float d = dot(m, m);
    return (d != 0.0f && fabsf(d) <= FLT_MAX) ? normalize(m) : splat(0.0f);
}
} // namespace rf
