// rf_ray_query.hip -- the kernels of rf_renderer_cast_rays (gfx950): rays from caller-owned device memory through the renderer's production traversal, the hit and the
// surface attributes at it into caller-owned device memory.  Per chunk of rays (rf_ray_query_request.hpp: planChunks) the driver (rf_renderer.hip: Renderer::castRays)
// enqueues
//     kCastLoad     the caller's strided rays -> the packed P3 ray streams, the identity queue and its count (any-hit: pending = 1, rad = 0 as well)
//     kTraceWide    the instantiation, record layout and parameters the launch policy picks (rf_launch_policy.cpp: planRayQuery), through Impl::launchWide, unedited
//                   (kCastScalar instead where the scene's wide records are unusable: the reference-order traversal over the 32-byte nodes, same streams)
//     kCastResolve  the hit stream -> the requested outputs at the chunk's offset
// on the handle's stream, with no host synchronisation in between.
//
// The ray streams are always COPIES, also where both strides are 3.  kTraceWide does not write ps.rayO / ps.rayD (its only stores go to ps.hit, ps.rad and, with
// kFlagOccluderCache, the occluder grid; a ray it hands to the scalar traversal is re-read from registers), so the streams could alias the caller's memory there.
// They do not: one code path for every stride is worth more to this unit than the copy it would save (24 bytes read and 24 written per ray by a streaming kernel),
// and a chunk's rays are then never read from the caller's buffers after kCastLoad.  Measured at 1 M rays (profiles/cast_rays/README.md, "Kernel times"): kCastLoad
// takes 11 - 14 us next to a kTraceWide launch of 210 - 300 us, 3 - 5 % of a call's kernel time -- that is all aliasing could save.
//
// Origins outside the scene.  The launch is planned as the render path plans bounce 2 (rf_launch_policy.cpp: planRayQuery), where rays start on surfaces.  On the
// conservative record layouts (half-precision / local-grid quad records) kTraceWide hands every ray whose origin lies outside the records' origin bound (4 R + 1 for a
// root box within +-R) to the reference-order scalar traversal inside the kernel: the values are the same, the ray is slower.  The render path guards bounce 1 against
// a camera out there by picking the exact quad records (closestLayoutFor); a query has no such guard, because its origins are not known on the host.  Probe rays from
// far outside the scene therefore take the slow road ray by ray; what that costs has not been measured.
//
// kCastResolve takes the request mask as a kernel argument (a uniform branch per output): the ten outputs give 2^9 closest-hit combinations, and the branches are
// scalar compares around code that is bound by the record fetch and the stores.  Its attribute arithmetic is rf_shade_device.hpp's: offsetHitPoint,
// interpolateAttributes, unitShadingNormal, evalTexture -- the functions shadeHit calls, so a 1-sample render's first-hit AOVs are this kernel's albedo, normal and t.
#include "rf_ray_query.hpp"
#include "rf_ray_query_request.hpp"
#include "rf_shade_device.hpp"

namespace rf
{
namespace
{
// One thread per ray of the chunk.  origins / directions: the chunk's first ray
template<bool ANY_HIT>
__global__ __launch_bounds__(kCastBlock) void kCastLoad(const float* origins, const float* directions, uint32_t originStride, uint32_t directionStride, uint32_t n, PathStreams ps,
                                                        uint32_t* queue, uint32_t* count)
{
    const uint32_t i = blockIdx.x * kCastBlock + threadIdx.x;
    if (i == 0u) *count = n;
    if (i >= n) return;
    const float* const o = origins + static_cast<size_t>(i) * originStride;
    const float* const d = directions + static_cast<size_t>(i) * directionStride;
    store3(ps.rayO + i, vec3(o[0], o[1], o[2]));
    store3(ps.rayD + i, vec3(d[0], d[1], d[2]));
    queue[i] = i; // the identity queue: slot = queue position
    if constexpr (ANY_HIT)
    {
        // what the any-hit write-back expects: rad += (pending * visibility) * SOLAR_INV_PDF, an occluded ray's sum left alone -- rad.x != 0 iff the ray is unoccluded
        store3(ps.pending + i, vec3(1.0f, 1.0f, 1.0f));
        ps.rad[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// The scene's wide records are unusable (boxes that are NaN or inverted): the reference's own visit order over the 32-byte nodes, one ray per thread, results where
// kTraceWide leaves them
template<bool ANY_HIT>
__global__ __launch_bounds__(kBlock) void kCastScalar(DeviceScene scene, PathStreams ps, uint32_t n, float tMax)
{
    __shared__ uint32_t sStack[kLdsStack * kBlock];
    const uint32_t      i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    ClosestHit        h;
    TraversalCounters tc;
    const bool        found = traverse<ANY_HIT, false>(scene, load3(ps.rayO + i), load3(ps.rayD + i), tMax, &sStack[threadIdx.x], h, tc);
    if constexpr (ANY_HIT) ps.rad[i] = make_float4(found ? 0.0f : 1.0f, 0.0f, 0.0f, 0.0f);
    else ps.hit[i] = make_float4(__uint_as_float(h.triangle), found ? h.u : 0.0f, found ? h.v : 0.0f, found ? h.t : tMax);
}

// W floats per ray, packed: through the workgroup's stage so that consecutive lanes store consecutive dwords (W * 256 of them per workgroup) instead of W strided
// ones per lane.  Reached by every thread of the workgroup (`wanted` is uniform); first: the workgroup's first ray, live: its rays inside the chunk
template<int W>
__device__ __forceinline__ void storeStaged(float* stage, float* dst, bool wanted, uint32_t first, uint32_t live, const float (&v)[W])
{
    if (!wanted) return;
#pragma unroll
    for (int k = 0; k < W; ++k) stage[W * threadIdx.x + k] = v[k];
    __syncthreads();
    float* const out = dst + static_cast<size_t>(first) * W;
#pragma unroll
    for (int k = 0; k < W; ++k)
    {
        const uint32_t e = k * kCastBlock + threadIdx.x;
        if (e < live * W) out[e] = stage[e];
    }
    __syncthreads(); // (the next output overwrites the stage)
}

// One lane per ray: {tri, u, v, t} of the hit stream, the triangle's shading record once, the requested outputs.  A miss: every float +0, the words 0xFFFFFFFF
__global__ __launch_bounds__(kCastBlock) void kCastResolve(DeviceScene scene, const float4* hit, const float4* rad, CastOutputs out, uint32_t n, uint32_t mask)
{
    __shared__ float sStage[3 * kCastBlock];
    const uint32_t   first = blockIdx.x * kCastBlock, i = first + threadIdx.x;
    const uint32_t   live = min(n - first, kCastBlock);
    const bool       inside = i < n;
    if (mask & kCastVisibility)
    {
        if (inside) out.visibility[i] = rad[i].x != 0.0f ? 1.0f : 0.0f;
        return; // (uniform: the any-hit request has no other output)
    }
    const float4   h = inside ? hit[i] : make_float4(__uint_as_float(kMiss), 0.0f, 0.0f, 0.0f);
    const uint32_t tri = __float_as_uint(h.x);
    const bool     found = tri != kMiss;
    if (inside)
    {
        if (mask & kCastTriangle) out.triangle[i] = tri;
        if (mask & kCastT) out.t[i] = found ? h.w : 0.0f;
    }
    float bary[2] = {found ? h.y : 0.0f, found ? h.z : 0.0f};
    storeStaged(sStage, out.bary, (mask & kCastBary) != 0u, first, live, bary);
    if ((mask & kCastNeedsRecord) == 0u) return;

    float    position[3] = {0.0f, 0.0f, 0.0f}, geometric[3] = {0.0f, 0.0f, 0.0f}, normal[3] = {0.0f, 0.0f, 0.0f}, texcoord[2] = {0.0f, 0.0f}, albedo[3] = {0.0f, 0.0f, 0.0f};
    uint32_t texture = 0xFFFFFFFFu;
    if (found)
    {
        const ShadeRecord cur = fetchShadeRecord<false>(scene, tri, false);
        if (mask & (kCastPosition | kCastGeometricNormal))
        {
            Vec3       g;
            const Vec3 p = offsetHitPoint(cur, h.y, h.z, g);
            position[0] = p.x, position[1] = p.y, position[2] = p.z;
            geometric[0] = g.x, geometric[1] = g.y, geometric[2] = g.z;
        }
        texture = __float_as_uint(cur.a3.w);
        if (mask & (kCastNormal | kCastTexcoord | kCastAlbedo))
        {
            Vec3  nrm;
            float uvx, uvy;
            interpolateAttributes(cur, h.y, h.z, nrm, uvx, uvy);
            texcoord[0] = uvx, texcoord[1] = uvy;
            if (mask & kCastNormal)
            {
                const Vec3 u = unitShadingNormal(nrm);
                normal[0] = u.x, normal[1] = u.y, normal[2] = u.z;
            }
            if (mask & kCastAlbedo)
            {
                // (the table in global memory: kShade's copy in LDS holds the same 256 floats)
                const Vec3 a = evalTexture(scene, scene.albedoLut, texture, uvx, uvy);
                albedo[0] = a.x, albedo[1] = a.y, albedo[2] = a.z;
            }
        }
    }
    storeStaged(sStage, out.position, (mask & kCastPosition) != 0u, first, live, position);
    storeStaged(sStage, out.geometricNormal, (mask & kCastGeometricNormal) != 0u, first, live, geometric);
    storeStaged(sStage, out.normal, (mask & kCastNormal) != 0u, first, live, normal);
    storeStaged(sStage, out.texcoord, (mask & kCastTexcoord) != 0u, first, live, texcoord);
    storeStaged(sStage, out.albedo, (mask & kCastAlbedo) != 0u, first, live, albedo);
    if ((mask & kCastTexture) && inside) out.texture[i] = texture;
}
} // namespace

namespace kern
{
CastLoadKernel    castLoadKernel(bool anyHit) { return anyHit ? kCastLoad<true> : kCastLoad<false>; }
CastScalarKernel  castScalarKernel(bool anyHit) { return anyHit ? kCastScalar<true> : kCastScalar<false>; }
CastResolveKernel castResolveKernel() { return kCastResolve; }
} // namespace kern
} // namespace rf
