// rf_shade_device.hpp -- one hit's shading as device functions: the shading record's fetch and the body of kShade's per-hit stage (albedo, NEE term, own-triangle
// test of the shadow ray, cosine bounce: wgsl:189-228,294-319,546-592).  Shared by kShade (rf_shade.hip) and by kPrimaryFused (rf_primary_lists.hip), which shades a
// primary hit in the lane that found it: same functions, same values, same order of operations per path.
#pragma once

#include "rf_kernels.hpp"

namespace rf
{
namespace kern
{
// one slot's first-hit AOV record (kShade<false, true>): two 16-byte stores, non-temporal like kShade's other streams (read once, by the AOV sum kernel after the last bounce)
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void storeAov(float4* aov, uint32_t slot, Vec3 albedo, float coverage, Vec3 normal, float depth)
{
    v4f* const p = reinterpret_cast<v4f*>(aov + 2 * static_cast<size_t>(slot));
    __builtin_nontemporal_store(v4f{albedo.x, albedo.y, albedo.z, coverage}, p);
    __builtin_nontemporal_store(v4f{normal.x, normal.y, normal.z, depth}, p + 1);
}

// everything the shading stage needs of the triangle sits in ONE 128-byte record (positions + packed attributes): one L2 line
// per shaded hit instead of a triangle line and an attribute line (kShade 56.1 -> 53.0 ms per 128 spp)
struct ShadeRecord
{
    Vec3   p0, p1, p2;
    float4 a0, a1, a2, a3; // packed vertex attributes (one 64-byte sector): {n0.xyz n1.x} {n1.yz n2.xy} {n2.z uv0.xy uv1.x} {uv1.y uv2.xy textureIdx}
    Vec3   boxLo;          // kShadeSelfShadow: the exact box of the triangle's leaf (the .w of the three position float4s) ...
    float4 boxHi;          // ... {hi.xyz, 1.0f if the box may be used (the triangle sits in exactly one leaf of a tree with nested boxes), else 0}
};

// (SORTED: only the timing-only ablations of the sorted kernel read it)
template<bool SORTED>
__device__ __forceinline__ ShadeRecord fetchShadeRecord(const DeviceScene& scene, uint32_t tri, bool selfShadow)
{
    ShadeRecord   r;
    const float4* rec = scene.shadeRecords + 8 * static_cast<size_t>(tri);
#if defined(RF_EXP_SHADE_ABLATE) && RF_EXP_SHADE_ABLATE >= 3
    if constexpr (SORTED) rec = scene.shadeRecords + 8 * static_cast<size_t>(tri & 63u); // ablation (timing only): 64 records, all L1 hits
#endif
    // (round 5 measured the same fetch as straight-line code -- eight loads, no branch, every lane fetching A record -- so that entry k + 1's record really is in flight
    // while entry k is shaded (as written here the compiler waits for each group of four loads on the spot): `kShade` +3.5 %.  The kernel is bound by what the fabric
    // delivers, not by the latency of its requests; profiles/r05_shademlp)
    if (selfShadow)
    {
        const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
        r.p0 = vec3(q0.x, q0.y, q0.z), r.p1 = vec3(q1.x, q1.y, q1.z), r.p2 = vec3(q2.x, q2.y, q2.z);
        r.boxLo = vec3(q0.w, q1.w, q2.w);
        r.boxHi = rec[7];
    }
    else
    {
        r.p0 = load3(rec), r.p1 = load3(rec + 1), r.p2 = load3(rec + 2);
        r.boxLo = Vec3{}, r.boxHi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    r.a0 = rec[3], r.a1 = rec[4], r.a2 = rec[5], r.a3 = rec[6];
    return r;
}

// The surface at a hit, barycentrics (hu, hv) on the triangle of `cur`: what shadeHit computes of it, as functions of their own so that the ray queries' resolve kernel
// (kCastResolve, rf_ray_query.hip) gives a caller the very values the shading stage uses -- same functions, same order of operations.
// The hit point pushed off the surface along the geometric normal (wgsl:511-519,523-544): origin of the shadow ray and of the next bounce; same arithmetic as the scalar
// traversal (rf_device.hpp).  geometricNormal: normalize(cross(e1, e2)), the normal it is pushed along.
// (The point is computed BEFORE the normal, as the arguments of the one offsetRay call shadeHit used to make were evaluated: with the two statements exchanged kShade and
// kPrimaryFused compile to other instructions -- same values, another schedule -- and tools/kernel_code_compare.py against the commit before says CHANGED.)
__device__ __forceinline__ Vec3 offsetHitPoint(const ShadeRecord& cur, float hu, float hv, Vec3& geometricNormal)
{
    const Vec3 p0 = cur.p0, p1 = cur.p1, p2 = cur.p2;
    const Vec3 e1 = p1 - p0, e2 = p2 - p0;
    const Vec3 p = p0 + hu * e1 + hv * e2;
    geometricNormal = normalize(cross(e1, e2));
    return offsetRay(p, geometricNormal);
}
// The interpolated shading normal (not normalised, wgsl:396) and texture coordinates (not wrapped); the texture's descriptor index is __float_as_uint(cur.a3.w)
__device__ __forceinline__ void interpolateAttributes(const ShadeRecord& cur, float hu, float hv, Vec3& n, float& uvx, float& uvy)
{
    const float4  a0 = cur.a0, a1 = cur.a1, a2 = cur.a2, a3 = cur.a3;
    const Vec3    n0 = vec3(a0.x, a0.y, a0.z), n1 = vec3(a0.w, a1.x, a1.y), n2 = vec3(a1.z, a1.w, a2.x);
    const float   b0 = 1.0f - hu - hv, b1 = hu, b2 = hv; // wgsl:515
    n = (b0 * n0 + b1 * n1) + b2 * n2;
    uvx = (b0 * a2.y + b1 * a2.w) + b2 * a3.y;
    uvy = (b0 * a2.z + b1 * a3.x) + b2 * a3.z;
}
// The first-hit AOV's normal: the unit shading normal, 0 where n has no direction (|n|^2 zero or not finite)
__device__ __forceinline__ Vec3 unitShadingNormal(Vec3 n)
{
    const float nn = dot(n, n);
    return (nn != 0.0f && isfinite(nn)) ? normalize(n) : Vec3{};
}

// Shade one hit: barycentrics (hu, hv) on the triangle of `cur`, written at position `out` of the next queue.  `inputs(throughput, nz)` hands in the path's throughput
// and blue-noise triple {u.x, cos(2 pi u.y), sin(2 pi u.y)} (asked for after the origin's store, where kShade has always loaded them); `slotOf()` the path's slot
// (needed by the AOV record and by a settled shadow ray only).  -> false: the shadow ray was stopped by the triangle it starts on (kShadeSelfShadow) and is finished
// here; true: it is still to be traced, its NEE term waits in ps.pending[out].
//
// ---- The shadow ray's FIRST candidate occluder is the triangle it starts on (round 5).  The reference pushes the hit point off the surface along the GEOMETRIC normal whatever
// side the path arrived from (wgsl:511-519), and then asks shadowRay (wgsl:321-368) whether ANY triangle stops the ray towards the sun: wherever the sun stands behind that
// normal the ray crosses the plane of its own triangle a hair's breadth from its origin -- inside the triangle -- and the reference reports it occluded (half of all surfaces).
// The shading stage holds everything that test needs in registers: the origin it has just computed, the sun sample, the triangle's positions -- and, in the spare floats of the
// shading record, the EXACT box of the triangle's leaf.  selfShadow: it applies the leaf's box with the reference's formula, then the reference's triangle test; a ray that this
// stops is FINISHED here (its NEE term times 0, exactly as the traversal's write-back adds it), and only the positions of the other hits go onto the shadow list, which the
// bounce's any-hit launches (kShadowFirstLook, kTraceWide) work through instead of the whole queue.
// Same visibility bit as the reference's walk, by the argument of the occluder cache (rf_trace.hip): the reference tests this triangle iff its walk reaches the leaf, i.e. iff
// the boxes of the leaf and of all its ancestors pass; an ancestor's box contains the leaf's and the slab arithmetic is monotone in the planes, so a ray that passes the leaf's
// own test passes every ancestor's: the reference either reaches this leaf -- and finds this triangle, or an earlier one of the leaf -- or has found another occluder before.
// Occluded either way.  A ray the test does NOT stop proves nothing and is traced as before.  (Trees whose boxes are not nested, triangles that sit in two leaves or in
// none, rays that are not class A: no shortcut -- the record's flag is 0 / the ray goes onto the list.)
template<bool SORTED, bool AOV, typename Inputs, typename SlotOf>
__device__ __forceinline__ bool shadeHit(const DeviceScene& scene, const SkyStateGpu& sky, const SunBasis& sunBasis, const PathStreams& ps, const float* sLut, bool isFirstBounce,
                                         bool isLastBounce, bool selfShadow, float hu, float hv, float hitT, const ShadeRecord& cur, uint32_t out, float4* aov, Inputs&& inputs,
                                         SlotOf&& slotOf)
{
    Vec3 shadowOrigin;
    {
        Vec3       geometricNormal;
        const Vec3 hp = offsetHitPoint(cur, hu, hv, geometricNormal);
        store3nt(ps.rayO + out, hp); // (this bounce's origins have been consumed by the closest-hit launch)
        shadowOrigin = hp;
    }
    Vec3 throughput, nz;
    inputs(throughput, nz);
    const float nx = nz.x, cosPhi = nz.y, sinPhi = nz.z;
    store3nt(ps.noiseOut + out, nz); // travels with the path: dense for this bounce's shadow launch and for the next kShade
    const float4  a3 = cur.a3;
    Vec3          n; // not normalised, wgsl:396
    float         uvx, uvy;
    interpolateAttributes(cur, hu, hv, n, uvx, uvy);
#if defined(RF_EXP_SHADE_ABLATE) && (RF_EXP_SHADE_ABLATE == 1 || RF_EXP_SHADE_ABLATE == 4)
    const Vec3    albedo = SORTED ? vec3(sLut[__float_as_uint(a3.w) & 255u], uvx - floorf(uvx), uvy - floorf(uvy)) : evalTexture(scene, sLut, __float_as_uint(a3.w), uvx, uvy); // ablation (timing only): no texel fetch
#else
    const Vec3    albedo = evalTexture(scene, sLut, __float_as_uint(a3.w), uvx, uvy);
#endif
    if constexpr (AOV)
    {
        // first-hit AOVs: the texel, the unit shading normal (0 where n has no direction: |n|^2 zero or not finite) and the distance along the unit primary direction
        storeAov(aov, slotOf(), albedo, 1.0f, unitShadingNormal(n), hitT);
    }
    else (void)hitT, (void)aov;

    // next-event estimation towards the sun, wgsl:194-203 (cosine is not clamped)
    const Vec3 lightDirection = sunSample(sky, sunBasis, nx, cosPhi, sinPhi);
    const Vec3 lightIntensity = vec3(sky.solarRadiances[0], sky.solarRadiances[1], sky.solarRadiances[2]);
    const Vec3 brdf = albedo * kFrac1Pi;
    const Vec3 reflectance = brdf * dot(n, lightDirection);
    const Vec3 pend = (throughput * lightIntensity) * reflectance;
    bool       settled = false; // selfShadow: the shadow ray is stopped by the triangle it starts on
    if (selfShadow && cur.boxHi.w != 0.0f)
    {
        const RayPrep ray = prepareRay(shadowOrigin, lightDirection);
        if (classifyRay(ray) == kRayPlain)
        {
            const PackedRay pr = packRay(ray);
            float           bn, bf;
            bool            boxNaN;
            slabSingleBounds(pr, cur.boxLo.x, cur.boxLo.y, cur.boxLo.z, cur.boxHi.x, cur.boxHi.y, cur.boxHi.z, bn, bf, boxNaN);
            if (bn <= bf && bf > 0.0f && bn < kTMax) // the reference reaches this leaf (kShadowFirstLook applies the same test to the leaves its cell names)
            {
                TriangleHit th;
                settled = intersectTriangle(shadowOrigin, lightDirection, cur.p0, cur.p1, cur.p2, kTMax, th);
            }
        }
    }
    if (settled)
    {
        // the traversal's write-back for an occluded ray (kTraceWide): radiance += (pending * 0) * invPdf -- a sum that keeps its bits unless the product is NaN, or the
        // sum is not in memory yet (bounce 1)
        const Vec3 add = (pend * 0.0f) * __uint_as_float(kSolarInvPdfBits);
        const bool unchanged = !isFirstBounce && add.x == 0.0f && add.y == 0.0f && add.z == 0.0f;
        if (!unchanged)
        {
            const uint32_t slot = slotOf();
            const Vec3     radiance = (isFirstBounce ? vec3(0.0f, 0.0f, 0.0f) : load3(ps.rad + slot)) + add;
            ps.rad[slot] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
        }
    }
    else store3nt(ps.pending + out, pend); // read by the shadow launch at the same queue position

    if (!isLastBounce)
    {
        // cosine-weighted bounce about the interpolated normal, wgsl:209-211,294-301,582-592
        const float sinTheta = rf_sqrt(1.0f - nx);
        const Vec3  local = vec3(cosPhi * sinTheta, sinPhi * sinTheta, rf_sqrt(nx));
        Vec3        bu, bv;
        pixarOnb(n, bu, bv);
        const Vec3 wi = basisTimes(bu, bv, n, local); // not renormalised
        const Vec3 t2 = throughput * albedo;
        store3nt(ps.rayDOut + out, wi);
        store3nt(ps.thrOut + out, t2);
    }
    return !settled;
}
} // namespace kern
} // namespace rf
