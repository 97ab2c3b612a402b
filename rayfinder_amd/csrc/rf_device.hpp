// rf_device.hpp -- device-side building blocks of the wavefront path tracer (gfx950).
//
// Behavioural reference (what must come out, not how): src/pt/reference_path_tracer.wgsl.
//   slab test           wgsl:447-475  == src/common/ray_intersection.cpp:101-136
//   Moller-Trumbore     wgsl:477-521  == ray_intersection.cpp:38-90
//   offsetRay           wgsl:523-544  == ray_intersection.cpp:17-35
//   closest-hit order   wgsl:370-429  == ray_intersection.cpp:138-213
//   any-hit             wgsl:321-368
//
// HBM layout (chosen for the hardware, not the reference's):
//   nodes      32 B each, two float4: {min.xyz, link} {max.xyz, meta}
//              link = leaf ? trianglesOffset : secondChildOffset (the other one is always 0 in the
//              reference's 48-B node, bvh.cpp:31-55); meta = triangleCount << 2 | axis (axis 3 =
//              leaf).  32-B alignment means a node never straddles a 64-B line and one visit is
//              two dwordx4 loads instead of three; results are bit-identical.
//   triangles  the reference's 48-B PositionAttribute (three float4) padded to 64 B, so that one
//              triangle test is one 64-B L2 request instead of 1.5 on average.
//   traversal stack: per-lane, first RF_LDS_STACK entries in LDS ([depth][lane], conflict free
//              because lanes l and l+32 sit in different halves), overflow in scratch.
#pragma once

#include "rf_launch_constants.hpp"
#include "rf_types.hpp"

#include <hip/hip_runtime.h>

namespace rf
{
constexpr int      kLdsStack = 24;        // entries kept in LDS per lane
constexpr int      kSpillStack = 72;      // further entries in scratch (total depth 96)
constexpr uint32_t kMiss = 0xFFFFFFFFu;
constexpr uint32_t kLeafAxis = 3u;
constexpr uint32_t kTriStride = 4u;     // float4 per device triangle: 48 B of PositionAttribute padded to one 64-B sector
constexpr uint32_t kSortBins = 256; // kShade<SORTED>: triangle ranges of its counting sort (the host derives sortScale from it: rf_scene_pack.cpp)

struct DeviceScene
{
    const float4*            nodes;      // 2 per node
    const float4*            triangles;  // kTriStride per triangle (p0, p1, p2, pad)
    const float4*            attributes; // 4 per triangle: the 80-B VertexAttributes packed to 64 B (rf_renderer.hip)
    const float4*            shadeRecords; // 8 per triangle (128 B, 128-B aligned): p0 p1 p2 + the 4 attribute float4 -- everything kShade needs of a triangle in one L2 line
    const TextureDescriptor* textureDescriptors;
    const uint32_t*          texels;
    uint64_t                 numTexels;
    const uint8_t*           blueNoise; // 128*128*2
    const float*             albedoLut; // 256 entries: pow(i/255, 2.2)
};

#if defined(__HIPCC__) // device code below; the host only needs the layout constants above (tools/sanitize builds rf_wide.hpp with g++)
struct RayPrep
{
    Vec3     origin;
    Vec3     direction;
    Vec3     invDir;
    uint32_t negX, negY, negZ;
};

__device__ __forceinline__ RayPrep prepareRay(Vec3 o, Vec3 d)
{
    RayPrep r;
    r.origin = o;
    r.direction = d;
    r.invDir = vec3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    r.negX = r.invDir.x < 0.0f;
    r.negY = r.invDir.y < 0.0f;
    r.negZ = r.invDir.z < 0.0f;
    return r;
}

__device__ __forceinline__ bool slabTest(const RayPrep& r, float4 lo, float4 hi, float rayTMax)
{
    float       tmin = ((r.negX ? hi.x : lo.x) - r.origin.x) * r.invDir.x;
    float       tmax = ((r.negX ? lo.x : hi.x) - r.origin.x) * r.invDir.x;
    const float tymin = ((r.negY ? hi.y : lo.y) - r.origin.y) * r.invDir.y;
    const float tymax = ((r.negY ? lo.y : hi.y) - r.origin.y) * r.invDir.y;
    if ((tmin > tymax) || (tymin > tmax)) return false;
    tmin = maxf(tymin, tmin);
    tmax = minf(tymax, tmax);
    const float tzmin = ((r.negZ ? hi.z : lo.z) - r.origin.z) * r.invDir.z;
    const float tzmax = ((r.negZ ? lo.z : hi.z) - r.origin.z) * r.invDir.z;
    if ((tmin > tzmax) || (tzmin > tmax)) return false;
    tmin = maxf(tzmin, tmin);
    tmax = minf(tzmax, tmax);
    return (tmin < rayTMax) && (tmax > 0.0f);
}

__device__ __forceinline__ Vec3 offsetRay(Vec3 p, Vec3 n)
{
    constexpr float kOrigin = 1.0f / 32.0f;
    constexpr float kFloatScale = 1.0f / 65536.0f;
    constexpr float kIntScale = 256.0f;
    const int       ox = static_cast<int>(kIntScale * n.x);
    const int       oy = static_cast<int>(kIntScale * n.y);
    const int       oz = static_cast<int>(kIntScale * n.z);
    const Vec3      shifted = vec3(__int_as_float(__float_as_int(p.x) + (p.x < 0 ? -ox : ox)),
                                   __int_as_float(__float_as_int(p.y) + (p.y < 0 ? -oy : oy)),
                                   __int_as_float(__float_as_int(p.z) + (p.z < 0 ? -oz : oz)));
    return vec3(fabsf(p.x) < kOrigin ? p.x + kFloatScale * n.x : shifted.x,
                fabsf(p.y) < kOrigin ? p.y + kFloatScale * n.y : shifted.y,
                fabsf(p.z) < kOrigin ? p.z + kFloatScale * n.z : shifted.z);
}

struct TriangleHit
{
    float t, u, v;
};

// Returns true when the triangle is hit with 1e-5 < t < rayTMax.
__device__ __forceinline__ bool
intersectTriangle(Vec3 origin, Vec3 direction, Vec3 p0, Vec3 p1, Vec3 p2, float rayTMax, TriangleHit& hit)
{
    constexpr float kEpsilon = 0.00001f;
    const Vec3      e1 = p1 - p0;
    const Vec3      e2 = p2 - p0;
    const Vec3      h = cross(direction, e2);
    const float     det = dot(e1, h);
    if (det > -kEpsilon && det < kEpsilon) return false;
    const float invDet = 1.0f / det;
    const Vec3  s = origin - p0;
    const float u = invDet * dot(s, h);
    if (u < 0.0f || u > 1.0f) return false;
    const Vec3  q = cross(s, e1);
    const float v = invDet * dot(direction, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = invDet * dot(e2, q);
    if (t > kEpsilon && t < rayTMax)
    {
        hit.t = t;
        hit.u = u;
        hit.v = v;
        return true;
    }
    return false;
}
__device__ __forceinline__ bool
intersectTriangle(const RayPrep& r, Vec3 p0, Vec3 p1, Vec3 p2, float rayTMax, TriangleHit& hit)
{
    return intersectTriangle(r.origin, r.direction, p0, p1, p2, rayTMax, hit);
}

struct ClosestHit
{
    uint32_t triangle; // kMiss when nothing was hit
    float    t, u, v;
    Vec3     p; // hit point already pushed off the surface (offsetRay)
};

struct TraversalCounters
{
    uint32_t nodesVisited = 0;
    uint32_t triangleTests = 0;
    uint32_t stackHigh = 0;
    uint32_t abandoned = 0; // maintained in every build: the ray needed more than kLdsStack + kSpillStack stack entries
};

// One ray, the reference's visit order.  ANY_HIT: return at the first accepted triangle
// (shadowRay); otherwise keep the closest (rayIntersectBvh).  COUNT: maintain counters.
// LDS: stack entries kept in LDS (0: the whole stack in scratch, ldsStackLane unused).
template<bool ANY_HIT, bool COUNT, int LDS = kLdsStack>
__device__ __forceinline__ bool traverse(const DeviceScene& scene, Vec3 origin, Vec3 direction, float rayTMax,
                                         uint32_t* ldsStackLane, ClosestHit& out, TraversalCounters& counters)
{
    const RayPrep ray = prepareRay(origin, direction);
    // stack: first kLdsStack entries in LDS (ldsStackLane[depth * kBlock]), the rest in scratch;
    // size and pointer are plain locals so they stay in registers
    constexpr int kSpill = kLdsStack + kSpillStack - LDS;
    uint32_t      spill[kSpill];
    int           stackSize = 0;
    uint32_t      current = 0;
    bool          found = false;
    out.triangle = kMiss;

    for (;;)
    {
        const float4 lo = scene.nodes[2 * current];
        const float4 hi = scene.nodes[2 * current + 1];
        if (COUNT) ++counters.nodesVisited;
        bool advance = false; // true: `current` already holds the next node
        if (slabTest(ray, lo, hi, rayTMax))
        {
            const uint32_t link = __float_as_uint(lo.w);
            const uint32_t meta = __float_as_uint(hi.w);
            const uint32_t axis = meta & 3u;
            if (axis == kLeafAxis)
            {
                const uint32_t count = meta >> 2;
                for (uint32_t i = 0; i < count; ++i)
                {
                    const uint32_t tri = link + i;
                    const float4   a = scene.triangles[kTriStride * tri];
                    const float4   b = scene.triangles[kTriStride * tri + 1];
                    const float4   c = scene.triangles[kTriStride * tri + 2];
                    if (COUNT) ++counters.triangleTests;
                    TriangleHit th;
                    const Vec3  p0 = vec3(a.x, a.y, a.z), p1 = vec3(b.x, b.y, b.z), p2 = vec3(c.x, c.y, c.z);
                    if (intersectTriangle(ray, p0, p1, p2, rayTMax, th))
                    {
                        if (ANY_HIT) return true;
                        rayTMax = th.t;
                        found = true;
                        const Vec3 e1 = p1 - p0, e2 = p2 - p0;
                        const Vec3 p = p0 + th.u * e1 + th.v * e2;
                        const Vec3 n = normalize(cross(e1, e2));
                        out.p = offsetRay(p, n);
                        out.t = th.t;
                        out.u = th.u;
                        out.v = th.v;
                        out.triangle = tri;
                    }
                }
            }
            else
            {
                const uint32_t neg = axis == 0 ? ray.negX : (axis == 1 ? ray.negY : ray.negZ);
                const uint32_t deferred = neg ? current + 1 : link;
                current = neg ? link : current + 1;
                if (LDS > 0 && stackSize < LDS) ldsStackLane[stackSize * kBlock] = deferred;
                else if (stackSize - LDS < kSpill) spill[stackSize - LDS] = deferred;
                else
                {
                    // deeper than kLdsStack + kSpillStack = 96 entries: the ray is abandoned with what it has found so
                    // far (the reference's 32-entry stack is overrun, i.e. undefined, long before); reported through
                    // rf_stats.abandoned_rays so that a caller can tell that it happened
                    counters.abandoned = 1;
                    break;
                }
                ++stackSize;
                if (COUNT) counters.stackHigh = max(counters.stackHigh, static_cast<uint32_t>(stackSize));
                advance = true;
            }
        }
        if (!advance)
        {
            if (stackSize == 0) break;
            --stackSize;
            if constexpr (LDS > 0)
            {
                current = ldsStackLane[min(stackSize, LDS - 1) * kBlock]; // see kTraceWide's pop()
                asm volatile("" : "+v"(current));
                if (stackSize >= LDS) current = spill[stackSize - LDS];
            }
            else
            {
                current = spill[stackSize];
            }
        }
    }
    return found;
}

// ---------------------------------------------------------------------------------------------
// WGSL builtins with implementation-defined precision (sin cos acos exp, and the sky model's pow(x, 1.5)).  Documented choice since
// round 3 (DESIGN.md "Floating point policy"): the f32 rounding of a SPECIFIED f64 evaluation -- the classic fdlibm kernels written
// out as plain sequences of IEEE f64 operations (+ - * / sqrt fma rint ldexp), each within about an ulp(f64) of the true value, i.e.
// the correctly rounded f32 except about once in 2^29 calls.  The test oracle evaluates the same sequences on the CPU, so the two sides agree
// bit for bit by construction (ocml against the C library did not: they differ in the last f64 bit now and then, and once in ~10^9
// calls that bit decided an f32 rounding).  No special cases beyond NaN / out-of-range: leaner than the library calls as well.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double dExp(double x)
{
    if (x != x) return x;
    if (x > 709.0) return __builtin_inf();
    if (x < -745.0) return 0.0;
    const double k = __builtin_rint(x * 1.44269504088896338700e+00);
    double       r = __builtin_fma(-k, 6.93147180369123816490e-01, x);
    r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;                 // 1/13!: Taylor polynomial of degree 13 on |r| <= 0.3466, Horner with fma
    p = __builtin_fma(p, r, 2.08767569878681e-09);    // 1/12!
    p = __builtin_fma(p, r, 2.505210838544172e-08);   // 1/11!
    p = __builtin_fma(p, r, 2.755731922398589e-07);   // 1/10!
    p = __builtin_fma(p, r, 2.7557319223985893e-06);  // 1/9!
    p = __builtin_fma(p, r, 2.48015873015873e-05);    // 1/8!
    p = __builtin_fma(p, r, 0.0001984126984126984);   // 1/7!
    p = __builtin_fma(p, r, 0.001388888888888889);    // 1/6!
    p = __builtin_fma(p, r, 0.008333333333333333);    // 1/5!
    p = __builtin_fma(p, r, 0.041666666666666664);    // 1/4!
    p = __builtin_fma(p, r, 0.16666666666666666);     // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, static_cast<int>(k));
}
// argument reduction by pi/2 in three parts (exact products through fma); meant for the |x| <= 2 pi of this renderer, defined for all x
__device__ __forceinline__ double dReduce(double x, long long& quadrant)
{
    const double k = __builtin_rint(x * 6.36619772367581382433e-01);
    double       r = __builtin_fma(-k, 1.57079632673412561417e+00, x);
    r = __builtin_fma(-k, 6.07710050650619224932e-11, r);
    r = __builtin_fma(-k, 2.02226624879595063154e-21, r);
    quadrant = static_cast<long long>(k);
    return r;
}
// sin or cos on [-pi/4, pi/4]: fdlibm __kernel_sin / __kernel_cos without the tail argument.  One polynomial per call -- which of the
// two the quadrant asks for is decided first (the other one's value is never used, and a `switch` over both would evaluate both for
// every lane of the wave); the operations on the chosen path are the kernel's own.
__device__ __forceinline__ double dSinCosKernel(double r, bool cosine)
{
    const double z = r * r;
    const double c5 = cosine ? -1.13596475577881948265e-11 : 1.58969099521155010221e-10, c4 = cosine ? 2.08757232129817482790e-09 : -2.50507602534068634195e-08;
    const double c3 = cosine ? -2.75573143513906633035e-07 : 2.75573137070700676789e-06, c2 = cosine ? 2.48015872894767294178e-05 : -1.98412698298579493134e-04;
    const double c1 = cosine ? -1.38888888888741095749e-03 : 8.33333333332248946124e-03, c0 = cosine ? 4.16666666666666019037e-02 : -1.66666666666666324348e-01;
    const double t = c0 + z * (c1 + z * (c2 + z * (c3 + z * (c4 + z * c5))));
    return cosine ? (1.0 - 0.5 * z) + (z * z) * t : r + (r * z) * t;
}
__device__ __forceinline__ double dSin(double x)
{
    if (!(__builtin_fabs(x) < 1.0e15)) return x - x; // inf, NaN: NaN
    long long    q;
    const double r = dReduce(x, q), v = dSinCosKernel(r, (q & 1) != 0);
    return (q & 2) ? -v : v; // quadrants 0..3: s, c, -s, -c
}
__device__ __forceinline__ double dCos(double x)
{
    if (!(__builtin_fabs(x) < 1.0e15)) return x - x;
    long long    q;
    const double r = dReduce(x, q), v = dSinCosKernel(r, (q & 1) == 0);
    return ((q + 1) & 2) ? -v : v; // quadrants 0..3: c, -s, -c, s
}
// fdlibm __ieee754_acos
__device__ __forceinline__ double dAcosRatio(double z)
{
    const double p = z * (1.66666666666666657415e-01 + z * (-3.25565818622400915405e-01 + z * (2.01212532134862925881e-01 + z * (-4.00555345006794114027e-02 + z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
    const double q = 1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)));
    return p / q;
}
__device__ __forceinline__ double dAcos(double x)
{
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    if (x != x) return x;
    if (__builtin_fabs(x) >= 1.0)
    {
        if (x == 1.0) return 0.0;
        if (x == -1.0) return pi + 2.0 * pio2_lo;
        return (x - x) / (x - x); // |x| > 1: NaN
    }
    // The three ranges of fdlibm share ONE evaluation of the rational function and ONE square root (the lanes of a wave fall into all
    // three, and as separate branches each would run its own division and square root for the whole wave); every lane still performs
    // exactly the operations of its own range.
    const bool   small = __builtin_fabs(x) < 0.5, negative = x < 0.0;
    if (small && __builtin_fabs(x) <= 6.938893903907228e-18) return pio2_hi + pio2_lo; // 2^-57
    const double z = small ? x * x : (negative ? (1.0 + x) * 0.5 : (1.0 - x) * 0.5);
    const double r = dAcosRatio(z);
    if (small) return pio2_hi - (x - (pio2_lo - x * r));
    const double s = __builtin_sqrt(z);
    if (negative)
    {
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double df = __longlong_as_double(__double_as_longlong(s) & static_cast<long long>(0xFFFFFFFF00000000ull));
    const double c = (z - df * df) / (s + df), w = r * s + c;
    return 2.0 * (df + w);
}
__device__ __forceinline__ float wSin(float x) { return static_cast<float>(dSin(static_cast<double>(x))); }
__device__ __forceinline__ float wCos(float x) { return static_cast<float>(dCos(static_cast<double>(x))); }
__device__ __forceinline__ float wAcos(float x) { return static_cast<float>(dAcos(static_cast<double>(x))); }
__device__ __forceinline__ float wExp(float x) { return static_cast<float>(dExp(static_cast<double>(x))); }
// (display side only -- the tonemap's pow(y, 1 / 2.2), quantised to 8 bits: the library call)
__device__ __forceinline__ float wPow(float x, float y)
{
    return static_cast<float>(pow(static_cast<double>(x), static_cast<double>(y)));
}
// wgsl:59-63,277-285 -> the BGRA8Unorm texel of one pixel's radiance sum, for kTemporalReproject (rf_temporal.hip), which forms its texel in the lane that blended the
// pixel.  The text is kTonemap's body (rf_shade.hip), operation for operation.  kTonemap keeps its own copy: calling this function from it compiled to the same
// arithmetic behind an inverted loop branch, and rf_shade.hip's code object is held byte for byte.  tests/test_gpu_temporal.py holds the texels to the CPU restatement of the display transform.
__device__ __forceinline__ uint32_t tonemapTexel(float4 px, uint32_t accumulatedSamples, float exposure)
{
    const float in[3] = {px.x, px.y, px.z};
    uint32_t    q[3];
    for (int c = 0; c < 3; ++c)
    {
        const float est = in[c] / static_cast<float>(accumulatedSamples);
        const float x = exposure * est;
        const float a = 2.51f, b = 0.03f, cc = 2.43f, d = 0.59f, e = 0.14f;
        float       y = (x * (a * x + b)) / (x * (cc * x + d) + e);
        y = minf(maxf(y, 0.0f), 1.0f);
        const float srgb = wPow(y, 1.0f / 2.2f);
        q[c] = static_cast<uint32_t>(floorf(srgb * 255.0f + 0.5f));
    }
    return q[2] | (q[1] << 8) | (q[0] << 16) | (255u << 24);
}
// pow(x, 1.5f) of the sky model's Mie term = x * sqrt(x) in f64 (correctly rounded sqrt, one rounded product: within 1.5 ulp(f64) of
// x^1.5), the same expression in the test oracle.  Negative x gives NaN, -0 gives +0... as pow does.
__device__ __forceinline__ float wPow15(float x)
{
    const double xd = static_cast<double>(x);
    return static_cast<float>(xd * __builtin_sqrt(xd));
}
__device__ __forceinline__ float wFract(float x) { return x - floorf(x); }

// ---- round 6: the OPT-IN f32 evaluation of the same builtins (renderer option `transcendentals` = 1).  WGSL's own sin / cos / acos / exp / pow are f32 with
// implementation-defined accuracy (wgsl:247-275,568-616 call them): the specified-f64 evaluation above is one documented choice that makes GPU == test oracle
// bit for bit, not the only legitimate one.  This mode calls the device math library's f32 functions (ocml: sinf / cosf within 2 ulp, acosf / expf within 1-2,
// powf within 1 ulp -- "libm-grade", NOT the __sinf / __expf fast intrinsics) and is graded by SURVEY 8(d)'s stated tolerance against the test oracle instead of
// bit-identity (tests/test_gpu_parity.py: test_f32_transcendentals_mode_within_the_stated_tolerance).  The default stays the specified f64 evaluation.
template<bool F32> __device__ __forceinline__ float tSin(float x) { if constexpr (F32) return sinf(x); else return wSin(x); }
template<bool F32> __device__ __forceinline__ float tCos(float x) { if constexpr (F32) return cosf(x); else return wCos(x); }
template<bool F32> __device__ __forceinline__ float tAcos(float x) { if constexpr (F32) return acosf(x); else return wAcos(x); }
template<bool F32> __device__ __forceinline__ float tExp(float x) { if constexpr (F32) return expf(x); else return wExp(x); }
template<bool F32> __device__ __forceinline__ float tPow15(float x) { if constexpr (F32) return powf(x, 1.5f); else return wPow15(x); }

constexpr float kPi = 3.1415927f;       // wgsl:68
constexpr float kFrac1Pi = 0.31830987f; // wgsl:69
constexpr float kTMax = 10000.0f;       // wgsl:73
// wgsl:79-83 evaluated in f32: cos(0.255 deg) and 2*pi*(1-cos); 1 ulp of the cosine is 0.6 % of
// the direct light, so the bit patterns are fixed here.
constexpr uint32_t kSolarCosThetaMaxBits = 0x3F7FFF5Au;
constexpr uint32_t kSolarInvPdfBits = 0x38826048u;

// Duff et al. orthonormal basis, wgsl:309-319.  Returns columns u, v (third column is n).
__host__ __device__ __forceinline__ void pixarOnb(Vec3 n, Vec3& u, Vec3& v)
{
    const float s = (n.z >= 0.0f) ? 1.0f : -1.0f;
    const float a = -1.0f / (s + n.z);
    const float b = n.x * n.y * a;
    u = vec3(1.0f + s * n.x * n.x * a, s * b, -s * n.x);
    v = vec3(b, s + n.y * n.y * a, -n.y);
}

__device__ __forceinline__ Vec3 basisTimes(Vec3 c0, Vec3 c1, Vec3 c2, Vec3 v)
{
    return (v.x * c0 + v.y * c1) + v.z * c2;
}

// wgsl:247-275 (sky dome only; the solar disk is reached through next-event estimation).  cosTheta = |cos(theta)| and
// cosGamma = cos(gamma) are the same for the three channels: the caller evaluates them once (identical values).
template<bool F32 = false>
__device__ __forceinline__ float skyRadiance(const SkyStateGpu& sky, float cosTheta, float gamma, float cosGamma, int channel)
{
    const float  r = sky.skyRadiances[channel];
    const float* p = sky.params + 9 * channel;
    const float  cosGamma2 = cosGamma * cosGamma;
    const float  expM = tExp<F32>(p[4] * gamma);
    const float  mieLhs = 1.0f + cosGamma2;
    const float  mieRhs = tPow15<F32>(1.0f + p[8] * p[8] - 2.0f * p[8] * cosGamma);
    const float  mie = mieLhs / mieRhs;
    const float  zenith = rf_sqrt(cosTheta);
    const float  lhs = 1.0f + p[0] * tExp<F32>(p[1] / (cosTheta + 0.01f));
    const float  rhs = p[2] + p[3] * expM + p[5] * cosGamma2 + p[6] * mie + p[7] * zenith;
    return r * (lhs * rhs);
}

// wgsl:303-307,552-565.  An index past the end of the texel array (fract()*w rounding up on the
// last row of the last texture) is clamped into the array, as WGSL robust buffer access does.  (The same rounding on another
// row reads the first texel of the next row; on the last row of a texture that is not the last, the first texel of the next texture.)
// A NaN or infinite uv (fract(inf) = inf - inf = NaN) reads texel (0,0) of its texture: the float -> u32 conversion of a NaN is 0 here
// (v_cvt_u32_f32), the documented choice next to the clamp; tests/test_gpu_shade_edges.py holds the kernels to it.
// `lut`: the 256-entry sRGB -> linear table, in LDS in kShade (three look-ups per hit that then bypass the vector L1)
__device__ __forceinline__ Vec3 evalTexture(const DeviceScene& scene, const float* lut, uint32_t descriptorIdx, float uvx, float uvy)
{
    // (round 6 measured the same texels in 8 x 8 tiles -- four 64-byte lines of 8 x 2 texels instead of 16 x 1: kShade of bounce 1 -3.1 %, L1->L2 requests per hit 0.51 -> 0.46, the
    // other bounces unchanged; below the 5 % it was to be adopted at: profiles/r06_texel)
    const TextureDescriptor d = scene.textureDescriptors[descriptorIdx];
    const float             u = wFract(uvx);
    const float             v = wFract(uvy);
    const uint32_t          j = static_cast<uint32_t>(u * static_cast<float>(d.width));
    const uint32_t          i = static_cast<uint32_t>(v * static_cast<float>(d.height));
    uint64_t                idx = static_cast<uint64_t>(d.offset) + static_cast<uint64_t>(i * d.width + j);
    if (idx >= scene.numTexels) idx = scene.numTexels - 1;
    const uint32_t bgra = scene.texels[idx];
    return vec3(lut[(bgra >> 16) & 0xffu], lut[(bgra >> 8) & 0xffu], lut[bgra & 0xffu]);
}

// wgsl:602-616; table texel = u8 / 255.0f (reference_path_tracer.cpp:174-178)
// (n = frameIdx % totalSampleCount, wgsl:608, computed by the caller: kRaygen has it without a software division, rf_kernels.hpp FastDiv)
__device__ __forceinline__ void animatedBlueNoiseN(const uint8_t* table, uint32_t x, uint32_t y, uint32_t n, float& nx, float& ny)
{
    const uint32_t idx = (y % 128u) * 128u + (x % 128u);
    const float    bx = static_cast<float>(table[2 * idx]) / 255.0f;
    const float    by = static_cast<float>(table[2 * idx + 1]) / 255.0f;
    const float    a1 = 0.7548776662466927f;
    const float    a2 = 0.5698402909980532f;
    nx = wFract(bx + wFract(a1 * static_cast<float>(n)));
    ny = wFract(by + wFract(a2 * static_cast<float>(n)));
}
__device__ __forceinline__ void animatedBlueNoise(const uint8_t* table, uint32_t x, uint32_t y, uint32_t frameIdx, uint32_t totalSampleCount, float& nx, float& ny)
{
    animatedBlueNoiseN(table, x, y, frameIdx % totalSampleCount, nx, ny);
}
#endif // __HIPCC__
} // namespace rf
