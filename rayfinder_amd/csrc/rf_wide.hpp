// rf_wide.hpp -- the render path's BVH layout: 64-byte "children in the parent" nodes.
//
// The reference visits one 48-byte node per step and decides with
//     hit(node) = P(node, ray) && tmin(node, ray) < rayTMax            (wgsl:447-475)
// where P (the two slab early-outs and `tmax > 0`) and tmin depend on the box and the ray only;
// rayTMax enters through the last comparison alone.  That makes the following re-arrangement
// decision-for-decision identical to the reference (same leaves entered in the same order, same
// triangles tested against the same rayTMax, hence bit-identical hits):
//
//   * one record per INTERIOR node holding BOTH children's boxes (16 dwords = 64 B, 64-B aligned:
//     one cache line, four dwordx4 loads, one dependent fetch per two box tests), laid out
//     {c0.lo.xy c0.hi.xy | c0.lo.z c0.hi.z c1.lo.z c1.hi.z | c1.lo.xy c1.hi.xy | word0 word1 - -} so that
//     consecutive float pairs are (x,y) or (z,z): six v_pk_add_f32 + six v_pk_mul_f32 do all twelve slab
//     planes, and the lane holds its ray ONCE ((x,y) as a register pair, z splatted by op_sel) -- the
//     (x,y) (z,x) (y,z) pairing of a plain xyz order needs every component in two pairs, 6 VGPRs more;
//   * the near child (reference order: dirNeg[splitAxis], wgsl:409-417) is handled at once; the
//     far child is pushed together with its tmin only if P holds, and when popped it is accepted
//     iff tmin < rayTMax *then* -- exactly the test the reference performs at pop time;
//   * a leaf is described by its parent's child word, so leaf nodes are never fetched.
//
// Child word: bit 31 = leaf; bits 30..29 = split axis of the record's node (first child word only);
// interior: bits 25..0 = index of the child's wide record.  Leaf: bits 28..26 = min(count-1, 7),
// bits 25..0 = first triangle (count <= 7) or index into the big-leaf table {first triangle, count}
// (count >= 8, or offsets >= 2^26).  A tree with 2^26 or more interior nodes is not representable
// (WideBuild::boxesRegular is cleared: the renderer then uses the 32-byte node kernels).
//
// nodesVisited bookkeeping (the counting build): the reference counts a node when it is visited,
// i.e. root once, the near child at its parent's step, the far child when popped -- also when its
// box test then fails.  The counting build therefore pushes every far child (tmin = +inf when P
// fails) so that visit counts AND the stack high-water mark equal the reference's exactly.
//
// This header: the constants, WideScene and the device functions that read the records.  The host side -- WideBuild, buildWide, leafBoxesIntoTriangles and
// checkWideLayouts -- is rf_wide_build.hpp / rf_wide_build.cpp, compiled once by the host compiler.
#pragma once

#include "rf_device.hpp"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <limits>
#include <vector>

namespace rf
{
constexpr uint32_t kWideLeafBit = 0x80000000u;
constexpr uint32_t kWideIndexBits = 26;  // record / first-triangle / big-leaf index
constexpr uint32_t kWideAxisShift = 29;  // bits 30..29 of the FIRST child word carry the node's split axis
constexpr uint32_t kWideNone = 0xFFFFFFFFu; // scene.rootLeaf when the root is interior
// Which 64-byte quad records a scene gets by default, from WideBuild::quadHalfAreaRatio (how coarse binary16 of absolute coordinates is for
// its boxes).  tools/half_ratio_sweep.py on the atrium at tessellation scales 1 / 2 / 3 / 4 / 6 / 8 = ratios 1.035 / 1.063 / 1.089 / 1.117 /
// 1.166 / 1.223, launch time against the exact quad records:
//     closest-hit   half-precision  -17 / -17 / -14 / -10 /  -3 /  +7 %      local grid  -14 / -15 / -15 / -15 / -13 /  -9 %
//     shadow        half-precision   -7 /  -5 /  -1 / +10 / +28 / +54 %      local grid   -8 /  -8 /  -5 /  -1 /  +4 / +20 %
// (a shadow ray crosses the whole scene: every leaf box it only grazes conservatively costs a triangle line, from HBM in a large scene)
// -> closest-hit: half-precision up to kQuadHalfMaxAreaRatio, local grid beyond; shadow: local grid up to kQuadLocalShadowMaxAreaRatio,
//    exact quad records beyond.
constexpr float    kQuadHalfMaxAreaRatio = 1.075f, kQuadLocalShadowMaxAreaRatio = 1.10f;
constexpr uint32_t kHalfEmptyPlanes = 0x7BFFu | (0xFBFFu << 16); // half-precision quad records: the plane word {lower = +65504, upper = -65504} of an empty slot (an inverted box)
constexpr uint32_t kQuadEmpty = 0xFFFFFFFFu; // quad records: an entry slot that holds no node (its child is a leaf and fills one slot only)
#if defined(RF_EXP_WAVES)
constexpr int      kWideWaves = RF_EXP_WAVES;                 // experiment builds: resident workgroups per CU of kTraceWide
constexpr int      kWideLdsStack = 160 * 1024 / RF_EXP_WAVES / 2048; // as deep as the LDS allows at that occupancy (7: 11, 8: 10)
#else
constexpr int      kWideWaves = 6;
#if defined(RF_EXP_STACK)
constexpr int      kWideLdsStack = RF_EXP_STACK; // experiment builds: a shallower LDS stack (what would it cost to free LDS for other lane state?)
#else
constexpr int      kWideLdsStack = 12;
#endif
#endif
// kWideLdsStack: (child word, tmin) pairs per lane in LDS; a full stack evicts its oldest entries to a per-lane scratch array (kTraceWide, rf_renderer.hip);
// only a ray with more than kWideLdsStack + 36 pending entries is redone by the scalar traversal

struct WideScene
{
    const float4* nodes;     // 4 float4 per interior node
    const float4* compact;   // the same records in the compact-capable layout (see buildWide), or nullptr
    const float4* hot;       // 2 float4 per interior node: the 32-byte records of the all-planes-carried layout (see buildWide), or nullptr
    const float4* own;       // 2 float4 per interior node: the node's own box {lo.x lo.y hi.x hi.y} {lo.z hi.z - -} (read after a pop only)
    const float4* quad;      // 8 float4 per quad record: TWO levels in one 128-byte record (see buildWide), or nullptr
    const uint4*  quadHalf;  // 4 uint4 per quad record: the same records with CONSERVATIVE half-precision planes, 64 bytes (see buildWide), or nullptr
    float         originBound; // quadHalf / quadLocal: rays whose origin has a coordinate beyond this magnitude take the scalar traversal (margin proofs)
    const uint4*  quadLocal; // 4 uint4 per quad record: conservative 8-bit planes on a per-record grid, 64 bytes (see buildWide), or nullptr
    const uint4*  oct;       // 8 uint4 per oct record (128-byte aligned, 112 bytes read): THREE levels per fetch, local-grid planes (see WideBuild::oct), or nullptr
    const uint2*  bigLeaves; // {first triangle, count}
    float4        rootLo;    // root box (w unused)
    float4        rootHi;
    uint32_t      rootLeaf;  // child word of the root if the whole tree is one leaf, else kWideNone
    uint32_t      numRecords;
    // occluder grid of the any-hit launches (kTraceWide, kFlagOccluderCache): a hash table over cells of the scene's space -- entry = the leaf (child word) in
    // which the last shadow ray that left that cell found its occluder, 0: nothing known.  Hints only: any leaf word a kernel wrote is a valid first visit.
    uint32_t*     occGrid;   // or nullptr
    float         occScale;  // cells per unit length
    uint32_t      occMask;   // cells - 1 (a power of two)
    // any-hit launches behind kShadowFirstLook: the queue POSITIONS of the rays still to trace (bit 31: the ray has tried its cell's leaves), or nullptr = every
    // position of the queue; the launch's count argument is then the length of this list
    const uint32_t* rayList;
    // closest-hit launch of bounce 1 under a pinhole camera (kFlagConstOrigin): the one origin of all its rays
    float constOriginX, constOriginY, constOriginZ;
};

#if defined(__HIPCC__)
// The slab test split into its ray-only part: returns P and writes tmin.  Arithmetic and
// comparison order are those of slabTest() in rf_device.hpp.
__device__ __forceinline__ bool slabBounds(const RayPrep& r, float4 lo, float4 hi, float& tminOut)
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
    tminOut = tmin;
    return tmax > 0.0f;
}

// ---------------------------------------------------------------------------------------------
// Both boxes of one record at once.  Precondition: none of the twelve slab products
// (b - o) * inv is NaN.  Then per axis t(lo) <= t(hi) for inv >= 0 and t(hi) <= t(lo) for inv < 0
// (IEEE rounding is monotonic; +-inf included), so the reference's sign-selected near/far planes
// equal min(t(lo), t(hi)) / max(t(lo), t(hi)) bit for bit, its ternary max/min chains equal the
// hardware max3/min3, and its pairwise early-outs
//     !(tmin > tymax) && !(tymin > tmax) && !(max(tmin,tymin) > tzmax) && !(tzmin > min(tmax,tymax))
// are together equivalent to  max3(near) <= min3(far)  (each axis has near <= far; the remaining six
// cross pairs are exactly the four tests).  So P and tmin are those of slabBounds(), with 12 packed
// f32 ops + 16 min/max/compare instead of ~70 VALU and no data-dependent branches.
//
// When can a product be NaN, given ordered finite boxes (WideBuild::boxesRegular)?
//   class A  origin finite (|o| < 1e30), 1/direction finite on all axes: never
//            (b - o is finite, finite * finite is not NaN);
//   class B  origin finite, some 1/direction component = +-inf (direction component +-0 or denormal:
//            axis-aligned walls + a blue-noise value of exactly 0 make these ~0.3 % of all rays):
//            only 0 * inf, i.e. when the origin lies EXACTLY on a plane of the box being tested --
//            checked per step (slabPairHasNaN) for these lanes only;
//   class C  anything else (NaN direction, non-finite origin): always assumed.
// A ray for which a NaN is possible (class C) or occurs (class B) is redone whole by the
// reference-ordered scalar traversal (kTraceWide), so results stay bit-identical in every case.
// Bit-equality with slabBounds() is checked on the GPU by tests/test_gpu_parity.py.
// ---------------------------------------------------------------------------------------------
typedef float v2f __attribute__((ext_vector_type(2)));

struct PackedRay
{
    v2f   oXY, iXY; // origin and 1 / direction: x, y as a register pair
    float oZ, iZ;   // z (splatted into both halves of a packed operand)
};

enum RayClass : uint32_t
{
    kRayPlain = 0,    // class A
    kRayHasInf = 1,   // class B
    kRayIrregular = 2 // class C
};

__device__ __forceinline__ uint32_t classifyRay(const RayPrep& r)
{
    const bool fo = fabsf(r.origin.x) < 1e30f && fabsf(r.origin.y) < 1e30f && fabsf(r.origin.z) < 1e30f; // false for NaN
    const bool nanInv = r.invDir.x != r.invDir.x || r.invDir.y != r.invDir.y || r.invDir.z != r.invDir.z;
    if (!fo || nanInv) return kRayIrregular;
    const bool fi = __builtin_isfinite(r.invDir.x) && __builtin_isfinite(r.invDir.y) && __builtin_isfinite(r.invDir.z);
    return fi ? kRayPlain : kRayHasInf;
}

__device__ __forceinline__ PackedRay packRay(const RayPrep& r)
{
    PackedRay p;
    p.oXY = v2f{r.origin.x, r.origin.y};
    p.iXY = v2f{r.invDir.x, r.invDir.y};
    p.oZ = r.origin.z;
    p.iZ = r.invDir.z;
    return p;
}

// q0 = {c0.lo.xy, c0.hi.xy}  q1 = {c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z}  q2 = {c1.lo.xy, c1.hi.xy}
// slabPairBounds: max3(near) / min3(far) of both boxes; slabPair: P and tmin from them.
__device__ __forceinline__ void slabPairBounds(const PackedRay& r, float4 q0, float4 q1, float4 q2, float& near0, float& far0, float& near1, float& far1)
{
    const v2f oZZ = v2f{r.oZ, r.oZ}, iZZ = v2f{r.iZ, r.iZ};
    const v2f a = (v2f{q0.x, q0.y} - r.oXY) * r.iXY; // c0: t(lo.x), t(lo.y)
    const v2f b = (v2f{q0.z, q0.w} - r.oXY) * r.iXY; // c0: t(hi.x), t(hi.y)
    const v2f c = (v2f{q1.x, q1.y} - oZZ) * iZZ;     // c0: t(lo.z), t(hi.z)
    const v2f d = (v2f{q1.z, q1.w} - oZZ) * iZZ;     // c1: t(lo.z), t(hi.z)
    const v2f e = (v2f{q2.x, q2.y} - r.oXY) * r.iXY; // c1: t(lo.x), t(lo.y)
    const v2f f = (v2f{q2.z, q2.w} - r.oXY) * r.iXY; // c1: t(hi.x), t(hi.y)
    near0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(a.x, b.x), __builtin_fminf(a.y, b.y)), __builtin_fminf(c.x, c.y));
    far0 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(a.x, b.x), __builtin_fmaxf(a.y, b.y)), __builtin_fmaxf(c.x, c.y));
    near1 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(e.x, f.x), __builtin_fminf(e.y, f.y)), __builtin_fminf(d.x, d.y));
    far1 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(e.x, f.x), __builtin_fmaxf(e.y, f.y)), __builtin_fmaxf(d.x, d.y));
}
// slabPairBounds that also hands out the four x-plane products (what a lane carries into the child it enters, compact-capable records)
__device__ __forceinline__ void slabPairBoundsX(const PackedRay& r, float4 q0, float4 q1, float4 q2, float& near0, float& far0, float& near1, float& far1,
                                                float& c0LoX, float& c0HiX, float& c1LoX, float& c1HiX)
{
    const v2f oZZ = v2f{r.oZ, r.oZ}, iZZ = v2f{r.iZ, r.iZ};
    const v2f a = (v2f{q0.x, q0.y} - r.oXY) * r.iXY;
    const v2f b = (v2f{q0.z, q0.w} - r.oXY) * r.iXY;
    const v2f c = (v2f{q1.x, q1.y} - oZZ) * iZZ;
    const v2f d = (v2f{q1.z, q1.w} - oZZ) * iZZ;
    const v2f e = (v2f{q2.x, q2.y} - r.oXY) * r.iXY;
    const v2f f = (v2f{q2.z, q2.w} - r.oXY) * r.iXY;
    c0LoX = a.x, c0HiX = b.x, c1LoX = e.x, c1HiX = f.x;
    near0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(a.x, b.x), __builtin_fminf(a.y, b.y)), __builtin_fminf(c.x, c.y));
    far0 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(a.x, b.x), __builtin_fmaxf(a.y, b.y)), __builtin_fmaxf(c.x, c.y));
    near1 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(e.x, f.x), __builtin_fminf(e.y, f.y)), __builtin_fminf(d.x, d.y));
    far1 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(e.x, f.x), __builtin_fmaxf(e.y, f.y)), __builtin_fmaxf(d.x, d.y));
}
__device__ __forceinline__ void slabPair(const PackedRay& r, float4 q0, float4 q1, float4 q2, bool& ok0, float& tmin0, bool& ok1, float& tmin1)
{
    float far0, far1;
    slabPairBounds(r, q0, q1, q2, tmin0, far0, tmin1, far1);
    ok0 = tmin0 <= far0 && far0 > 0.0f;
    ok1 = tmin1 <= far1 && far1 > 0.0f;
}

// (v_bfi_b32 / v_min_f32 / v_max3_f32 ... are written out: the carried t-values reach this block through phi nodes, the compiler
// no longer knows them to be canonical and would spend twelve `v_max x, x` on quieting them in front of its own min / max;
// none of them is a signalling NaN -- they are products -- and a quiet NaN means a class B ray, which is redone anyway.)
__device__ __forceinline__ float isaMin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float isaMax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float isaMax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float isaMin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
// bit `BIT` of `word` set ? a : b, as a bitwise select under the sign-extended bit (v_bfe_i32 + v_bfi_b32 per pair of selects)
template<int BIT>
__device__ __forceinline__ void swapUnderBit(uint32_t word, float shared, float inner, float& child0, float& child1)
{
    uint32_t m;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(word), "n"(BIT));
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(child0) : "v"(m), "v"(shared), "v"(inner));
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(child1) : "v"(m), "v"(inner), "v"(shared));
}
// The compact-capable record (buildWide): q0 = {innerLoX c0.lo.y innerHiX c0.hi.y}  q1 = {c0.lo.z c0.hi.z c1.lo.z c1.hi.z}
// q2 = {word0 c1.lo.y word1 c1.hi.y}; tOuterLo / tOuterHi = (value - o.x) * inv.x of the node's own x planes (carried from the
// parent's step or computed from the record's fourth piece); selLo / selHi: child 1 holds the inner value.  Outputs as
// slabPairBounds plus the four x-plane t-values of the children (what the lane carries into the child it enters).
// (The x lanes of the two products on q2 work on the child words' bit patterns: never read.)
__device__ __forceinline__ void slabPairCompactBounds(const PackedRay& r, float4 q0, float4 q1, float4 q2, float tOuterLo, float tOuterHi, uint32_t word1,
                                                      float& near0, float& far0, float& near1, float& far1, float& c0LoX, float& c0HiX, float& c1LoX, float& c1HiX)
{
    const v2f oZZ = v2f{r.oZ, r.oZ}, iZZ = v2f{r.iZ, r.iZ};
    const v2f a = (v2f{q0.x, q0.y} - r.oXY) * r.iXY; // t(innerLoX), c0: t(lo.y)
    const v2f b = (v2f{q0.z, q0.w} - r.oXY) * r.iXY; // t(innerHiX), c0: t(hi.y)
    const v2f c = (v2f{q1.x, q1.y} - oZZ) * iZZ;     // c0: t(lo.z), t(hi.z)
    const v2f d = (v2f{q1.z, q1.w} - oZZ) * iZZ;     // c1: t(lo.z), t(hi.z)
    const v2f e = (v2f{q2.x, q2.y} - r.oXY) * r.iXY; // -, c1: t(lo.y)
    const v2f f = (v2f{q2.z, q2.w} - r.oXY) * r.iXY; // -, c1: t(hi.y)
    swapUnderBit<kWideAxisShift>(word1, tOuterLo, a.x, c0LoX, c1LoX);
    swapUnderBit<kWideAxisShift + 1>(word1, tOuterHi, b.x, c0HiX, c1HiX);
    near0 = isaMax3(isaMin(c0LoX, c0HiX), isaMin(a.y, b.y), isaMin(c.x, c.y));
    far0 = isaMin3(isaMax(c0LoX, c0HiX), isaMax(a.y, b.y), isaMax(c.x, c.y));
    near1 = isaMax3(isaMin(c1LoX, c1HiX), isaMin(e.y, f.y), isaMin(d.x, d.y));
    far1 = isaMin3(isaMax(c1LoX, c1HiX), isaMax(e.y, f.y), isaMax(d.x, d.y));
}

// The 32-byte record (buildWide): h0 = {innerLoX innerLoY innerHiX innerHiY}, h1 = {innerLoZ innerHiZ word0 word1}.  `own` = the
// t-values (value - o) * inv of the six planes of the node's own box, carried from the parent's step (or computed from the
// own-box array after a pop / from the root box at refill).  Per plane the selector bit says which child shares the node's plane
// (1: child 0) -- the other one gets the record's inner value.  Same planes and the same product per plane as slabPairBounds().
struct BoxT
{
    float loX, loY, hiX, hiY, loZ, hiZ;
};
__device__ __forceinline__ BoxT boxPlaneT(const PackedRay& r, float4 q0, float q1x, float q1y) // q0 = {lo.x lo.y hi.x hi.y}, q1 = {lo.z hi.z}
{
    const v2f oZZ = v2f{r.oZ, r.oZ}, iZZ = v2f{r.iZ, r.iZ};
    const v2f a = (v2f{q0.x, q0.y} - r.oXY) * r.iXY;
    const v2f b = (v2f{q0.z, q0.w} - r.oXY) * r.iXY;
    const v2f c = (v2f{q1x, q1y} - oZZ) * iZZ;
    return BoxT{a.x, a.y, b.x, b.y, c.x, c.y};
}
__device__ __forceinline__ void slabPairHotBounds(const PackedRay& r, float4 h0, float h1x, float h1y, uint32_t w0, uint32_t w1, const BoxT& own,
                                                  float& near0, float& far0, float& near1, float& far1, BoxT& c0, BoxT& c1)
{
    const BoxT inner = boxPlaneT(r, h0, h1x, h1y);
    swapUnderBit<25>(w0, own.loX, inner.loX, c0.loX, c1.loX);
    swapUnderBit<24>(w0, own.loY, inner.loY, c0.loY, c1.loY);
    swapUnderBit<25>(w1, own.hiX, inner.hiX, c0.hiX, c1.hiX);
    swapUnderBit<24>(w1, own.hiY, inner.hiY, c0.hiY, c1.hiY);
    swapUnderBit<30>(w1, own.loZ, inner.loZ, c0.loZ, c1.loZ);
    swapUnderBit<29>(w1, own.hiZ, inner.hiZ, c0.hiZ, c1.hiZ);
    near0 = isaMax3(isaMin(c0.loX, c0.hiX), isaMin(c0.loY, c0.hiY), isaMin(c0.loZ, c0.hiZ));
    far0 = isaMin3(isaMax(c0.loX, c0.hiX), isaMax(c0.loY, c0.hiY), isaMax(c0.loZ, c0.hiZ));
    near1 = isaMax3(isaMin(c1.loX, c1.hiX), isaMin(c1.loY, c1.hiY), isaMin(c1.loZ, c1.hiZ));
    far1 = isaMin3(isaMax(c1.loX, c1.hiX), isaMax(c1.loY, c1.hiY), isaMax(c1.loZ, c1.hiZ));
}
// Class B lanes only: is any of the twelve slab products of the step NaN (0 * inf)?
__device__ __forceinline__ bool boxPairHasNaN(const BoxT& c0, const BoxT& c1)
{
    return __builtin_isunordered(c0.loX, c0.hiX) || __builtin_isunordered(c0.loY, c0.hiY) || __builtin_isunordered(c0.loZ, c0.hiZ) ||
           __builtin_isunordered(c1.loX, c1.hiX) || __builtin_isunordered(c1.loY, c1.hiY) || __builtin_isunordered(c1.loZ, c1.hiZ);
}

// Class B lanes only: is any of the twelve slab products of this compact-capable record NaN (0 * inf)?  (The four x-plane values are
// the step's own; the other eight are recomputed here, in the rare path.)
__device__ __forceinline__ bool slabPairCompactHasNaN(const PackedRay& r, float4 q0, float4 q1, float4 q2, float c0LoX, float c0HiX, float c1LoX, float c1HiX)
{
    const float ay = (q0.y - r.oXY.y) * r.iXY.y, by = (q0.w - r.oXY.y) * r.iXY.y, ey = (q2.y - r.oXY.y) * r.iXY.y, fy = (q2.w - r.oXY.y) * r.iXY.y;
    const float cx = (q1.x - r.oZ) * r.iZ, cy = (q1.y - r.oZ) * r.iZ, dx = (q1.z - r.oZ) * r.iZ, dy = (q1.w - r.oZ) * r.iZ;
    return __builtin_isunordered(c0LoX, c0HiX) || __builtin_isunordered(c1LoX, c1HiX) || __builtin_isunordered(ay, by) || __builtin_isunordered(cx, cy) ||
           __builtin_isunordered(dx, dy) || __builtin_isunordered(ey, fy);
}

// Half-precision quad records: t' = fma(plane', inv, b) with plane' the low / high binary16 half of `h` (converted exactly), one
// rounding (v_fma_mix_f32: no decode instruction).  The S variants take the word from an SGPR (wave-uniform steps).
__device__ __forceinline__ float fmixLo(uint32_t h, float inv, float b) { float r; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(inv), "v"(b)); return r; }
__device__ __forceinline__ float fmixHi(uint32_t h, float inv, float b) { float r; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(inv), "v"(b)); return r; }
__device__ __forceinline__ float fmixLoS(uint32_t h, float inv, float b) { float r; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "s"(h), "v"(inv), "v"(b)); return r; }
__device__ __forceinline__ float fmixHiS(uint32_t h, float inv, float b) { float r; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "s"(h), "v"(inv), "v"(b)); return r; }
// conservative [near, far] of one entry from its three plane words (x, y, z); NaNs drop out of v_min / v_max (see WideBuild::quadHalf)
// `rx ry rz`: 0 or 16 in bits 4..0 -- the plane word rotated by 16 when 1/d < 0 on that axis, so that its low half is the NEAR plane (the
// reference's sign-selected planes: no per-axis min / max; the conservative planes keep near' < far' by the margin even for a flat box).
template<bool SCALAR>
__device__ __forceinline__ void halfEntryBounds(uint32_t wx, uint32_t wy, uint32_t wz, uint32_t rx, uint32_t ry, uint32_t rz, float ix, float iy, float iz, float bx, float by,
                                                float bz, float& near, float& far)
{
    const uint32_t sx = __builtin_amdgcn_alignbit(wx, wx, rx), sy = __builtin_amdgcn_alignbit(wy, wy, ry), sz = __builtin_amdgcn_alignbit(wz, wz, rz);
    (void)SCALAR;
    near = isaMax3(fmixLo(sx, ix, bx), fmixLo(sy, iy, by), fmixLo(sz, iz, bz));
    far = isaMin3(fmixHi(sx, ix, bx), fmixHi(sy, iy, by), fmixHi(sz, iz, bz));
}
// Local-grid quad records: conservative [near, far] of entry `pair` (0 / 1) of the axis words wx wy wz.  sx sy sz: the v_perm_b32 selectors of
// pair 0 -- 0x00050004 when 1/d >= 0 on that axis (low half = 1024 + lo byte, high half = 1024 + hi byte), 0x00040005 when 1/d < 0 (swapped:
// the low half is always the NEAR plane); pair 1 sits two bytes further (+ 0x00020002).  A = scale / d, B = (anchor - o) / d - 1024 A.
template<int PAIR>
__device__ __forceinline__ void localEntryBounds(uint32_t wx, uint32_t wy, uint32_t wz, uint32_t sx, uint32_t sy, uint32_t sz, float ax, float ay, float az, float bx, float by,
                                                 float bz, float& near, float& far)
{
    constexpr uint32_t kStep = PAIR ? 0x00020002u : 0u;
    const uint32_t     px = __builtin_amdgcn_perm(wx, 0x64646464u, sx + kStep), py = __builtin_amdgcn_perm(wy, 0x64646464u, sy + kStep),
                   pz = __builtin_amdgcn_perm(wz, 0x64646464u, sz + kStep);
    near = isaMax3(fmixLo(px, ax, bx), fmixLo(py, ay, by), fmixLo(pz, az, bz));
    far = isaMin3(fmixHi(px, ax, bx), fmixHi(py, ay, by), fmixHi(pz, az, bz));
}
// The EXACT slab bounds of one box (a leaf's, from its triangle record) in the packed arithmetic of slabPairBounds: same planes, same
// (plane - o) * inv per plane, so the same decisions as the reference's whenever no product is NaN; `hasNaN` says whether one is.
__device__ __forceinline__ void slabSingleBounds(const PackedRay& r, float loX, float loY, float loZ, float hiX, float hiY, float hiZ, float& near, float& far, bool& hasNaN)
{
    const v2f oZZ = v2f{r.oZ, r.oZ}, iZZ = v2f{r.iZ, r.iZ};
    const v2f a = (v2f{loX, loY} - r.oXY) * r.iXY; // t(lo.x), t(lo.y)
    const v2f b = (v2f{hiX, hiY} - r.oXY) * r.iXY; // t(hi.x), t(hi.y)
    const v2f c = (v2f{loZ, hiZ} - oZZ) * iZZ;     // t(lo.z), t(hi.z)
    near = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(a.x, b.x), __builtin_fminf(a.y, b.y)), __builtin_fminf(c.x, c.y));
    far = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(a.x, b.x), __builtin_fmaxf(a.y, b.y)), __builtin_fmaxf(c.x, c.y));
    // (pinned here so that the min / max chains stay in the basic block of their products: sunk behind the callers' rare class-B branch, the compiler no longer knows the
    // products to be canonical and spends six v_max x,x on quieting them -- as in slabStep, rf_trace.hip)
    asm volatile("" : "+v"(near), "+v"(far));
    hasNaN = __builtin_isunordered(a.x, a.y) || __builtin_isunordered(b.x, b.y) || __builtin_isunordered(c.x, c.y);
}

// Class B lanes only: is any of the twelve slab products of this record NaN (0 * inf)?
__device__ __forceinline__ bool slabPairHasNaN(const PackedRay& r, float4 q0, float4 q1, float4 q2)
{
    const v2f oZZ = v2f{r.oZ, r.oZ}, iZZ = v2f{r.iZ, r.iZ};
    const v2f a = (v2f{q0.x, q0.y} - r.oXY) * r.iXY;
    const v2f b = (v2f{q0.z, q0.w} - r.oXY) * r.iXY;
    const v2f c = (v2f{q1.x, q1.y} - oZZ) * iZZ;
    const v2f d = (v2f{q1.z, q1.w} - oZZ) * iZZ;
    const v2f e = (v2f{q2.x, q2.y} - r.oXY) * r.iXY;
    const v2f f = (v2f{q2.z, q2.w} - r.oXY) * r.iXY;
    return __builtin_isunordered(a.x, a.y) || __builtin_isunordered(b.x, b.y) || __builtin_isunordered(c.x, c.y) ||
           __builtin_isunordered(d.x, d.y) || __builtin_isunordered(e.x, e.y) || __builtin_isunordered(f.x, f.y);
}

#endif
} // namespace rf
