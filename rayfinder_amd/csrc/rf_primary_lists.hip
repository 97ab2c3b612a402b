// rf_primary_lists.hip -- bounce 1 under a pinhole camera without the tree walk: kPixelLeafLists (once per batch, one thread per pixel: the leaves ANY primary ray
// of that pixel can reach, in the reference's visit order) and kTraceLeafLists (one ray per lane: the exact box and the triangles of the leaves on its pixel's
// list).  Launched from rf_renderer.hip (enqueueClosest) through the accessors at the end of this file; kTraceWide is not touched and takes whatever the lists do
// not cover.  kPrimaryFused (further down): the same walk in the lane that generates the ray and shades its hit -- bounce 1 as one kernel per path.
//
// Why.  A batch holds hundreds of samples of a pixel; under a pinhole camera they share one origin and their directions lie within the pixel's footprint, so the
// traversal's interior decisions come out the same hundreds of times.  The wave-uniform fetches of kTraceWide save the memory traffic of that, not the per-lane
// slab arithmetic that binds the launch.  Here the interior nodes are walked ONCE per pixel, with interval arithmetic over the pixel's direction box, and a sample
// only pays for the handful of leaves that survive.
//
// Why the hits are bit-identical to the reference's (wgsl:370-429), i.e. to kTraceWide's:
//   Same decision per leaf.  The reference tests a leaf's triangles iff its walk reaches the leaf, i.e. iff the leaf's own box and every ancestor's pass
//     P(box) && tmin(box) < rayTMax at the time each is visited.  The boxes are nested (WideBuild::boxesNested) and the slab arithmetic is monotone in the planes
//     (rf_wide.hpp): a ray that passes the leaf's own exact box, with the rayTMax of the moment the leaf's turn comes, passes every ancestor's earlier test
//     (a containing box has tmin no larger, tmax no smaller, and rayTMax only shrinks).  Conversely a ray that reaches the leaf has applied that very test.  So
//     "leaf's exact box from its triangle record, then its triangles" -- what kShadowFirstLook and the conservative layouts' leaf phase do -- decides as the reference does.
//   Same order.  For fixed direction signs the reference's depth-first order (near child first by dirNeg[splitAxis], wgsl:409-417) is one total order of the
//     leaves.  kPixelLeafLists walks the 32-byte nodes in exactly that order for the pixel's sign pattern and emits every leaf whose box, and all of whose ancestors'
//     boxes, COULD pass for some direction of the pixel (no rayTMax at all): a superset of any one ray's visits, in that order.  A ray's own visits are therefore a
//     subsequence of its pixel's list; the walker applies the exact test to every entry in turn, so it tests the same triangles in the same order against the same
//     rayTMax, and ties in t resolve as in the reference.
//   Everything else falls back.  A pixel whose direction box touches zero on an axis (mixed signs), a list that overflows, a leaf with a table-encoded count, a
//     walk deeper than its stack, and -- per ray -- anything that is not class A or whose signs are not the list's: the ray's queue position goes onto a list that
//     the bounce's ordinary kTraceWide launch works through (WideScene::rayList).
#include "rf_kernels.hpp"
#include "rf_shade_device.hpp"

namespace rf
{
namespace
{
constexpr int kListWalkStack = 64; // pending far children of the per-pixel walk (the reference's own stack holds 32); deeper: the pixel gets no list

// ------------------------------------------------------------------------------------------------
// kPixelLeafLists: one thread per local pixel of the batch (kRaygen's local-pixel -> frame-pixel mapping, so tile lists, shards and render_adaptive batches
// need nothing of their own).  Writes the pixel's list at its RANK among the batch's valid pixels -- kRaygen's dense queue holds sample k of that pixel at
// position rank * numSamples + k -- and its length word: bits 7..0 the length, bits 10..8 the direction signs the order was made for; bit 31 (kNoPrimaryList): no list,
// bits 2..0 then say why (kNoList...).
//
// The direction box.  kRaygen's direction is normalize(D(s, t)) with D = lowerLeft + s horizontal + t vertical - origin affine in (s, t), and (s, t) runs over
// the pixel's rectangle as the blue-noise pair (nx, ny) runs over [0, 1]^2 (wFract: never above 1).  The four corners are evaluated with kRaygen's own f32
// expressions.  Per component the box is the corners' [min, max], widened by
//   * a quarter of its size (the issue's margin: slack that costs a few per cent more entries at most),
//   * diag^2, the squared distance between the farthest two corner directions: the set of directions is the spherical quadrilateral spanned by the corners, and
//     a component of a unit vector along a great-circle arc of length theta exceeds its values at the arc's ends by at most 1 - cos(theta / 2) <= theta^2 / 8
//     (an extremum inside the quadrilateral means a coordinate pole inside it, i.e. a sign change of the other two components: such a pixel gets no list),
//   * 64 ulp(1) x (M / |D| + 1), M the largest magnitude among the camera vectors' components: every f32 evaluation of D is within ~8 roundings of size
//     ulp(M) of the exact affine value, which lies in the hull of the corners' exact values; normalising divides by |D| and adds a few roundings of its own.
// All of it in f64, where the arithmetic's own error is nine orders of magnitude below these margins.
//
// The node test.  For a direction d of the box (no component zero, all of one sign per axis) the reference computes t = fl(fl(plane - o) * fl(1 / d)) per plane:
// three correctly rounded operations, so within a factor (1 +- 2^-24)^3 of the real (plane - o) / d -- which, for d in [lo, hi], lies between (plane - o) / lo
// and (plane - o) / hi.  The interval ends are computed in f64 and widened by 1e-6 relative (four times that factor) plus 1e-30.  The reference accepts a node
// only if max(near) <= min(far) and min(far) > 0 (rf_wide.hpp: its pairwise early-outs are equivalent to that for NaN-free products, and class A rays have no
// NaN); here a node is accepted iff max(lower bounds of near) <= min(upper bounds of far) and that minimum is > 0: whenever the reference could accept for ANY
// direction in the box, this does.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kPixelLeafLists(FrameParams fp, DeviceScene scene, const uint32_t* tileIds, uint32_t capacity, uint32_t* lists, uint32_t* lengths)
{
    const uint32_t lp = blockIdx.x * kBlock + threadIdx.x;
    if (lp >= fp.pixelsPadded) return;
    uint32_t x, y;
    if (!localPixelToXY(fp, tileIds, lp, x, y)) return;
    uint32_t rank;
    {
        const uint32_t tile = tileIds[lp >> 10];
        uint32_t       tileX, tileY;
        fp.divTilesX.divmod(tile, tileY, tileX);
        const uint32_t x0 = tileX * kTileSize, y0 = tileY * kTileSize;
        rank = fp.tileValidBefore[lp >> 10] + validRankInTile(lp & 1023u, min(kTileSize, fp.width - x0), min(kTileSize, fp.height - y0));
    }
    // ---- the four corner directions, with kRaygen's expressions
    const float u = (static_cast<float>(x) + 0.5f) / static_cast<float>(fp.width);
    const float v = (static_cast<float>(y) + 0.5f) / static_cast<float>(fp.height);
    const Vec3  origin = fp.camera.origin;
    double      lo[3] = {2.0, 2.0, 2.0}, hi[3] = {-2.0, -2.0, -2.0}, corner[4][3], minLen = 1e300;
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
        const float nx = (c & 1) ? 1.0f : 0.0f, ny = (c & 2) ? 1.0f : 0.0f;
        const float s = u + nx / static_cast<float>(fp.width);
        const float t = (1.0f - v) + ny / static_cast<float>(fp.height);
        const Vec3  D = fp.camera.lowerLeftCorner + s * fp.camera.horizontal + t * fp.camera.vertical - origin;
        const Vec3  dir = normalize(D);
        const double len = sqrt(static_cast<double>(D.x) * D.x + static_cast<double>(D.y) * D.y + static_cast<double>(D.z) * D.z);
        minLen = fmin(minLen, len);
        corner[c][0] = dir.x, corner[c][1] = dir.y, corner[c][2] = dir.z;
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fmin(lo[a], corner[c][a]), hi[a] = fmax(hi[a], corner[c][a]);
    }
    double diag2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i + 1; j < 4; ++j)
        {
            const double dx = corner[i][0] - corner[j][0], dy = corner[i][1] - corner[j][1], dz = corner[i][2] - corner[j][2];
            diag2 = fmax(diag2, dx * dx + dy * dy + dz * dz);
        }
    const Camera& cam = fp.camera;
    const double  big = fmax(fmax(fmax(fmax(fabs(cam.origin.x), fabs(cam.origin.y)), fmax(fabs(cam.origin.z), fabs(cam.lowerLeftCorner.x))),
                                  fmax(fmax(fabs(cam.lowerLeftCorner.y), fabs(cam.lowerLeftCorner.z)), fmax(fabs(cam.horizontal.x), fabs(cam.horizontal.y)))),
                             fmax(fmax(fabs(cam.horizontal.z), fabs(cam.vertical.x)), fmax(fabs(cam.vertical.y), fabs(cam.vertical.z))));
    const double  rounding = 64.0 * 5.9604644775390625e-08 * (big / minLen + 1.0);
    uint32_t      noList = (!(minLen > 0.0) || !(big < 1e30)) ? kNoListSigns : 0u;
    double        invLo[3], invHi[3];
    uint32_t      neg[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
        const double margin = 0.25 * (hi[a] - lo[a]) + diag2 + rounding;
        lo[a] -= margin, hi[a] += margin;
        if (!(lo[a] > 0.0 || hi[a] < 0.0)) noList = kNoListSigns; // the box touches zero on this axis (or is NaN)
        neg[a] = hi[a] < 0.0 ? 1u : 0u;
        invLo[a] = 1.0 / hi[a], invHi[a] = 1.0 / lo[a]; // (1 / d decreases on either side of zero)
    }
    if (noList != 0u)
    {
        lengths[rank] = kNoPrimaryList | noList;
        return;
    }
    const double o[3] = {origin.x, origin.y, origin.z};
    uint32_t*    out = lists + static_cast<size_t>(rank) * capacity;
    uint32_t     n = 0;
    uint32_t     stack[kListWalkStack];
    int          stackSize = 0;
    uint32_t     current = 0;
    for (;;)
    {
        const float4 nlo = scene.nodes[2 * current];
        const float4 nhi = scene.nodes[2 * current + 1];
        const float  blo[3] = {nlo.x, nlo.y, nlo.z}, bhi[3] = {nhi.x, nhi.y, nhi.z};
        double       nearLower = -1e300, farUpper = 1e300;
#pragma unroll
        for (int a = 0; a < 3; ++a)
        {
            const double qn = static_cast<double>(neg[a] ? bhi[a] : blo[a]) - o[a], qf = static_cast<double>(neg[a] ? blo[a] : bhi[a]) - o[a];
            double       tn = fmin(qn * invLo[a], qn * invHi[a]), tf = fmax(qf * invLo[a], qf * invHi[a]);
            tn -= fabs(tn) * 1e-6 + 1e-30;
            tf += fabs(tf) * 1e-6 + 1e-30;
            nearLower = fmax(nearLower, tn), farUpper = fmin(farUpper, tf);
        }
        bool advance = false;
        if (nearLower <= farUpper && farUpper > 0.0)
        {
            const uint32_t link = __float_as_uint(nlo.w), meta = __float_as_uint(nhi.w), axis = meta & 3u;
            if (axis == kLeafAxis)
            {
                const uint32_t count = meta >> 2;
                // (a leaf word with its count in the word: 1 .. 7 triangles from a first triangle below 2^26; longer leaves live in the big-leaf table, which the walker does not read)
                if (count == 0u || count > 7u || link >= (1u << kWideIndexBits) || n == capacity)
                {
                    noList = n == capacity ? kNoListOverflow : kNoListBigLeaf;
                    break;
                }
                out[n++] = kWideLeafBit | ((count - 1u) << kWideIndexBits) | link;
            }
            else
            {
                const uint32_t deferred = neg[axis] ? current + 1 : link;
                current = neg[axis] ? link : current + 1;
                if (stackSize == kListWalkStack)
                {
                    noList = kNoListStack;
                    break;
                }
                stack[stackSize++] = deferred;
                advance = true;
            }
        }
        if (!advance)
        {
            if (stackSize == 0) break;
            current = stack[--stackSize];
        }
    }
    lengths[rank] = noList != 0u ? (kNoPrimaryList | noList) : (n | (neg[0] << 8) | (neg[1] << 9) | (neg[2] << 10));
}

// ------------------------------------------------------------------------------------------------
// kTraceLeafLists: bounce 1's closest-hit launch over the lists.  Dense, one ray per lane, grid-stride over tiles of kItems x kBlock queue positions (the shape
// of kShadowFirstLook): queue position -> pixel rank (a pixel's samples are contiguous: FastDiv by the batch's sample count) -> the pixel's list; per entry the
// leaf's exact box from its first triangle record (leafBoxesIntoTriangles) with the lane's rayTMax of that moment, then the leaf's triangles in order with the
// reference's Moller-Trumbore.  Writes the 16-byte hit record kTraceWide writes, at the queue position, a miss included.  What the lists do not cover goes
// onto `fallback` (queue positions, one atomic per block) for the kTraceWide launch behind this one.
//
// A wave is 64 consecutive queue positions: with 64 or more samples per pixel nearly every wave holds ONE pixel's samples (every wave, where the batch depth is a
// multiple of 64), so its lanes walk the same list and test the same leaves.  Such a wave (UNIFORM) reads the length word, the list and the triangle records
// through the scalar cache -- the pointers are cast to the constant address space, whose loads from a wave-uniform address are s_load: neither the kernel nor
// anything that runs beside it writes these arrays -- and the planes and vertices reach the lanes' arithmetic as SGPR operands.  With per-lane loads the launch
// was bound by the vector L1's return path (four 16-byte loads of one address per lane and entry), not by its arithmetic.  A wave that straddles two pixels takes
// the per-lane loads.  Same values, same operations per lane either way.
// ------------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) uint32_t* ConstU32;
typedef const __attribute__((address_space(4))) float*    ConstF32;

struct ListHit
{
    uint32_t tri;
    float    u, v, tMax;
};

// one ray over one list of `len` leaf words (`walks` false: a lane of a UNIFORM wave whose ray is handed on -- it runs the wave's loop and tests nothing)
template<bool UNIFORM>
__device__ __forceinline__ void walkLeafList(const DeviceScene& scene, const uint32_t* list, uint32_t len, Vec3 o, Vec3 dir, const PackedRay& pr, bool walks, ListHit& best)
{
    for (uint32_t e = 0; e < len; ++e)
    {
        if constexpr (UNIFORM)
        {
            const uint32_t w = ((ConstU32)list)[e];
            const uint32_t first = w & ((1u << kWideIndexBits) - 1u), n = ((w >> kWideIndexBits) & 7u) + 1u;
            ConstF32       t0 = (ConstF32)scene.triangles + 4u * kTriStride * static_cast<size_t>(first);
            float          bn, bf;
            bool           boxNaN;
            slabSingleBounds(pr, t0[3], t0[7], t0[11], t0[12], t0[13], t0[14], bn, bf, boxNaN);
            if (!(walks && bn <= bf && bf > 0.0f && bn < best.tMax)) continue; // the reference does not reach this leaf
            for (uint32_t t = 0; t < n; ++t)
            {
                ConstF32    q = t0 + 4u * kTriStride * t;
                TriangleHit th;
                if (intersectTriangle(o, dir, vec3(q[0], q[1], q[2]), vec3(q[4], q[5], q[6]), vec3(q[8], q[9], q[10]), best.tMax, th))
                    best.tMax = th.t, best.u = th.u, best.v = th.v, best.tri = first + t;
            }
        }
        else
        {
            const uint32_t w = list[e];
            const uint32_t first = w & ((1u << kWideIndexBits) - 1u), n = ((w >> kWideIndexBits) & 7u) + 1u;
            const float4*  t0 = scene.triangles + kTriStride * static_cast<size_t>(first);
            // (four loads, each pinned in its own register tuple: see the leaf phase of kTraceWide)
            typedef float v4f __attribute__((ext_vector_type(4)));
            const v4f*     t4 = reinterpret_cast<const v4f*>(t0);
            v4f            a = t4[0], b = t4[1], c = t4[2];
            v3f            bhi = *reinterpret_cast<const v3f*>(t0 + 3);
            asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(bhi));
            float          bn, bf;
            bool           boxNaN;
            slabSingleBounds(pr, a.w, b.w, c.w, bhi.x, bhi.y, bhi.z, bn, bf, boxNaN);
            if (!(bn <= bf && bf > 0.0f && bn < best.tMax)) continue; // the reference does not reach this leaf
            TriangleHit th;
            if (intersectTriangle(o, dir, vec3(a.x, a.y, a.z), vec3(b.x, b.y, b.z), vec3(c.x, c.y, c.z), best.tMax, th))
                best.tMax = th.t, best.u = th.u, best.v = th.v, best.tri = first;
            for (uint32_t t = 1; t < n; ++t)
            {
                const v3f q0 = *reinterpret_cast<const v3f*>(t0 + kTriStride * t), q1 = *reinterpret_cast<const v3f*>(t0 + kTriStride * t + 1),
                          q2 = *reinterpret_cast<const v3f*>(t0 + kTriStride * t + 2);
                if (intersectTriangle(o, dir, vec3(q0.x, q0.y, q0.z), vec3(q1.x, q1.y, q1.z), vec3(q2.x, q2.y, q2.z), best.tMax, th))
                    best.tMax = th.t, best.u = th.u, best.v = th.v, best.tri = first + t;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void kTraceLeafLists(DeviceScene scene, PathStreams ps, const uint32_t* queueCount, FastDiv divNumSamples, float originX, float originY,
                                                           float originZ, const uint32_t* lists, const uint32_t* lengths, uint32_t capacity, uint32_t* fallback,
                                                           uint32_t* fallbackCount, DeviceCounters* counters, float tMax)
{
    __shared__ uint32_t sScratch[8];
    const uint32_t      count = *queueCount;
    const uint32_t      tiles = (count + kItems * kBlock - 1) / (kItems * kBlock);
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        atomicAdd(&counters->closestRays, static_cast<unsigned long long>(count));
        atomicAdd(&counters->primaryListRays, static_cast<unsigned long long>(count));
    }
    const Vec3 o = vec3(originX, originY, originZ);
    uint32_t   handedOn = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    {
        bool     keep[kItems];
        uint32_t entry[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k)
        {
            const uint32_t j = (tile * kItems + k) * kBlock + threadIdx.x;
            keep[k] = false;
            entry[k] = j;
            if (j >= count) continue;
            const uint32_t  rank = divNumSamples.div(j);
            const Vec3      dir = load3(ps.rayD + j);
            const RayPrep   ray = prepareRay(o, dir);
            const PackedRay pr = packRay(ray);
            const uint32_t  signs = ray.negX | (ray.negY << 1) | (ray.negZ << 2);
            const bool      plain = classifyRay(ray) == kRayPlain;
            ListHit         best{kMiss, 0.0f, 0.0f, tMax};
            // (the lanes that are here -- the wave's positions inside the queue -- and whether they all hold one pixel's samples)
            const uint32_t uRank = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(rank)));
            bool           walks;
            if (__ballot(rank != uRank) == 0ull)
            {
                const uint32_t word = ((ConstU32)lengths)[uRank];
                // (no list for the pixel; not class A; or not the signs the list's order was made for -- the direction box says that cannot happen, and nothing rests on it)
                walks = (word & kNoPrimaryList) == 0u && plain && ((word >> 8) & 7u) == signs;
                if ((word & kNoPrimaryList) == 0u) walkLeafList<true>(scene, lists + static_cast<size_t>(uRank) * capacity, word & 0xFFu, o, dir, pr, walks, best);
            }
            else
            {
                const uint32_t word = lengths[rank];
                walks = (word & kNoPrimaryList) == 0u && plain && ((word >> 8) & 7u) == signs;
                if (walks) walkLeafList<false>(scene, lists + static_cast<size_t>(rank) * capacity, word & 0xFFu, o, dir, pr, true, best);
            }
            if (walks) store4s(ps.hit + j, __uint_as_float(best.tri), best.u, best.v, best.tMax); // (.w = t of the hit, tMax for a miss: kTraceWide's record)
            else keep[k] = true;
        }
#pragma unroll
        for (int k = 0; k < kItems; ++k) handedOn += keep[k] ? 1u : 0u;
        blockAppend<kItems>(keep, entry, fallback, fallbackCount, sScratch);
    }
    // (rare: one atomic per wave that handed rays on)
    const unsigned long long total = waveSum(static_cast<unsigned long long>(handedOn));
    if (__lane_id() == 0 && total != 0ull) atomicAdd(&counters->primaryFallbackRays, total);
}
// ------------------------------------------------------------------------------------------------
// kPrimaryFused: bounce 1 of a batch whose primary launch runs over the lists, in ONE kernel per path -- kRaygen's generation, kTraceLeafLists' walk and kShade's
// shading (BatchPlan::primaryFused: the lists, no AOVs, the specified f64 sin / cos).  The three kernels handed a path to each other through memory, one lane per
// path, in the same order: queue entry, direction, hit record and blue-noise triple were written once to be read back once, 88 of the chain's 156 bytes per path.
// Here the lane that generates the ray walks its pixel's list and shades the hit out of its registers, and only kShade's outputs are left to write.
//
// kRaygen's shape: kItems slots per thread, slot = (blockIdx * kItems + k) * kBlock + tid, pixel-major slots (slotGroupShift 0) with closed-form queue positions:
// consecutive lanes hold consecutive samples of one pixel, which is what the walk's scalar-cache path wants (a wave is UNIFORM where its valid lanes hold one
// pixel's samples).  Per slot the same device functions run on the same values in the same order as in the three kernels, so every output keeps its bits:
//   a covered ray (`walks`) that hits is appended to the hit queue and shaded on the spot (shadeHit, rf_shade_device.hpp) with the batch's bounce-1 shade flags;
//     one that misses goes onto the miss lists with its queue position, where it writes its direction -- all kSky reads of it at bounce 1;
//   an uncovered ray (no list, overflow, big leaf, not class A, sign mismatch) writes what kRaygen wrote -- queue entry, direction, triple -- and its queue position
//     onto `fallback`: the bounce's kTraceWide launch and kShade<false, false, true> work through that list behind this kernel.
// A covered ray writes no queue entry, no hit record and no input triple: nothing else reads them at bounce 1 (the AOV kernel would, and keeps the three launches).
// `fallback` cannot be the bounce's output queue as under kTraceLeafLists -- this kernel appends hits there; the driver hands in the bounce's input throughput
// stream, which holds nothing at bounce 1.
// ------------------------------------------------------------------------------------------------
#if defined(RF_EXP_FUSED_WAVES)
#define RF_FUSED_BOUNDS __launch_bounds__(kBlock, RF_EXP_FUSED_WAVES)
#else
#define RF_FUSED_BOUNDS __launch_bounds__(kBlock) // (102 registers, four waves per SIMD; forced into 96 for five, bounce 1's group measured 17.3 -> 18.4 ms per 256 spp)
#endif
__global__ RF_FUSED_BOUNDS void kPrimaryFused(FrameParams fp, DeviceScene scene, SkyStateGpu sky, SunBasis sunBasis, const uint32_t* tileIds, PathStreams ps, uint32_t* queue,
                                                         uint32_t* queueCount, const uint32_t* lists, const uint32_t* lengths, uint32_t capacity, uint32_t* hitQueue, uint32_t* hitCount,
                                                         uint32_t* missQueue, uint32_t* missSlots, uint32_t* missCount, uint32_t* shadowList, uint32_t* shadowListCount, uint32_t* fallback,
                                                         uint32_t* fallbackCount, DeviceCounters* counters, uint32_t bounceFlags, float tMax)
{
    __shared__ uint32_t sScratch[8];
    __shared__ float    sLut[256];
    static_assert(kBlock == 256, "one table entry per thread");
    sLut[threadIdx.x] = scene.albedoLut[threadIdx.x];
    __syncthreads();
    const uint32_t total = fp.numSamples * fp.pixelsPadded;
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        const uint32_t count = fp.validPixels * fp.numSamples;
        *queueCount = count;
        atomicAdd(&counters->closestRays, static_cast<unsigned long long>(count));
        atomicAdd(&counters->primaryListRays, static_cast<unsigned long long>(count));
        atomicAdd(&counters->primaryFusedRays, static_cast<unsigned long long>(count));
    }
    const bool isLastBounce = (bounceFlags & kShadeLastBounce) != 0u, selfShadow = (bounceFlags & kShadeSelfShadow) != 0u;
    const Vec3 o = fp.camera.origin; // (the batch's one origin: BatchPlan::constOrigin)
    bool       isHit[kItems], isMiss[kItems], handOn[kItems];
    uint32_t   slots[kItems], pos[kItems], hitTri[kItems], outPos[kItems];
    float      hitU[kItems], hitV[kItems];
    Vec3       noise[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k)
    {
        // ---- generate (kRaygen's pass 1 and pass 2)
        const uint32_t slot = (blockIdx.x * kItems + k) * kBlock + threadIdx.x;
        bool           valid = slot < total;
        uint32_t       x = 0, y = 0, sampleIdx = 0, lp = 0;
        if (valid) slotToSamplePixel(fp, slot, sampleIdx, lp);
        if (valid) valid = localPixelToXY(fp, tileIds, lp, x, y);
        slots[k] = slot;
        isHit[k] = isMiss[k] = handOn[k] = false;
        pos[k] = 0u, hitTri[k] = kMiss, hitU[k] = hitV[k] = 0.0f, noise[k] = Vec3{};
        if (!valid) continue;
        uint32_t rank;
        {
            const uint32_t tile = tileIds[lp >> 10];
            uint32_t       tileX, tileY;
            fp.divTilesX.divmod(tile, tileY, tileX);
            const uint32_t x0 = tileX * kTileSize, y0 = tileY * kTileSize;
            rank = fp.tileValidBefore[lp >> 10] + validRankInTile(lp & 1023u, min(kTileSize, fp.width - x0), min(kTileSize, fp.height - y0));
        }
        const uint32_t j = rank * fp.numSamples + sampleIdx; // the path's position in the bounce's queue
        pos[k] = j;
        const uint32_t frame = fp.firstFrame + (fp.samplePerm ? fp.samplePerm[sampleIdx] : sampleIdx);
        float          nx, ny;
        animatedBlueNoiseN(scene.blueNoise, x, y, frame - fp.divSamplesPerPixel.div(frame) * fp.samplesPerPixel, nx, ny);

        const float u = (static_cast<float>(x) + 0.5f) / static_cast<float>(fp.width);
        const float v = (static_cast<float>(y) + 0.5f) / static_cast<float>(fp.height);
        const float s = u + nx / static_cast<float>(fp.width);
        const float t = (1.0f - v) + ny / static_cast<float>(fp.height);

        const float phi = 2.0f * kPi * ny;
        const float cosPhi = tCos<false>(phi), sinPhi = tSin<false>(phi);
        const float r = rf_sqrt(nx);
        const float lensX = fp.camera.lensRadius * (r * cosPhi);
        const float lensY = fp.camera.lensRadius * (r * sinPhi);
        const Vec3  origin = fp.camera.origin + (lensX * fp.camera.right + lensY * fp.camera.up);
        const Vec3  dir = normalize(fp.camera.lowerLeftCorner + s * fp.camera.horizontal + t * fp.camera.vertical - origin);
        noise[k] = vec3(nx, cosPhi, sinPhi);

        // ---- intersect (kTraceLeafLists' body)
        const RayPrep   ray = prepareRay(o, dir);
        const PackedRay pr = packRay(ray);
        const uint32_t  signs = ray.negX | (ray.negY << 1) | (ray.negZ << 2);
        const bool      plain = classifyRay(ray) == kRayPlain;
        ListHit         best{kMiss, 0.0f, 0.0f, tMax};
        // (the lanes that are here -- the wave's slots that are pixels of the image -- and whether they all hold one pixel's samples)
        const uint32_t uRank = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(rank)));
        bool           walks;
        if (__ballot(rank != uRank) == 0ull)
        {
            const uint32_t word = ((ConstU32)lengths)[uRank];
            walks = (word & kNoPrimaryList) == 0u && plain && ((word >> 8) & 7u) == signs;
            if ((word & kNoPrimaryList) == 0u) walkLeafList<true>(scene, lists + static_cast<size_t>(uRank) * capacity, word & 0xFFu, o, dir, pr, walks, best);
        }
        else
        {
            const uint32_t word = lengths[rank];
            walks = (word & kNoPrimaryList) == 0u && plain && ((word >> 8) & 7u) == signs;
            if (walks) walkLeafList<false>(scene, lists + static_cast<size_t>(rank) * capacity, word & 0xFFu, o, dir, pr, true, best);
        }
        isHit[k] = walks && best.tri != kMiss;
        isMiss[k] = walks && best.tri == kMiss;
        handOn[k] = !walks;
        hitTri[k] = best.tri, hitU[k] = best.u, hitV[k] = best.v;
        // (a miss: its direction, for kSky; a ray handed on: what kRaygen writes, for kTraceWide and the listed kShade; a hit keeps everything in registers)
        if (!isHit[k]) store3(ps.rayD + j, dir);
        if (handOn[k])
        {
            queue[j] = slot;
            store3(ps.noise + j, noise[k]);
        }
    }
    uint32_t handedOn = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) handedOn += handOn[k] ? 1u : 0u;
    // kShade's appends: the hits know their position in the next queue before they are shaded; the misses carry queue position and slot
    blockAppend<kItems>(isHit, slots, hitQueue, hitCount, sScratch, &outPos);
    blockAppend<kItems>(isMiss, pos, missQueue, missCount, sScratch, nullptr, &slots, missSlots);
    blockAppend<kItems>(handOn, pos, fallback, fallbackCount, sScratch);

    // ---- shade the hits (kShade<false, false>'s pass 2: one entry at a time)
    bool needShadow[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) needShadow[k] = false;
    // (one entry at a time, as kShade<false, false>: unrolled -- 113 registers, the per-item arrays in registers instead of LDS -- the group measured 17.1 against 17.3 ms
    // and the frame the same: profiles/primary_fused)
#if defined(RF_EXP_FUSED_UNROLL)
#pragma unroll
#else
#pragma unroll 1
#endif
    for (int k = 0; k < kItems; ++k)
    {
        if (!isHit[k]) continue;
        const auto inputs = [&](Vec3& throughput, Vec3& nz) {
            throughput = vec3(1.0f, 1.0f, 1.0f); // wgsl:184
            nz = noise[k];
        };
        const bool need = shadeHit<false, false>(scene, sky, sunBasis, ps, sLut, true, isLastBounce, selfShadow, hitU[k], hitV[k], 0.0f, fetchShadeRecord<false>(scene, hitTri[k], selfShadow),
                                                 outPos[k], nullptr, inputs, [&] { return slots[k]; });
#pragma unroll
        for (int i = 0; i < kItems; ++i) needShadow[i] = i == k ? need : needShadow[i];
    }
    if (selfShadow) blockAppend<kItems>(needShadow, outPos, shadowList, shadowListCount, sScratch);
    // (rare: one atomic per wave that handed rays on)
    const unsigned long long sum = waveSum(static_cast<unsigned long long>(handedOn));
    if (__lane_id() == 0 && sum != 0ull) atomicAdd(&counters->primaryFallbackRays, sum);
}
} // namespace

namespace kern
{
PixelLeafListsKernel pixelLeafListsKernel() { return kPixelLeafLists; }
TraceLeafListsKernel traceLeafListsKernel() { return kTraceLeafLists; }
PrimaryFusedKernel   primaryFusedKernel() { return kPrimaryFused; }
} // namespace kern
} // namespace rf
