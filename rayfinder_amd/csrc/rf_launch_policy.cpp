// rf_launch_policy.cpp -- host only: see rf_launch_policy.hpp.  Pure arithmetic over the options and the facts the driver hands in.
#include "rf_launch_policy.hpp"

#include "rf_trace_wide_list.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace rf
{
void LaunchOptions::applySceneDefaults(const SceneFacts& f)
{
    optQuadHalfFromBounce = f.quadHalfFromBounce, optQuadHalfShadowFromBounce = f.quadHalfShadowFromBounce;
    optQuadLocalFromBounce = f.quadLocalFromBounce, optQuadLocalShadowFromBounce = f.quadLocalShadowFromBounce;
    optOctFromBounce = f.octFromBounce;
}

void LaunchOptions::applyEnvironment(bool wideUsable)
{
    if (const char* v = std::getenv("RF_TRAVERSAL_VARIANT")) traversalVariant = std::atoi(v);
    if (const char* v = std::getenv("RF_PACKET_BOUNCES")) optPacketBounces = static_cast<uint32_t>(std::max(std::atoi(v), 0)); // experiments: whole test suite through kTracePacket
    // soak runs (tools/gpu_fuzz.py): the leaf lists of bounce 1 for batches of any depth, at a given capacity -- what the options primary_list_min_samples / primary_list_capacity set per handle
    if (const char* v = std::getenv("RF_PRIMARY_LIST_MIN_SAMPLES")) optPrimaryListMinSamples = static_cast<uint32_t>(std::clamp(std::atoi(v), 1, 1 << 30));
    if (const char* v = std::getenv("RF_PRIMARY_LIST_CAPACITY")) optPrimaryListCapacity = static_cast<uint32_t>(std::clamp(std::atoi(v), 1, static_cast<int>(kPrimaryListMaxCapacity)));
    if (const char* v = std::getenv("RF_PRIMARY_FUSED")) optPrimaryFused = std::atoi(v) != 0; // (soak runs: the three bounce-1 launches against the fused one)
    if (!wideUsable) traversalVariant = 0;
}

bool LaunchOptions::set(const std::string& name, int64_t value, bool wideUsable)
{
    if (name == "traversal_variant") traversalVariant = wideUsable ? static_cast<int>(value) : 0;
    else if (name == "refill_min") optRefillMin = optRefillMinDeep = optRefillMinDeepDense = optRefillMinDeepQuad = static_cast<uint32_t>(value); // (all: a sweep of one value covers every launch)
    else if (name == "refill_min_deep") optRefillMinDeep = optRefillMinDeepDense = optRefillMinDeepQuad = static_cast<uint32_t>(value);
    else if (name == "refill_deep_from_bounce") optRefillDeepFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 1));
    else if (name == "leaf_vote") optLeafVote = optLeafVoteClosest = static_cast<uint32_t>(value);
    else if (name == "dense_leaf_min") optDenseLeafMin = static_cast<uint32_t>(std::clamp<int64_t>(value, 0, 15));
    else if (name == "dense_leaf_from_bounce") optDenseLeafFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 1));
    else if (name == "chunk") optChunk = optChunkEarly = static_cast<uint32_t>(std::clamp<int64_t>(value, 1, 1 << 20)); // (both, as refill_min)
    else if (name == "chunk_early") optChunkEarly = static_cast<uint32_t>(std::clamp<int64_t>(value, 1, 1 << 20));
    else if (name == "shade_sort_from_bounce") optShadeSortFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "chunk_early_bounces") optChunkEarlyBounces = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "sample_sort") optSampleSort = value != 0;
    else if (name == "accumulate_runs") optAccumulateRuns = value != 0;
    else if (name == "uniform_fetch") optUniformFetch = static_cast<int>(value);
    else if (name == "compact_from_bounce") optCompactFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "compact_shadow_from_bounce") optCompactShadowFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "query_compact") optQueryCompact = static_cast<int>(value);
    else if (name == "quad_from_bounce") optQuadFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "quad_shadow_from_bounce") optQuadShadowFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "quad_local_from_bounce") optQuadLocalFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "quad_local_shadow_from_bounce") optQuadLocalShadowFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "quad_half_from_bounce") optQuadHalfFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "quad_half_shadow_from_bounce") optQuadHalfShadowFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "quad_except_mask") optQuadExceptMask = static_cast<uint32_t>(value);
    else if (name == "quad_shadow_except_mask") optQuadShadowExceptMask = static_cast<uint32_t>(value);
    else if (name == "oct_from_bounce") optOctFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "hot_from_bounce") optHotFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "hot_shadow_from_bounce") optHotShadowFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "packet_bounces") optPacketBounces = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "shade_blocks") optShadeBlocks = static_cast<uint32_t>(value);
    else if (name == "const_primary_origin") optConstPrimaryOrigin = value != 0;
    else if (name == "shadow_self_test") optShadowSelfTest = value != 0;
    // bounce 1 over per-pixel leaf lists (rf_primary_lists.hip; planBatch says when): 0 keeps the kTraceWide launch alone -- same image either way
    else if (name == "primary_lists") optPrimaryLists = value != 0;
    else if (name == "primary_list_capacity") optPrimaryListCapacity = static_cast<uint32_t>(std::clamp<int64_t>(value, 1, kPrimaryListMaxCapacity));
    // ... generated, walked and shaded by one kernel (kPrimaryFused; planBatch says when): 0 keeps kRaygen, kTraceLeafLists and kShade -- same image either way
    else if (name == "primary_fused") optPrimaryFused = value != 0;
    else if (name == "primary_list_min_samples") optPrimaryListMinSamples = static_cast<uint32_t>(std::clamp<int64_t>(value, 1, 1 << 30));
    // 0 (default): sin / cos / acos / exp / pow as the f32 rounding of a specified f64 evaluation (bit-identical to the test oracle); 1: the device math library's f32 functions
    // (kRaygen's lens / cone angle, kSky's dome: rf_device.hpp tSin ...), graded by SURVEY 8(d)'s tolerance.  Set it before the first sample of an accumulation.
    else if (name == "transcendentals") optTranscendentalsF32 = value != 0;
    else if (name == "dense_raygen") optDenseRaygen = value != 0; // 0: kRaygen appends to the first queue with one atomic per 1 024 slots (until round 6)
    else if (name == "slot_group_shift") optSlotGroupShift = value < 0 || value > 10 ? kSlotSampleMajor : static_cast<uint32_t>(value); // -1: sample-major
    else if (name == "shadow_nearest_first") shadowNearestFirst = value != 0;
    else if (name == "shadow_sign_order" || name == "shadow_record_order") optShadowSignOrder = value != 0;
    else if (name == "shadow_first_look_from_bounce") optShadowFirstLookFromBounce = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "occluder_grid_log2_cells") optOccluderGridLog2Cells = static_cast<uint32_t>(std::clamp<int64_t>(value, 4, 26));
    else if (name == "occluder_grid_cells") optOccluderGridCells = static_cast<uint32_t>(std::clamp<int64_t>(value, 0, 1 << 16));
    else if (name == "occluder_cache_bounces") optOccluderCacheBounces = static_cast<uint32_t>(std::max<int64_t>(value, 0));
    else if (name == "query_variant") queryVariant = wideUsable ? static_cast<int>(value) : 0;
    else if (name == "cast_chunk") optCastChunk = static_cast<uint32_t>(std::clamp<int64_t>(value, 0, 0xFFFFFFFFll));
    else if (name == "extra_lds") optExtraLds = static_cast<uint32_t>(std::max<int64_t>(value, 0)); // (the driver then sizes its persistent grid again: Renderer::setOption)
    else return false;
    return true;
}

bool traceWideInstantiated(bool anyHit, bool count, bool nearest, int layout, bool dense)
{
#define RF_TW(A, C, N, L, D) \
    if (anyHit == A && count == C && nearest == N && layout == L && dense == D) return true;
    RF_TRACE_WIDE_INSTANTIATIONS(RF_TW)
#undef RF_TW
    return false;
}

int layoutIfPresent(const PolicyInputs& in, int want)
{
    switch (want)
    {
    case kLayoutOct: return in.has(kLayoutOct) ? want : kLayoutBinary;
    case kLayoutQuadLocal: return in.has(kLayoutQuadLocal) ? want : kLayoutBinary;
    case kLayoutQuadHalf: return in.has(kLayoutQuadHalf) ? want : kLayoutBinary;
    case kLayoutQuad: return in.has(kLayoutQuad) ? want : kLayoutBinary;
    case kLayoutHot: return in.has(kLayoutHot) ? want : kLayoutBinary;
    case kLayoutCompact: return in.has(kLayoutCompact) ? want : kLayoutBinary;
    default: return kLayoutBinary;
    }
}

bool primaryListsPossible(const LaunchOptions& o, const PolicyInputs& in) { return o.optPrimaryLists && !o.counting && o.traversalVariant != 0 && in.facts.selfShadowOk && in.facts.leafBoxesValid; }

uint64_t primaryListBytesWanted(const LaunchOptions& o, const PolicyInputs& in, uint64_t pixels)
{
    return primaryListsPossible(o, in) ? pixels * (std::min(std::max(o.optPrimaryListCapacity, 1u), kPrimaryListMaxCapacity) + 1ull) * sizeof(uint32_t) : 0u;
}

namespace
{
// does a launch with these flags want the dense leaf phase?  (the scene has a leaf as long as the threshold the flags carry: the instantiations that
// contain the block -- the layouts the renderer picks by itself -- are used only then: its mere presence costs a launch 2.5 %, profiles/r05_leaf)
bool denseWanted(const PolicyInputs& in, uint32_t flags)
{
    const uint32_t threshold = (flags >> kFlagDenseLeafShift) & 15u;
    return threshold != 0u && in.facts.maxLeafTriangles >= threshold;
}
// the conservative layouts (VALU bound): the half-precision and the local-grid quad records
bool conservativeLayout(int layout) { return layout == kLayoutQuadLocal || layout == kLayoutQuadHalf; }
// the layouts whose any-hit launch can work through a list of queue positions (the kTraceWide instantiations with the occluder-cache code: quad / half / local-grid records)
bool worksThroughList(int layout) { return layout == kLayoutQuad || layout == kLayoutQuadHalf || layout == kLayoutQuadLocal; }
} // namespace

TraversalPlan resolveTraversal(const LaunchOptions& o, const PolicyInputs& in, bool anyHit, int layout, bool count, bool nearest, uint32_t flags, uint32_t refillMin, uint32_t chunk,
                               uint32_t leafVote, uint32_t extraLds)
{
    TraversalPlan t{};
    t.kernel = layout == kLayoutScalar ? kKernelScalar : (layout == kLayoutPacket ? kKernelPacket : kKernelWide);
    t.layout = layout, t.anyHit = anyHit, t.count = count, t.flags = flags;
    if (t.kernel != kKernelWide) return t;
    if (count) t.layout = kLayoutBinary, t.nearest = anyHit && nearest;
    else if (!anyHit) t.layout = layout <= kLayoutOct ? layout : kLayoutBinary;
    else
    {
        t.layout = (layout <= kLayoutQuadLocal) ? layout : kLayoutBinary;
        t.nearest = (t.layout == kLayoutCompact || t.layout == kLayoutHot) ? true : nearest;
    }
    t.dense = !count && denseWanted(in, flags) && traceWideInstantiated(anyHit, false, t.nearest, t.layout, true);
    t.refillMin = refillMin, t.chunk = chunk, t.leafVote = leafVote ? leafVote : o.optLeafVote, t.extraLds = extraLds; // (leafVote 0: optLeafVote)
    return t;
}

int closestLayoutFor(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce)
{
    if (o.traversalVariant == 0) return kLayoutScalar;
    if (o.counting) return kLayoutBinary;
#if defined(RF_EXP_LEGACY_LAYOUTS)
    if (bounce <= o.optPacketBounces) return kLayoutPacket;
#endif
    const bool  quadNow = in.has(kLayoutQuad) && o.optQuadFromBounce != 0u && bounce >= o.optQuadFromBounce && !((o.optQuadExceptMask >> std::min(bounce - 1u, 31u)) & 1u);
    // A camera that stands outside the conservative records' origin bound (4 R + 1 for a root box within +-R: a turntable shot from far away) would
    // send EVERY primary ray to the scalar traversal (2 x the launch, tools/gpu_far_camera.py): that launch reads the exact quad records, which have
    // no such bound.  Later bounces start on surfaces, inside the bound.
    const float camReach = std::max({std::fabs(in.camera.origin.x), std::fabs(in.camera.origin.y), std::fabs(in.camera.origin.z)}) + (std::fabs(in.camera.lensRadius) * 2.0f);
    const bool  primaryOutside = bounce == 1u && !(camReach <= in.originBound);
    if (quadNow && !primaryOutside)
    {
        if (in.has(kLayoutOct) && o.optOctFromBounce != 0u && bounce >= o.optOctFromBounce) return kLayoutOct;
        if (in.has(kLayoutQuadHalf) && o.optQuadHalfFromBounce != 0u && bounce >= o.optQuadHalfFromBounce) return kLayoutQuadHalf;
        if (in.has(kLayoutQuadLocal) && o.optQuadLocalFromBounce != 0u && bounce >= o.optQuadLocalFromBounce) return kLayoutQuadLocal;
    }
    if (quadNow) return kLayoutQuad;
    if (in.has(kLayoutHot) && o.optHotFromBounce != 0u && bounce >= o.optHotFromBounce) return kLayoutHot;
    if (in.has(kLayoutCompact) && o.optCompactFromBounce != 0u && bounce >= o.optCompactFromBounce) return kLayoutCompact;
    return kLayoutBinary;
}

int shadowLayoutFor(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce)
{
    if (o.traversalVariant == 0) return kLayoutScalar;
#if defined(RF_EXP_LEGACY_LAYOUTS)
    if (!o.counting && bounce <= o.optPacketBounces) return kLayoutPacket;
#endif
    if (o.counting || !o.shadowNearestFirst) return kLayoutBinary;
    const bool quadShadowNow = o.optQuadShadowFromBounce != 0u && bounce >= o.optQuadShadowFromBounce && !((o.optQuadShadowExceptMask >> std::min(bounce - 1u, 31u)) & 1u);
    if (quadShadowNow)
    {
        if (in.has(kLayoutQuadLocal) && o.optQuadLocalShadowFromBounce != 0u && bounce >= o.optQuadLocalShadowFromBounce) return kLayoutQuadLocal;
        if (in.has(kLayoutQuadHalf) && o.optQuadHalfShadowFromBounce != 0u && bounce >= o.optQuadHalfShadowFromBounce) return kLayoutQuadHalf;
        if (in.has(kLayoutQuad)) return kLayoutQuad;
    }
    if (in.has(kLayoutHot) && o.optHotShadowFromBounce != 0u && bounce >= o.optHotShadowFromBounce) return kLayoutHot;
    if (in.has(kLayoutCompact) && o.optCompactShadowFromBounce != 0u && bounce >= o.optCompactShadowFromBounce) return kLayoutCompact;
    return kLayoutBinary;
}

bool cachedShadowFor(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce)
{
    const int layout = shadowLayoutFor(o, in, bounce);
    const bool exactQuad = layout == kLayoutQuad && in.facts.leafBoxesValid; // (its leaf visits then apply the box in the leaf's triangle record)
    return layout != kLayoutScalar && layout != kLayoutPacket && !o.counting && o.shadowNearestFirst && (conservativeLayout(layout) || exactQuad) && bounce <= o.optOccluderCacheBounces &&
           o.optOccluderGridCells != 0u;
}

BatchPlan planBatch(const LaunchOptions& o, const PolicyInputs& in, uint32_t numSamples)
{
    BatchPlan b{};
    const ActiveTiles* active = in.active ? &*in.active : nullptr;
    const uint64_t validPixels = active ? active->validPixels : in.validPixels;
    b.numSamples = numSamples;
    b.numBounces = in.numBounces;
    b.numTiles = active ? active->numTiles : in.numTiles;
    b.pixelsPadded = b.numTiles * 1024u;
    // (kSamplePermutation ranks by counting, O(S^2): fine for the few hundred samples a batch of a real frame holds,
    // skipped for the huge sample counts a tiny frame can put into one batch)
    b.samplePerm = o.optSampleSort && numSamples > 1 && numSamples <= 8192 && o.optSlotGroupShift != kSlotSampleMajor;
    // Pinhole camera (lensRadius == 0): kRaygen's origin = camera.origin + (0 * right + 0 * up) is camera.origin itself for every path, bit for bit, as long as no
    // component of camera.origin is a zero (whose sign the +-0 addend could flip) and right / up are finite (0 * inf = NaN).  The primary launch then takes it as a kernel
    // argument and kRaygen writes 28 instead of 40 bytes per path.  Only the wide traversal kernels know the flag (the scalar kernels read ps.rayO).
    const auto finite3 = [](Vec3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); };
    const Camera& camNow = in.camera;
    b.primaryLayout = closestLayoutFor(o, in, 1);
    b.constOrigin = o.optConstPrimaryOrigin && camNow.lensRadius == 0.0f && camNow.origin.x != 0.0f && camNow.origin.y != 0.0f && camNow.origin.z != 0.0f &&
                    finite3(camNow.origin) && finite3(camNow.right) && finite3(camNow.up) && b.primaryLayout != kLayoutScalar && b.primaryLayout != kLayoutPacket;
    // (kRaygen computes its queue positions instead of appending with one atomic per 1 024 slots, where the slot order allows it: FrameParams::tileValidBefore)
    b.denseRaygen = o.optDenseRaygen && (o.optSlotGroupShift == 0u || o.optSlotGroupShift == kSlotSampleMajor) && static_cast<uint64_t>(validPixels) * numSamples <= 0xFFFFFFFFull;
    // Bounce 1 over per-pixel leaf lists: one origin for the whole batch (constOrigin: a pinhole camera, primary launch on kTraceWide), the scene's gates
    // (primaryListsPossible), a queue in which a pixel's samples are contiguous by the pixel's rank (dense kRaygen, pixel-major slots), at least one bounce, and enough
    // samples per pixel for the once-per-pixel walk to pay.  A thin-lens camera, a counting build and small batches keep the kTraceWide launch alone.
    b.primaryListCapacity = std::min(std::max(o.optPrimaryListCapacity, 1u), kPrimaryListMaxCapacity);
    b.primaryLists = primaryListsPossible(o, in) && b.constOrigin && b.denseRaygen && o.optSlotGroupShift == 0u && b.numBounces != 0u && numSamples >= std::max(o.optPrimaryListMinSamples, 1u);
    // ... fused with generation and shading (kPrimaryFused): the instantiation that exists writes no AOV records and evaluates sin / cos as specified
    b.primaryFused = b.primaryLists && o.optPrimaryFused && !in.aovs && !o.optTranscendentalsF32;
    b.occluderGrid = o.optOccluderCacheBounces != 0u && o.optOccluderGridCells != 0u;
    if (b.occluderGrid)
    {
        b.occluderGridEntries = (uint64_t{1} << o.optOccluderGridLog2Cells) * kOccSlots;
        const float extent = std::max({in.rootHi.x - in.rootLo.x, in.rootHi.y - in.rootLo.y, in.rootHi.z - in.rootLo.z, 1e-20f});
        b.occScale = static_cast<float>(o.optOccluderGridCells) / extent;
        b.occMask = static_cast<uint32_t>(b.occluderGridEntries / kOccSlots - 1);
    }
    // The sums in sample order.  Where the slot order is pixel-major and the step long enough, the LDS-staged "runs" kernels (a 64-lane workgroup per
    // `pixelsPerGroup` pixels); else one thread per pixel
    b.runs = o.optSlotGroupShift == 0u && numSamples > 4u && o.optAccumulateRuns;
    b.tileList = active != nullptr;
    b.shardList = b.tileList && active->shardSlots;
    const uint32_t perThread = static_cast<uint32_t>(kBlock);
    if (b.tileList) b.accumulateKernel = kAccumulateTiles, b.accumulatePixels = b.runs ? kMomentPixels : perThread;
    else if (b.runs && numSamples <= kAccMaxSamples)
    {
        // (pixels per workgroup by the LDS their runs take: <= ~8 KB per workgroup keeps twenty of them resident per CU)
        b.accumulateKernel = kAccumulateRuns, b.accumulatePixels = numSamples > 640u ? 1u : (numSamples > 160u ? 2u : kAccPixels);
    }
    else b.accumulateKernel = kAccumulatePixels, b.accumulatePixels = perThread;
    // the first-hit AOV sums (no bounce, no primary hit: the records were not written): a launch of their own, under a tile list the tile-list AOV kernel; the
    // radiance second moments: a launch of their own unless the tile-list kernel adds them with the image
    b.aovPixels = (in.aovs && b.numBounces != 0u) ? (b.runs ? kAovPixels : perThread) : 0u;
    b.momentPixels = (!b.tileList && in.moments) ? (b.runs ? kMomentPixels : perThread) : 0u;
    // the bucket sums (under a tile list -- kBucketsTileCounts, checkAdaptive -- their tile-list kernels, under a shard's -- kBucketsShardTileCounts -- their
    // slot-list kernels: every active tile holds bucketSamples samples, so one phase serves the list): the batch's first sample has ordinal bucketSamples
    b.bucketPixels = in.buckets ? (b.runs ? kBucketPixels : perThread) : 0u;
    b.buckets = in.buckets ? in.bucketPlanes : 0u;
    b.bucketPhase = in.buckets ? in.bucketSamples % in.bucketPlanes : 0u;
    return b;
}

BouncePlan planBounce(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce, const BatchPlan& batch)
{
    BouncePlan p{};
    const uint32_t uniformFlag = ((o.optUniformFetch < 0 ? bounce <= 2 : o.optUniformFetch > 0) ? kFlagUniformFetch : 0u) | (o.optUniformFetch >= 2 ? kFlagUniformTri : 0u) |
                                 (bounce >= o.optDenseLeafFromBounce ? (std::min(o.optDenseLeafMin, 15u) << kFlagDenseLeafShift) : 0u);
    // incoherent closest-hit launches refill earlier: their rays differ most in length, so lanes go idle sooner (per-bounce
    // sweep, profiles/r02_final/bounce_sweep*.log: bounces 3-8 -4 % at 20-24 idle lanes, bounces 1-2 and the shadow launches +6 .. +10 %)
    // ... and the coherent launches of the first bounces, whose rays are short and alike, claim larger chunks (one cursor atomic = one
    // wave-wide stall: bounce 1 -4 % at 256 entries, the deep bounces +0.5 %)
    const uint32_t chunkNow = bounce <= o.optChunkEarlyBounces ? o.optChunkEarly : o.optChunk;
    const int      layoutClosest = closestLayoutFor(o, in, bounce);
    // (scenes with long leaves -- the DENSE_LEAVES instantiations -- keep 22: a phase over dense (lane, triangle) pairs wants many parked lanes; clutter atrium +2.4 % at 12: profiles/r06_lanes)
    const uint32_t refillClosest = bounce >= o.optRefillDeepFromBounce ? (layoutClosest == kLayoutQuad ? o.optRefillMinDeepQuad : (denseWanted(in, uniformFlag) ? o.optRefillMinDeepDense : o.optRefillMinDeep)) : o.optRefillMin;
    // (kInfinityCacheBytes: the scene's records + triangles against the 256-MB Infinity Cache, as the layout selector's own test)
    const uint32_t leafVoteClosest = (!o.counting && !denseWanted(in, uniformFlag) && in.facts.treeBytes <= (192ull << 20)) ? o.optLeafVoteClosest : 0u;
    const bool     wideClosest = layoutClosest != kLayoutScalar && layoutClosest != kLayoutPacket; // (the other two kernels take no flags)
    p.closest = resolveTraversal(o, in, false, layoutClosest, o.counting, false, wideClosest ? (uniformFlag | (bounce == 1 && batch.constOrigin ? kFlagConstOrigin : 0u)) : 0u,
                                 o.counting ? o.optRefillMin : refillClosest, chunkNow, leafVoteClosest, o.counting ? 0u : o.optExtraLds);
    // kShade's own-triangle test of the shadow rays (kShadeSelfShadow): wherever this bounce's any-hit launch is one that can work through a list of queue positions
    // and nothing has to be counted node by node
    const int layoutShadow = shadowLayoutFor(o, in, bounce);
    // (bounce <= 64: kBounceTotals keeps one mask bit per bounce -- as for firstLook below; deeper bounces trace every shadow ray and count them in the launch: ADVICE r5)
    p.selfShadow = o.optShadowSelfTest && in.facts.selfShadowOk && !o.counting && bounce <= 64u && worksThroughList(layoutShadow);
    // (the first-hit AOVs are written by the unsorted bounce-1 kernel, whatever shade_sort_from_bounce says: the sort is a scheduling choice)
    p.shadeAov = in.aovs && bounce == 1;
    p.shadeSorted = !p.shadeAov && o.optShadeSortFromBounce != 0u && bounce >= o.optShadeSortFromBounce;
    p.shadeFlags = (bounce == batch.numBounces ? kShadeLastBounce : 0u) | (bounce == 1 ? kShadeFirstBounce : 0u) | (p.selfShadow ? kShadeSelfShadow : 0u);
    p.sortScale = p.shadeSorted ? in.facts.sortScale : 0u;
    p.skyFirstBounce = bounce == 1 ? 1u : 0u;
    p.itemGridCap = o.optShadeBlocks;
    // occluder cache (kTraceWide, kFlagOccluderCache): the conservative-record any-hit launches of bounces 1..optOccluderCacheBounces; their rays are
    // short (a third of the steps), so the deep launches refill earlier
    p.cached = cachedShadowFor(o, in, bounce);
    // ... behind kShadowFirstLook (see there) from the second batch on: the first batch of a renderer fills the grid (the traversal kernel's own first look serves)
    p.firstLook = p.cached && in.facts.occluderHintLevels == 0u && o.optShadowFirstLookFromBounce != 0u && bounce >= o.optShadowFirstLookFromBounce && bounce <= 64u && batch.firstLookReady;
    p.shadowSource = p.firstLook ? kFromLookList : (p.selfShadow ? kFromShadeList : kFromQueue);
    p.lookFlags = p.firstLook ? ((bounce == 1 ? kLookFirstBounce : 0u) | (p.selfShadow ? kLookNoRayCount : 0u)) : 0u;
    const uint32_t shadowFlags = (bounce == 1 ? kFlagFirstBounce : 0u) | uniformFlag | (p.cached ? kFlagOccluderCache : 0u) | (p.firstLook ? (kFlagOccluderNoTry | kFlagNoRayCount) : 0u) | (p.selfShadow ? kFlagNoRayCount : 0u);
    // the conservative layouts (VALU bound) visit a record's entries in record order unless asked otherwise; the exact and binary records nearest-first
    const bool nearest = o.shadowNearestFirst && !(conservativeLayout(layoutShadow) && o.optShadowSignOrder);
    // (the one-ray-per-thread kernel takes "first bounce" alone, the packet kernel that bit of the flag word)
    const uint32_t flagsRun = layoutShadow == kLayoutScalar ? (bounce == 1 ? 1u : 0u) : (layoutShadow == kLayoutPacket ? (shadowFlags & kFlagFirstBounce) : shadowFlags);
    p.shadow = resolveTraversal(o, in, true, layoutShadow, o.counting, nearest, flagsRun, o.optRefillMin, chunkNow, 0u, o.counting ? 0u : o.optExtraLds);
    return p;
}

TraversalPlan planRayQuery(const LaunchOptions& o, const PolicyInputs& in, bool anyHit)
{
    constexpr uint32_t kIncoherentBounce = 2u;
    PolicyInputs       q = in;
    q.numBounces = std::max(in.numBounces, kIncoherentBounce); // (bounce 2 is then never "the last bounce"; the traversal plans do not read it)
    q.active.reset();
    BatchPlan batch = planBatch(o, q, 1u);
    batch.firstLookReady = false;
    const BouncePlan p = planBounce(o, q, kIncoherentBounce, batch);
    TraversalPlan    t = anyHit ? p.shadow : p.closest;
    if (!in.facts.wideUsable || t.kernel != kKernelWide)
    {
        t = TraversalPlan{};
        t.kernel = kKernelScalar, t.layout = kLayoutScalar, t.anyHit = anyHit;
        return t;
    }
    // (an any-hit launch without the cache applies the exact quad records' boxes at the parent's step, as its uncached launches in the render path do)
    t.flags &= ~(kFlagOccluderCache | kFlagOccluderNoTry | kFlagNoRayCount | kFlagFirstBounce | kFlagConstOrigin);
    if (anyHit) t.flags |= kFlagShadowDirFromStream;
    return t;
}

void writeLaunchPlan(const BatchPlan& batch, const BouncePlan& p, uint32_t bounce, rf_launch_plan& out)
{
    const BatchCounters words{nullptr, batch.numBounces};
    static_assert(sizeof(rf_launch_plan) == 52 * sizeof(uint32_t) && offsetof(rf_launch_plan, closest_extra_lds) - offsetof(rf_launch_plan, closest_kernel) == 9 * sizeof(uint32_t) &&
                  offsetof(rf_launch_plan, shadow_extra_lds) - offsetof(rf_launch_plan, shadow_kernel) == 9 * sizeof(uint32_t));
    out = rf_launch_plan{};
    out.num_samples = batch.numSamples, out.num_bounces = batch.numBounces;
    out.sample_perm = batch.samplePerm, out.dense_raygen = batch.denseRaygen, out.const_origin = batch.constOrigin, out.primary_layout = static_cast<uint32_t>(batch.primaryLayout);
    out.occluder_grid = batch.occluderGrid, out.occluder_mask = batch.occMask;
    std::memcpy(&out.occluder_scale_bits, &batch.occScale, sizeof(uint32_t));
    out.runs = batch.runs, out.tile_list = batch.tileList, out.accumulate_kernel = batch.accumulateKernel, out.accumulate_pixels = batch.accumulatePixels;
    out.aov_pixels = batch.aovPixels, out.moment_pixels = batch.momentPixels, out.raygen_count_word = words.queueWord(0);
    const auto traversal = [](const TraversalPlan& t, uint32_t* w) { // the ten words of a traversal launch, in the struct's order
        const uint32_t v[10] = {t.kernel, static_cast<uint32_t>(t.layout), t.count, t.nearest, t.dense, t.refillMin, t.chunk, t.leafVote, t.flags, t.extraLds};
        std::memcpy(w, v, sizeof v);
    };
    traversal(p.closest, &out.closest_kernel);
    out.closest_count_word = words.queueWord(bounce - 1), out.closest_cursor_word = p.closest.kernel == kKernelWide ? words.cursorClosestWord(bounce) : 0u;
    out.shade_sorted = p.shadeSorted, out.shade_aov = p.shadeAov, out.shade_flags = p.shadeFlags, out.shade_sort_scale = p.sortScale, out.shade_grid_cap = p.itemGridCap;
    traversal(p.shadow, &out.shadow_kernel);
    out.shadow_count_word = words.shadowCountWord(bounce, p.shadowSource);
    out.shadow_cursor_word = p.shadow.kernel == kKernelWide ? words.cursorShadowWord(bounce) : 0u;
    out.shadow_cached = p.cached, out.shadow_first_look = p.firstLook, out.shadow_self = p.selfShadow, out.shadow_source = p.shadowSource, out.look_flags = p.lookFlags;
    if (p.firstLook) out.look_count_word = words.shadowCountWord(bounce, p.selfShadow ? kFromShadeList : kFromQueue), out.look_list_word = words.listWord(bounce);
}

void writeLayoutInfo(const LaunchOptions& o, const PolicyInputs& in, uint32_t (&layouts)[48], uint32_t (&misc)[4], float& quadHalfAreaRatio, uint64_t& treeBytes)
{
    const BatchPlan batch = planBatch(o, in, 1u);
    for (uint32_t b = 1; b <= 16; ++b)
    {
        const BouncePlan p = planBounce(o, in, b, batch);
        layouts[b - 1] = static_cast<uint32_t>(p.closest.layout);
        layouts[16 + b - 1] = static_cast<uint32_t>(p.shadow.layout);
        layouts[32 + b - 1] = p.cached ? 1u : 0u;
    }
    misc[0] = in.facts.occluderHintLevels, misc[1] = o.optShadowFirstLookFromBounce, misc[2] = o.optDenseLeafMin;
#if defined(RF_EXP_LEGACY_LAYOUTS)
    misc[3] = 1u;
#else
    misc[3] = 0u;
#endif
    quadHalfAreaRatio = in.facts.quadHalfAreaRatio;
    treeBytes = in.facts.treeBytes;
}
} // namespace rf
