// rf_launch_policy.hpp -- host only: the launch policy of the wavefront path tracer and its options.  planBatch (once per batch) and planBounce (once per bounce) are
// the only places that decide which kernel runs with which parameters, and BatchCounters is the only place that knows the words of queueCounts; the driver
// (rf_renderer.hip: traceBatch and its launch members) enqueues what the plans say.  The plans hold no pointer, and planning enqueues nothing and touches no device
// memory: rf_renderer_launch_plan reads the same plans out.  No HIP runtime call: the unit links into a program without libamdhip64 (tests/launch_policy_main.cpp).
#pragma once

#include "rayfinder_amd.h"
#include "rf_launch_constants.hpp"
#include "rf_scene_pack.hpp"
#include "rf_types.hpp"

#include <cstdint>
#include <optional>
#include <string>

namespace rf
{
// Every knob of the policy: what rf_renderer_set_option, rf_renderer_set_counting, the scene's defaults and the environment set.  The comments are the record of what
// was measured.
struct LaunchOptions
{
    bool     optDenseRaygen = true;
    bool     counting = false;
    int      traversalVariant = 2; // 0 = one ray per thread over 32-B nodes (A/B baseline), 2 = persistent waves over 64-B wide nodes
    int      queryVariant = 0; // 2: rf_renderer_intersect_rays / _occluded_rays run through kTraceWide (test hook; no per-ray counters)
    bool     shadowNearestFirst = true; // shadow rays: nearest child first (visibility is order independent)
    // the cached any-hit launches of bounce >= this run behind kShadowFirstLook (0: never).  From bounce 2: the coherent launch of bounce 1 costs less per ray than
    // a pass over the queue does (atrium -4 %, Duck +14 % with it: profiles/r04_occluder/firstlook_scenes2.log)
    uint32_t optShadowFirstLookFromBounce = 2;
    uint32_t optOccluderGridLog2Cells = 22; // table size: 2^n cells of kOccSlots words
    uint32_t optOccluderGridCells = 1024; // occluder grid: cells along the longest axis of the root box (0: no occluder cache)
    uint32_t optOccluderCacheBounces = 64; // the any-hit launches of bounces 1..n first visit the leaves their ray's cell of the occluder grid names (kFlagOccluderCache)
    bool     optShadowSignOrder = true; // the half-precision / local-grid shadow launches (VALU bound) visit entries in record order: a cheaper step beats the shorter walks of nearest-first there
    uint32_t optRefillMin = kRefillMin, optLeafVote = kLeafVote, optChunk = kChunk;
    // closest-hit launches of scenes without long leaves whose tree stays cache resident leave the descend loop later (round 6: 14 instead of 20 lanes still descending; plain atrium
    // closest-hit -1.5 %, Duck -1.4 %; the dense-leaf instantiations +4.7 % and the out-of-cache scene +1 % with it: they keep 20 -- profiles/r06_lanes/ab_leaf_vote*.log)
    uint32_t optLeafVoteClosest = 14;
    // leaf phases in which a parked lane holds this many triangles or more run over dense (lane, triangle) pairs (kTraceWide; 0: never), from this bounce on
    uint32_t optDenseLeafMin = 5, optDenseLeafFromBounce = 1; // (5: the plain atrium's leaves of up to 4 triangles keep the loop -- 3 measured +1 % there; the clutter scene gains the same with 2 .. 5)
    uint32_t optShadeSortFromBounce = 2;                        // kShade of bounce >= this appends its tile's hits in triangle order (0: never)
    uint32_t optChunkEarly = 256, optChunkEarlyBounces = 2;      // queue entries per cursor claim at bounces 1-2
    uint32_t optRefillMinDeep = 12, optRefillMinDeepDense = 22, optRefillMinDeepQuad = 40, optRefillDeepFromBounce = 2; // closest-hit launches of bounce >= 2 (3 until the eager-leaves schedule: bounce 2 -2.6 % with it) refill at another count: 12 idle lanes (22 until round 6: with the
                                                                                             // refill trip's claim logic on the scalar unit and its one-test classification, 16 ... 4 measure the same and 1.3 % under 22: profiles/r06_lanes) on the 64-byte and the
                                                                                             // half-precision quad records (VALU bound: idle lanes cost most), 40 on the exact quad records (L1 bound: a refill is a wave-wide stall)
    // kShade grid cap (0: one workgroup per tile of 1024 entries, the default: workgroups then append to the hit queue in
    // roughly queue order, which keeps neighbouring pixels' rays together -- a capped, grid-striding kShade saved its empty
    // workgroups but cost the traversal kernels 2-5 %)
    uint32_t optShadeBlocks = 0;
    bool     optTranscendentalsF32 = false; // option `transcendentals`: kRaygen / kSky call the f32 math library instead of the specified f64 evaluation (opt-in)
    bool     optShadowSelfTest = true; // kShade tests every shadow ray against the triangle it starts on first (kShadeSelfShadow); needs selfShadowOk
    bool     optConstPrimaryOrigin = true; // a pinhole camera's primary launch takes its one origin as a kernel argument (kFlagConstOrigin): kRaygen writes no origins
    // Bounce 1 over per-pixel leaf lists (rf_primary_lists.hip; option primary_lists, default on): where the plan selects them (planBatch) kPixelLeafLists walks the tree once per
    // pixel and kTraceLeafLists gives every sample the exact tests of the few leaves on its pixel's list; what the lists do not cover takes the bounce's kTraceWide launch.
    // primary_list_capacity: entries per pixel (a longer list: no list for that pixel); primary_list_min_samples: batches with fewer samples per pixel keep the old launch
    // (the list pass costs a few rays' worth per pixel: profiles/primary_lists/README.md)
    bool     optPrimaryLists = true;
    uint32_t optPrimaryListCapacity = 64, optPrimaryListMinSamples = 16;
    // ... with generation, list walk and shading of a path in ONE kernel (kPrimaryFused; option primary_fused, default on): where the lists run, the AOVs are off and
    // `transcendentals` is the default.  Bounce 1's three streaming kernels handed each path to each other through memory; 0 keeps them (profiles/primary_fused/README.md)
    bool     optPrimaryFused = true;
    bool                   optSampleSort = true, optAccumulateRuns = true;
    uint32_t               optCompactFromBounce = 3;       // closest-hit launches of bounce >= this use the compact-capable records (0: never)
    uint32_t               optCompactShadowFromBounce = 2; // ... and the shadow launches of bounce >= this
    uint32_t               optQuadFromBounce = 1, optQuadShadowFromBounce = 1; // the 128-byte quad records (two levels per fetch) from this bounce on (0: never); takes precedence over the others
    uint32_t               optQuadExceptMask = 0, optQuadShadowExceptMask = 0; // ... except at the bounces whose bit (bounce - 1) is set here
    uint32_t               optQuadHalfFromBounce = 0, optQuadHalfShadowFromBounce = 0; // quad launches of bounce >= this read the 64-byte half-precision quad records (0: never; set to 1 at upload when the scene suits them)
    uint32_t               optQuadLocalFromBounce = 0, optQuadLocalShadowFromBounce = 0; // ... the 64-byte local-grid quad records (0: never; set to 1 at upload when the half-precision ones do not suit the scene)
    // closest-hit launches of bounce >= this read the 128-byte oct records (three levels per fetch; 0: never -- the default: measured slower, see the upload)
    uint32_t               optOctFromBounce = 0;
    uint32_t               optHotFromBounce = 0, optHotShadowFromBounce = 0; // the 32-byte records (all six planes carried) from this bounce on (0: never); takes precedence
    int                    optQueryCompact = 0;            // the ray-query entry points use the compact-capable (1) / 32-byte (2) records too (tests)
    uint32_t               optExtraLds = 0;      // experiment: dynamic LDS bytes added to the kTraceWide launches (lowers the occupancy)
    uint32_t               optPacketBounces = 0; // bounces 1..n traced by kTracePacket (one wave = one lockstep packet) instead of kTraceWide
    int                    optUniformFetch = 2; // scalar-cache fetch for wave-uniform steps: 0 = never (5 878 Mrays/s), 1 = records (6 039), 2 = records + leaf triangles (6 059), -1 = records at bounces 1-2 only
    uint32_t optCastChunk = 0; // option cast_chunk: rf_renderer_cast_rays traces at most this many rays per chunk (0: what the path depth and the free memory allow; tests force many small chunks)
    uint32_t optSlotGroupShift = 0; // see FrameParams::slotGroupShift (r02 A/B on the atrium, Mrays/s: sample-major 5282; unsorted g = 6: 5416, 2: 5507, 0: 5450; with sorted samples g = 2: 5519, 1: 5589, 0: 5650)

    // the layouts the scene gets with no option set (SceneFacts: the five *FromBounce defaults)
    void applySceneDefaults(const SceneFacts& facts);
    // RF_TRAVERSAL_VARIANT, RF_PACKET_BOUNCES, RF_PRIMARY_LIST_MIN_SAMPLES, RF_PRIMARY_LIST_CAPACITY, RF_PRIMARY_FUSED (experiments and soak runs), then the clamp of a scene whose
    // boxes the wide kernels cannot serve.  A new handle: applySceneDefaults, then this
    void applyEnvironment(bool wideUsable);
    // rf_renderer_set_option's names, but for the ones that need the device (rf_renderer.hip: Renderer::setOption).  false: a name it does not know
    bool set(const std::string& name, int64_t value, bool wideUsable);
};

// The tile list a batch of rf_renderer_render_adaptive traces: while one is in use, tileIds / tileValidBefore hold IT (uploadTileList) and not the shard's list
struct ActiveTiles
{
    uint32_t numTiles;
    uint64_t validPixels;
    bool     shardSlots; // the sums are addressed through the slots behind the ids (rf_comm_render_adaptive: the handle's sums are compact over its shard)
};

// Everything else the plans read, as the driver's state stands (rf_renderer.hip: Impl::policyInputs)
struct PolicyInputs
{
    SceneFacts facts;
    uint32_t   layouts = 0; // the record layouts the scene has on the device: bit kLayout* (binary always; compact and hot in RF_EXP_LEGACY_LAYOUTS builds only)
    bool       has(int layout) const { return ((layouts >> layout) & 1u) != 0u; }
    float4     rootLo{}, rootHi{};
    float      originBound = 0.0f;
    Camera     camera{};
    uint32_t   numBounces = 0;
    bool       aovs = false, moments = false, buckets = false; // which sums are on
    uint32_t   bucketPlanes = 1, bucketSamples = 0;            // the bucket sums' K, and the samples they hold
    uint32_t   numTiles = 0;                                   // of the shard
    uint64_t   validPixels = 0;                                // pixels of the shard's tiles that lie inside the frame
    std::optional<ActiveTiles> active;                         // a batch of rf_renderer_render_adaptive
};

enum : uint32_t { kKernelScalar = 0, kKernelPacket = 1, kKernelWide = 2 };            // TraversalPlan::kernel
enum : uint32_t { kFromQueue = 0, kFromShadeList = 1, kFromLookList = 2 };            // BouncePlan::shadowSource
enum : uint32_t { kAccumulatePixels = 0, kAccumulateRuns = 1, kAccumulateTiles = 2 }; // BatchPlan::accumulateKernel
// One traversal launch, resolved: what actually runs.  kKernelWide: the kTraceWide instantiation named by (any-hit, counting build, nearest-first, record layout,
// dense leaf phase) from rf_trace.hip's table and its scheduling arguments; the other two kernels take the flags only.
struct TraversalPlan
{
    uint32_t kernel;
    int      layout; // which record layout the launch reads (kTraceWide's COMPACT parameter), or kLayoutScalar / kLayoutPacket
    bool     anyHit, count, nearest, dense;
    uint32_t refillMin, chunk, leafVote, flags, extraLds;
};
struct BatchPlan
{
    uint32_t numSamples, numBounces, numTiles, pixelsPadded;
    bool     samplePerm, denseRaygen, constOrigin;
    bool     primaryLists;        // bounce 1's closest-hit group: kPixelLeafLists + kTraceLeafLists + the bounce's kTraceWide launch over what they hand on
    uint32_t primaryListCapacity; // entries per pixel
    bool     primaryFused;        // ... as kPixelLeafLists + kPrimaryFused (generates, walks and shades: no kRaygen launch) + kTraceWide and kShade<false, false, true> over what it hands on
    int      primaryLayout;
    bool     occluderGrid; // the batch's any-hit launches get the occluder grid: occluderGridEntries words, cells found by occScale / occMask
    uint64_t occluderGridEntries;
    float    occScale;
    uint32_t occMask;
    bool     firstLookReady; // a fact the batch mutates, as it stands for THIS batch (traceBatch / nextBatchFirstLookReady): the grid is warm and no hold-off runs
    bool     runs, tileList;
    bool     shardList; // a tile list under a tile shard: the sums are addressed through the slots behind the ids (SumAddressing::ShardList)
    uint32_t accumulateKernel, accumulatePixels, aovPixels, momentPixels; // pixels per workgroup of the sums' launches; 0: that sum is not launched
    uint32_t bucketPixels, buckets, bucketPhase; // the bucket sums' launch: K planes, the batch's sample k onto plane (bucketPhase + k) mod K
};
struct BouncePlan
{
    TraversalPlan closest, shadow;
    bool          shadeSorted, shadeAov;
    uint32_t      shadeFlags, sortScale, skyFirstBounce;
    uint32_t      itemGridCap; // kShade's and kShadowFirstLook's grid cap (0: one workgroup per 1 024 entries)
    bool          cached, firstLook, selfShadow;
    uint32_t      lookFlags, shadowSource; // shadowSource: whose count word and list the any-hit launch reads
};
// queueCounts by name.  Device words, one per 64-byte line (they are all hot atomics): the queue lengths [0, B] (0: raygen's queue, b: what kShade of bounce b
// leaves), the miss-list length per bounce, two work cursors of kShards lines per bounce for the traversal launches, the lengths of the lists kShadowFirstLook
// leaves to the any-hit launches per bounce, the lengths of kShade's lists of shadow rays still to trace (kShadeSelfShadow) per bounce.  b = 1 .. numBounces.
struct BatchCounters
{
    uint32_t*                 base;
    uint32_t                  numBounces;
    static constexpr uint32_t kLine = kLineWords, kCursorWords = kLine * kShards;
    uint32_t words() const { return primaryFallbackWord() + kLine; }
    // (behind everything else: the length of the list of bounce-1 rays kTraceLeafLists hands on to the bounce's kTraceWide launch)
    uint32_t primaryFallbackWord() const { return kLine * (2 * numBounces + 1) + kCursorWords * 2 * numBounces + kLine * numBounces + kLine * numBounces; }
    uint32_t* primaryFallbackCount() const { return base + primaryFallbackWord(); }
    uint32_t queueWord(uint32_t b) const { return kLine * b; }
    uint32_t missWord(uint32_t b) const { return kLine * (numBounces + 1) + kLine * (b - 1); }
    uint32_t cursorClosestWord(uint32_t b) const { return kLine * (2 * numBounces + 1) + kCursorWords * 2 * (b - 1); }
    uint32_t cursorShadowWord(uint32_t b) const { return cursorClosestWord(b) + kCursorWords; }
    uint32_t listWord(uint32_t b) const { return kLine * (2 * numBounces + 1) + kCursorWords * 2 * numBounces + kLine * (b - 1); }
    uint32_t shadowListWord(uint32_t b) const { return listWord(b) + kLine * numBounces; }
    // the count word an any-hit launch (or kShadowFirstLook) of bounce b reads, by BouncePlan::shadowSource
    uint32_t shadowCountWord(uint32_t b, uint32_t source) const { return source == kFromLookList ? listWord(b) : (source == kFromShadeList ? shadowListWord(b) : queueWord(b)); }
    uint32_t* queueCount(uint32_t b) const { return base + queueWord(b); }
    uint32_t* missCount(uint32_t b) const { return base + missWord(b); }
    uint32_t* cursorClosest(uint32_t b) const { return base + cursorClosestWord(b); }
    uint32_t* cursorShadow(uint32_t b) const { return base + cursorShadowWord(b); }
    uint32_t* listCount(uint32_t b) const { return base + listWord(b); }
    uint32_t* shadowListCount(uint32_t b) const { return base + shadowListWord(b); }
    uint32_t* shadowCount(uint32_t b, uint32_t source) const { return base + shadowCountWord(b, source); }
};

// is this kTraceWide instantiation compiled into the build?  (rf_trace_wide_list.hpp: the list rf_trace.hip's table of kernel addresses is made from)
bool traceWideInstantiated(bool anyHit, bool count, bool nearest, int layout, bool dense);
// the layout a test asks for, if this scene has it (else the binary records)
int layoutIfPresent(const PolicyInputs& in, int want);
// what does not depend on the batch: the option, and the gates the conservative records and kShade's own-triangle test already rest on -- boxes regular and nested all
// the way up, every leaf's exact box in its first triangle record
bool primaryListsPossible(const LaunchOptions& o, const PolicyInputs& in);
// the per-pixel leaf lists of bounce 1, where a batch would use them: capacity + 1 words per valid pixel of a batch (1080p at the default capacity of 64: 539 MB)
uint64_t primaryListBytesWanted(const LaunchOptions& o, const PolicyInputs& in, uint64_t pixels);
// The traversal launch of a layout, resolved (render path and ray queries alike).  nearest (any-hit): entries ordered by slab distance (NEAREST_FIRST); else record
// order (the conservative layouts' default: optShadowSignOrder) -- the compact and hot records always nearest-first.  A combination rf_trace.hip's table does not
// hold falls back to the same one without the dense leaf phase (options can ask for it on a layout it is not built for): the plan then says dense = false.
TraversalPlan resolveTraversal(const LaunchOptions& o, const PolicyInputs& in, bool anyHit, int layout, bool count, bool nearest, uint32_t flags, uint32_t refillMin, uint32_t chunk,
                               uint32_t leafVote, uint32_t extraLds);
// The layout the renderer picks BY ITSELF for the closest-hit / any-hit launch of a bounce (the per-scene defaults set at upload + the options; reported by
// rf_renderer_layout_info and used by traceBatch): kLayoutScalar = the one-ray-per-thread kernels (trees the packed tests cannot serve), kLayoutPacket = kTracePacket
int closestLayoutFor(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce);
int shadowLayoutFor(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce);
// does the any-hit launch of this bounce start at the occluder cache's entries? (kTraceWide, kFlagOccluderCache)
bool cachedShadowFor(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce);
// The traversal launch of a ray query (rf_renderer_cast_rays): a caller's rays are arbitrary, so they are planned as the render path plans an INCOHERENT launch of this
// scene -- the closest-hit / any-hit launch of bounce 2 (planBounce: its layout, instantiation, refill count, chunk and leaf vote) -- without what belongs to a render
// batch: no occluder cache and no first look (the cache is the batch's, a query neither uses nor disturbs it), no "first bounce", and an any-hit launch that reads its
// directions from the ray stream (kFlagShadowDirFromStream).  kernel == kKernelScalar: the reference-order scalar traversal (a scene whose wide records are unusable,
// traversal_variant 0, a packet-kernel experiment)
TraversalPlan planRayQuery(const LaunchOptions& o, const PolicyInputs& in, bool anyHit);
// The once-per-batch decisions, for a batch of numSamples samples of the shard's tiles (or of the `active` list of render_adaptive).  firstLookReady is the driver's
// to fill in (traceBatch / nextBatchFirstLookReady)
BatchPlan planBatch(const LaunchOptions& o, const PolicyInputs& in, uint32_t numSamples);
// Everything the launches of one bounce need
BouncePlan planBounce(const LaunchOptions& o, const PolicyInputs& in, uint32_t bounce, const BatchPlan& batch);
// rf_renderer_launch_plan's words: the plans of one bounce of a batch, field by field
void writeLaunchPlan(const BatchPlan& batch, const BouncePlan& p, uint32_t bounce, rf_launch_plan& out);
// rf_renderer_layout_info's rows: per bounce 1 .. 16 the closest-hit layout, the any-hit layout and whether that launch is cached, then the four misc words
void writeLayoutInfo(const LaunchOptions& o, const PolicyInputs& in, uint32_t (&layouts)[48], uint32_t (&misc)[4], float& quadHalfAreaRatio, uint64_t& treeBytes);
} // namespace rf
