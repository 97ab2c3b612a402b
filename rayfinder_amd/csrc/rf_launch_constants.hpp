// rf_launch_constants.hpp -- the plain constants that the kernels and the host-only launch policy (rf_launch_policy.cpp) both read: workgroup size, record layouts, launch
// flags, the scheduling constants of the traversal kernels, the pixels per workgroup of the sums.  No device code and no HIP type: the host compiler includes it as it is.
// rf_device.hpp, rf_kernels.hpp and rf_sums.hpp include it; each constant is defined here and nowhere else.
#pragma once

#include <cstdint>

namespace rf
{
constexpr int      kBlock = 256;          // 4 waves

namespace kern
{
constexpr uint32_t kSlotSampleMajor = 31u;

constexpr uint32_t kShadeLastBounce = 1u, kShadeFirstBounce = 2u;
// kShadeSelfShadow: kShade tests every hit's shadow ray against the hit triangle ITSELF (its leaf's exact box, then the triangle: both sit in the shading record it has in
// registers) and writes the positions of the hits that this does not settle to `shadowList`; the bounce's any-hit launches work through that list only (see kShade)
constexpr uint32_t kShadeSelfShadow = 4u;
constexpr uint32_t kLookFirstBounce = 1u, kLookNoRayCount = 2u; // kShadowFirstLook's flags

// ------------------------------------------------------------------------------------------------
// Scheduling constants of the persistent traversal kernel (tuned on the atrium, tools/gpu_ab.py).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kChunk = 128;   // queue entries claimed per atomic (small enough that the tail stays balanced)
constexpr uint32_t kShards = 16;   // work cursors per launch, one 64-byte line each: a single cursor
                                   // saturates near 90 claims/us (8 M rays / 64 per 1.2 ms = 100/us)
constexpr uint32_t kLineWords = 16;
constexpr uint32_t kRefillMin = 40; // refill once this many lanes are idle (r02 sweep: 32 -> 40 = +1 %)
constexpr uint32_t kLeafVote = 20; // leave the descent loop when fewer lanes than this are descending (16..24 measure the same)

// record layouts (kTraceWide's COMPACT parameter) + the two paths outside kTraceWide
constexpr int kLayoutBinary = 0, kLayoutCompact = 1, kLayoutHot = 2, kLayoutQuad = 3, kLayoutQuadHalf = 4, kLayoutQuadLocal = 5, kLayoutOct = 6, kLayoutScalar = 7, kLayoutPacket = 8;
constexpr uint32_t kFlagShadowDirFromStream = 1u; // any-hit: direction from ps.rayD instead of the sun sample
constexpr uint32_t kFlagUniformTri = 8u;          // the same for the triangles of a leaf phase
constexpr uint32_t kFlagUniformFetch = 4u;        // try the scalar-cache path for records that every descending lane shares
constexpr uint32_t kFlagFirstBounce = 2u;         // any-hit: radiance so far is 0 and not in memory yet (kRaygen does not store it)
constexpr uint32_t kFlagOccluderCache = 16u;      // any-hit: a new ray first visits the leaves that stopped the last rays from its cell of the scene (see kTraceWide)
constexpr uint32_t kFlagOccluderNoTry = 32u;      // ... the launch runs behind kShadowFirstLook: its rays have had their first look, it only records what stopped them
constexpr uint32_t kFlagNoRayCount = 64u;
constexpr uint32_t kFlagConstOrigin = 128u;      // closest-hit, bounce 1: every ray starts at WideScene::constOrigin (a pinhole camera: kRaygen does not write the origins, the refill does not read them)
constexpr uint32_t kFlagDenseLeafShift = 8u;       // bits 11..8: leaf phases in which a parked lane holds this many triangles or more run over dense (lane, triangle) pairs (0: never; see kTraceWide)         // the launch's rays are counted elsewhere (kShadowFirstLook counted the whole queue)
#if defined(RF_EXP_OCC_SLOTS)
constexpr int kOccSlots = RF_EXP_OCC_SLOTS;
#else
constexpr int kOccSlots = 4; // entries per cell of the occluder grid (1, 2 or 4: shadow launches of the atrium -19 / -29 / -34 %, profiles/r04_occluder)
#endif
static_assert(kOccSlots == 1 || kOccSlots == 2 || kOccSlots == 4, "one aligned load per cell");
constexpr uint32_t kPrimaryListMaxCapacity = 64u; // (the length sits in bits 7..0 of the word, the direction signs in bits 10..8)
} // namespace kern
using namespace kern;

// pixels per workgroup of the sums' LDS-staged kernels (rf_sums.hpp describes the kernels)
constexpr uint32_t kMomentPixels = 16;
constexpr uint32_t kAovPixels = 8;
#if defined(RF_EXP_ACC_PIXELS)
constexpr uint32_t kAccPixels = RF_EXP_ACC_PIXELS;
#else
constexpr uint32_t kAccPixels = 4;
#endif
constexpr uint32_t kAccMaxSamples = 1024;
constexpr uint32_t kBucketPixels = 4;
} // namespace rf
