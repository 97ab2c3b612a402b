// rf_wide_build.hpp -- host only: the builder of the render path's BVH record layouts (rf_wide.hpp describes the records and holds the device
// code that reads them) and the host-side check of what it builds.  Compiled once, by the host compiler (rf_wide_build.cpp); no HIP runtime call.
#pragma once

#include "rf_wide.hpp"

#include <span>
#include <vector>

namespace rf
{
struct WideBuild
{
    std::vector<float4> nodes;
    std::vector<float4> compact;       // compact-capable layout of the same records; empty when !compactUsable
    bool                compactUsable = true; // every node's x planes are attained by one of its children (true for boxes built as unions)
    std::vector<float4> hot, own;      // the 32-byte layout (all six planes carried) and the nodes' own boxes; empty when !hotUsable
    bool                hotUsable = true; // every plane of every node is attained by a child AND every index fits 24 bits
    // Quad records (kTraceWide<..., COMPACT = 3>): one 128-byte record per interior node at an EVEN level below the root holds the
    // boxes of the node's (up to four) GRANDCHILDREN -- a child that is a leaf fills one slot with itself -- i.e. two levels of
    // the reference's tree per dependent fetch:
    //     {E0.lo.xy E0.hi.xy | E0.lo.z E0.hi.z E1.lo.z E1.hi.z | E1.lo.xy E1.hi.xy |     entries of the FIRST child  (node + 1)
    //      E2.lo.xy E2.hi.xy | E2.lo.z E2.hi.z E3.lo.z E3.hi.z | E3.lo.xy E3.hi.xy |     entries of the SECOND child (secondChildOffset)
    //      word0 word1 word2 word3 | - - - -}
    // word k: child word of entry k (leaf descriptor as in the 64-byte records, or the index of the entry's own quad record);
    // kQuadEmpty in slots 1 / 3 when the child is a leaf.  Bits 30..29 carry split axes: word0 the node's, word1 the first
    // child's, word3 the second child's.
    // Decision-identical to the reference for the render path.  The reference visits a child c iff P(c) && tmin(c) < rayTMax
    // and then its children g under the same test; boxes are unions, so every plane of c is a plane of one of its children,
    // t = (plane - o) * inv is monotone in the plane under rounding, hence per axis the slab interval of g lies inside that of
    // c:  P(g) => P(c)  and  tmin(c) <= tmin(g).  So "g passes" already implies "c passes" (with the same rayTMax: no triangle
    // is tested between c's visit and its children's tests), a child none of whose children pass contributes no triangle test,
    // and the entries in the order [near child's near, far | far child's near, far] (each level by dirNeg[its own split axis])
    // with the later ones pushed together with their tmin and re-tested against rayTMax when popped are exactly the leaves /
    // subtrees the reference enters, in its order.  Not for the counting build (nodesVisited counts the skipped level).
    std::vector<float4> quad;
    bool                quadUsable = true; // every plane of every interior node is attained by one of its children (unions), indices fit
    // Half-precision quad records (kTraceWide<..., COMPACT = 4>): the quad records with their 24 planes stored as IEEE binary16,
    // 64 bytes -- four 16-byte loads per step instead of seven, half the bytes from L2:
    //     dword 3e + a (entry e = 0..3, axis a = 0..2) = {lo plane in the low half, hi plane in the high half};  dwords 12..15 = the quad record's words.
    // The planes are CONSERVATIVE: lo' <= lo - margin (rounded down to binary16), hi' >= hi + margin (rounded up); never subnormal.
    // The step evaluates t' = fma(plane', 1/d, -(o * 1/d)) in one v_fma_mix_f32 per plane (binary16 source, f32 result: no decode
    // instruction) where the reference evaluates t = ((plane - o) * 1/d) with two roundings.  With u = 2^-24, |o| <= originBound and
    // |plane| <= R (the root box):  t' <= T' + u |o / d| + u |t'|  and  t >= T - 2u |T|  for the real values T' = (plane' - o) / d,
    // T = (plane - o) / d, so  margin >= u (4 originBound + 3 R + margin)  makes every near t' <= its t and every far t' >= its t
    // (margin = 2^-21 (originBound + R) = u (40 R + 8) against u (19 R + 4 + margin): more than twice that at every R, for R << 1 as for R >> 1; checkWideLayouts
    // asks for exactly this inequality, with u = 2^-24).  NaNs (an axis-parallel ray: inf - inf) drop out of v_min / v_max, i.e. that
    // axis does not constrain: conservative as well.  So a quad-half step accepts a SUPERSET of what the exact step accepts --
    // which is all an interior test has to do, because every LEAF is then tested against its EXACT box (kept in the spare floats
    // of the leaf's first 64-byte triangle record: leafBoxesIntoTriangles) with the reference's formula, a leaf's exact slab
    // interval lies inside every ancestor's (boxes are unions, rounding is monotone), and entries are visited in the same order:
    // the same leaves have their triangles tested, in the same order, against the same rayTMax.
    std::vector<uint4>  quadHalf;
    float               originBound = 0.0f;
    // sum of the surface areas of the half-precision boxes / of the exact boxes, over all entries: how many more boxes a random ray
    // hits because of the binary16 grid (absolute coordinates: ~2^-11 of the coordinate's magnitude).  The renderer uses the half records
    // by default only where this stays below kQuadHalfMaxAreaRatio (a 17 M-triangle scene of centimetre triangles: 1.22 -> the local grid).
    float               quadHalfAreaRatio = 0.0f;
    // Local-grid quad records (kTraceWide<..., COMPACT = 5>): the same idea with the planes as 8-bit steps of a PER-RECORD power-of-two grid,
    // for scenes whose triangles are small against their coordinates (where binary16 of absolute coordinates is too coarse):
    //     {anchor.x anchor.y anchor.z scale.x} {scale.y scale.z X0 X1} {Y0 Y1 Z0 Z1} {word0..3}
    // anchor: a point below every lower plane of the record; scale = 2^e per axis (f32); axis words: X0 = {lo0 hi0 lo1 hi1} (one byte each,
    // entries 0 and 1), X1 = entries 2 and 3; plane' = anchor + byte * scale, lo' <= lo - margin, hi' >= hi + margin.
    // The step evaluates t' = fma(1024 + byte, A, B') with A = scale / d (exact: a power of two times 1/d), B' = ((anchor - o) / d) - 1024 A
    // -- "1024 + byte" is the binary16 0x6400 | byte, built by one v_perm_b32 per pair of planes (which also puts the NEAR plane into the
    // low half: the selector depends on the sign of 1/d), and v_fma_mix_f32 takes it straight into the f32 FMA.  Roundings: two in
    // (anchor - o) / d, one in B', one in t', against two in the reference's t: with u = 2^-24 and everything within originBound / R,
    //     |t' - T'| <= u (3.02 |anchor - o| + 1024 scale + |plane' - o|) / |d|,   |t - T| <= 2.01 u |plane - o| / |d|,
    // so  margin >= u (6.03 (originBound + R) + 1024 scale)  keeps every near t' <= its t and every far t' >= its t; 1024 scale <= 16.2 R,
    // i.e. u (46 R + 6) with originBound = 4 R + 1, and the builder leaves 2^-18 (originBound + R) = u (320 R + 64): 6.9 x that.
    std::vector<uint4>  quadLocal;
    float               quadLocalAreaRatio = 0.0f;
    // Oct records (kTraceWide<..., COMPACT = 6>, round 5): the local-grid idea one level further -- one 128-byte-aligned record per interior node reachable
    // from the root in steps of THREE levels holds the boxes of the node's (up to eight) GREAT-GRANDCHILDREN, i.e. three levels of the reference's tree per
    // dependent fetch.  Built for scenes whose tree does not fit the Infinity Cache, on the calibration that a random 128-byte line costs the memory system about
    // what a 64-byte one does (tools/microbench/fetch_calib.hip `wide`, 2-GiB table: 64-byte records 60 G/s = 3.8 TB/s, 128-byte records 51 G/s = 6.5 TB/s) -- and
    // MEASURED SLOWER in the kernel (out-of-cache atrium, bounces 3-8: +17 %; profiles/r05_hbm): those launches sit on the L1 -> L2 request rate (17.7 requests per ray
    // at 78 G/s), a 112-byte record is two 64-byte requests where the quad record is one, and 0.65 x the steps x 2 = 1.2 x the requests.  Kept as an option
    // (oct_from_bounce), bit-identical and tested; not selected by default.  Slot e = 4 c + 2 g + k: child c of the node, its child g, that one's child k; a child or
    // grandchild that is a leaf fills the FIRST slot of its range, the rest of the range is empty.  Layout (uint4 pieces; the eighth is padding):
    //     {anchor.x anchor.y anchor.z scale.x} {scale.y scale.z orderLo orderHi} {X01 X23 X45 X67} {Y01 Y23 Y45 Y67} {Z01 Z23 Z45 Z67} {word0..3} {word4..7}
    // planes as in the local-grid quad records (axis word of slots 2 j, 2 j + 1 = {lo hi lo hi} bytes; an EMPTY slot holds lo = 255, hi = 0 on every axis: it fails
    // the slab test for every ray, so the step has no "is the slot empty" test at all); words = child words without axis bits (a leaf descriptor or the index of
    // the entry's own oct record; kQuadEmpty in empty slots).
    // Visit order.  The reference orders the two children of every node by dirNeg[its split axis] (wgsl:409-417); applied at the three levels inside a record
    // that is a permutation of the eight slots which depends on the record's seven split axes and on the ray's three direction signs only -- so the builder
    // tabulates it: order{Lo,Hi} = four 16-bit fields, one per sign pattern (negX | negY << 1) with negZ = 0; nibble j = 2 c + g of a field = the POSITION (0 = first)
    // at which slot (c, g, 0) is visited, slot (c, g, 1) sits at that position ^ 1.  A ray with negZ = 1 reads the field of the opposite sign pattern and flips
    // every position (^ 7): with all three signs inverted every swap is inverted, i.e. the order is reversed.
    std::vector<uint4>  oct;
    std::vector<uint32_t> octIndexOfNode; // per reference node: its oct record (kQuadEmpty: none)
    float               octAreaRatio = 0.0f; // as quadLocalAreaRatio
    std::vector<uint2>  bigLeaves;
    float4              rootLo, rootHi;
    uint32_t            rootLeaf = kWideNone;
    bool                boxesRegular = true; // every child box finite (|x| < 1e30) with min <= max (see slabPair)
    // every child's box lies inside its parent's (true for boxes built as unions; a hand-made tree may break it).  What the two-levels-per-step records, the
    // conservative layouts' "exact box at the leaf" and the occluder cache's "a leaf whose own box passes is one the reference reaches" all rest on: without it the
    // renderer keeps to the binary records, which repeat the reference's test node by node
    bool                boxesNested = true;
    std::vector<uint32_t> quadIndexOfNode; // per reference node: its quad record, kQuadEmpty for the nodes that have none (leaves, odd levels, unreachable nodes)
};

// (each is described at its definition, rf_wide_build.cpp)
float     halfBitsToFloat(uint16_t h);
uint16_t  halfDirected(float v, bool down, bool& ok);
bool      leafBoxesIntoTriangles(const BvhNode* nodes, size_t count, float4* triangles /* 4 float4 per triangle */, size_t numTriangles, uint32_t hintLevels = 0,
                                 const std::vector<uint32_t>* quadIndexOfNode = nullptr);
WideBuild buildWide(const BvhNode* nodes, size_t count); // 48-byte reference nodes -> wide records; the tree must have passed validateScene

// Host-only check of the render path's BVH layouts (rf_wide.hpp) for a flattened tree: builds the 64-byte records and their
// compact-capable / 32-byte variants and verifies that every variant decodes to the same child planes and child words as the
// plain record, and that the carried "own" planes are the union of the children's.  Returns bit 0: boxes regular (wide layout
// usable), bit 1: compact-capable records usable, bit 2: 32-byte records usable; throws std::runtime_error on a mismatch.
uint32_t checkWideLayouts(std::span<const BvhNode> nodes, float* quadHalfAreaRatio = nullptr);
} // namespace rf
