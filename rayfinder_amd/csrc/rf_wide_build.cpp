// rf_wide_build.cpp -- 48-byte reference nodes -> the render path's record layouts (buildWide), the leaf boxes and occluder-cache entries in the
// triangle records (leafBoxesIntoTriangles), and the host-side check of all of them (checkWideLayouts).  Host only.
#include "rf_wide_build.hpp"

#include <algorithm>
#include <cmath>
#include <functional>
#include <initializer_list>
#include <limits>
#include <stdexcept>
#include <string>

namespace rf
{
// Host: 48-byte reference nodes -> wide records.
// binary16 <-> f32 for the half-precision quad records (host side; normal numbers and zero only: the builder never emits a subnormal)
float halfBitsToFloat(uint16_t h)
{
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e == 0) return bitsFloat(sign); // (+-0; subnormals are not produced)
    return bitsFloat(sign | ((e + 112u) << 23) | (m << 13));
}
// the largest binary16 <= v (down = true) / the smallest binary16 >= v (down = false); |v| must be finite; `ok` = false beyond +-65504
uint16_t halfDirected(float v, bool down, bool& ok)
{
    if (!(std::fabs(v) <= 65504.0f)) { ok = false; return 0; }
    if (v == 0.0f) return 0;
    const bool neg = v < 0.0f;
    if (std::fabs(v) < 6.103515625e-05f) // below the smallest normal binary16 (2^-14): 0 or +-2^-14, whichever lies on the requested side
        return (neg == down) ? static_cast<uint16_t>((neg ? 0x8000u : 0u) | 0x0400u) : static_cast<uint16_t>(0);
    const uint32_t b = floatBits(std::fabs(v));
    uint32_t       h = (((b >> 23) - 112u) << 10) | ((b >> 13) & 0x3FFu); // magnitude truncated towards zero
    const bool     inexact = (b & 0x1FFFu) != 0u;
    if (inexact && (neg == down)) ++h; // away from zero on the side that was asked for
    if (h > 0x7BFFu) { ok = false; return 0; }
    return static_cast<uint16_t>((neg ? 0x8000u : 0u) | h);
}

// The EXACT box of every leaf, written into the spare floats of the leaf's FIRST device triangle record (64 bytes: {p0 .} {p1 .} {p2 .}
// {. . . .}):  lo = (record[0].w, record[1].w, record[2].w),  hi = record[3].xyz.  Read by the half-precision quad kernels only.
// Returns false when two leaves claim the same first-triangle slot (a hand-made tree: validateScene only checks that leaf ranges lie inside the
// triangle array, not that they are disjoint): the later leaf's box would overwrite the earlier one's, the half-precision / local-grid kernels
// would cull with a box that is not the leaf's, and the image would depend on the record layout.  The caller keeps those layouts off then.
bool leafBoxesIntoTriangles(const BvhNode* nodes, size_t count, float4* triangles /* 4 float4 per triangle */, size_t numTriangles, uint32_t hintLevels,
                            const std::vector<uint32_t>* quadIndexOfNode)
{
    // record[3].w: what the occluder cache (kTraceWide, any-hit) remembers when a ray is stopped in this leaf.  0: the leaf's own child word.  Else the QUAD record
    // index of the record `hintLevels` quad levels above the leaf (1: the record that has the leaf among its entries) -- for scenes whose triangles are small against
    // the sun disc's footprint, where the NEXT ray from the same place is stopped by a neighbour of this triangle rather than by the triangle itself.  Any record is
    // a valid place to start an any-hit ray: the entry only decides what it looks at first.
    // The index comes from buildWide's OWN numbering (WideBuild::quadIndexOfNode: the nodes reachable from the root in two-level steps) and the ancestors from a walk
    // that starts at the root: a hand-made tree may hold interior nodes no parent reaches, or children with two parents (validateScene accepts both), and a
    // numbering recomputed here from node order and depth named the wrong record -- or one past the end -- for them.  A leaf the walk does not reach, or
    // whose ancestor is not a quad record, remembers itself (0).
    std::vector<uint32_t> parent;
    const bool            hints = hintLevels != 0 && quadIndexOfNode != nullptr && quadIndexOfNode->size() == count && count > 0 && nodes[0].triangleCount == 0;
    if (hints)
    {
        parent.assign(count, kQuadEmpty);
        std::vector<uint32_t> todo{0u};
        while (!todo.empty())
        {
            const uint32_t i = todo.back();
            todo.pop_back();
            if (nodes[i].triangleCount != 0) continue;
            for (const size_t c : {static_cast<size_t>(i) + 1, static_cast<size_t>(nodes[i].secondChildOffset)})
                if (c < count && c > i && parent[c] == kQuadEmpty) parent[c] = i, todo.push_back(static_cast<uint32_t>(c));
        }
    }
    std::vector<bool> claimed(numTriangles, false);
    bool              distinct = true;
    for (size_t i = 0; i < count; ++i)
    {
        const BvhNode& n = nodes[i];
        if (n.triangleCount == 0 || n.trianglesOffset >= numTriangles) continue;
        if (claimed[n.trianglesOffset]) distinct = false;
        claimed[n.trianglesOffset] = true;
        float4*  t = triangles + 4 * static_cast<size_t>(n.trianglesOffset);
        uint32_t hint = 0u;
        if (hints && i != 0 && parent[i] != kQuadEmpty)
        {
            const auto& quadIndex = *quadIndexOfNode;
            uint32_t    a = parent[i];
            if (quadIndex[a] == kQuadEmpty && a != 0u) a = parent[a]; // the record that holds the leaf as an entry
            for (uint32_t l = 1; l < hintLevels && a != 0u && a != kQuadEmpty; ++l)
            {
                const uint32_t up = parent[a];
                a = (up == 0u || up == kQuadEmpty) ? 0u : parent[up];
            }
            if (a != 0u && a != kQuadEmpty && quadIndex[a] != kQuadEmpty && quadIndex[a] < (1u << kWideIndexBits)) hint = quadIndex[a]; // (the root is where a ray starts anyway)
        }
        t[0].w = n.aabb.min.x, t[1].w = n.aabb.min.y, t[2].w = n.aabb.min.z;
        t[3] = make_float4(n.aabb.max.x, n.aabb.max.y, n.aabb.max.z, bitsFloat(hint));
    }
    return distinct;
}

WideBuild buildWide(const BvhNode* nodes, size_t count)
{
    WideBuild             out;
    std::vector<uint32_t> wideIndex(count, 0);
    uint32_t              numInterior = 0;
    for (size_t i = 0; i < count; ++i)
        if (nodes[i].triangleCount == 0) wideIndex[i] = numInterior++;
    if (numInterior >= (1u << kWideIndexBits)) out.boxesRegular = false; // index field too narrow: not usable
    std::vector<uint32_t> bigLeafOf; // per node: index into bigLeaves + 1 (0: none yet), so that every layout names the same table entry
    auto leafWord = [&](size_t idx) -> uint32_t {
        const BvhNode& n = nodes[idx];
        if (n.triangleCount <= 7 && n.trianglesOffset < (1u << kWideIndexBits)) return kWideLeafBit | ((n.triangleCount - 1) << kWideIndexBits) | n.trianglesOffset;
        if (bigLeafOf.empty()) bigLeafOf.assign(count, 0u);
        if (bigLeafOf[idx] == 0u)
        {
            out.bigLeaves.push_back(make_uint2(n.trianglesOffset, n.triangleCount));
            bigLeafOf[idx] = static_cast<uint32_t>(out.bigLeaves.size());
        }
        return kWideLeafBit | (7u << kWideIndexBits) | (bigLeafOf[idx] - 1u);
    };
    auto childWord = [&](size_t idx) -> uint32_t { return nodes[idx].triangleCount == 0 ? wideIndex[idx] : leafWord(idx); };
    out.rootLo = make_float4(nodes[0].aabb.min.x, nodes[0].aabb.min.y, nodes[0].aabb.min.z, 0.0f);
    out.rootHi = make_float4(nodes[0].aabb.max.x, nodes[0].aabb.max.y, nodes[0].aabb.max.z, 0.0f);
    if (nodes[0].triangleCount > 0) out.rootLeaf = childWord(0);
    out.nodes.resize(4 * static_cast<size_t>(numInterior > 0 ? numInterior : 1));
    for (size_t i = 0; i < count; ++i)
    {
        const BvhNode& n = nodes[i];
        if (n.triangleCount > 0) continue;
        const size_t   c0 = i + 1, c1 = n.secondChildOffset;
        const BvhNode &a = nodes[c0], &b = nodes[c1];
        float4*        w = &out.nodes[4 * static_cast<size_t>(wideIndex[i])];
        // 12 box floats as (x,y) and (z,z) pairs for packed f32 math (see the layout note above)
        w[0] = make_float4(a.aabb.min.x, a.aabb.min.y, a.aabb.max.x, a.aabb.max.y);
        w[1] = make_float4(a.aabb.min.z, a.aabb.max.z, b.aabb.min.z, b.aabb.max.z);
        w[2] = make_float4(b.aabb.min.x, b.aabb.min.y, b.aabb.max.x, b.aabb.max.y);
        // 14 dwords are read per step: 12 box floats + the two child words (the split axis rides in the first word)
        w[3] = make_float4(bitsFloat(childWord(c0) | ((n.splitAxis & 3u) << kWideAxisShift)), bitsFloat(childWord(c1)), 0.0f, 0.0f);
        // Compact-capable layout (kTraceWide<..., COMPACT>).  A node's box is the union of its children's, so each of its planes
        // is attained by (at least) one child; a lane that enters the node straight from its parent's step has the t-values of
        // the node's own planes in hand.  For the two x planes the record therefore names only the OTHER child's value ("inner")
        // and which child that is (bits 30..29 of the second child word), which leaves everything a step needs in 12 dwords:
        //     {innerLoX c0.lo.y innerHiX c0.hi.y | c0.lo.z c0.hi.z c1.lo.z c1.hi.z | word0 c1.lo.y word1 c1.hi.y | outerLoX outerHiX - -}
        // = three dwordx4 instead of 3 + 1 loads per step, i.e. three vector-L1 tag accesses instead of four -- the unit the deep
        // bounces exhaust.  The fourth piece (the shared values themselves) is read only by a lane that arrives from the stack or
        // starts at the root.  Same planes, same (value - o) * inv per plane: bit-identical decisions.
        {
            if (out.compact.empty()) out.compact.resize(out.nodes.size());
            float4*    c = &out.compact[4 * static_cast<size_t>(wideIndex[i])];
            const bool loFromA = a.aabb.min.x == n.aabb.min.x, loFromB = b.aabb.min.x == n.aabb.min.x; // which child attains the node's min.x
            const bool hiFromA = a.aabb.max.x == n.aabb.max.x, hiFromB = b.aabb.max.x == n.aabb.max.x;
            if (!(loFromA || loFromB) || !(hiFromA || hiFromB)) out.compactUsable = false;
            const uint32_t selLo = loFromA ? 1u : 0u, selHi = hiFromA ? 1u : 0u; // 1: child 1 holds the inner value (child 0 shares the node's plane)
            const float    innerLo = selLo ? b.aabb.min.x : a.aabb.min.x, outerLo = selLo ? a.aabb.min.x : b.aabb.min.x;
            const float    innerHi = selHi ? b.aabb.max.x : a.aabb.max.x, outerHi = selHi ? a.aabb.max.x : b.aabb.max.x;
            const uint32_t w0 = floatBits(w[3].x), w1 = floatBits(w[3].y); // the plain record's child words (split axis in word0)
            if ((w1 & (3u << kWideAxisShift)) != 0u) out.compactUsable = false; // (cannot happen: those bits are free in the second word)
            c[0] = make_float4(innerLo, a.aabb.min.y, innerHi, a.aabb.max.y);
            c[1] = make_float4(a.aabb.min.z, a.aabb.max.z, b.aabb.min.z, b.aabb.max.z);
            c[2] = make_float4(bitsFloat(w0), b.aabb.min.y, bitsFloat(w1 | (selLo << kWideAxisShift) | (selHi << (kWideAxisShift + 1))), b.aabb.max.y);
            c[3] = make_float4(outerLo, outerHi, 0.0f, 0.0f);
        }
        // The 32-byte layout (kTraceWide<..., COMPACT = 2>) takes the same idea to all six planes: the lane carries the t-values
        // of the whole box of the node it enters from its parent's step, and a step reads
        //     {innerLoX innerLoY innerHiX innerHiY | innerLoZ innerHiZ word0 word1}
        // = TWO dwordx4 (two vector-L1 tag accesses, one 32-byte piece of a line: two records per 64-byte L2 request, four per
        // 128-byte line) with six selector bits in the child words: bits 25..24 of word0 = {lo.x, lo.y}, bits 25..24 of
        // word1 = {hi.x, hi.y}, bits 30..29 of word1 = {lo.z, hi.z}; selector 1: child 0 shares the node's plane and child 1 holds
        // the inner value.  The index fields shrink to 24 bits for it.  The node's own box sits in a second array that only
        // a lane arriving from the stack reads (the root's box is a kernel argument).
        {
            if (out.hot.empty())
            {
                out.hot.resize(out.nodes.size() / 2);
                out.own.resize(out.nodes.size() / 2);
            }
            float4*        h = &out.hot[2 * static_cast<size_t>(wideIndex[i])];
            float4*        o = &out.own[2 * static_cast<size_t>(wideIndex[i])];
            const float    nv[6] = {n.aabb.min.x, n.aabb.min.y, n.aabb.max.x, n.aabb.max.y, n.aabb.min.z, n.aabb.max.z};
            const float    av[6] = {a.aabb.min.x, a.aabb.min.y, a.aabb.max.x, a.aabb.max.y, a.aabb.min.z, a.aabb.max.z};
            const float    bv[6] = {b.aabb.min.x, b.aabb.min.y, b.aabb.max.x, b.aabb.max.y, b.aabb.min.z, b.aabb.max.z};
            float          inner[6];
            uint32_t       sel[6];
            for (int k = 0; k < 6; ++k)
            {
                const bool fromA = av[k] == nv[k], fromB = bv[k] == nv[k];
                if (!(fromA || fromB)) out.hotUsable = false;
                sel[k] = fromA ? 1u : 0u;
                inner[k] = fromA ? bv[k] : av[k];
            }
            uint32_t w0 = floatBits(w[3].x), w1 = floatBits(w[3].y); // the plain record's child words (split axis in word0)
            if (((w0 | w1) & (3u << 24)) != 0u) out.hotUsable = false; // an index that needs more than 24 bits
            w0 |= (sel[0] << 25) | (sel[1] << 24);
            w1 |= (sel[2] << 25) | (sel[3] << 24) | (sel[4] << 30) | (sel[5] << 29);
            h[0] = make_float4(inner[0], inner[1], inner[2], inner[3]);
            h[1] = make_float4(inner[4], inner[5], bitsFloat(w0), bitsFloat(w1));
            o[0] = make_float4(nv[0], nv[1], nv[2], nv[3]);
            o[1] = make_float4(nv[4], nv[5], 0.0f, 0.0f);
        }
        // the packed slab test assumes ordered, finite boxes (always true for boxes of real triangles)
        const float lo[6] = {a.aabb.min.x, a.aabb.min.y, a.aabb.min.z, b.aabb.min.x, b.aabb.min.y, b.aabb.min.z};
        const float hi[6] = {a.aabb.max.x, a.aabb.max.y, a.aabb.max.z, b.aabb.max.x, b.aabb.max.y, b.aabb.max.z};
        for (int k = 0; k < 6; ++k)
            if (!(std::fabs(lo[k]) < 1e30f && std::fabs(hi[k]) < 1e30f && lo[k] <= hi[k])) out.boxesRegular = false;
        const float nlo[3] = {n.aabb.min.x, n.aabb.min.y, n.aabb.min.z}, nhi[3] = {n.aabb.max.x, n.aabb.max.y, n.aabb.max.z};
        for (int k = 0; k < 6; ++k)
            if (!(lo[k] >= nlo[k % 3] && hi[k] <= nhi[k % 3])) out.boxesNested = false;
    }
    // ---- quad records: the interior nodes reachable from the root in steps of two levels, numbered in node (= depth-first) order
    if (numInterior > 0 && out.boxesRegular && out.boxesNested)
    {
        std::vector<uint32_t>& quadIndex = out.quadIndexOfNode;
        quadIndex.assign(count, kQuadEmpty);
        {
            std::vector<uint8_t>  member(count, 0);
            std::vector<uint32_t> todo{0u};
            while (!todo.empty())
            {
                const uint32_t i = todo.back();
                todo.pop_back();
                member[i] = 1;
                for (const size_t c : {static_cast<size_t>(i) + 1, static_cast<size_t>(nodes[i].secondChildOffset)})
                    if (nodes[c].triangleCount == 0)
                        for (const size_t g : {c + 1, static_cast<size_t>(nodes[c].secondChildOffset)})
                            if (nodes[g].triangleCount == 0) todo.push_back(static_cast<uint32_t>(g));
            }
            uint32_t numQuad = 0;
            for (size_t i = 0; i < count; ++i)
                if (member[i]) quadIndex[i] = numQuad++;
            out.quad.assign(8 * static_cast<size_t>(numQuad), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        }
        struct Entry
        {
            Aabb     box;
            uint32_t word;
        };
        const auto attained = [&](const BvhNode& n) { // every plane of an interior node's box is a plane of one of its children
            const BvhNode &a = nodes[(&n - nodes) + 1], &b = nodes[n.secondChildOffset];
            return (a.aabb.min.x == n.aabb.min.x || b.aabb.min.x == n.aabb.min.x) && (a.aabb.min.y == n.aabb.min.y || b.aabb.min.y == n.aabb.min.y) &&
                   (a.aabb.min.z == n.aabb.min.z || b.aabb.min.z == n.aabb.min.z) && (a.aabb.max.x == n.aabb.max.x || b.aabb.max.x == n.aabb.max.x) &&
                   (a.aabb.max.y == n.aabb.max.y || b.aabb.max.y == n.aabb.max.y) && (a.aabb.max.z == n.aabb.max.z || b.aabb.max.z == n.aabb.max.z);
        };
        for (size_t i = 0; i < count; ++i)
        {
            if (quadIndex[i] == kQuadEmpty) continue;
            const BvhNode& n = nodes[i];
            Entry          e[4];
            uint32_t       axes[2] = {0u, 0u};
            const size_t   kids[2] = {i + 1, n.secondChildOffset};
            for (int k = 0; k < 2; ++k)
            {
                const BvhNode& c = nodes[kids[k]];
                if (c.triangleCount > 0)
                {
                    e[2 * k] = Entry{c.aabb, leafWord(kids[k])};
                    e[2 * k + 1] = Entry{Aabb{vec3(0.0f, 0.0f, 0.0f), 0.0f, vec3(0.0f, 0.0f, 0.0f), 0.0f}, kQuadEmpty};
                }
                else
                {
                    if (!attained(c)) out.quadUsable = false; // the skipped level must be implied by its children's tests
                    axes[k] = c.splitAxis & 3u;
                    const size_t g[2] = {kids[k] + 1, c.secondChildOffset};
                    for (int j = 0; j < 2; ++j)
                    {
                        const BvhNode& gn = nodes[g[j]];
                        const uint32_t w = gn.triangleCount > 0 ? leafWord(g[j]) : quadIndex[g[j]];
                        if (gn.triangleCount == 0 && w >= (1u << kWideIndexBits)) out.quadUsable = false;
                        e[2 * k + j] = Entry{gn.aabb, w};
                    }
                }
            }
            float4* q = &out.quad[8 * static_cast<size_t>(quadIndex[i])];
            for (int k = 0; k < 2; ++k)
            {
                const Aabb &a = e[2 * k].box, &b = e[2 * k + 1].box;
                q[3 * k] = make_float4(a.min.x, a.min.y, a.max.x, a.max.y);
                q[3 * k + 1] = make_float4(a.min.z, a.max.z, b.min.z, b.max.z);
                q[3 * k + 2] = make_float4(b.min.x, b.min.y, b.max.x, b.max.y);
            }
            const auto tag = [](uint32_t word, uint32_t axis) { return word == kQuadEmpty ? word : (word | (axis << kWideAxisShift)); };
            q[6] = make_float4(bitsFloat(tag(e[0].word, n.splitAxis & 3u)), bitsFloat(tag(e[1].word, axes[0])), bitsFloat(e[2].word), bitsFloat(tag(e[3].word, axes[1])));
        }
    }
    if (out.bigLeaves.empty()) out.bigLeaves.push_back(make_uint2(0, 0));
    if (!out.boxesRegular || !out.boxesNested || numInterior == 0) out.quadUsable = false;
    if (!out.quadUsable) out.quad.clear(), out.quadIndexOfNode.clear();
    if (!out.quad.empty())
    {
        // ---- half-precision quad records (see WideBuild::quadHalf)
        double R = 0.0;
        for (const float c : {out.rootLo.x, out.rootLo.y, out.rootLo.z, out.rootHi.x, out.rootHi.y, out.rootHi.z}) R = std::max(R, static_cast<double>(std::fabs(c)));
        const double bound = 4.0 * R + 1.0;
        out.originBound = static_cast<float>(bound);
        if (static_cast<double>(out.originBound) > bound) out.originBound = std::nextafterf(out.originBound, 0.0f);
        const double margin = (static_cast<double>(out.originBound) + R) * 4.76837158203125e-07; // 2^-21
        const size_t numQuad = out.quad.size() / 8;
        out.quadHalf.assign(4 * numQuad, make_uint4(0u, 0u, 0u, 0u));
        bool ok = true;
        const auto lower = [&](float v) { // the largest f32 <= v - margin, then down to binary16
            const double target = static_cast<double>(v) - margin;
            float        f = static_cast<float>(target);
            if (static_cast<double>(f) > target) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
            return halfDirected(f, true, ok);
        };
        const auto upper = [&](float v) {
            const double target = static_cast<double>(v) + margin;
            float        f = static_cast<float>(target);
            if (static_cast<double>(f) < target) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
            return halfDirected(f, false, ok);
        };
        double areaExact = 0.0, areaHalf = 0.0;
        const auto area = [](const double lo[3], const double hi[3]) {
            const double ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
            return 2.0 * (ex * ey + ey * ez + ez * ex);
        };
        for (size_t r = 0; r < numQuad && ok; ++r)
        {
            const float4* q = &out.quad[8 * r];
            uint32_t      d[16];
            for (int k = 0; k < 2; ++k) // entries 2k, 2k + 1 (see the quad layout above)
            {
                const float4 a = q[3 * k], z = q[3 * k + 1], b = q[3 * k + 2];
                const float  lo[2][3] = {{a.x, a.y, z.x}, {b.x, b.y, z.z}}, hi[2][3] = {{a.z, a.w, z.y}, {b.z, b.w, z.w}};
                for (int j = 0; j < 2; ++j)
                    for (int ax = 0; ax < 3; ++ax)
                        d[3 * (2 * k + j) + ax] = static_cast<uint32_t>(lower(lo[j][ax])) | (static_cast<uint32_t>(upper(hi[j][ax])) << 16);
            }
            d[12] = floatBits(q[6].x), d[13] = floatBits(q[6].y), d[14] = floatBits(q[6].z), d[15] = floatBits(q[6].w);
            // an EMPTY slot (its child is a leaf and fills one slot only) holds an INVERTED box -- lower planes +65504, upper planes -65504 -- that no ray can pass: its
            // near and far bounds are fma(+-65504, 1/d, b) with the same b, 131 008 |1/d| apart and the wrong way round, so `near <= far` fails -- FOR THE RAYS THAT REACH
            // THESE RECORDS: kTraceWide sends every ray whose origin lies beyond wide.originBound (4 R + 1) or whose 1/d is not of ordinary magnitude (1e-18 ... 1e18) to the
            // scalar traversal before its first step (the refill's `fastRay` / `ordinary` tests).  The invariant depends on that gate: with |o / d| beyond ~2^41 on all three
            // axes both fma results would round to the same b, `near == far` would pass, and -- the step no longer testing the word -- kQuadEmpty & kAxisMask would be followed
            // as a record index.  Under the gate |b| = |o / d| <= (4 R + 1) * 1e18 only where |1/d| itself is huge, and then 131 008 |1/d| >> ulp(b); the fuzz covers a
            // far diagonal camera with these records forced (tests/test_gpu_parity.py: test_far_camera_on_the_half_precision_records).
            // The step's hit test needs no `word != kQuadEmpty` for these records (kTraceWide, COMPACT == 4: two compares and two mask operations per step).
            for (int e = 0; e < 4; ++e)
                if (d[12 + e] == kQuadEmpty)
                    for (int ax = 0; ax < 3; ++ax) d[3 * e + ax] = kHalfEmptyPlanes;
            for (int k = 0; k < 4; ++k) out.quadHalf[4 * r + k] = make_uint4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
            for (int e = 0; e < 4 && ok; ++e)
            {
                if (d[12 + e] == kQuadEmpty) continue;
                const int    k = e / 2, j = e % 2;
                const float4 a = q[3 * k], z = q[3 * k + 1], b = q[3 * k + 2];
                const double lo[3] = {j ? b.x : a.x, j ? b.y : a.y, j ? z.z : z.x}, hi[3] = {j ? b.z : a.z, j ? b.w : a.w, j ? z.w : z.y};
                double       hlo[3], hhi[3];
                for (int ax = 0; ax < 3; ++ax)
                {
                    hlo[ax] = halfBitsToFloat(static_cast<uint16_t>(d[3 * e + ax] & 0xFFFFu));
                    hhi[ax] = halfBitsToFloat(static_cast<uint16_t>(d[3 * e + ax] >> 16));
                }
                areaExact += area(lo, hi);
                areaHalf += area(hlo, hhi);
            }
        }
        out.quadHalfAreaRatio = areaExact > 0.0 ? static_cast<float>(areaHalf / areaExact) : 1.0f;
        if (!ok) out.quadHalf.clear(); // a coordinate beyond the binary16 range: the f32 quad records serve
        // ---- local-grid quad records (see WideBuild::quadLocal)
        {
            const double marginL = (static_cast<double>(out.originBound) + R) * 3.814697265625e-06; // 2^-18
            out.quadLocal.assign(4 * numQuad, make_uint4(0u, 0u, 0u, 0u));
            double aExact = 0.0, aLocal = 0.0;
            bool   okL = true;
            for (size_t r = 0; r < numQuad && okL; ++r)
            {
                const float4* q = &out.quad[8 * r];
                const uint32_t words[4] = {floatBits(q[6].x), floatBits(q[6].y), floatBits(q[6].z), floatBits(q[6].w)};
                double         lo[4][3], hi[4][3];
                for (int e = 0; e < 4; ++e)
                {
                    const int    k = e / 2, j = e % 2;
                    const float4 a = q[3 * k], z = q[3 * k + 1], b = q[3 * k + 2];
                    lo[e][0] = j ? b.x : a.x, lo[e][1] = j ? b.y : a.y, lo[e][2] = j ? z.z : z.x;
                    hi[e][0] = j ? b.z : a.z, hi[e][1] = j ? b.w : a.w, hi[e][2] = j ? z.w : z.y;
                }
                float    anchor[3], scale[3];
                uint32_t axisWords[3][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}};
                double   dlo[4][3], dhi[4][3];
                for (int ax = 0; ax < 3; ++ax)
                {
                    double nlo = std::numeric_limits<double>::infinity(), nhi = -nlo;
                    for (int e = 0; e < 4; ++e)
                        if (words[e] != kQuadEmpty) nlo = std::min(nlo, lo[e][ax]), nhi = std::max(nhi, hi[e][ax]);
                    const double target = nlo - marginL;
                    float        an = static_cast<float>(target);
                    if (static_cast<double>(an) > target) an = std::nextafterf(an, -std::numeric_limits<float>::infinity());
                    const double span = (nhi + marginL) - static_cast<double>(an);
                    int          ex = 0;
                    (void)std::frexp(span / 254.0, &ex); // span / 254 = m * 2^ex, m in [0.5, 1): 2^ex >= span / 254
                    if (!(span > 0.0) || ex < -100 || ex > 100) { okL = false; break; }
                    const double sc = std::ldexp(1.0, ex);
                    anchor[ax] = an, scale[ax] = static_cast<float>(sc);
                    for (int e = 0; e < 4; ++e)
                    {
                        uint32_t bl = 0u, bh = 0u;
                        if (words[e] != kQuadEmpty)
                        {
                            const double fl = std::floor((lo[e][ax] - marginL - static_cast<double>(an)) / sc), ch = std::ceil((hi[e][ax] + marginL - static_cast<double>(an)) / sc);
                            if (!(fl >= 0.0 && ch <= 255.0 && fl <= ch)) { okL = false; break; }
                            bl = static_cast<uint32_t>(fl), bh = static_cast<uint32_t>(ch);
                        }
                        dlo[e][ax] = static_cast<double>(an) + bl * sc, dhi[e][ax] = static_cast<double>(an) + bh * sc;
                        axisWords[ax][e / 2] |= (bl | (bh << 8)) << (16 * (e % 2));
                    }
                }
                if (!okL) break;
                out.quadLocal[4 * r] = make_uint4(floatBits(anchor[0]), floatBits(anchor[1]), floatBits(anchor[2]), floatBits(scale[0]));
                out.quadLocal[4 * r + 1] = make_uint4(floatBits(scale[1]), floatBits(scale[2]), axisWords[0][0], axisWords[0][1]);
                out.quadLocal[4 * r + 2] = make_uint4(axisWords[1][0], axisWords[1][1], axisWords[2][0], axisWords[2][1]);
                out.quadLocal[4 * r + 3] = make_uint4(words[0], words[1], words[2], words[3]);
                for (int e = 0; e < 4; ++e)
                    if (words[e] != kQuadEmpty) aExact += area(lo[e], hi[e]), aLocal += area(dlo[e], dhi[e]);
            }
            out.quadLocalAreaRatio = aExact > 0.0 ? static_cast<float>(aLocal / aExact) : 1.0f;
            if (!okL) out.quadLocal.clear();
        }
    }

    if (!out.quadLocal.empty())
    {
        // ---- oct records (see WideBuild::oct): members = the root and every interior great-grandchild of a member, numbered in node order
        std::vector<uint32_t>& octIndex = out.octIndexOfNode;
        octIndex.assign(count, kQuadEmpty);
        struct Slots
        {
            uint32_t node[8];   // reference node in the slot, kQuadEmpty: empty
            uint32_t axis[7];   // split axes: [0] the member's, [1 + c] child c's, [3 + 2 c + g] grandchild (c, g)'s (0 where that node is a leaf / absent)
        };
        const auto slotsOf = [&](uint32_t i) {
            Slots sl;
            for (uint32_t& v : sl.node) v = kQuadEmpty;
            for (uint32_t& v : sl.axis) v = 0u;
            sl.axis[0] = nodes[i].splitAxis & 3u;
            const size_t kids[2] = {static_cast<size_t>(i) + 1, nodes[i].secondChildOffset};
            for (int c = 0; c < 2; ++c)
            {
                const BvhNode& cn = nodes[kids[c]];
                if (cn.triangleCount > 0) { sl.node[4 * c] = static_cast<uint32_t>(kids[c]); continue; }
                sl.axis[1 + c] = cn.splitAxis & 3u;
                const size_t gk[2] = {kids[c] + 1, cn.secondChildOffset};
                for (int g = 0; g < 2; ++g)
                {
                    const BvhNode& gn = nodes[gk[g]];
                    if (gn.triangleCount > 0) { sl.node[4 * c + 2 * g] = static_cast<uint32_t>(gk[g]); continue; }
                    sl.axis[3 + 2 * c + g] = gn.splitAxis & 3u;
                    sl.node[4 * c + 2 * g] = static_cast<uint32_t>(gk[g] + 1);
                    sl.node[4 * c + 2 * g + 1] = gn.secondChildOffset;
                }
            }
            return sl;
        };
        {
            std::vector<uint8_t>  member(count, 0);
            std::vector<uint32_t> todo{0u};
            while (!todo.empty())
            {
                const uint32_t i = todo.back();
                todo.pop_back();
                member[i] = 1;
                const Slots sl = slotsOf(i);
                for (const uint32_t nd : sl.node)
                    if (nd != kQuadEmpty && nodes[nd].triangleCount == 0) todo.push_back(nd);
            }
            uint32_t numOct = 0;
            for (size_t i = 0; i < count; ++i)
                if (member[i]) octIndex[i] = numOct++;
            out.oct.assign(8 * static_cast<size_t>(numOct), make_uint4(0u, 0u, 0u, 0u));
        }
        double R = 0.0;
        for (const float c : {out.rootLo.x, out.rootLo.y, out.rootLo.z, out.rootHi.x, out.rootHi.y, out.rootHi.z}) R = std::max(R, static_cast<double>(std::fabs(c)));
        const double marginL = (static_cast<double>(out.originBound) + R) * 3.814697265625e-06; // 2^-18, as for the local-grid quad records
        const auto   area = [](const double lo[3], const double hi[3]) {
            const double ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
            return 2.0 * (ex * ey + ey * ez + ez * ex);
        };
        double aExact = 0.0, aLocal = 0.0;
        bool   okO = true;
        for (size_t i = 0; i < count && okO; ++i)
        {
            if (octIndex[i] == kQuadEmpty) continue;
            const Slots sl = slotsOf(static_cast<uint32_t>(i));
            uint32_t    words[8];
            double      lo[8][3], hi[8][3];
            for (int e = 0; e < 8; ++e)
            {
                words[e] = kQuadEmpty;
                if (sl.node[e] == kQuadEmpty) continue;
                const BvhNode& en = nodes[sl.node[e]];
                words[e] = en.triangleCount > 0 ? leafWord(sl.node[e]) : octIndex[sl.node[e]];
                if (en.triangleCount == 0 && words[e] >= (1u << kWideIndexBits)) okO = false;
                lo[e][0] = en.aabb.min.x, lo[e][1] = en.aabb.min.y, lo[e][2] = en.aabb.min.z;
                hi[e][0] = en.aabb.max.x, hi[e][1] = en.aabb.max.y, hi[e][2] = en.aabb.max.z;
            }
            float    anchor[3], scale[3];
            uint32_t axisWords[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
            double   dlo[8][3], dhi[8][3];
            for (int ax = 0; ax < 3 && okO; ++ax)
            {
                double nlo = std::numeric_limits<double>::infinity(), nhi = -nlo;
                for (int e = 0; e < 8; ++e)
                    if (words[e] != kQuadEmpty) nlo = std::min(nlo, lo[e][ax]), nhi = std::max(nhi, hi[e][ax]);
                const double target = nlo - marginL;
                float        an = static_cast<float>(target);
                if (static_cast<double>(an) > target) an = std::nextafterf(an, -std::numeric_limits<float>::infinity());
                const double span = (nhi + marginL) - static_cast<double>(an);
                int          ex = 0;
                (void)std::frexp(span / 254.0, &ex); // span / 254 = m * 2^ex, m in [0.5, 1): 2^ex >= span / 254
                if (!(span > 0.0) || ex < -100 || ex > 100) { okO = false; break; }
                const double sc = std::ldexp(1.0, ex);
                anchor[ax] = an, scale[ax] = static_cast<float>(sc);
                for (int e = 0; e < 8; ++e)
                {
                    uint32_t bl = 255u, bh = 0u; // an empty slot: no ray passes lo = 255, hi = 0
                    if (words[e] != kQuadEmpty)
                    {
                        const double fl = std::floor((lo[e][ax] - marginL - static_cast<double>(an)) / sc), ch = std::ceil((hi[e][ax] + marginL - static_cast<double>(an)) / sc);
                        if (!(fl >= 0.0 && ch <= 255.0 && fl <= ch)) { okO = false; break; }
                        bl = static_cast<uint32_t>(fl), bh = static_cast<uint32_t>(ch);
                    }
                    dlo[e][ax] = static_cast<double>(an) + bl * sc, dhi[e][ax] = static_cast<double>(an) + bh * sc;
                    axisWords[ax][e / 2] |= (bl | (bh << 8)) << (16 * (e % 2));
                }
            }
            if (!okO) break;
            // visit positions of the eight slots for the four sign patterns with negZ = 0 (see WideBuild::oct)
            uint32_t order[2] = {0u, 0u};
            for (uint32_t pattern = 0; pattern < 4; ++pattern)
            {
                const auto     neg = [&](uint32_t axis) -> uint32_t { return axis < 2u ? (pattern >> axis) & 1u : 0u; };
                const uint32_t sN = neg(sl.axis[0]);
                uint32_t       field = 0u;
                for (uint32_t c = 0; c < 2; ++c)
                    for (uint32_t g = 0; g < 2; ++g)
                    {
                        const uint32_t position = ((c ^ sN) << 2) | ((g ^ neg(sl.axis[1 + c])) << 1) | (0u ^ neg(sl.axis[3 + 2 * c + g]));
                        field |= position << (4 * (2 * c + g));
                    }
                order[pattern / 2] |= field << (16 * (pattern % 2));
            }
            uint4* o = &out.oct[8 * static_cast<size_t>(octIndex[i])];
            o[0] = make_uint4(floatBits(anchor[0]), floatBits(anchor[1]), floatBits(anchor[2]), floatBits(scale[0]));
            o[1] = make_uint4(floatBits(scale[1]), floatBits(scale[2]), order[0], order[1]);
            o[2] = make_uint4(axisWords[0][0], axisWords[0][1], axisWords[0][2], axisWords[0][3]);
            o[3] = make_uint4(axisWords[1][0], axisWords[1][1], axisWords[1][2], axisWords[1][3]);
            o[4] = make_uint4(axisWords[2][0], axisWords[2][1], axisWords[2][2], axisWords[2][3]);
            o[5] = make_uint4(words[0], words[1], words[2], words[3]);
            o[6] = make_uint4(words[4], words[5], words[6], words[7]);
            for (int e = 0; e < 8; ++e)
                if (words[e] != kQuadEmpty) aExact += area(lo[e], hi[e]), aLocal += area(dlo[e], dhi[e]);
        }
        out.octAreaRatio = aExact > 0.0 ? static_cast<float>(aLocal / aExact) : 1.0f;
        if (!okO) out.oct.clear(), out.octIndexOfNode.clear();
    }
    if (!out.boxesRegular) out.compactUsable = false;
    if (!out.compactUsable || numInterior == 0) out.compact.clear();
    if (!out.boxesRegular) out.hotUsable = false;
    if (!out.hotUsable || numInterior == 0)
    {
        out.hot.clear();
        out.own.clear();
    }
    return out;
}

uint32_t checkWideLayouts(std::span<const BvhNode> nodes, float* quadHalfAreaRatio)
{
    if (nodes.empty()) throw std::runtime_error("checkWideLayouts: no nodes");
    const WideBuild wb = buildWide(nodes.data(), nodes.size());
    if (quadHalfAreaRatio) *quadHalfAreaRatio = wb.quadHalf.empty() ? 0.0f : wb.quadHalfAreaRatio;
    const uint32_t  flags = (wb.boxesRegular ? 1u : 0u) | (!wb.compact.empty() ? 2u : 0u) | (!wb.hot.empty() ? 4u : 0u) | (!wb.quad.empty() ? 8u : 0u) | (!wb.quadHalf.empty() ? 16u : 0u) | (!wb.quadLocal.empty() ? 32u : 0u) | (!wb.oct.empty() ? 64u : 0u);
    const size_t    records = wb.nodes.size() / 4;
    const auto      fail = [](size_t r, const char* what) { throw std::runtime_error("wide layout mismatch at record " + std::to_string(r) + ": " + what); };
    if (!wb.quadHalf.empty())
    {
        // The half-precision quad records: same words as the f32 quad records, every binary16 plane on the conservative side of the f32
        // plane by at least the margin of the proof (rf_wide.hpp), never subnormal, finite.
        if (wb.quadHalf.size() * 2 != wb.quad.size()) throw std::runtime_error("wide layout mismatch: half-precision quad records do not pair up with the quad records");
        double R = 0.0;
        for (const float c : {wb.rootLo.x, wb.rootLo.y, wb.rootLo.z, wb.rootHi.x, wb.rootHi.y, wb.rootHi.z}) R = std::max(R, static_cast<double>(std::fabs(c)));
        // What the proof needs (rf_wide.hpp): margin >= u (4 originBound + 3 R + margin) with u = 2^-24, the unit roundoff of the f32 operations it counts.  `built` is
        // the margin buildWide adds before its directed roundings, the largest a plane can be displaced by, and stands for the `+ margin` term.  The builder's
        // 2^-21 (originBound + R) = u (40 R + 8) is more than twice u (19 R + 4 + margin) at EVERY R.  (Until the scale sweep this line had 2^-23 for u: a requirement of
        // 2^-21 (4.75 R + 1) * 1.0001, which for R < 4e-4 is MORE than the builder's 2^-21 (5 R + 1) -- a plane that the directed rounding leaves exactly on the
        // builder's target, such as an upper plane rounded to binary16 zero, then failed a check that the proof does not ask for.  The builder was right.)
        const double built = (static_cast<double>(wb.originBound) + R) * 4.76837158203125e-07;
        const double margin = 5.9604644775390625e-08 * (4.0 * static_cast<double>(wb.originBound) + 3.0 * R + built) * 1.0001;
        if (!(static_cast<double>(wb.originBound) >= 4.0 * R)) throw std::runtime_error("wide layout mismatch: origin bound of the half-precision quad records");
        for (size_t r = 0; r < wb.quadHalf.size() / 4; ++r)
        {
            const float4* q = &wb.quad[8 * r];
            const uint4*  h = &wb.quadHalf[4 * r];
            const uint32_t d[16] = {h[0].x, h[0].y, h[0].z, h[0].w, h[1].x, h[1].y, h[1].z, h[1].w, h[2].x, h[2].y, h[2].z, h[2].w, h[3].x, h[3].y, h[3].z, h[3].w};
            if (d[12] != floatBits(q[6].x) || d[13] != floatBits(q[6].y) || d[14] != floatBits(q[6].z) || d[15] != floatBits(q[6].w)) fail(r, "half-precision quad record: words differ");
            for (int k = 0; k < 2; ++k)
            {
                const float4 a = q[3 * k], z = q[3 * k + 1], b = q[3 * k + 2];
                const float  lo[2][3] = {{a.x, a.y, z.x}, {b.x, b.y, z.z}}, hi[2][3] = {{a.z, a.w, z.y}, {b.z, b.w, z.w}};
                for (int j = 0; j < 2; ++j)
                    for (int ax = 0; ax < 3; ++ax)
                    {
                        const uint32_t w = d[3 * (2 * k + j) + ax];
                        if (d[12 + 2 * k + j] == kQuadEmpty)
                        {
                            // (an empty slot holds the inverted box that no ray passes: the traversal kernel does not test its word)
                            if (w != kHalfEmptyPlanes) fail(r, "half-precision quad record: an empty slot does not hold the inverted box");
                            continue;
                        }
                        const uint16_t l16 = static_cast<uint16_t>(w & 0xFFFFu), h16 = static_cast<uint16_t>(w >> 16);
                        for (const uint16_t v : {l16, h16})
                            if (((v >> 10) & 0x1Fu) == 0x1Fu || (((v >> 10) & 0x1Fu) == 0u && (v & 0x3FFu) != 0u)) fail(r, "half-precision quad record: a plane is not a normal number or zero");
                        if (!(static_cast<double>(halfBitsToFloat(l16)) <= static_cast<double>(lo[j][ax]) - margin)) fail(r, "half-precision quad record: a lower plane is not below its f32 plane by the margin");
                        if (!(static_cast<double>(halfBitsToFloat(h16)) >= static_cast<double>(hi[j][ax]) + margin)) fail(r, "half-precision quad record: an upper plane is not above its f32 plane by the margin");
                    }
            }
        }
    }
    if (!wb.quadLocal.empty())
    {
        // The local-grid quad records: same words, power-of-two scales, every decoded plane (anchor + byte * scale, exact in double) on the
        // conservative side of the f32 plane by at least the margin of the proof (rf_wide.hpp).
        if (wb.quadLocal.size() * 2 != wb.quad.size()) throw std::runtime_error("wide layout mismatch: local-grid quad records do not pair up with the quad records");
        double R = 0.0;
        for (const float c : {wb.rootLo.x, wb.rootLo.y, wb.rootLo.z, wb.rootHi.x, wb.rootHi.y, wb.rootHi.z}) R = std::max(R, static_cast<double>(std::fabs(c)));
        for (size_t r = 0; r < wb.quadLocal.size() / 4; ++r)
        {
            const float4*  q = &wb.quad[8 * r];
            const uint4*   l = &wb.quadLocal[4 * r];
            const uint32_t words[4] = {l[3].x, l[3].y, l[3].z, l[3].w};
            if (words[0] != floatBits(q[6].x) || words[1] != floatBits(q[6].y) || words[2] != floatBits(q[6].z) || words[3] != floatBits(q[6].w)) fail(r, "local-grid quad record: words differ");
            const float    anchor[3] = {bitsFloat(l[0].x), bitsFloat(l[0].y), bitsFloat(l[0].z)}, scale[3] = {bitsFloat(l[0].w), bitsFloat(l[1].x), bitsFloat(l[1].y)};
            const uint32_t axisWords[3][2] = {{l[1].z, l[1].w}, {l[2].x, l[2].y}, {l[2].z, l[2].w}};
            for (int ax = 0; ax < 3; ++ax)
            {
                int          ex = 0;
                const double m = std::frexp(static_cast<double>(scale[ax]), &ex);
                if (!(m == 0.5) || !std::isfinite(anchor[ax])) fail(r, "local-grid quad record: scale is not a power of two, or the anchor is not finite");
                // (u = 2^-24 as in the proof; the builder's 2^-18 (originBound + R) = u (320 R + 64) against u (46 R + 6) here: 6.9 x at R >> 1, 10.6 x at R << 1)
                const double margin = 5.9604644775390625e-08 * (6.03 * (static_cast<double>(wb.originBound) + R) + 1024.0 * static_cast<double>(scale[ax])) * 1.0001;
                for (int e = 0; e < 4; ++e)
                {
                    if (words[e] == kQuadEmpty) continue;
                    const int    k = e / 2, j = e % 2;
                    const float4 a = q[3 * k], z = q[3 * k + 1], b = q[3 * k + 2];
                    const double lo = ax == 0 ? (j ? b.x : a.x) : ax == 1 ? (j ? b.y : a.y) : (j ? z.z : z.x), hi = ax == 0 ? (j ? b.z : a.z) : ax == 1 ? (j ? b.w : a.w) : (j ? z.w : z.y);
                    const uint32_t pair = (axisWords[ax][e / 2] >> (16 * (e % 2))) & 0xFFFFu;
                    const double   dlo = static_cast<double>(anchor[ax]) + static_cast<double>(pair & 0xFFu) * static_cast<double>(scale[ax]),
                                 dhi = static_cast<double>(anchor[ax]) + static_cast<double>(pair >> 8) * static_cast<double>(scale[ax]);
                    if (!(dlo <= lo - margin)) fail(r, "local-grid quad record: a lower plane is not below its f32 plane by the margin");
                    if (!(dhi >= hi + margin)) fail(r, "local-grid quad record: an upper plane is not above its f32 plane by the margin");
                }
            }
        }
    }
    if (!wb.quad.empty())
    {
        // The leaf boxes and occluder-cache entries leafBoxesIntoTriangles writes into the triangle records (round 4): every leaf's box is its node's; an entry is 0
        // ("the leaf itself") or the index of a quad record from which the leaf is reached within `levels` steps -- in range, and really above THAT leaf.
        size_t numTriangles = 0;
        for (const BvhNode& n : nodes)
            if (n.triangleCount != 0) numTriangles = std::max(numTriangles, static_cast<size_t>(n.trianglesOffset) + n.triangleCount);
        const size_t numQuad = wb.quad.size() / 8;
        for (uint32_t levels = 0; levels <= 3; ++levels)
        {
            std::vector<float4> tri(4 * numTriangles, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            const bool          distinct = leafBoxesIntoTriangles(nodes.data(), nodes.size(), tri.data(), numTriangles, levels, &wb.quadIndexOfNode);
            if (!distinct) break; // (leaves sharing a first triangle: the renderer keeps the layouts that read these slots off)
            for (size_t i = 0; i < nodes.size(); ++i)
            {
                const BvhNode& n = nodes[i];
                if (n.triangleCount == 0) continue;
                const float4* t = &tri[4 * static_cast<size_t>(n.trianglesOffset)];
                if (floatBits(t[0].w) != floatBits(n.aabb.min.x) || floatBits(t[1].w) != floatBits(n.aabb.min.y) || floatBits(t[2].w) != floatBits(n.aabb.min.z) ||
                    floatBits(t[3].x) != floatBits(n.aabb.max.x) || floatBits(t[3].y) != floatBits(n.aabb.max.y) || floatBits(t[3].z) != floatBits(n.aabb.max.z))
                    fail(i, "leaf box in the triangle record differs from the node's");
                const uint32_t hint = floatBits(t[3].w);
                if (levels == 0 && hint != 0u) fail(i, "occluder-cache entry of a leaf: not 0 at level 0");
                if (hint == 0u) continue;
                if (hint >= numQuad) fail(i, "occluder-cache entry of a leaf: quad record index out of range");
                std::vector<uint32_t> frontier{hint};
                bool                  found = false;
                for (uint32_t l = 0; l < levels && !found; ++l)
                {
                    std::vector<uint32_t> next;
                    for (const uint32_t r : frontier)
                    {
                        const float4*  q = &wb.quad[8 * static_cast<size_t>(r)];
                        const uint32_t raw[4] = {floatBits(q[6].x), floatBits(q[6].y), floatBits(q[6].z), floatBits(q[6].w)};
                        for (int e = 0; e < 4; ++e)
                        {
                            if (raw[e] == kQuadEmpty) continue;
                            const uint32_t w = e == 2 ? raw[e] : raw[e] & ~(3u << kWideAxisShift); // (entries 0, 1 and 3 carry split axes)
                            if ((w & kWideLeafBit) == 0u)
                            {
                                if (w >= numQuad) fail(i, "occluder-cache entry of a leaf: a record below it names a record out of range");
                                next.push_back(w);
                                continue;
                            }
                            uint32_t first = w & ((1u << kWideIndexBits) - 1u);
                            if (((w >> kWideIndexBits) & 7u) == 7u) first = wb.bigLeaves[first].x;
                            if (first == n.trianglesOffset) found = true;
                        }
                    }
                    frontier.swap(next);
                }
                if (!found) fail(i, "occluder-cache entry of a leaf: the leaf is not below the record it names");
            }
        }
    }
    if (!wb.quad.empty())
    {
        // Walk the quad records from the root next to the 64-byte records: the entries of a quad record must be the children of
        // the children the plain record of the same node names (a leaf child filling one slot), with the same leaf words, the
        // split axes of both levels, and the skipped child's box must be the union of its entries (what makes the skip exact).
        struct Pair
        {
            uint32_t plain, quad;
        };
        std::vector<Pair> todo{{0u, 0u}};
        size_t            visited = 0;
        while (!todo.empty())
        {
            const Pair at = todo.back();
            todo.pop_back();
            ++visited;
            if (at.plain >= records || 8 * static_cast<size_t>(at.quad) + 8 > wb.quad.size()) fail(at.plain, "quad record index out of range");
            const float4*  w = &wb.nodes[4 * static_cast<size_t>(at.plain)];
            const float4*  q = &wb.quad[8 * static_cast<size_t>(at.quad)];
            const uint32_t qw[4] = {floatBits(q[6].x), floatBits(q[6].y), floatBits(q[6].z), floatBits(q[6].w)};
            const uint32_t pw[2] = {floatBits(w[3].x) & ~(3u << kWideAxisShift), floatBits(w[3].y)};
            if (((qw[0] >> kWideAxisShift) & 3u) != ((floatBits(w[3].x) >> kWideAxisShift) & 3u)) fail(at.plain, "quad record: split axis of the node differs");
            const float cbox[2][6] = {{w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y}, {w[2].x, w[2].y, w[2].z, w[2].w, w[1].z, w[1].w}};
            for (int k = 0; k < 2; ++k)
            {
                const float4*  e = q + 3 * k;
                const float    b0[6] = {e[0].x, e[0].y, e[0].z, e[0].w, e[1].x, e[1].y}, b1[6] = {e[2].x, e[2].y, e[2].z, e[2].w, e[1].z, e[1].w};
                const uint32_t wa = qw[2 * k], wb2 = qw[2 * k + 1];
                if (pw[k] & kWideLeafBit)
                {
                    // a leaf child fills slot 2k with itself
                    if ((wa & ~(3u << kWideAxisShift)) != pw[k] || wb2 != kQuadEmpty) fail(at.plain, "quad record: leaf child not passed through");
                    for (int j = 0; j < 6; ++j)
                        if (!(b0[j] == cbox[k][j])) fail(at.plain, "quad record: leaf child's box differs");
                    continue;
                }
                const float4*  cw = &wb.nodes[4 * static_cast<size_t>(pw[k])]; // the child's own plain record = its children
                const float    g0[6] = {cw[0].x, cw[0].y, cw[0].z, cw[0].w, cw[1].x, cw[1].y}, g1[6] = {cw[2].x, cw[2].y, cw[2].z, cw[2].w, cw[1].z, cw[1].w};
                const uint32_t gw[2] = {floatBits(cw[3].x) & ~(3u << kWideAxisShift), floatBits(cw[3].y)};
                const uint32_t childAxis = (floatBits(cw[3].x) >> kWideAxisShift) & 3u;
                for (int j = 0; j < 6; ++j)
                {
                    if (!(b0[j] == g0[j]) || !(b1[j] == g1[j])) fail(at.plain, "quad record: grandchild box differs");
                    const float u = (j == 0 || j == 1 || j == 4) ? std::min(g0[j], g1[j]) : std::max(g0[j], g1[j]);
                    if (!(u == cbox[k][j])) fail(at.plain, "quad record: skipped child's box is not the union of its children's");
                }
                const uint32_t tagged = k == 0 ? wb2 : wb2; // slot 2k+1 carries the child's split axis
                if (((tagged >> kWideAxisShift) & 3u) != childAxis) fail(at.plain, "quad record: split axis of a child differs");
                const uint32_t ea = k == 0 ? (wa & ~(3u << kWideAxisShift)) : wa, eb = wb2 & ~(3u << kWideAxisShift);
                const uint32_t ent[2] = {ea, eb};
                for (int j = 0; j < 2; ++j)
                {
                    if (gw[j] & kWideLeafBit)
                    {
                        if (ent[j] != gw[j]) fail(at.plain, "quad record: grandchild leaf word differs");
                    }
                    else
                    {
                        if (ent[j] & kWideLeafBit) fail(at.plain, "quad record: interior grandchild encoded as a leaf");
                        todo.push_back(Pair{gw[j], ent[j]});
                    }
                }
            }
        }
        if (visited != wb.quad.size() / 8) fail(0, "quad records: not every record is reachable from the root exactly once");
    }
    if (!wb.oct.empty())
    {
        // Oct records (round 5): walk them from the root next to the reference nodes.  Slot e = 4 c + 2 g + k must hold what the three levels below the member hold
        // at that place (a leaf fills the first slot of its range), every plane must lie outside its f32 plane by the margin, an empty slot must fail for every
        // ray (lo = 255, hi = 0), and for each of the eight direction-sign patterns the positions the KERNEL derives from the order table (kTraceWide, COMPACT == 6)
        // must put the slots into the order in which the reference's walk (wgsl:409-417 at each of the three levels) reaches them.
        double R = 0.0;
        for (const float c : {wb.rootLo.x, wb.rootLo.y, wb.rootLo.z, wb.rootHi.x, wb.rootHi.y, wb.rootHi.z}) R = std::max(R, static_cast<double>(std::fabs(c)));
        // 2^-18 (originBound + R), the margin the builder ADDS (a hair less: its floor / ceil run in double) -- 6.9 x what the proof of the local-grid records needs at
        // any R (see the local-grid check above), so this asks for more than the proof; it holds because the decoded planes anchor + byte * scale are exact in double
        const double margin = (static_cast<double>(wb.originBound) + R) * 3.814697265625e-06 * 0.999;
        const size_t numOct = wb.oct.size() / 8;
        struct Item
        {
            uint32_t node, rec;
        };
        std::vector<Item> todo{{0u, 0u}};
        size_t            visited = 0;
        while (!todo.empty())
        {
            const Item at = todo.back();
            todo.pop_back();
            ++visited;
            if (at.rec >= numOct || at.node >= nodes.size() || nodes[at.node].triangleCount != 0) fail(at.rec, "oct record: index out of range or not an interior node");
            uint32_t slotNode[8];
            for (uint32_t& v : slotNode) v = kQuadEmpty;
            const std::function<void(uint32_t, int, int)> place = [&](uint32_t nd, int depth, int base) {
                if (depth == 3 || (depth > 0 && nodes[nd].triangleCount != 0)) { slotNode[base] = nd; return; }
                place(nd + 1, depth + 1, base);
                place(nodes[nd].secondChildOffset, depth + 1, base + (4 >> depth));
            };
            place(at.node, 0, 0);
            const uint4*   o = &wb.oct[8 * static_cast<size_t>(at.rec)];
            const float    anchor[3] = {bitsFloat(o[0].x), bitsFloat(o[0].y), bitsFloat(o[0].z)}, scale[3] = {bitsFloat(o[0].w), bitsFloat(o[1].x), bitsFloat(o[1].y)};
            const uint32_t words[8] = {o[5].x, o[5].y, o[5].z, o[5].w, o[6].x, o[6].y, o[6].z, o[6].w};
            const uint32_t axisWords[3][4] = {{o[2].x, o[2].y, o[2].z, o[2].w}, {o[3].x, o[3].y, o[3].z, o[3].w}, {o[4].x, o[4].y, o[4].z, o[4].w}};
            for (int e = 0; e < 8; ++e)
            {
                for (int ax = 0; ax < 3; ++ax)
                {
                    const uint32_t pair = (axisWords[ax][e / 2] >> (16 * (e % 2))) & 0xFFFFu;
                    if (slotNode[e] == kQuadEmpty)
                    {
                        if (pair != 0x00FFu) fail(at.rec, "oct record: an empty slot does not hold the planes no ray passes");
                        continue;
                    }
                    const BvhNode& en = nodes[slotNode[e]];
                    const double   lo = ax == 0 ? en.aabb.min.x : ax == 1 ? en.aabb.min.y : en.aabb.min.z, hi = ax == 0 ? en.aabb.max.x : ax == 1 ? en.aabb.max.y : en.aabb.max.z;
                    const double   dlo = static_cast<double>(anchor[ax]) + static_cast<double>(pair & 0xFFu) * static_cast<double>(scale[ax]),
                                 dhi = static_cast<double>(anchor[ax]) + static_cast<double>(pair >> 8) * static_cast<double>(scale[ax]);
                    if (!(dlo <= lo - margin)) fail(at.rec, "oct record: a lower plane is not below its f32 plane by the margin");
                    if (!(dhi >= hi + margin)) fail(at.rec, "oct record: an upper plane is not above its f32 plane by the margin");
                }
                if (slotNode[e] == kQuadEmpty)
                {
                    if (words[e] != kQuadEmpty) fail(at.rec, "oct record: an empty slot names something");
                    continue;
                }
                const BvhNode& en = nodes[slotNode[e]];
                if (en.triangleCount != 0)
                {
                    if ((words[e] & kWideLeafBit) == 0u) fail(at.rec, "oct record: a leaf encoded as an interior entry");
                    uint32_t first = words[e] & ((1u << kWideIndexBits) - 1u), cnt = ((words[e] >> kWideIndexBits) & 7u) + 1u;
                    if (cnt == 8u) cnt = wb.bigLeaves[first].y, first = wb.bigLeaves[first].x;
                    if (first != en.trianglesOffset || cnt != en.triangleCount) fail(at.rec, "oct record: leaf word names other triangles");
                }
                else
                {
                    if ((words[e] & kWideLeafBit) != 0u || words[e] != wb.octIndexOfNode[slotNode[e]]) fail(at.rec, "oct record: interior entry names another record");
                    todo.push_back(Item{slotNode[e], words[e]});
                }
            }
            const unsigned long long table = (static_cast<unsigned long long>(o[1].w) << 32) | o[1].z;
            for (uint32_t signs = 0; signs < 8; ++signs)
            {
                std::vector<int>                              want; // slots in the order the reference reaches them
                const std::function<void(uint32_t, int, int)> walk = [&](uint32_t nd, int depth, int base) {
                    if (depth == 3 || (depth > 0 && nodes[nd].triangleCount != 0)) { want.push_back(base); return; }
                    const bool     neg = ((signs >> (nodes[nd].splitAxis & 3u)) & 1u) != 0u;
                    const uint32_t kid[2] = {nd + 1, nodes[nd].secondChildOffset};
                    const int      kidBase[2] = {base, base + (4 >> depth)};
                    for (int k = 0; k < 2; ++k) walk(kid[neg ? 1 - k : k], depth + 1, kidBase[neg ? 1 - k : k]);
                };
                walk(at.node, 0, 0);
                // the kernel's rule (refill + oct step)
                const uint32_t signXY = signs & 3u, negZ = signs >> 2;
                const uint32_t octKey = negZ ? ((16u * (3u - signXY)) | (0x7777u << 8)) : 16u * signXY;
                const uint32_t ord = static_cast<uint32_t>(table >> (octKey & 63u)) ^ (octKey >> 8);
                int            slotAt[8];
                for (int& v : slotAt) v = -1;
                for (int j = 0; j < 4; ++j)
                {
                    const uint32_t p0 = (ord >> (4 * j)) & 7u;
                    if (slotNode[2 * j] != kQuadEmpty) slotAt[p0] = 2 * j;
                    if (slotNode[2 * j + 1] != kQuadEmpty) slotAt[p0 ^ 1u] = 2 * j + 1;
                }
                std::vector<int> got;
                for (const int v : slotAt)
                    if (v >= 0) got.push_back(v);
                if (got != want) fail(at.rec, "oct record: the order table does not reproduce the reference's visit order");
            }
        }
        if (visited != numOct) fail(0, "oct records: not every record is reachable from the root exactly once");
    }
    for (size_t r = 0; r < records; ++r)
    {
        const float4* w = &wb.nodes[4 * r];
        // child planes of the plain record, in the order {lo.x lo.y hi.x hi.y lo.z hi.z}
        const float    c0[6] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y}, c1[6] = {w[2].x, w[2].y, w[2].z, w[2].w, w[1].z, w[1].w};
        const uint32_t word0 = floatBits(w[3].x), word1 = floatBits(w[3].y);
        float          own[6]; // the node's own box: the union of its children's (lo: min, hi: max)
        for (int k = 0; k < 6; ++k) own[k] = (k == 0 || k == 1 || k == 4) ? std::min(c0[k], c1[k]) : std::max(c0[k], c1[k]);
        if (!wb.compact.empty())
        {
            const float4*  c = &wb.compact[4 * r];
            const uint32_t cw0 = floatBits(c[2].x), cw1 = floatBits(c[2].z);
            const bool     selLo = (cw1 >> kWideAxisShift) & 1u, selHi = (cw1 >> (kWideAxisShift + 1)) & 1u;
            const float    d0[6] = {selLo ? c[3].x : c[0].x, c[0].y, selHi ? c[3].y : c[0].z, c[0].w, c[1].x, c[1].y};
            const float    d1[6] = {selLo ? c[0].x : c[3].x, c[2].y, selHi ? c[0].z : c[3].y, c[2].w, c[1].z, c[1].w};
            for (int k = 0; k < 6; ++k)
                if (!(d0[k] == c0[k]) || !(d1[k] == c1[k])) fail(r, "compact-capable record decodes to other planes");
            if (cw0 != word0 || (cw1 & ~(3u << kWideAxisShift)) != word1) fail(r, "compact-capable record holds other child words");
            if (!(c[3].x == own[0]) || !(c[3].y == own[2])) fail(r, "compact-capable record: outer x planes are not the node's");
        }
        if (!wb.hot.empty())
        {
            const float4*  h = &wb.hot[2 * r];
            const float4*  o = &wb.own[2 * r];
            const uint32_t hw0 = floatBits(h[1].z), hw1 = floatBits(h[1].w);
            const float    inner[6] = {h[0].x, h[0].y, h[0].z, h[0].w, h[1].x, h[1].y}, outer[6] = {o[0].x, o[0].y, o[0].z, o[0].w, o[1].x, o[1].y};
            const bool     sel[6] = {((hw0 >> 25) & 1u) != 0u, ((hw0 >> 24) & 1u) != 0u, ((hw1 >> 25) & 1u) != 0u,
                                     ((hw1 >> 24) & 1u) != 0u, ((hw1 >> 30) & 1u) != 0u, ((hw1 >> 29) & 1u) != 0u};
            for (int k = 0; k < 6; ++k)
            {
                if (!((sel[k] ? outer[k] : inner[k]) == c0[k]) || !((sel[k] ? inner[k] : outer[k]) == c1[k])) fail(r, "32-byte record decodes to other planes");
                if (!(outer[k] == own[k])) fail(r, "own-box array does not hold the union of the children");
            }
            if ((hw0 & ~(3u << 24)) != word0 || (hw1 & ~((3u << 24) | (3u << kWideAxisShift))) != word1) fail(r, "32-byte record holds other child words");
        }
    }
    return flags;
}
} // namespace rf
