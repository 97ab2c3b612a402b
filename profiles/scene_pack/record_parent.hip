// record_parent.hip -- the throw-away recorder of tests/golden/scene_pack_parent.json.  Built against the PARENT commit's headers and library, never by the tree's
// build: see README.md here for the command.  packScene below is the packing code of the parent's Renderer::Renderer (rf_renderer.hip, from the sortScale line
// to the albedo LUT), copied line for line and compiled the way it was compiled there: as host code of a .hip file with the Makefile's HIPFLAGS.  The only edits:
// `m` is a stand-in whose buffers keep what was "uploaded" in host memory, the WideBuild is kept (one added line, marked), and the blue-noise upload is left out.
// checkWideLayouts is the parent library's own, through rf_wide_layout_stats.  The reading and printing is tests/scene_pack_main.cpp, included at the end.
#include "rayfinder_amd.h"
#include "rf_kernels.hpp"

#include <span>
#include <stdexcept>
#include <vector>

namespace rf
{
struct SceneFacts
{
    uint64_t sceneCounts[4] = {};
    uint32_t sceneRootBounds[6] = {};
    uint32_t sortScale = 0;
    bool     wideUsable = true, leafBoxesValid = false, selfShadowOk = false; // (Impl's initial values)
    uint32_t maxLeafTriangles = 0, occluderHintLevels = 0;
    uint64_t treeBytes = 0;
    float    quadHalfAreaRatio = 0.0f;
    uint32_t quadHalfFromBounce = 0, quadHalfShadowFromBounce = 0, quadLocalFromBounce = 0, quadLocalShadowFromBounce = 0, octFromBounce = 0;
};
struct PackedScene
{
    std::vector<float4>            nodes;
    WideBuild                      wide;
    std::vector<float4>            triangles, attributes, shadeRecords;
    std::vector<TextureDescriptor> textureDescriptors;
    std::vector<uint32_t>          texels;
    std::vector<float>             albedoLut;
    SceneFacts                     facts;
};

namespace
{
template<typename T>
struct HostBuffer // DeviceBuffer's interface, in host memory
{
    std::vector<T> host;
    T*             ptr = nullptr;
    size_t         count = 0;
    void upload(const T* src, size_t n)
    {
        host.assign(src, src + n);
        ptr = n ? host.data() : nullptr;
        count = n;
    }
    void release()
    {
        host.clear();
        ptr = nullptr;
        count = 0;
    }
};
struct ImplStandIn // the members the copied code touches, with Impl's names and initial values
{
    HostBuffer<float4>            nodes, triangles, wideNodes, wideCompact, wideHot, wideOwn, wideQuad;
    HostBuffer<uint4>             wideQuadHalf, wideQuadLocal, wideOct;
    HostBuffer<uint2>             bigLeaves;
    WideScene                     wide{};
    HostBuffer<float4>            attributes, shadeRecords;
    HostBuffer<TextureDescriptor> textureDescriptors;
    HostBuffer<uint32_t>          texels;
    HostBuffer<float>             albedoLut;
    DeviceScene                   scene{};
    uint64_t sceneCounts[4] = {};
    uint32_t sceneRootBounds[6] = {};
    bool     wideUsable = true;
    uint32_t occluderHintLevels = 0;
    bool     leafBoxesValid = false;
    uint32_t maxLeafTriangles = 0, sortScale = 0;
    bool     selfShadowOk = false;
    uint32_t optQuadHalfFromBounce = 0, optQuadHalfShadowFromBounce = 0;
    float    quadHalfAreaRatio = 0.0f;
    uint32_t optQuadLocalFromBounce = 0, optQuadLocalShadowFromBounce = 0, optOctFromBounce = 0;
    uint64_t treeBytes = 0;
};
} // namespace

PackedScene packScene(const SceneView& sceneView)
{
    ImplStandIn m;
    WideBuild   keptWide;
    // ---------------------------------------------------------------- the parent's constructor, copied
    m.sortScale = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(kSortBins) << 32) / std::max<uint64_t>(sceneView.positionAttributes.size(), 1), 0xFFFFFFFFull));
    {
        uint64_t texelCount = 0;
        for (const TextureView& t : sceneView.baseColorTextures) texelCount += static_cast<uint64_t>(t.width) * t.height;
        m.sceneCounts[0] = sceneView.bvhNodes.size(), m.sceneCounts[1] = sceneView.positionAttributes.size(), m.sceneCounts[2] = sceneView.baseColorTextures.size(), m.sceneCounts[3] = texelCount;
        const Aabb& root = sceneView.bvhNodes[0].aabb;
        const float bounds[6] = {root.min.x, root.min.y, root.min.z, root.max.x, root.max.y, root.max.z};
        std::memcpy(m.sceneRootBounds, bounds, sizeof bounds);
    }

    // 48-B reference nodes -> 32-B device nodes
    bool                  treeNestedRegular = false; // every child's box inside its parent's, all finite and ordered (buildWide)
    std::vector<uint32_t> quadIndexOfNode; // buildWide's numbering of the quad records, for the occluder-cache entries of the leaves (leafBoxesIntoTriangles)
    {
        std::vector<float4> packed(2 * sceneView.bvhNodes.size());
        for (size_t i = 0; i < sceneView.bvhNodes.size(); ++i)
        {
            const BvhNode& n = sceneView.bvhNodes[i];
            const bool     leaf = n.triangleCount > 0;
            if (n.triangleCount >= (1u << 30)) throw std::runtime_error("BVH leaf too large");
            const uint32_t link = leaf ? n.trianglesOffset : n.secondChildOffset;
            const uint32_t meta = leaf ? ((n.triangleCount << 2) | kLeafAxis) : (n.splitAxis & 3u);
            if (!leaf && n.splitAxis > 2) throw std::runtime_error("interior BVH node with invalid split axis");
            packed[2 * i] = make_float4(n.aabb.min.x, n.aabb.min.y, n.aabb.min.z, bitsFloat(link));
            packed[2 * i + 1] = make_float4(n.aabb.max.x, n.aabb.max.y, n.aabb.max.z, bitsFloat(meta));
        }
        m.nodes.upload(packed.data(), packed.size());
        const WideBuild wb = buildWide(sceneView.bvhNodes.data(), sceneView.bvhNodes.size());
        quadIndexOfNode = wb.quadIndexOfNode;
        treeNestedRegular = wb.boxesNested && wb.boxesRegular;
        m.wideNodes.upload(wb.nodes.data(), wb.nodes.size());
        m.bigLeaves.upload(wb.bigLeaves.data(), wb.bigLeaves.size());
        m.wide.nodes = m.wideNodes.ptr;
        m.wide.compact = nullptr;
#if defined(RF_EXP_LEGACY_LAYOUTS)
        if (wb.compactUsable && !wb.compact.empty())
        {
            m.wideCompact.upload(wb.compact.data(), wb.compact.size());
            m.wide.compact = m.wideCompact.ptr;
        }
#endif
        m.wide.hot = m.wide.own = nullptr;
#if defined(RF_EXP_LEGACY_LAYOUTS)
        if (wb.hotUsable && !wb.hot.empty())
        {
            m.wideHot.upload(wb.hot.data(), wb.hot.size());
            m.wideOwn.upload(wb.own.data(), wb.own.size());
            m.wide.hot = m.wideHot.ptr;
            m.wide.own = m.wideOwn.ptr;
        }
#endif
        m.wide.quad = nullptr;
        if (wb.quadUsable && !wb.quad.empty())
        {
            m.wideQuad.upload(wb.quad.data(), wb.quad.size());
            m.wide.quad = m.wideQuad.ptr;
        }
        m.wide.quadHalf = nullptr;
        m.wide.originBound = wb.originBound;
        if (!wb.quadHalf.empty())
        {
            m.wideQuadHalf.upload(wb.quadHalf.data(), wb.quadHalf.size());
            m.wide.quadHalf = m.wideQuadHalf.ptr;
            // default (rf_wide.hpp, kQuadHalfMaxAreaRatio): the closest-hit launches read the half-precision records unless the binary16
            // grid is too coarse for this scene; the shadow launches prefer the local-grid records (below)
            m.optQuadHalfFromBounce = m.optQuadHalfShadowFromBounce = wb.quadHalfAreaRatio <= kQuadHalfMaxAreaRatio ? 1u : 0u;
            m.quadHalfAreaRatio = wb.quadHalfAreaRatio;
        }
        m.wide.quadLocal = nullptr;
        if (!wb.quadLocal.empty())
        {
            m.wideQuadLocal.upload(wb.quadLocal.data(), wb.quadLocal.size());
            m.wide.quadLocal = m.wideQuadLocal.ptr;
            // closest-hit: the per-record 8-bit grid where binary16 of absolute coordinates is too coarse (small triangles far from the
            // origin); shadow: the local grid unless the scene is so finely tessellated that the exact records win (kQuadLocalShadowMaxAreaRatio)
            const float ratio = wb.quadHalf.empty() ? 2.0f : wb.quadHalfAreaRatio;
            // (from bounce 2: the coherent launches of bounce 1 gain nothing from it and lose 5 - 25 % in the larger scenes; the shadow launches
            // of bounce 1 stay on the half-precision records where those suit the scene, on the exact ones elsewhere)
            m.optQuadLocalFromBounce = m.optQuadHalfFromBounce == 0u ? 2u : 0u;
            m.optQuadLocalShadowFromBounce = ratio <= kQuadLocalShadowMaxAreaRatio ? 2u : 0u;
        }
        m.wide.oct = nullptr;
        m.treeBytes = static_cast<uint64_t>(wb.quadLocal.size()) * sizeof(uint4) + static_cast<uint64_t>(sceneView.positionAttributes.size()) * kTriStride * sizeof(float4);
        if (!wb.oct.empty())
        {
            m.wideOct.upload(wb.oct.data(), wb.oct.size());
            m.wide.oct = m.wideOct.ptr;
            // NOT selected by default: measured 17 % SLOWER than the local-grid quad records on the out-of-cache atrium (profiles/r05_hbm: the launch is bound by
            // L1 -> L2 requests, and a 112-byte record is two of them per step for 0.65 x the steps); option oct_from_bounce turns it on
            m.optOctFromBounce = 0u;
        }
        m.wide.bigLeaves = m.bigLeaves.ptr;
        m.wide.rootLo = wb.rootLo;
        m.wide.rootHi = wb.rootHi;
        m.wide.rootLeaf = wb.rootLeaf;
        m.wide.numRecords = static_cast<uint32_t>(wb.nodes.size() / 4);
        keptWide = wb; // (ADDED for the recorder)
        m.wideUsable = wb.boxesRegular; // NaN / inverted boxes: only the reference-ordered scalar kernels are exact
    }
    {
        // 48-B PositionAttribute -> 64-B aligned device triangles (one L2 sector per triangle test)
        const size_t        n = sceneView.positionAttributes.size();
        std::vector<float4> padded(kTriStride * n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (size_t i = 0; i < n; ++i)
        {
            const PositionAttribute& t = sceneView.positionAttributes[i];
            padded[kTriStride * i] = make_float4(t.p0.x, t.p0.y, t.p0.z, 0.0f);
            padded[kTriStride * i + 1] = make_float4(t.p1.x, t.p1.y, t.p1.z, 0.0f);
            padded[kTriStride * i + 2] = make_float4(t.p2.x, t.p2.y, t.p2.z, 0.0f);
        }
        // ... and the exact box of every leaf in the spare floats of its first triangle (read by the half-precision quad kernels)
        {
            // What the occluder cache remembers per stopped ray: the leaf -- or, where the leaves are small against the sun disc's footprint at the occluder (the
            // next ray from the same place is stopped by a NEIGHBOUR of that triangle), a record a few levels above it.  Footprint: the disc's 0.51 degrees over a
            // third of the scene = 0.003 extents; every quad level doubles the patch.  Atrium (18-cm leaves in 30 m): 0 -- the leaf; its x8 tessellation (2.3 cm): 2
            // (shadow launches -22 % against -2 % with leaves: profiles/r04_occluder/x8_hint_levels.log).
            std::vector<float> diag;
            diag.reserve(sceneView.bvhNodes.size() / 2 + 1);
            for (const BvhNode& nd : sceneView.bvhNodes)
                if (nd.triangleCount != 0)
                {
                    m.maxLeafTriangles = std::max(m.maxLeafTriangles, nd.triangleCount);
                    const float dx = nd.aabb.max.x - nd.aabb.min.x, dy = nd.aabb.max.y - nd.aabb.min.y, dz = nd.aabb.max.z - nd.aabb.min.z;
                    diag.push_back(std::sqrt(dx * dx + dy * dy + dz * dz));
                }
            const Aabb& root = sceneView.bvhNodes[0].aabb;
            const float extent = std::max({root.max.x - root.min.x, root.max.y - root.min.y, root.max.z - root.min.z});
            m.occluderHintLevels = 0;
            if (!diag.empty() && extent > 0.0f)
            {
                std::nth_element(diag.begin(), diag.begin() + diag.size() / 2, diag.end());
                const float median = diag[diag.size() / 2];
                if (median > 0.0f && std::isfinite(median) && std::isfinite(extent))
                    m.occluderHintLevels = static_cast<uint32_t>(std::clamp(static_cast<int>(std::floor(std::log2(0.003f * extent / median))) + 1, 0, 3));
            }
            if (const char* v = std::getenv("RF_OCCLUDER_HINT_LEVELS")) m.occluderHintLevels = static_cast<uint32_t>(std::clamp(std::atoi(v), 0, 8)); // experiments
        }
        m.leafBoxesValid = leafBoxesIntoTriangles(sceneView.bvhNodes.data(), sceneView.bvhNodes.size(), padded.data(), n, m.occluderHintLevels, &quadIndexOfNode);
        if (!m.leafBoxesValid)
        {
            // leaves that share a first triangle (hand-made tree): one slot cannot hold two exact boxes, so the layouts that cull a leaf by
            // the box in that slot stay off and the exact records (which carry every box themselves) are used
            m.wide.quadHalf = m.wide.quadLocal = m.wide.oct = nullptr;
            m.wideQuadHalf.release(), m.wideQuadLocal.release(), m.wideOct.release();
            m.optQuadHalfFromBounce = m.optQuadHalfShadowFromBounce = m.optQuadLocalFromBounce = m.optQuadLocalShadowFromBounce = m.optOctFromBounce = 0u;
        }
        m.triangles.upload(padded.data(), padded.size());
    }
    {
        // 80-B VertexAttributes (three padded normals, three uvs, texture index, pad) -> 64 B = one L2 sector per shaded hit
        const size_t        n = sceneView.vertexAttributes.size();
        std::vector<float4> packed(4 * n);
        for (size_t i = 0; i < n; ++i)
        {
            const VertexAttributes& v = sceneView.vertexAttributes[i];
            packed[4 * i] = make_float4(v.n0.x, v.n0.y, v.n0.z, v.n1.x);
            packed[4 * i + 1] = make_float4(v.n1.y, v.n1.z, v.n2.x, v.n2.y);
            packed[4 * i + 2] = make_float4(v.n2.z, v.uv0.x, v.uv0.y, v.uv1.x);
            packed[4 * i + 3] = make_float4(v.uv1.y, v.uv2.x, v.uv2.y, bitsFloat(v.textureIdx));
        }
        m.attributes.upload(packed.data(), packed.size());
        // kShade's record: positions + these four float4, 128 B per triangle
        std::vector<float4> rec(8 * n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (size_t i = 0; i < n; ++i)
        {
            const PositionAttribute& t = sceneView.positionAttributes[i];
            rec[8 * i] = make_float4(t.p0.x, t.p0.y, t.p0.z, 0.0f);
            rec[8 * i + 1] = make_float4(t.p1.x, t.p1.y, t.p1.z, 0.0f);
            rec[8 * i + 2] = make_float4(t.p2.x, t.p2.y, t.p2.z, 0.0f);
            for (int k = 0; k < 4; ++k) rec[8 * i + 3 + k] = packed[4 * i + k];
        }
        // kShadeSelfShadow: the exact box of the leaf a triangle sits in, in the spare floats of its record ({p0 lo.x} {p1 lo.y} {p2 lo.z} ... {hi.xyz, 1}).  Only where the
        // argument holds (kShade): boxes nested and regular all the way up (buildWide checked every parent / child pair), and the triangle in exactly ONE leaf.
        m.selfShadowOk = treeNestedRegular;
        if (m.selfShadowOk)
        {
            std::vector<uint8_t> leaves(n, 0);
            for (const BvhNode& nd : sceneView.bvhNodes)
                for (uint32_t t = 0; t < nd.triangleCount; ++t)
                {
                    const size_t i = static_cast<size_t>(nd.trianglesOffset) + t;
                    if (i >= n) continue; // (validateScene has rejected this)
                    const bool regular = std::fabs(nd.aabb.min.x) < 1e30f && std::fabs(nd.aabb.min.y) < 1e30f && std::fabs(nd.aabb.min.z) < 1e30f && std::fabs(nd.aabb.max.x) < 1e30f &&
                                         std::fabs(nd.aabb.max.y) < 1e30f && std::fabs(nd.aabb.max.z) < 1e30f && nd.aabb.min.x <= nd.aabb.max.x && nd.aabb.min.y <= nd.aabb.max.y &&
                                         nd.aabb.min.z <= nd.aabb.max.z;
                    leaves[i] = static_cast<uint8_t>(std::min(leaves[i] + (regular ? 1 : 2), 2));
                    rec[8 * i].w = nd.aabb.min.x, rec[8 * i + 1].w = nd.aabb.min.y, rec[8 * i + 2].w = nd.aabb.min.z;
                    rec[8 * i + 7] = make_float4(nd.aabb.max.x, nd.aabb.max.y, nd.aabb.max.z, 0.0f);
                }
            for (size_t i = 0; i < n; ++i) rec[8 * i + 7].w = leaves[i] == 1 ? 1.0f : 0.0f;
        }
        m.shadeRecords.upload(rec.data(), rec.size());
    }

    // texture blob + descriptors in the order of the model's textures (reference_path_tracer.cpp:210-270)
    {
        std::vector<TextureDescriptor> descs;
        std::vector<uint32_t>          blob;
        for (const TextureView& t : sceneView.baseColorTextures)
        {
            const uint32_t offset = static_cast<uint32_t>(blob.size());
            const size_t   n = static_cast<size_t>(t.width) * t.height;
            blob.insert(blob.end(), t.pixels, t.pixels + n);
            descs.push_back({t.width, t.height, offset});
        }
        // the reference refuses texture blobs above its 1 GiB binding limit (reference_path_tracer.cpp:254-263,
        // gpu_limits.hpp); HBM has room, but u32 texel offsets cap the blob at 2^32 texels
        if (blob.size() > 0xFFFFFFFFull) throw std::runtime_error("Texture buffer size exceeds the 32-bit texel offset range.");
        if (blob.empty()) blob.push_back(0xFFFFFFFFu);
        if (descs.empty()) descs.push_back({1, 1, 0});
        m.textureDescriptors.upload(descs.data(), descs.size());
        m.texels.upload(blob.data(), blob.size());
    }
    {
        float lut[256];
        for (int i = 0; i < 256; ++i)
            lut[i] = static_cast<float>(std::pow(static_cast<double>(static_cast<float>(i) / 255.0f), static_cast<double>(2.2f)));
        m.albedoLut.upload(lut, 256);
    }
    m.scene.nodes = m.nodes.ptr;
    m.scene.triangles = m.triangles.ptr;
    m.scene.attributes = m.attributes.ptr;
    m.scene.shadeRecords = m.shadeRecords.ptr;
    m.scene.textureDescriptors = m.textureDescriptors.ptr;
    m.scene.texels = m.texels.ptr;
    m.scene.numTexels = m.texels.count;
    m.scene.albedoLut = m.albedoLut.ptr;
    // ---------------------------------------------------------------- end of the copy: what was uploaded, under packScene's names
    PackedScene out;
    out.nodes = m.nodes.host;
    out.wide = keptWide;
    out.wide.nodes = m.wideNodes.host, out.wide.quad = m.wideQuad.host, out.wide.quadHalf = m.wideQuadHalf.host, out.wide.quadLocal = m.wideQuadLocal.host;
    out.wide.oct = m.wideOct.host, out.wide.bigLeaves = m.bigLeaves.host;
    out.triangles = m.triangles.host, out.attributes = m.attributes.host, out.shadeRecords = m.shadeRecords.host;
    out.textureDescriptors = m.textureDescriptors.host, out.texels = m.texels.host, out.albedoLut = m.albedoLut.host;
    SceneFacts& f = out.facts;
    std::memcpy(f.sceneCounts, m.sceneCounts, sizeof f.sceneCounts);
    std::memcpy(f.sceneRootBounds, m.sceneRootBounds, sizeof f.sceneRootBounds);
    f.sortScale = m.sortScale, f.wideUsable = m.wideUsable, f.leafBoxesValid = m.leafBoxesValid, f.selfShadowOk = m.selfShadowOk;
    f.maxLeafTriangles = m.maxLeafTriangles, f.occluderHintLevels = m.occluderHintLevels, f.treeBytes = m.treeBytes, f.quadHalfAreaRatio = m.quadHalfAreaRatio;
    f.quadHalfFromBounce = m.optQuadHalfFromBounce, f.quadHalfShadowFromBounce = m.optQuadHalfShadowFromBounce;
    f.quadLocalFromBounce = m.optQuadLocalFromBounce, f.quadLocalShadowFromBounce = m.optQuadLocalShadowFromBounce, f.octFromBounce = m.optOctFromBounce;
    // what the uploads leave behind must agree with the pointers the kernels were given
    if ((m.wide.quad != nullptr) != !out.wide.quad.empty() || (m.wide.quadHalf != nullptr) != !out.wide.quadHalf.empty() ||
        (m.wide.quadLocal != nullptr) != !out.wide.quadLocal.empty() || (m.wide.oct != nullptr) != !out.wide.oct.empty() || m.wide.originBound != keptWide.originBound ||
        m.wide.numRecords != out.wide.nodes.size() / 4 || m.wide.rootLeaf != keptWide.rootLeaf || m.scene.numTexels != out.texels.size())
        throw std::logic_error("recorder: the stand-in's pointers and its buffers disagree");
    return out;
}

uint32_t checkWideLayouts(std::span<const BvhNode> nodes, float* quadHalfAreaRatio)
{
    uint32_t flags = 0;
    if (rf_wide_layout_stats(nodes.data(), nodes.size(), &flags, quadHalfAreaRatio) != RF_OK) throw std::runtime_error(rf_last_error_message());
    return flags;
}
} // namespace rf

#define SCENE_PACK_PARENT_RECORDER
#include "scene_pack_main.cpp"
