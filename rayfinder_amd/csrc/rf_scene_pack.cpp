// rf_scene_pack.cpp -- the scene preparation of the renderer: reference arrays -> device layouts in host memory (rf_scene_pack.hpp).  Host only.
#include "rf_scene_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace rf
{
PackedScene packScene(const SceneView& sceneView)
{
    PackedScene out;
    SceneFacts& f = out.facts;
    f.sortScale = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(kSortBins) << 32) / std::max<uint64_t>(sceneView.positionAttributes.size(), 1), 0xFFFFFFFFull));
    {
        uint64_t texelCount = 0;
        for (const TextureView& t : sceneView.baseColorTextures) texelCount += static_cast<uint64_t>(t.width) * t.height;
        f.sceneCounts[0] = sceneView.bvhNodes.size(), f.sceneCounts[1] = sceneView.positionAttributes.size(), f.sceneCounts[2] = sceneView.baseColorTextures.size(), f.sceneCounts[3] = texelCount;
        const Aabb& root = sceneView.bvhNodes[0].aabb;
        const float bounds[6] = {root.min.x, root.min.y, root.min.z, root.max.x, root.max.y, root.max.z};
        std::memcpy(f.sceneRootBounds, bounds, sizeof bounds);
    }

    // 48-B reference nodes -> 32-B device nodes
    {
        out.nodes.resize(2 * sceneView.bvhNodes.size());
        for (size_t i = 0; i < sceneView.bvhNodes.size(); ++i)
        {
            const BvhNode& n = sceneView.bvhNodes[i];
            const bool     leaf = n.triangleCount > 0;
            if (n.triangleCount >= (1u << 30)) throw std::runtime_error("BVH leaf too large");
            const uint32_t link = leaf ? n.trianglesOffset : n.secondChildOffset;
            const uint32_t meta = leaf ? ((n.triangleCount << 2) | kLeafAxis) : (n.splitAxis & 3u);
            if (!leaf && n.splitAxis > 2) throw std::runtime_error("interior BVH node with invalid split axis");
            out.nodes[2 * i] = make_float4(n.aabb.min.x, n.aabb.min.y, n.aabb.min.z, bitsFloat(link));
            out.nodes[2 * i + 1] = make_float4(n.aabb.max.x, n.aabb.max.y, n.aabb.max.z, bitsFloat(meta));
        }
    }
    // ... -> the render path's records, and the layouts the scene gets with no option set
    out.wide = buildWide(sceneView.bvhNodes.data(), sceneView.bvhNodes.size());
    const WideBuild& wb = out.wide;
    if (!wb.quadHalf.empty())
    {
        // default (rf_wide.hpp, kQuadHalfMaxAreaRatio): the closest-hit launches read the half-precision records unless the binary16
        // grid is too coarse for this scene; the shadow launches prefer the local-grid records (below)
        f.quadHalfFromBounce = f.quadHalfShadowFromBounce = wb.quadHalfAreaRatio <= kQuadHalfMaxAreaRatio ? 1u : 0u;
        f.quadHalfAreaRatio = wb.quadHalfAreaRatio;
    }
    if (!wb.quadLocal.empty())
    {
        // closest-hit: the per-record 8-bit grid where binary16 of absolute coordinates is too coarse (small triangles far from the
        // origin); shadow: the local grid unless the scene is so finely tessellated that the exact records win (kQuadLocalShadowMaxAreaRatio)
        const float ratio = wb.quadHalf.empty() ? 2.0f : wb.quadHalfAreaRatio;
        // (from bounce 2: the coherent launches of bounce 1 gain nothing from it and lose 5 - 25 % in the larger scenes; the shadow launches
        // of bounce 1 stay on the half-precision records where those suit the scene, on the exact ones elsewhere)
        f.quadLocalFromBounce = f.quadHalfFromBounce == 0u ? 2u : 0u;
        f.quadLocalShadowFromBounce = ratio <= kQuadLocalShadowMaxAreaRatio ? 2u : 0u;
    }
    f.treeBytes = static_cast<uint64_t>(wb.quadLocal.size()) * sizeof(uint4) + static_cast<uint64_t>(sceneView.positionAttributes.size()) * kTriStride * sizeof(float4);
    // the oct records are NOT selected by default: measured 17 % SLOWER than the local-grid quad records on the out-of-cache atrium (profiles/r05_hbm: the launch is
    // bound by L1 -> L2 requests, and a 112-byte record is two of them per step for 0.65 x the steps); option oct_from_bounce turns them on
    f.octFromBounce = 0u;
    f.wideUsable = wb.boxesRegular; // NaN / inverted boxes: only the reference-ordered scalar kernels are exact
    {
        // 48-B PositionAttribute -> 64-B aligned device triangles (one L2 sector per triangle test)
        const size_t n = sceneView.positionAttributes.size();
        out.triangles.assign(kTriStride * n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (size_t i = 0; i < n; ++i)
        {
            const PositionAttribute& t = sceneView.positionAttributes[i];
            out.triangles[kTriStride * i] = make_float4(t.p0.x, t.p0.y, t.p0.z, 0.0f);
            out.triangles[kTriStride * i + 1] = make_float4(t.p1.x, t.p1.y, t.p1.z, 0.0f);
            out.triangles[kTriStride * i + 2] = make_float4(t.p2.x, t.p2.y, t.p2.z, 0.0f);
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
                    f.maxLeafTriangles = std::max(f.maxLeafTriangles, nd.triangleCount);
                    const float dx = nd.aabb.max.x - nd.aabb.min.x, dy = nd.aabb.max.y - nd.aabb.min.y, dz = nd.aabb.max.z - nd.aabb.min.z;
                    diag.push_back(std::sqrt(dx * dx + dy * dy + dz * dz));
                }
            const Aabb& root = sceneView.bvhNodes[0].aabb;
            const float extent = std::max({root.max.x - root.min.x, root.max.y - root.min.y, root.max.z - root.min.z});
            f.occluderHintLevels = 0;
            if (!diag.empty() && extent > 0.0f)
            {
                std::nth_element(diag.begin(), diag.begin() + diag.size() / 2, diag.end());
                const float median = diag[diag.size() / 2];
                if (median > 0.0f && std::isfinite(median) && std::isfinite(extent))
                    f.occluderHintLevels = static_cast<uint32_t>(std::clamp(static_cast<int>(std::floor(std::log2(0.003f * extent / median))) + 1, 0, 3));
            }
            if (const char* v = std::getenv("RF_OCCLUDER_HINT_LEVELS")) f.occluderHintLevels = static_cast<uint32_t>(std::clamp(std::atoi(v), 0, 8)); // experiments
        }
        f.leafBoxesValid = leafBoxesIntoTriangles(sceneView.bvhNodes.data(), sceneView.bvhNodes.size(), out.triangles.data(), n, f.occluderHintLevels, &wb.quadIndexOfNode);
        if (!f.leafBoxesValid)
        {
            // leaves that share a first triangle (hand-made tree): one slot cannot hold two exact boxes, so the layouts that cull a leaf by
            // the box in that slot stay off and the exact records (which carry every box themselves) are used
            out.wide.quadHalf.clear(), out.wide.quadLocal.clear(), out.wide.oct.clear();
            f.quadHalfFromBounce = f.quadHalfShadowFromBounce = f.quadLocalFromBounce = f.quadLocalShadowFromBounce = f.octFromBounce = 0u;
        }
    }
    {
        // 80-B VertexAttributes (three padded normals, three uvs, texture index, pad) -> 64 B = one L2 sector per shaded hit
        const size_t         n = sceneView.vertexAttributes.size();
        std::vector<float4>& packed = out.attributes;
        packed.resize(4 * n);
        for (size_t i = 0; i < n; ++i)
        {
            const VertexAttributes& v = sceneView.vertexAttributes[i];
            packed[4 * i] = make_float4(v.n0.x, v.n0.y, v.n0.z, v.n1.x);
            packed[4 * i + 1] = make_float4(v.n1.y, v.n1.z, v.n2.x, v.n2.y);
            packed[4 * i + 2] = make_float4(v.n2.z, v.uv0.x, v.uv0.y, v.uv1.x);
            packed[4 * i + 3] = make_float4(v.uv1.y, v.uv2.x, v.uv2.y, bitsFloat(v.textureIdx));
        }
        // kShade's record: positions + these four float4, 128 B per triangle
        std::vector<float4>& rec = out.shadeRecords;
        rec.assign(8 * n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
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
        f.selfShadowOk = wb.boxesNested && wb.boxesRegular;
        if (f.selfShadowOk)
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
    }

    // texture blob + descriptors in the order of the model's textures (reference_path_tracer.cpp:210-270)
    {
        std::vector<TextureDescriptor>& descs = out.textureDescriptors;
        std::vector<uint32_t>&          blob = out.texels;
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
    }
    out.albedoLut.resize(256);
    for (int i = 0; i < 256; ++i)
        out.albedoLut[i] = static_cast<float>(std::pow(static_cast<double>(static_cast<float>(i) / 255.0f), static_cast<double>(2.2f)));
    return out;
}
} // namespace rf
