// rf_scene_pack.hpp -- host only: a SceneView -> the host arrays the renderer uploads, and the facts about the scene that its launch policy takes as given.
// No HIP runtime call: the renderer's constructor uploads what packScene returns, a test or a sanitizer driver can look at it without a device.
#pragma once

#include "rf_bvh.hpp"
#include "rf_wide_build.hpp"

#include <vector>

namespace rf
{
// What the launch policy (rf_launch_policy.cpp: planBatch, planBounce, resolveTraversal) and the checkpoint's scene guard are told about the scene
struct SceneFacts
{
    uint64_t sceneCounts[4] = {};     // BVH nodes, triangles, textures, texels
    uint32_t sceneRootBounds[6] = {}; // the root node's box, as bit patterns
    uint32_t sortScale = 0;           // kShade<SORTED>: bin of triangle t = (t * sortScale) >> 32
    bool     wideUsable = true;       // every box finite and ordered; false: only the reference-ordered scalar kernels are exact
    bool     leafBoxesValid = false;  // every leaf's exact box sits in its first triangle record (leafBoxesIntoTriangles)
    bool     selfShadowOk = false;    // the tree's boxes are nested and regular, and the shading records carry their triangles' leaf boxes
    uint32_t maxLeafTriangles = 0;
    uint32_t occluderHintLevels = 0;  // see leafBoxesIntoTriangles (0: the occluder cache remembers leaves)
    uint64_t treeBytes = 0;           // local-grid quad records + triangle records: what the traversal launches touch
    float    quadHalfAreaRatio = 0.0f;
    // the layouts the scene gets with no option set: launches of bounce >= this read those records (0: never)
    uint32_t quadHalfFromBounce = 0, quadHalfShadowFromBounce = 0, quadLocalFromBounce = 0, quadLocalShadowFromBounce = 0, octFromBounce = 0;
};

struct PackedScene
{
    std::vector<float4>            nodes;        // 2 per node: the 32-byte device nodes
    WideBuild                      wide;         // quadHalf / quadLocal / oct are empty when !facts.leafBoxesValid
    std::vector<float4>            triangles;    // kTriStride per triangle, with the leaf boxes and occluder-cache entries
    std::vector<float4>            attributes;   // 4 per triangle
    std::vector<float4>            shadeRecords; // 8 per triangle, with the own-leaf boxes where facts.selfShadowOk
    std::vector<TextureDescriptor> textureDescriptors;
    std::vector<uint32_t>          texels;
    std::vector<float>             albedoLut;    // 256 entries: pow(i / 255, 2.2)
    SceneFacts                     facts;
};

// The scene must have passed validateScene (child links and leaf ranges are followed blindly).  Reads RF_OCCLUDER_HINT_LEVELS (experiments).  Throws
// std::runtime_error for a leaf of 2^30 triangles or more, an interior node with a split axis above 2, or more than 2^32 - 1 texels.
PackedScene packScene(const SceneView& sceneView);
} // namespace rf
