// scene_pack_main.cpp -- packScene + checkWideLayouts on scenes read from files, without a device: one JSON line per scene with a 64-bit FNV-1a hash of the
// bytes of every packed array, every derived fact and layout default, and the flags of checkWideLayouts.  tests/test_scene_pack.py compares the lines with
// tests/golden/scene_pack_parent.json, recorded from the renderer's constructor before the packing left it (profiles/scene_pack/record_parent.hip includes this
// file with its own copy of that code behind the same names).
//
// Scene file: tests/scene_file.hpp.
// Usage: scene_pack_main [--time N] file...      (--time N: also N timed runs of packScene alone per scene, "pack_ms" in the line)
#if !defined(SCENE_PACK_PARENT_RECORDER)
#include "rf_bvh.hpp"
#include "rf_scene_pack.hpp"
#include "rf_wide_build.hpp"
#endif

#include "scene_file.hpp"

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace
{
uint64_t fnv(const void* data, size_t bytes, uint64_t h = 0xcbf29ce484222325ull)
{
    const auto* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

struct Line
{
    std::string text = "{";
    void raw(const char* key, const std::string& value) { text += (text.size() > 1 ? ", \"" : "\"") + std::string(key) + "\": " + value; }
    void num(const char* key, uint64_t v) { raw(key, std::to_string(v)); }
    void flag(const char* key, bool v) { raw(key, v ? "true" : "false"); }
    void str(const char* key, const std::string& v)
    {
        std::string q = "\"";
        for (const char c : v) q += (c == '"' || c == '\\') ? std::string("\\") + c : std::string(1, c);
        raw(key, q + "\"");
    }
    void hex(const char* key, uint64_t v)
    {
        char buf[24];
        std::snprintf(buf, sizeof buf, "\"%016llx\"", static_cast<unsigned long long>(v));
        raw(key, buf);
    }
    void bits(const char* key, float v) // a float as its bit pattern: equality means the same bits, NaNs included
    {
        uint32_t u;
        std::memcpy(&u, &v, sizeof u);
        char buf[16];
        std::snprintf(buf, sizeof buf, "\"%08x\"", u);
        raw(key, buf);
    }
    template<typename T>
    void array(const std::string& key, const std::vector<T>& v) // {element count, hash of the bytes}
    {
        char buf[48];
        std::snprintf(buf, sizeof buf, "[%zu, \"%016llx\"]", v.size(), static_cast<unsigned long long>(fnv(v.data(), v.size() * sizeof(T))));
        raw(key.c_str(), buf);
    }
};

std::string describe(const std::string& name, const SceneFile& scene, int timedRuns)
{
    Line line;
    line.str("scene", name);
    try
    {
        const rf::SceneView view = scene.view();
        if (view.bvhNodes.empty()) throw std::runtime_error("scene has no BVH nodes");
        rf::validateScene(view.bvhNodes, view.positionAttributes.size(), view.vertexAttributes, view.baseColorTextures.size());
        const rf::PackedScene p = rf::packScene(view);
        const rf::WideBuild&  w = p.wide;
        line.array("nodes", p.nodes);
        line.array("wide.nodes", w.nodes), line.array("wide.compact", w.compact), line.array("wide.hot", w.hot), line.array("wide.own", w.own);
        line.array("wide.quad", w.quad), line.array("wide.quadHalf", w.quadHalf), line.array("wide.quadLocal", w.quadLocal), line.array("wide.oct", w.oct);
        line.array("wide.bigLeaves", w.bigLeaves), line.array("wide.quadIndexOfNode", w.quadIndexOfNode), line.array("wide.octIndexOfNode", w.octIndexOfNode);
        line.flag("wide.compactUsable", w.compactUsable), line.flag("wide.hotUsable", w.hotUsable), line.flag("wide.quadUsable", w.quadUsable);
        line.flag("wide.boxesRegular", w.boxesRegular), line.flag("wide.boxesNested", w.boxesNested);
        line.bits("wide.originBound", w.originBound), line.bits("wide.quadHalfAreaRatio", w.quadHalfAreaRatio);
        line.bits("wide.quadLocalAreaRatio", w.quadLocalAreaRatio), line.bits("wide.octAreaRatio", w.octAreaRatio);
        line.hex("wide.rootBox", fnv(&w.rootHi, sizeof w.rootHi, fnv(&w.rootLo, sizeof w.rootLo)));
        line.num("wide.rootLeaf", w.rootLeaf);
        line.num("wide.bigLeaves.first.count", w.bigLeaves.empty() ? 0u : w.bigLeaves.front().y); // (0: the table holds its placeholder alone)
        line.array("triangles", p.triangles), line.array("attributes", p.attributes), line.array("shadeRecords", p.shadeRecords);
        line.array("textureDescriptors", p.textureDescriptors), line.array("texels", p.texels), line.array("albedoLut", p.albedoLut);
        line.num("textureDescriptors.last.offset", p.textureDescriptors.back().offset);
        const rf::SceneFacts& f = p.facts;
        line.hex("facts.sceneCounts", fnv(f.sceneCounts, sizeof f.sceneCounts)), line.hex("facts.sceneRootBounds", fnv(f.sceneRootBounds, sizeof f.sceneRootBounds));
        line.num("facts.sortScale", f.sortScale);
        line.flag("facts.wideUsable", f.wideUsable), line.flag("facts.leafBoxesValid", f.leafBoxesValid), line.flag("facts.selfShadowOk", f.selfShadowOk);
        line.num("facts.maxLeafTriangles", f.maxLeafTriangles), line.num("facts.occluderHintLevels", f.occluderHintLevels), line.num("facts.treeBytes", f.treeBytes);
        line.bits("facts.quadHalfAreaRatio", f.quadHalfAreaRatio);
        line.num("facts.quadHalfFromBounce", f.quadHalfFromBounce), line.num("facts.quadHalfShadowFromBounce", f.quadHalfShadowFromBounce);
        line.num("facts.quadLocalFromBounce", f.quadLocalFromBounce), line.num("facts.quadLocalShadowFromBounce", f.quadLocalShadowFromBounce);
        line.num("facts.octFromBounce", f.octFromBounce);
        try
        {
            float ratio = -1.0f;
            line.num("check.flags", rf::checkWideLayouts(view.bvhNodes, &ratio));
            line.bits("check.quadHalfAreaRatio", ratio);
        }
        catch (const std::exception& e)
        {
            line.str("check.error", e.what());
        }
        if (timedRuns > 0)
        {
            std::string ms = "[";
            for (int r = 0; r < timedRuns; ++r)
            {
                const auto            t0 = std::chrono::steady_clock::now();
                const rf::PackedScene again = rf::packScene(view);
                const auto            t1 = std::chrono::steady_clock::now();
                if (again.nodes.size() != p.nodes.size()) throw std::runtime_error("packScene is not repeatable");
                ms += (r ? ", " : "") + std::to_string(std::chrono::duration<double, std::milli>(t1 - t0).count());
            }
            line.raw("pack_ms", ms + "]");
        }
    }
    catch (const std::exception& e)
    {
        line.str("error", e.what());
    }
    return line.text + "}";
}
} // namespace

int main(int argc, char** argv)
{
    int timedRuns = 0, first = 1;
    if (argc > 2 && std::strcmp(argv[1], "--time") == 0) timedRuns = std::atoi(argv[2]), first = 3;
    for (int i = first; i < argc; ++i)
    {
        std::string name = argv[i];
        name = name.substr(name.find_last_of('/') + 1);
        name = name.substr(0, name.find_last_of('.'));
        try
        {
            std::puts(describe(name, readScene(argv[i]), timedRuns).c_str());
        }
        catch (const std::exception& e)
        {
            std::fprintf(stderr, "%s: %s\n", argv[i], e.what());
            return 1;
        }
    }
    return 0;
}
