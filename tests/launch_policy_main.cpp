// launch_policy_main.cpp -- the launch policy (rayfinder_amd/csrc/rf_launch_policy.cpp) on a scene read from a file, without a device: packScene, the PolicyInputs a
// fresh handle would assemble from the packed scene, then per case the options and switches as rf_renderer_set_option / set_counting / set_aovs / set_moments would
// leave them, and one JSON row per (sample count, bounce) under rf_launch_plan's field names -- what rf_renderer_launch_plan answers on a device.
// tests/test_launch_policy.py compares the rows with tests/golden/launch_plan_parent.json.  Scene file: tests/scene_file.hpp.
//
// Usage: launch_policy_main scene-file case [-- case ...]          a case is a run of words:
//   case=LABEL  state=cold|warm  width=W height=H bounces=B  samples=N[,N...]  camera=<the 76 bytes of a Camera, hex>  counting  aovs  moments
//   and any other name=value: an option, in the order given.  An unknown option: the row {"case": LABEL, "unknown_option": name} and nothing else for that case.
// state=warm: the handle has traced one batch since it was created -- its occluder grid, if the batch plan has one, is allocated and filled, no first look ran in that
// batch, so none is reported and no hold-off runs (rf_renderer.hip: traceBatch / nextBatchFirstLookReady); cold: nothing traced, no grid yet.
#include "rf_bvh.hpp"
#include "rf_launch_policy.hpp"
#include "rf_renderer.hpp" // TileGrid
#include "rf_scene_pack.hpp"

#include "scene_file.hpp"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <numeric>
#include <sstream>

namespace
{
// rf_launch_plan, word by word
const char* const kFields[] = {
    "num_samples", "num_bounces", "sample_perm", "dense_raygen", "const_origin", "primary_layout", "occluder_grid", "occluder_scale_bits", "occluder_mask", "runs",
    "tile_list", "accumulate_kernel", "accumulate_pixels", "aov_pixels", "moment_pixels", "raygen_count_word",
    "closest_kernel", "closest_layout", "closest_counting", "closest_nearest", "closest_dense", "closest_refill_min", "closest_chunk", "closest_leaf_vote", "closest_flags",
    "closest_extra_lds", "closest_count_word", "closest_cursor_word",
    "shade_sorted", "shade_aov", "shade_flags", "shade_sort_scale", "shade_grid_cap",
    "shadow_kernel", "shadow_layout", "shadow_counting", "shadow_nearest", "shadow_dense", "shadow_refill_min", "shadow_chunk", "shadow_leaf_vote", "shadow_flags",
    "shadow_extra_lds", "shadow_count_word", "shadow_cursor_word", "shadow_cached", "shadow_first_look", "shadow_self", "shadow_source", "look_flags", "look_count_word",
    "look_list_word"};
constexpr size_t kNumFields = sizeof kFields / sizeof kFields[0];

rf::PolicyInputs inputsOf(const rf::PackedScene& p)
{
    rf::PolicyInputs     in;
    const rf::WideBuild& w = p.wide;
    in.facts = p.facts;
    // (what the renderer's constructor uploads: the compact and hot records in RF_EXP_LEGACY_LAYOUTS builds only)
    const auto have = [&](int layout, bool present) { in.layouts |= present ? 1u << layout : 0u; };
    have(rf::kLayoutBinary, !w.nodes.empty()), have(rf::kLayoutQuad, !w.quad.empty()), have(rf::kLayoutQuadHalf, !w.quadHalf.empty());
    have(rf::kLayoutQuadLocal, !w.quadLocal.empty()), have(rf::kLayoutOct, !w.oct.empty());
#if defined(RF_EXP_LEGACY_LAYOUTS)
    have(rf::kLayoutCompact, !w.compact.empty()), have(rf::kLayoutHot, !w.hot.empty());
#endif
    in.rootLo = w.rootLo, in.rootHi = w.rootHi, in.originBound = w.originBound;
    return in;
}

void runCase(const rf::PackedScene& packed, char** first, char** last)
{
    rf::LaunchOptions options;
    options.applySceneDefaults(packed.facts);
    options.applyEnvironment(packed.facts.wideUsable);
    rf::PolicyInputs      in = inputsOf(packed);
    std::string           label, state = "cold";
    uint32_t              width = 0, height = 0;
    std::vector<uint32_t> samples;
    for (char** a = first; a != last; ++a)
    {
        const std::string word = *a;
        const size_t      eq = word.find('=');
        const std::string name = word.substr(0, eq), value = eq == std::string::npos ? "" : word.substr(eq + 1);
        if (word == "counting") options.counting = true;
        else if (word == "aovs") in.aovs = true;
        else if (word == "moments") in.moments = true;
        else if (eq == std::string::npos) throw std::runtime_error("not a switch and not name=value: " + word);
        else if (name == "case") label = value;
        else if (name == "state") state = value;
        else if (name == "width") width = static_cast<uint32_t>(std::stoul(value));
        else if (name == "height") height = static_cast<uint32_t>(std::stoul(value));
        else if (name == "bounces") in.numBounces = static_cast<uint32_t>(std::stoul(value));
        else if (name == "samples")
        {
            std::stringstream list(value);
            for (std::string n; std::getline(list, n, ',');) samples.push_back(static_cast<uint32_t>(std::stoul(n)));
        }
        else if (name == "camera")
        {
            if (value.size() != 2 * sizeof(rf::Camera)) throw std::runtime_error("camera: 76 bytes as 152 hex digits");
            auto* bytes = reinterpret_cast<unsigned char*>(&in.camera);
            for (size_t i = 0; i < sizeof(rf::Camera); ++i) bytes[i] = static_cast<unsigned char>(std::stoul(value.substr(2 * i, 2), nullptr, 16));
        }
        else if (!options.set(name, std::stoll(value), packed.facts.wideUsable))
        {
            std::printf("{\"case\": \"%s\", \"unknown_option\": \"%s\"}\n", label.c_str(), name.c_str());
            return;
        }
    }
    if (state != "cold" && state != "warm") throw std::runtime_error("state: cold or warm");
    // one shard: every tile of the frame, in order
    const rf::TileGrid    grid(width, height);
    std::vector<uint32_t> tiles(grid.count());
    std::iota(tiles.begin(), tiles.end(), 0u);
    in.numTiles = grid.count(), in.validPixels = grid.validPrefix(tiles).total;
    for (const uint32_t n : samples)
    {
        rf::BatchPlan batch = rf::planBatch(options, in, n);
        batch.firstLookReady = state == "warm" && batch.occluderGrid;
        for (uint32_t bounce = 1; bounce <= in.numBounces; ++bounce)
        {
            rf_launch_plan plan;
            rf::writeLaunchPlan(batch, rf::planBounce(options, in, bounce, batch), bounce, plan);
            uint32_t words[kNumFields];
            static_assert(sizeof plan == sizeof words); // (every field is one uint32_t: include/rayfinder_amd.h)
            std::memcpy(words, &plan, sizeof plan);
            std::printf("{\"case\": \"%s\", \"state\": \"%s\", \"bounce\": %u, \"plan\": {", label.c_str(), state.c_str(), bounce);
            for (size_t i = 0; i < kNumFields; ++i) std::printf("%s\"%s\": %u", i ? ", " : "", kFields[i], words[i]);
            std::puts("}}");
        }
    }
}
} // namespace

int main(int argc, char** argv)
{
    try
    {
        if (argc < 3) throw std::runtime_error("usage: launch_policy_main scene-file case [-- case ...]");
        const SceneFile     scene = readScene(argv[1]);
        const rf::SceneView view = scene.view();
        if (view.bvhNodes.empty()) throw std::runtime_error("scene has no BVH nodes");
        rf::validateScene(view.bvhNodes, view.positionAttributes.size(), view.vertexAttributes, view.baseColorTextures.size());
        const rf::PackedScene packed = rf::packScene(view);
        for (char **first = argv + 2, **end = argv + argc; first < end;)
        {
            char** last = first;
            while (last != end && std::strcmp(*last, "--") != 0) ++last;
            runCase(packed, first, last);
            first = last == end ? end : last + 1;
        }
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "launch_policy_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
