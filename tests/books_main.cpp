// books_main.cpp -- the accumulation's books (rayfinder_amd/csrc/rf_books.cpp) through a script of calls, without a device: every call is played on one
// AccumulationBooks as rf_renderer.hip plays it on a handle's -- the refusal, then the transitions, in the renderer's order -- and answered with one JSON line:
//   {"call": "...", "outcome": "accepted" | "invalid_argument" | "logic_error" | "runtime_error", "message": "...", "accumulated": L, "frame_count": n,
//    "tile_counts": [one per slot of the shard], "families": {"image" | "aovs" | "moments" | "direct" | "buckets": {"on", "samples", "covers"}},
//    "denoised": {"valid", "samples"}, "robust": {"valid", "samples"}}
// tests/test_books.py walks it against tests/handle_model.py and compares its messages with tests/golden/refusals_parent.json.
//
// Usage: books_main tiles=T spp=N call [-- call ...]     or     books_main @file (the same words, one per line or blank-separated)
// A call is a run of words, the name first; the walk's call kinds (tests/handle_walk.py) take the walk's own arguments:
//   render N | render_until TARGET EVERY MAX_FRAMES frames=F | render_adaptive TARGET EVERY MIN MAX counts=c0,c1,... | set_moments 0|1 | set_aovs WORD |
//   set_buckets WORD | set_exposure X | set_tile_shard RANK WORLD tiles=T | bind | unbind | noise_estimate | denoise [ITERATIONS] | robust_mean | denoise_robust [ITERATIONS]
// and beside them: set_direct WORD | denoise_split | export_features READS TWO_SAMPLES | read_denoised | read_robust_mean | check_adaptive TARGET EVERY SHARDED
// What depends on pixel values the books do not have rides on the line: frames= is how many frames render_until rendered, counts= the per-slot counts render_adaptive
// left (a tile leaves the active list at the check where it reaches its count); tiles= is the shard's tile count (the tile deal is the renderer's).
// The three set calls whose words the C ABI checks in front of the handle (rf_c_api.cpp) get that check here too: the recording holds what the ABI says.
#include "rf_books.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <stdexcept>

namespace
{
using Books = rf::AccumulationBooks;
using Words = std::vector<std::string>;

// a mistake of the script, not an answer of the books: ends the run
struct ScriptError
{
    std::string what;
};
uint32_t u32(const std::string& s)
{
    char*                    end = nullptr;
    const unsigned long long v = std::strtoull(s.c_str(), &end, 0);
    if (s.empty() || *end != '\0' || v > 0xFFFFFFFFull) throw ScriptError{"not a 32-bit number: " + s};
    return static_cast<uint32_t>(v);
}
float f32(const std::string& s)
{
    char*       end = nullptr;
    const float v = std::strtof(s.c_str(), &end);
    if (s.empty() || *end != '\0') throw ScriptError{"not a number: " + s};
    return v;
}
// name=value among a call's words
std::string named(const Words& w, const std::string& name)
{
    for (const std::string& s : w)
        if (s.rfind(name + "=", 0) == 0) return s.substr(name.size() + 1);
    throw ScriptError{w[0] + ": " + name + "= is missing"};
}
std::vector<uint32_t> list(const std::string& s)
{
    std::vector<uint32_t> out;
    std::stringstream     in(s);
    for (std::string n; std::getline(in, n, ',');) out.push_back(u32(n));
    return out;
}

struct Handle
{
    Books    books;
    uint32_t spp = 0;
    float    exposure = 0.25f;

    // rf_c_api.cpp's checks of a word, in front of the handle
    static void abiRequire(bool cond, const char* what)
    {
        if (!cond) throw std::invalid_argument(what);
    }
    // Renderer::render
    void render(uint32_t numFrames)
    {
        books.refuseRender();
        uint32_t remaining = numFrames;
        while (const uint32_t todo = books.framesToTrace(remaining))
        {
            clearStale();
            books.recordStep(todo);
            remaining -= todo;
        }
    }
    // Renderer::clearStaleSums
    void clearStale()
    {
        for (uint32_t f = 0; f < Books::kFamilies; ++f)
            if (books.stale(static_cast<Books::Family>(f))) books.zeroed(static_cast<Books::Family>(f));
    }
    void robustMean()
    {
        books.refuseRobustMean();
        books.noteRobustMean();
    }
    // Renderer::renderAdaptiveFrom over the whole frame, the estimate's verdicts read from the counts the call left
    void renderAdaptive(uint32_t every, uint32_t minSamples, uint32_t maxSamples, const std::vector<uint32_t>& final)
    {
        books.requireSlotAddressing(false);
        const uint32_t        cap = maxSamples == 0u ? spp : std::min(maxSamples, spp), firstCheck = std::max(2u, minSamples);
        std::vector<uint32_t> counts = books.tileCounts(), active;
        if (final.size() != counts.size()) throw ScriptError{"render_adaptive: one final count per slot"};
        for (uint32_t k = 0; k < counts.size(); ++k)
            if (counts[k] == books.accumulated()) active.push_back(k);
        while (!active.empty() && books.accumulated() < cap)
        {
            clearStale();
            books.recordStep(std::min(every, cap - books.accumulated()));
            for (const uint32_t k : active) counts[k] = books.accumulated();
            books.setTileSamples(counts);
            if (books.accumulated() < firstCheck) continue;
            std::vector<uint32_t> still;
            for (const uint32_t k : active)
                if (final[k] > books.accumulated()) still.push_back(k);
            active.swap(still);
        }
        books.settleTileSamples(counts);
        if (counts != final) throw ScriptError{"render_adaptive: the loop cannot leave these counts"};
    }

    void play(const Words& w)
    {
        const std::string& name = w[0];
        const auto         arg = [&](size_t i) -> const std::string& {
            if (i >= w.size()) throw ScriptError{name + ": an argument is missing"};
            return w[i];
        };
        if (name == "render") render(u32(arg(1)));
        else if (name == "render_until")
        {
            const uint32_t every = u32(arg(2)), maxFrames = u32(arg(3));
            books.refuseRenderUntil(every);
            const uint32_t rendered = u32(named(w, "frames"));
            uint32_t       frames = 0;
            while (frames < rendered && frames < maxFrames && books.accumulated() < spp)
            {
                const uint32_t n = std::min({every, maxFrames - frames, spp - books.accumulated()});
                render(n);
                frames += n;
            }
            if (frames != rendered) throw ScriptError{"render_until: the loop cannot render this many frames"};
        }
        else if (name == "render_adaptive")
        {
            books.refuseRenderAdaptive(u32(arg(2)), f32(arg(1)));
            renderAdaptive(u32(arg(2)), u32(arg(3)), u32(arg(4)), list(named(w, "counts")));
        }
        else if (name == "check_adaptive") books.refuseAdaptive(u32(arg(2)), f32(arg(1)), u32(arg(3)) != 0u);
        else if (name == "set_moments") books.setMoments(u32(arg(1)) != 0u);
        else if (name == "set_aovs")
        {
            const uint32_t flags = u32(arg(1));
            abiRequire((flags & ~0x101u) == 0u, "unknown AOV flag bits");
            abiRequire((flags & 0x100u) == 0u || (flags & 1u) != 0u, "RF_AOV_TILE_COUNTS says how the AOVs are kept: valid only together with RF_AOV_FIRST_HIT");
            books.setAovs(flags);
        }
        else if (name == "set_direct")
        {
            const uint32_t word = u32(arg(1));
            abiRequire((word & ~0x101u) == 0u, "unknown direct flag bits: the word is 0, 1 or 1 | RF_DIRECT_TILE_COUNTS");
            abiRequire((word & 0x100u) == 0u || (word & 1u) != 0u, "RF_DIRECT_TILE_COUNTS says how the direct sums are kept: valid only together with 1");
            books.setDirect(word);
        }
        else if (name == "set_direct_unchecked") books.setDirect(u32(arg(1))); // (Renderer::setDirect itself, as C++ code calls it)
        else if (name == "set_buckets") books.setBuckets(u32(arg(1)));
        else if (name == "set_exposure")
        {
            // Renderer::setRenderParameters: a change of the parameters restarts the accumulation
            if (f32(arg(1)) != exposure) exposure = f32(arg(1)), books.restartAccumulation();
        }
        else if (name == "set_tile_shard")
        {
            const uint32_t rank = u32(arg(1)), world = u32(arg(2));
            abiRequire(world > 0 && rank < world, "invalid rank / world size");
            books.refuseSetTileShard(rank, world);
            books.setShard(rank, world);
            books.setShardTiles(u32(named(w, "tiles")));
            books.restartAccumulation();
        }
        else if (name == "set_tile_shard_unchecked") books.refuseSetTileShard(u32(arg(1)), u32(arg(2)));
        else if (name == "bind" || name == "unbind") books.restartAccumulation(); // Renderer::bindAccumulationBuffer
        else if (name == "noise_estimate") books.refuseNoiseEstimate();
        else if (name == "denoise") books.refuseDenoise(), books.noteDenoised();
        else if (name == "denoise_split") books.refuseDenoiseSplit(), books.noteDenoised();
        else if (name == "robust_mean") robustMean();
        else if (name == "denoise_robust") books.refuseDenoiseRobust(), robustMean(), books.noteDenoised();
        else if (name == "export_features") books.refuseExportFeatures(u32(arg(1)), u32(arg(2)) != 0u);
        else if (name == "read_denoised") books.refuseReadDenoised();
        else if (name == "read_robust_mean") books.refuseReadRobustMean();
        else throw ScriptError{"unknown call " + name};
    }

    void print(const Words& w, const char* outcome, const std::string& message) const
    {
        std::string call, text;
        for (const std::string& s : w) call += (call.empty() ? "" : " ") + s;
        for (const char c : message)
        {
            if (c == '"' || c == '\\') text += '\\';
            text += c;
        }
        std::printf("{\"call\": \"%s\", \"outcome\": \"%s\", \"message\": \"%s\", \"accumulated\": %u, \"frame_count\": %u, \"tile_counts\": [", call.c_str(), outcome, text.c_str(),
                    books.accumulated(), books.frameCount());
        const std::vector<uint32_t> counts = books.tileCounts();
        for (size_t k = 0; k < counts.size(); ++k) std::printf("%s%u", k ? ", " : "", counts[k]);
        std::printf("], \"families\": {");
        const char* const names[Books::kFamilies] = {"image", "aovs", "moments", "direct", "buckets"};
        for (uint32_t i = 0; i < Books::kFamilies; ++i)
        {
            const Books::Family f = static_cast<Books::Family>(i);
            std::printf("%s\"%s\": {\"on\": %s, \"samples\": %u, \"covers\": %s}", i ? ", " : "", names[i], books.on(f) ? "true" : "false", books.readCount(f),
                        books.covers(f) ? "true" : "false");
        }
        std::printf("}, \"denoised\": {\"valid\": %s, \"samples\": %u}, \"robust\": {\"valid\": %s, \"samples\": %u}}\n", books.denoisedValid() ? "true" : "false",
                    books.denoisedValid() ? books.denoisedSamples() : 0u, books.robustValid() ? "true" : "false", books.robustValid() ? books.robustSamples() : 0u);
    }
};
} // namespace

int main(int argc, char** argv)
{
    try
    {
        Words words(argv + 1, argv + argc);
        if (words.size() == 1 && words[0][0] == '@')
        {
            std::ifstream file(words[0].substr(1));
            if (!file) throw std::runtime_error("cannot read " + words[0].substr(1));
            words.assign(std::istream_iterator<std::string>(file), std::istream_iterator<std::string>());
        }
        if (words.size() < 3) throw std::runtime_error("usage: books_main tiles=T spp=N call [-- call ...] | books_main @file");
        Handle h;
        h.spp = u32(named(words, "spp"));
        h.books.setSampleCap(h.spp);
        h.books.setShardTiles(u32(named(words, "tiles")));
        h.books.restartAccumulation();
        for (size_t first = 2; first < words.size();)
        {
            size_t last = first;
            while (last != words.size() && words[last] != "--") ++last;
            const Words call(words.begin() + first, words.begin() + last);
            if (call.empty()) throw std::runtime_error("an empty call");
            try
            {
                h.play(call);
                h.print(call, "accepted", "");
            }
            // (the three types rf_c_api.cpp tells apart)
            catch (const std::invalid_argument& e) { h.print(call, "invalid_argument", e.what()); }
            catch (const std::logic_error& e) { h.print(call, "logic_error", e.what()); }
            catch (const std::runtime_error& e) { h.print(call, "runtime_error", e.what()); }
            first = last == words.size() ? last : last + 1;
        }
    }
    catch (const ScriptError& e)
    {
        std::fprintf(stderr, "books_main: %s\n", e.what.c_str());
        return 1;
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "books_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
