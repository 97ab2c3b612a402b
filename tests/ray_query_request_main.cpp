// A stand-alone program over rf_ray_query_request.hpp (host only, no HIP): every refusal rf_renderer_cast_rays makes without a device, the byte ranges near 2^64, the
// overlap test and the chunk plans for N around multiples of C.  tests/test_cast_rays_api.py compiles it with -fsanitize=address,undefined and runs it as a plain
// executable: exit 0, "0 failures", no sanitizer report.
#include "rf_ray_query_request.hpp"

#include <cstdio>
#include <limits>
#include <vector>

using namespace rf;

static int checks = 0, failures = 0;
#define EXPECT(cond)                                                             \
    do                                                                           \
    {                                                                            \
        ++checks;                                                                \
        if (!(cond)) ++failures, std::printf("line %d: %s\n", __LINE__, #cond);  \
    } while (0)

template<typename F>
static bool refused(F&& f, const char* word = nullptr)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument& e)
    {
        return word == nullptr || std::string(e.what()).find(word) != std::string::npos;
    }
    return false;
}

static RayQueryRequest closest(uint64_t n = 100)
{
    RayQueryRequest q;
    q.origins = 0x10000, q.directions = 0x20000, q.numRays = n, q.tMax = 10000.0f;
    q.outputs[0] = 0x100000, q.outputs[1] = 0x200000;
    return q;
}

int main()
{
    constexpr uint64_t kMax = ~uint64_t{0};
    // ---- the request's own refusals
    EXPECT(!refused([] { checkRayQueryRequest(closest()); }));
    {
        RayQueryRequest q = closest();
        q.origins = 0;
        EXPECT(refused([&] { checkRayQueryRequest(q); }, "origins"));
        q = closest(), q.directions = 0;
        EXPECT(refused([&] { checkRayQueryRequest(q); }, "directions"));
        for (uint32_t stride : {0u, 1u, 2u})
        {
            q = closest(), q.originStride = stride;
            EXPECT(refused([&] { checkRayQueryRequest(q); }, "stride"));
            q = closest(), q.directionStride = stride;
            EXPECT(refused([&] { checkRayQueryRequest(q); }, "stride"));
        }
        q = closest(), q.originStride = 3, q.directionStride = 0xFFFFFFFFu;
        EXPECT(!refused([&] { checkRayQueryRequest(q); }));
        for (uint32_t kind : {2u, 3u, 0x80000000u, 0xFFFFFFFFu})
        {
            q = closest(), q.kind = kind;
            EXPECT(refused([&] { checkRayQueryRequest(q); }, "kind"));
        }
        q = closest(), q.reserved[0] = 1;
        EXPECT(refused([&] { checkRayQueryRequest(q); }, "reserved"));
        q = closest(), q.reserved[1] = 0x80000000u;
        EXPECT(refused([&] { checkRayQueryRequest(q); }, "reserved"));
        q = closest(), q.outputs[0] = q.outputs[1] = 0;
        EXPECT(refused([&] { checkRayQueryRequest(q); }, "no output"));
        // every closest-hit output with RF_RAYS_ANY, visibility with RF_RAYS_CLOSEST
        for (uint32_t i = 0; i < kCastOutputs; ++i)
        {
            RayQueryRequest a;
            a.origins = 0x10000, a.directions = 0x20000, a.numRays = 4, a.tMax = 1.0f, a.kind = kRaysAny;
            a.outputs[9] = 0x300000, a.outputs[i] = 0x400000;
            EXPECT(refused([&] { checkRayQueryRequest(a); }, "RF_RAYS_ANY") == (i != 9));
            RayQueryRequest c = closest();
            c.outputs[i] = 0x400000;
            EXPECT(refused([&] { checkRayQueryRequest(c); }, "visibility") == (i == 9));
        }
        q = closest(), q.tMax = std::numeric_limits<float>::quiet_NaN();
        EXPECT(refused([&] { checkRayQueryRequest(q); }, "NaN"));
        for (float t : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 0.0f, -1.0f, std::numeric_limits<float>::max()})
        {
            q = closest(), q.tMax = t;
            EXPECT(!refused([&] { checkRayQueryRequest(q); }));
        }
        EXPECT(closest().mask() == (kCastTriangle | kCastT));
    }
    // ---- byte ranges, also near 2^64
    {
        ByteRange r = checkedRange(1000, 10, 3, "x");
        EXPECT(r.begin == 1000 && r.end == 1120);
        r = checkedRange(kMax - 120, 10, 3, "x");
        EXPECT(r.end == kMax);
        EXPECT(refused([&] { checkedRange(kMax - 119, 10, 3, "x"); }, "address space"));
        EXPECT(refused([&] { checkedRange(0, kMax / 12 + 1, 3, "x"); }, "overflows"));
        EXPECT(!refused([&] { checkedRange(0, kMax / 12, 3, "x"); }));
        EXPECT(refused([&] { checkedRange(16, kMax / 12, 3, "x"); }, "address space"));
        EXPECT(refused([&] { checkedRange(0, uint64_t{1} << 62, 1, "x"); }, "overflows"));
        EXPECT(refused([&] { checkedRange(0, kMax, 0xFFFFFFFFull, "x"); }, "overflows"));
        // a strided input ends behind its last ray's third float
        r = inputRange(4096, 10, 6, "origins");
        EXPECT(r.begin == 4096 && r.end == 4096 + 9 * 24 + 12);
        r = inputRange(4096, 1, 0xFFFFFFFFu, "origins");
        EXPECT(r.end == 4096 + 12);
        r = inputRange(4096, 0, 3, "origins");
        EXPECT(r.empty());
        EXPECT(refused([&] { inputRange(0, kMax, 3, "origins"); }, "overflows"));
        EXPECT(refused([&] { inputRange(kMax - 100, 10, 3, "origins"); }, "address space"));
        RayQueryRequest q = closest(uint64_t{1} << 61);
        EXPECT(refused([&] { checkRayQueryOverlaps(q); }));
        q = closest(10), q.outputs[3] = kMax - 100;
        EXPECT(refused([&] { checkRayQueryOverlaps(q); }, "position"));
    }
    // ---- overlaps
    {
        EXPECT(!rangesOverlap({0, 10}, {10, 20}) && !rangesOverlap({10, 20}, {0, 10}) && rangesOverlap({0, 11}, {10, 20}) && rangesOverlap({10, 20}, {0, 11}));
        EXPECT(rangesOverlap({0, 100}, {40, 41}) && !rangesOverlap({5, 5}, {0, 10}) && !rangesOverlap({0, 10}, {5, 5}));
        EXPECT(!refused([] { checkRayQueryOverlaps(closest()); }));
        // the two halves of an (N, 6) tensor: the inputs interleave, which is fine -- they are only read
        RayQueryRequest q = closest();
        q.directions = q.origins + 12, q.originStride = q.directionStride = 6;
        EXPECT(!refused([&] { checkRayQueryOverlaps(q); }));
        q.directions = q.origins;
        EXPECT(!refused([&] { checkRayQueryOverlaps(q); }));
        // output against output: t starts inside triangle's 400 bytes / right behind them
        q = closest(), q.outputs[1] = q.outputs[0] + 396;
        EXPECT(refused([&] { checkRayQueryOverlaps(q); }, "triangle overlaps t"));
        q.outputs[1] = q.outputs[0] + 400;
        EXPECT(!refused([&] { checkRayQueryOverlaps(q); }));
        q = closest(), q.outputs[7] = q.outputs[0];
        EXPECT(refused([&] { checkRayQueryOverlaps(q); }, "triangle overlaps albedo"));
        // output against input: the last float of the origins, the first of the directions
        q = closest(), q.outputs[3] = q.origins + 99 * 12 + 8;
        EXPECT(refused([&] { checkRayQueryOverlaps(q); }, "position overlaps origins"));
        q.outputs[3] = q.origins + 100 * 12;
        EXPECT(!refused([&] { checkRayQueryOverlaps(q); }));
        q = closest(), q.outputs[1] = q.directions - 396;
        EXPECT(refused([&] { checkRayQueryOverlaps(q); }, "t overlaps directions"));
        q.outputs[1] = q.directions - 400;
        EXPECT(!refused([&] { checkRayQueryOverlaps(q); }));
        // an output in the padding of a strided input still lies inside its range
        q = closest(), q.originStride = 8, q.outputs[1] = q.origins + 12;
        EXPECT(refused([&] { checkRayQueryOverlaps(q); }, "t overlaps origins"));
        // every pair of outputs on one address
        for (uint32_t i = 0; i < 9; ++i)
            for (uint32_t j = i + 1; j < 9; ++j)
            {
                RayQueryRequest p;
                p.origins = 0x10000, p.directions = 0x20000, p.numRays = 7, p.outputs[i] = p.outputs[j] = 0x500000;
                EXPECT(refused([&] { checkRayQueryOverlaps(p); }, kCastOutputName[j]));
            }
    }
    // ---- chunk plans
    {
        for (uint64_t C : {uint64_t{1}, uint64_t{2}, uint64_t{1000}, uint64_t{4096}})
            for (uint64_t k : {uint64_t{0}, uint64_t{1}, uint64_t{2}, uint64_t{3}, uint64_t{7}})
                for (int d = -1; d <= 1; ++d)
                {
                    if (k * C + static_cast<uint64_t>(d + 1) == 0) continue;
                    const uint64_t  N = k * C + static_cast<uint64_t>(d + 1) - 1;
                    const ChunkPlan p = planChunks(N, 1u << 20, 1u << 24, C);
                    EXPECT(p.chunk == C && p.count() == (N + C - 1) / C);
                    uint64_t covered = 0;
                    bool     ok = true;
                    for (uint64_t c = 0; c < p.count(); ++c)
                    {
                        ok = ok && p.first(c) == covered && p.size(c) >= 1 && p.size(c) <= C && (c + 1 == p.count() || p.size(c) == C);
                        covered += p.size(c);
                    }
                    EXPECT(ok && covered == N && p.size(p.count()) == 0 && p.depth() == (N < C ? N : C));
                }
        EXPECT(planChunks(10, 0, 100, 0).chunk == 1 && planChunks(10, 100, 0, 0).chunk == 1 && planChunks(10, 0, 0, 5).chunk == 1); // never 0
        EXPECT(planChunks(10, 100, 50, 0).chunk == 50 && planChunks(10, 50, 100, 0).chunk == 50 && planChunks(10, 100, 50, 70).chunk == 50 && planChunks(10, 100, 50, 7).chunk == 7);
        EXPECT(planChunks(kMax / 16, kMax, kMax, 0).chunk == 0xFFFFFFFFull); // queue positions are 32-bit
        const ChunkPlan big = planChunks(uint64_t{1} << 40, kMax, kMax, 0);
        EXPECT(big.count() == ((uint64_t{1} << 40) + 0xFFFFFFFEull) / 0xFFFFFFFFull && big.size(big.count() - 1) == (uint64_t{1} << 40) - big.first(big.count() - 1));
        EXPECT(planChunks(0, 100, 100, 0).count() == 0 && planChunks(0, 100, 100, 0).depth() == 0);
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
