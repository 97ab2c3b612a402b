// rf_denoise.hip -- edge-aware a-trous wavelet denoiser (Dammertz et al. 2010) over the accumulation and the first-hit AOVs.  The arithmetic is the one
// include/rayfinder_amd.h writes out ("Edge-aware a-trous denoiser"), one IEEE f32 operation at a time in that order (-ffp-contract=off, correctly
// rounded divide and sqrt, no denormal flushing): tests/denoise_restatement.py reproduces it bit for bit.  No atomics: every output is one lane's
// fixed sequence of operations.
//   kDenoisePrep    one lane per pixel: demodulated irradiance {e, ℓ}, guide {n, z}, a + εa (or, for L = 0, the mean itself)
//   kDenoisePrepTiles  the same with the sample count of the pixel's 32x32 tile (a frame of rf_renderer_render_adaptive, rf_denoise_tiles)
//   kDenoisePrepMean   the same with the colour c taken from a row-major mean image (the robust mean, rf_renderer_denoise_robust) instead of S / Nf
//   kDenoisePrepMeanTiles  kDenoisePrepMean with the sample count of the pixel's tile (rf_renderer_denoise_robust in the non-uniform state)
//   kDenoiseAtrous  one lane per pixel, 16x16-pixel workgroups of four 8x8-pixel waves (the 25 taps of a wave touch few cache lines); the last pass
//                   remodulates and writes the mean
//   kDenoisePrepSplit    the split-component filter's prep (rf_renderer_denoise_split): two demodulated irradiances, of D and of S - D, over one guide and one a + εa
//   kDenoisePrepSplitTiles  the same with the sample count of the pixel's tile (rf_renderer_denoise_split in the non-uniform state, rf_denoise_split_tiles)
//   kDenoiseAtrousSplit  one pass of both components at once: one guide load per tap (and one evaluation of the normal and depth terms when the components share
//                   σn and σz), two colour terms, two accumulator sets; a component past its own iteration count is not filtered; the last pass adds the two,
//                   remodulates and writes the mean
// The display image is the existing kTonemap over the mean with accumulatedSamples = 1.
#include "rf_denoise.hpp"

#include "rf_kernels.hpp"
#include "rf_math.hpp"

namespace rf
{
namespace
{
constexpr float    kEpsAlbedo = 0.00390625f; // εa = 2^-8
constexpr float    kEpsLum = 0.00390625f;    // εℓ = 2^-8
constexpr uint32_t kDenoiseBlock = 256;      // kDenoiseAtrous: 16x16 pixels

// index of pixel (x, y) in a compact tile-major buffer that holds every tile of the frame in tile order (localPixelToXY's layout)
__device__ __forceinline__ uint32_t tileMajorIndex(uint32_t x, uint32_t y, uint32_t tilesX)
{
    const uint32_t tile = (y >> 5) * tilesX + (x >> 5);
    const uint32_t block = ((y & 31u) >> 3) * 4u + ((x & 31u) >> 3);
    return tile * 1024u + block * 64u + (y & 7u) * 8u + (x & 7u);
}

__device__ __forceinline__ float tukey(float x)
{
    const float m = 1.0f - x;
    return x < 1.0f ? m * m : 0.0f; // (NaN: 0)
}

// prep of pixel i = (x, y) with its sample count as a float: shared by kDenoisePrep (one count for the frame), kDenoisePrepTiles (the count of the pixel's tile) and
// kDenoisePrepMean (MEAN: colorSum is a row-major image of means and c = its rgb as it is; the AOV sums are divided by nf as ever)
template<bool MEAN = false>
__device__ __forceinline__ void prepPixel(const float4* colorSum, const float4* albedoCoverage, const float4* normalDepth, uint32_t i, uint32_t x, uint32_t y, uint32_t tilesX,
                                          float nf, float4* e, float4* guide, float4* albedo, float4* meanOut)
{
    const uint32_t src = tilesX ? tileMajorIndex(x, y, tilesX) : i;
    const float4   S = colorSum[MEAN ? i : src];
    const Vec3     c = MEAN ? vec3(S.x, S.y, S.z) : vec3(S.x / nf, S.y / nf, S.z / nf); // (kTonemap's division)
    if (meanOut) // L = 0: the mean, exactly
    {
        meanOut[i] = make_float4(c.x, c.y, c.z, 1.0f);
        return;
    }
    const float4 AC = albedoCoverage[src], ND = normalDepth[src];
    const float  z = ND.w / AC.w;
    if (AC.w == 0.0f || !(z > 0.0f)) // background: passes through, never a neighbour
    {
        e[i] = make_float4(c.x, c.y, c.z, 0.0f);
        guide[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        albedo[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const Vec3  a = vec3(AC.x / nf, AC.y / nf, AC.z / nf);
    const Vec3  m = vec3(ND.x / nf, ND.y / nf, ND.z / nf);
    const float d = dot(m, m);
    const Vec3  n = (d != 0.0f && fabsf(d) <= FLT_MAX) ? normalize(m) : splat(0.0f);
    const Vec3  ae = a + splat(kEpsAlbedo);
    const Vec3  ev = vec3(c.x / ae.x, c.y / ae.y, c.z / ae.z);
    e[i] = make_float4(ev.x, ev.y, ev.z, (ev.x + ev.y) + ev.z);
    guide[i] = make_float4(n.x, n.y, n.z, z);
    albedo[i] = make_float4(ae.x, ae.y, ae.z, 0.0f);
}

__global__ __launch_bounds__(256) void kDenoisePrep(const float4* colorSum, const float4* albedoCoverage, const float4* normalDepth, uint32_t width, uint32_t height,
                                                    uint32_t tilesX, float nf, float4* e, float4* guide, float4* albedo, float4* meanOut)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    prepPixel(colorSum, albedoCoverage, normalDepth, i, x, y, tilesX, nf, e, guide, albedo, meanOut);
}

// The same with one sample count per 32x32 tile of the frame: Nf = float(tileSamples[tile of the pixel]), tile = tile_y * frameTilesX + tile_x (the estimate's
// numbering).  frameTilesX is the frame's tiles per row whatever the layout of the sums (tilesX is 0 for row-major sums); every count is > 0.
__global__ __launch_bounds__(256) void kDenoisePrepTiles(const float4* colorSum, const float4* albedoCoverage, const float4* normalDepth, uint32_t width, uint32_t height,
                                                         uint32_t tilesX, const uint32_t* tileSamples, uint32_t frameTilesX, float4* e, float4* guide, float4* albedo,
                                                         float4* meanOut)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    const float    nf = static_cast<float>(tileSamples[(y >> 5) * frameTilesX + (x >> 5)]);
    prepPixel(colorSum, albedoCoverage, normalDepth, i, x, y, tilesX, nf, e, guide, albedo, meanOut);
}

// The same with the colour given: c = mean[i].rgb (row-major, the robust mean of rf_robust.hip) instead of S.rgb / Nf; a and m are AC.rgb / Nf and ND.xyz / Nf.
__global__ __launch_bounds__(256) void kDenoisePrepMean(const float4* mean, const float4* albedoCoverage, const float4* normalDepth, uint32_t width, uint32_t height,
                                                        uint32_t tilesX, float nf, float4* e, float4* guide, float4* albedo, float4* meanOut)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    prepPixel<true>(mean, albedoCoverage, normalDepth, i, x, y, tilesX, nf, e, guide, albedo, meanOut);
}

// kDenoisePrepMean with one sample count per 32x32 tile: c = mean[i].rgb as it is, a = AC.rgb / Nf and m = ND.xyz / Nf with Nf = float(tileSamples[tile of the pixel])
__global__ __launch_bounds__(256) void kDenoisePrepMeanTiles(const float4* mean, const float4* albedoCoverage, const float4* normalDepth, uint32_t width, uint32_t height,
                                                             uint32_t tilesX, const uint32_t* tileSamples, uint32_t frameTilesX, float4* e, float4* guide, float4* albedo,
                                                             float4* meanOut)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    const float    nf = static_cast<float>(tileSamples[(y >> 5) * frameTilesX + (x >> 5)]);
    prepPixel<true>(mean, albedoCoverage, normalDepth, i, x, y, tilesX, nf, e, guide, albedo, meanOut);
}

// One pass of step `step` = 2^i: sc2 = (σc σc) 2^-i, szs = σz step.  last: out = the mean {e' (a + εa), 1} (background: {c, 1}); else out = {e', ℓ'}.
__global__ __launch_bounds__(kDenoiseBlock) void kDenoiseAtrous(const float4* eIn, const float4* guide, const float4* albedo, float4* out, uint32_t width, uint32_t height,
                                                               int step, float sc2, float sigmaN, float szs, uint32_t last)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
    if (x >= width || y >= height) return;
    const uint32_t p = y * width + x;
    const float4   ep = eIn[p];
    const float4   gp = guide[p];
    if (!(gp.w > 0.0f))
    {
        out[p] = last ? make_float4(ep.x, ep.y, ep.z, 1.0f) : ep;
        return;
    }
    constexpr float k[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float     denC = sc2 * (ep.w * ep.w + kEpsLum);
    const float     denZ = szs * gp.w;
    float           sumW = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
    {
        const int qy = static_cast<int>(y) + step * dy;
        if (qy < 0 || qy >= static_cast<int>(height)) continue; // (a row outside the frame: all five taps skipped)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
        {
            const int   qx = static_cast<int>(x) + step * dx;
            const float h = k[dx + 2] * k[dy + 2];
            float       w;
            float4      eq;
            if (dx == 0 && dy == 0)
            {
                w = h;
                eq = ep;
            }
            else
            {
                if (qx < 0 || qx >= static_cast<int>(width)) continue;
                const uint32_t q = static_cast<uint32_t>(qy) * width + static_cast<uint32_t>(qx);
                const float4   gq = guide[q];
                if (!(gq.w > 0.0f)) continue;
                eq = eIn[q];
                const float dr = eq.x - ep.x, dg = eq.y - ep.y, db = eq.z - ep.z;
                const float xc = ((dr * dr + dg * dg) + db * db) / denC;
                const float xn = (1.0f - ((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z)) / sigmaN;
                const float xz = fabsf(gq.w - gp.w) / denZ;
                w = ((h * tukey(xc)) * tukey(xn)) * tukey(xz);
            }
            sumW += w;
            sx += w * eq.x;
            sy += w * eq.y;
            sz += w * eq.z;
        }
    }
    const float ex = sx / sumW, ey = sy / sumW, ez = sz / sumW;
    if (last)
    {
        const float4 ae = albedo[p];
        out[p] = make_float4(ex * ae.x, ey * ae.y, ez * ae.z, 1.0f);
    }
    else
        out[p] = make_float4(ex, ey, ez, (ex + ey) + ez);
}

// ---- The split-component filter (include/rayfinder_amd.h, "Split-component denoiser"): the direct light D and the indirect light S - D, demodulated by the same
// a + εa, each filtered by a chain of its own -- today's pass with its own σ and its own e, ℓ -- and added before the remodulation.

// prep: c, the background test, a, n, z and a + εa exactly as prepPixel; then eD = (D.rgb / Nf) / (a + εa), eI = ((S.rgb - D.rgb) / Nf) / (a + εa), each with its own ℓ.
// Background: eD = {c, 0}, eI = 0.  meanOut (L_D = L_I = 0): the mean c, exactly.  tilesX != 0: S, D and the AOV sums are compact tile-major; 0: row-major.
// Pixel i = (x, y) with its sample count as a float: shared by kDenoisePrepSplit (one count for the frame) and kDenoisePrepSplitTiles (the count of the pixel's tile).
__device__ __forceinline__ void prepSplitPixel(const float4* colorSum, const float4* directSum, const float4* albedoCoverage, const float4* normalDepth, uint32_t i, uint32_t x,
                                               uint32_t y, uint32_t tilesX, float nf, float4* eD, float4* eI, float4* guide, float4* albedo, float4* meanOut)
{
    const uint32_t src = tilesX ? tileMajorIndex(x, y, tilesX) : i;
    const float4   S = colorSum[src];
    const Vec3     c = vec3(S.x / nf, S.y / nf, S.z / nf);
    if (meanOut)
    {
        meanOut[i] = make_float4(c.x, c.y, c.z, 1.0f);
        return;
    }
    const float4 AC = albedoCoverage[src], ND = normalDepth[src];
    const float  z = ND.w / AC.w;
    if (AC.w == 0.0f || !(z > 0.0f)) // background: passes through, never a neighbour
    {
        eD[i] = make_float4(c.x, c.y, c.z, 0.0f);
        eI[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        guide[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        albedo[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 D = directSum[src];
    const Vec3   a = vec3(AC.x / nf, AC.y / nf, AC.z / nf);
    const Vec3   m = vec3(ND.x / nf, ND.y / nf, ND.z / nf);
    const float  d = dot(m, m);
    const Vec3   n = (d != 0.0f && fabsf(d) <= FLT_MAX) ? normalize(m) : splat(0.0f);
    const Vec3   ae = a + splat(kEpsAlbedo);
    const Vec3   cD = vec3(D.x / nf, D.y / nf, D.z / nf);
    const Vec3   cI = vec3((S.x - D.x) / nf, (S.y - D.y) / nf, (S.z - D.z) / nf);
    const Vec3   vD = vec3(cD.x / ae.x, cD.y / ae.y, cD.z / ae.z);
    const Vec3   vI = vec3(cI.x / ae.x, cI.y / ae.y, cI.z / ae.z);
    eD[i] = make_float4(vD.x, vD.y, vD.z, (vD.x + vD.y) + vD.z);
    eI[i] = make_float4(vI.x, vI.y, vI.z, (vI.x + vI.y) + vI.z);
    guide[i] = make_float4(n.x, n.y, n.z, z);
    albedo[i] = make_float4(ae.x, ae.y, ae.z, 0.0f);
}

__global__ __launch_bounds__(256) void kDenoisePrepSplit(const float4* colorSum, const float4* directSum, const float4* albedoCoverage, const float4* normalDepth, uint32_t width,
                                                         uint32_t height, uint32_t tilesX, float nf, float4* eD, float4* eI, float4* guide, float4* albedo, float4* meanOut)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    prepSplitPixel(colorSum, directSum, albedoCoverage, normalDepth, i, x, y, tilesX, nf, eD, eI, guide, albedo, meanOut);
}

// The same with one sample count per 32x32 tile of the frame, for c, a, m, cD and cI alike: Nf = float(tileSamples[tile of the pixel]) as kDenoisePrepTiles takes it
// (frameTilesX: the frame's tiles per row whatever the layout of the sums; every count is > 0).  With every count equal to N: kDenoisePrepSplit's bits.
__global__ __launch_bounds__(256) void kDenoisePrepSplitTiles(const float4* colorSum, const float4* directSum, const float4* albedoCoverage, const float4* normalDepth,
                                                              uint32_t width, uint32_t height, uint32_t tilesX, const uint32_t* tileSamples, uint32_t frameTilesX, float4* eD,
                                                              float4* eI, float4* guide, float4* albedo, float4* meanOut)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    const float    nf = static_cast<float>(tileSamples[(y >> 5) * frameTilesX + (x >> 5)]);
    prepSplitPixel(colorSum, directSum, albedoCoverage, normalDepth, i, x, y, tilesX, nf, eD, eI, guide, albedo, meanOut);
}

// one component's constants of a pass of step 2^i: sc2 = (σc σc) 2^-i, σn, szs = σz step
struct SplitPass
{
    float sc2, sigmaN, szs;
};

// One pass of step `step` over both components.  DIRECT / INDIRECT: the component is active in this pass (it has not run its own L passes yet) -- it is filtered from
// dIn / iIn exactly as kDenoiseAtrous filters, with its own constants; an inactive one is neither filtered nor written, and the last pass reads its value at the pixel
// itself.  SHARED (both active, the same σn and szs): the normal and depth terms of a tap are evaluated once for both.
// last: out = {(eD' + eI') (a + εa), 1} (background: {eD.rgb, 1} = {c, 1}); else the active components' {e', ℓ'} go to dOut / iOut (background: a copy).
template<bool DIRECT, bool INDIRECT, bool SHARED>
__global__ __launch_bounds__(kDenoiseBlock) void kDenoiseAtrousSplit(const float4* dIn, const float4* iIn, const float4* guide, const float4* albedo, float4* dOut, float4* iOut,
                                                                    float4* out, uint32_t width, uint32_t height, int step, SplitPass pd, SplitPass pi, uint32_t last)
{
    static_assert(DIRECT || INDIRECT, "a pass filters at least one component");
    static_assert(!SHARED || (DIRECT && INDIRECT), "only two active components share their guide terms");
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
    if (x >= width || y >= height) return;
    const uint32_t p = y * width + x;
    const float4   gp = guide[p];
    // (an inactive component's value is needed by the last pass alone)
    const float4   dp = (DIRECT || last) ? dIn[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4   ip = (INDIRECT || last) ? iIn[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(gp.w > 0.0f))
    {
        if (last) out[p] = make_float4(dp.x, dp.y, dp.z, 1.0f);
        else
        {
            if (DIRECT) dOut[p] = dp;
            if (INDIRECT) iOut[p] = ip;
        }
        return;
    }
    constexpr float k[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float     denCD = pd.sc2 * (dp.w * dp.w + kEpsLum), denCI = pi.sc2 * (ip.w * ip.w + kEpsLum);
    const float     denZD = pd.szs * gp.w, denZI = pi.szs * gp.w;
    float           sumWD = 0.0f, dx_ = 0.0f, dy_ = 0.0f, dz_ = 0.0f;
    float           sumWI = 0.0f, ix_ = 0.0f, iy_ = 0.0f, iz_ = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
    {
        const int qy = static_cast<int>(y) + step * dy;
        if (qy < 0 || qy >= static_cast<int>(height)) continue; // (a row outside the frame: all five taps skipped)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
        {
            const int   qx = static_cast<int>(x) + step * dx;
            const float h = k[dx + 2] * k[dy + 2];
            float       wD = h, wI = h;
            float4      dq = dp, iq = ip;
            if (!(dx == 0 && dy == 0))
            {
                if (qx < 0 || qx >= static_cast<int>(width)) continue;
                const uint32_t q = static_cast<uint32_t>(qy) * width + static_cast<uint32_t>(qx);
                const float4   gq = guide[q];
                if (!(gq.w > 0.0f)) continue;
                const float nd = 1.0f - ((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
                const float zd = fabsf(gq.w - gp.w);
                const float tnD = tukey(nd / pd.sigmaN), tzD = tukey(zd / denZD);
                const float tnI = SHARED ? tnD : tukey(nd / pi.sigmaN), tzI = SHARED ? tzD : tukey(zd / denZI);
                if (DIRECT)
                {
                    dq = dIn[q];
                    const float dr = dq.x - dp.x, dg = dq.y - dp.y, db = dq.z - dp.z;
                    const float xc = ((dr * dr + dg * dg) + db * db) / denCD;
                    wD = ((h * tukey(xc)) * tnD) * tzD;
                }
                if (INDIRECT)
                {
                    iq = iIn[q];
                    const float dr = iq.x - ip.x, dg = iq.y - ip.y, db = iq.z - ip.z;
                    const float xc = ((dr * dr + dg * dg) + db * db) / denCI;
                    wI = ((h * tukey(xc)) * tnI) * tzI;
                }
            }
            if (DIRECT)
            {
                sumWD += wD;
                dx_ += wD * dq.x;
                dy_ += wD * dq.y;
                dz_ += wD * dq.z;
            }
            if (INDIRECT)
            {
                sumWI += wI;
                ix_ += wI * iq.x;
                iy_ += wI * iq.y;
                iz_ += wI * iq.z;
            }
        }
    }
    // e' of an active component; an inactive one keeps its value
    const float dX = DIRECT ? dx_ / sumWD : dp.x, dY = DIRECT ? dy_ / sumWD : dp.y, dZ = DIRECT ? dz_ / sumWD : dp.z;
    const float iX = INDIRECT ? ix_ / sumWI : ip.x, iY = INDIRECT ? iy_ / sumWI : ip.y, iZ = INDIRECT ? iz_ / sumWI : ip.z;
    if (last)
    {
        const float4 ae = albedo[p];
        out[p] = make_float4((dX + iX) * ae.x, (dY + iY) * ae.y, (dZ + iZ) * ae.z, 1.0f);
        return;
    }
    if (DIRECT) dOut[p] = make_float4(dX, dY, dZ, (dX + dY) + dZ);
    if (INDIRECT) iOut[p] = make_float4(iX, iY, iZ, (iX + iY) + iZ);
}
} // namespace

void DenoiseWork::reserve(uint64_t n, hipStream_t stream, bool split)
{
    // (bgra and eI[1] are allocated last: each has room only when every buffer of its set has)
    const bool needSplit = split && eI[1].count < n;
    if (n <= bgra.count && !needSplit) return;
    RF_HIP(hipStreamSynchronize(stream)); // (a smaller set may still be in use by the last run)
    const bool            withSplit = split || eI[1].count != 0;
    const uint64_t        room = std::max<uint64_t>(n, bgra.count);
    DeviceBuffer<float4>* const f4[] = {&e[0], &e[1], &guide, &albedo, &out};
    for (auto* b : f4) b->release(); // (the whole set goes before any of the new one comes)
    bgra.release();
    eI[0].release(), eI[1].release();
    for (auto* b : f4) b->alloc(room);
    bgra.alloc(room);
    if (withSplit) eI[0].alloc(room), eI[1].alloc(room);
}

void enqueueDenoise(hipStream_t stream, DenoiseWork& w, const FrameSums& s, const DenoiseParameters& p, float exposure, const float4* mean)
{
    const uint32_t width = s.width, height = s.height, n = width * height;
    w.reserve(n, stream);
    const float nf = static_cast<float>(s.samples);
    const dim3  prepGrid((n + 255) / 256);
    // prep into (e, guide, albedo), or for L = 0 into the mean: with the frame's one count, or with each pixel's tile's own
    const auto prep = [&](float4* e, float4* guide, float4* albedo, float4* meanOut) {
        if (mean && s.tileSamples)
            hipLaunchKernelGGL(kDenoisePrepMeanTiles, prepGrid, dim3(256), 0, stream, mean, s.albedoCoverage, s.normalDepth, width, height, s.tilesX, s.tileSamples,
                               TileGrid(width, height).tilesX, e, guide, albedo, meanOut);
        else if (mean)
            hipLaunchKernelGGL(kDenoisePrepMean, prepGrid, dim3(256), 0, stream, mean, s.albedoCoverage, s.normalDepth, width, height, s.tilesX, nf, e, guide, albedo, meanOut);
        else if (s.tileSamples)
            hipLaunchKernelGGL(kDenoisePrepTiles, prepGrid, dim3(256), 0, stream, s.colorSum, s.albedoCoverage, s.normalDepth, width, height, s.tilesX, s.tileSamples,
                               TileGrid(width, height).tilesX, e, guide, albedo, meanOut);
        else
            hipLaunchKernelGGL(kDenoisePrep, prepGrid, dim3(256), 0, stream, s.colorSum, s.albedoCoverage, s.normalDepth, width, height, s.tilesX, nf, e, guide, albedo, meanOut);
    };
    if (p.iterations == 0) prep(nullptr, nullptr, nullptr, w.out.ptr);
    else
    {
        prep(w.e[0].ptr, w.guide.ptr, w.albedo.ptr, nullptr);
        const dim3 grid((width + 15) / 16, (height + 15) / 16);
        for (uint32_t i = 0; i < p.iterations; ++i)
        {
            const bool  last = i + 1 == p.iterations;
            const float sc2 = (p.sigmaColor * p.sigmaColor) * std::ldexp(1.0f, -static_cast<int>(i)); // (exact: a power of two)
            const float szs = p.sigmaDepth * static_cast<float>(1u << i);
            hipLaunchKernelGGL(kDenoiseAtrous, grid, dim3(kDenoiseBlock), 0, stream, w.e[i & 1u].ptr, w.guide.ptr, w.albedo.ptr, last ? w.out.ptr : w.e[(i + 1) & 1u].ptr, width, height,
                               static_cast<int>(1u << i), sc2, p.sigmaNormal, szs, last ? 1u : 0u);
        }
    }
    hipLaunchKernelGGL(tonemapKernel(), dim3((n + 255) / 256), dim3(256), 0, stream, static_cast<const float4*>(w.out.ptr), n, 1u, exposure, w.bgra.ptr);
    RF_HIP(hipGetLastError());
}

// The pair with the lowest error of the sweep over both components' L and σc (profiles/split_denoise/README.md: 4-spp frames against 1024 spp): the direct light is all
// but noise-free and wants next to no filtering; the indirect light wants a short chain whose colour term is as good as off, its edges left to the normal and depth terms.
SplitDenoiseDefaults splitDenoiseDefaults() { return SplitDenoiseDefaults{DenoiseParameters{1u, 0.25f, 0.1f, 0.1f}, DenoiseParameters{2u, 256.0f, 0.1f, 0.1f}}; }

void enqueueDenoiseSplit(hipStream_t stream, DenoiseWork& w, const FrameSums& s, const DenoiseParameters& pd, const DenoiseParameters& pi, float exposure)
{
    const uint32_t width = s.width, height = s.height, n = width * height;
    w.reserve(n, stream, true);
    const float    nf = static_cast<float>(s.samples);
    const dim3     prepGrid((n + 255) / 256);
    const uint32_t passes = std::max(pd.iterations, pi.iterations);
    // prep into (eD, eI, guide, albedo), or for L_D = L_I = 0 into the mean: with the frame's one count, or with each pixel's tile's own
    const auto prep = [&](float4* eD, float4* eI, float4* guide, float4* albedo, float4* meanOut) {
        if (s.tileSamples)
            hipLaunchKernelGGL(kDenoisePrepSplitTiles, prepGrid, dim3(256), 0, stream, s.colorSum, s.directSum, s.albedoCoverage, s.normalDepth, width, height, s.tilesX, s.tileSamples,
                               TileGrid(width, height).tilesX, eD, eI, guide, albedo, meanOut);
        else
            hipLaunchKernelGGL(kDenoisePrepSplit, prepGrid, dim3(256), 0, stream, s.colorSum, s.directSum, s.albedoCoverage, s.normalDepth, width, height, s.tilesX, nf, eD, eI, guide,
                               albedo, meanOut);
    };
    if (passes == 0) prep(nullptr, nullptr, nullptr, nullptr, w.out.ptr);
    else
    {
        prep(w.e[0].ptr, w.eI[0].ptr, w.guide.ptr, w.albedo.ptr, nullptr);
        const dim3 grid((width + 15) / 16, (height + 15) / 16);
        uint32_t   curD = 0, curI = 0; // which of its two buffers holds each component's current value
        for (uint32_t i = 0; i < passes; ++i)
        {
            const bool last = i + 1 == passes, actD = i < pd.iterations, actI = i < pi.iterations;
            const auto pass = [&](const DenoiseParameters& p) {
                return SplitPass{(p.sigmaColor * p.sigmaColor) * std::ldexp(1.0f, -static_cast<int>(i)) /* exact: a power of two */, p.sigmaNormal,
                                 p.sigmaDepth * static_cast<float>(1u << i)};
            };
            const SplitPass sd = pass(pd), si = pass(pi);
            const bool      shared = actD && actI && sd.sigmaN == si.sigmaN && sd.szs == si.szs;
            const auto      kernel = actD && actI ? (shared ? kDenoiseAtrousSplit<true, true, true> : kDenoiseAtrousSplit<true, true, false>)
                                                  : (actD ? kDenoiseAtrousSplit<true, false, false> : kDenoiseAtrousSplit<false, true, false>);
            hipLaunchKernelGGL(kernel, grid, dim3(kDenoiseBlock), 0, stream, static_cast<const float4*>(w.e[curD].ptr), static_cast<const float4*>(w.eI[curI].ptr),
                               static_cast<const float4*>(w.guide.ptr), static_cast<const float4*>(w.albedo.ptr), w.e[curD ^ 1u].ptr, w.eI[curI ^ 1u].ptr, w.out.ptr, width, height,
                               static_cast<int>(1u << i), sd, si, last ? 1u : 0u);
            if (actD) curD ^= 1u;
            if (actI) curI ^= 1u;
        }
    }
    hipLaunchKernelGGL(tonemapKernel(), dim3((n + 255) / 256), dim3(256), 0, stream, static_cast<const float4*>(w.out.ptr), n, 1u, exposure, w.bgra.ptr);
    RF_HIP(hipGetLastError());
}

void denoiseSplitImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* directSum, const float* albedoCoverage,
                        const float* normalDepth, const DenoiseParameters& direct, const DenoiseParameters& indirect, float exposure, float* outRgba, uint32_t* outBgra8)
{
    denoiseSplitTiles(deviceOrdinal, width, height, nullptr, samples, colorSum, directSum, albedoCoverage, normalDepth, direct, indirect, exposure, outRgba, outBgra8);
}

void denoiseSplitTiles(int deviceOrdinal, uint32_t width, uint32_t height, const uint32_t* tileSamples, uint32_t samples, const float* colorSum, const float* directSum,
                       const float* albedoCoverage, const float* normalDepth, const DenoiseParameters& direct, const DenoiseParameters& indirect, float exposure,
                       float* outRgba, uint32_t* outBgra8)
{
    DenoiseWork work; // (before the stage: freed after it has drained its stream)
    StagedFrame f(deviceOrdinal, width, height, samples, tileSamples, colorSum, nullptr, albedoCoverage, normalDepth, directSum);
    enqueueDenoiseSplit(f.stream.handle, work, f.sums, direct, indirect, exposure);
    f.download(outRgba, work.out.ptr, f.pixels() * sizeof(float4));
    f.download(outBgra8, work.bgra.ptr, f.pixels() * sizeof(uint32_t));
    f.wait();
}

void denoiseImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* albedoCoverage, const float* normalDepth,
                   const DenoiseParameters& params, float exposure, float* outRgba, uint32_t* outBgra8)
{
    denoiseTiles(deviceOrdinal, width, height, nullptr, samples, colorSum, albedoCoverage, normalDepth, params, exposure, outRgba, outBgra8);
}

void denoiseTiles(int deviceOrdinal, uint32_t width, uint32_t height, const uint32_t* tileSamples, uint32_t samples, const float* colorSum, const float* albedoCoverage,
                  const float* normalDepth, const DenoiseParameters& params, float exposure, float* outRgba, uint32_t* outBgra8)
{
    DenoiseWork work; // (before the stage: freed after it has drained its stream)
    StagedFrame f(deviceOrdinal, width, height, samples, tileSamples, colorSum, nullptr, albedoCoverage, normalDepth, nullptr);
    enqueueDenoise(f.stream.handle, work, f.sums, params, exposure);
    f.download(outRgba, work.out.ptr, f.pixels() * sizeof(float4));
    f.download(outBgra8, work.bgra.ptr, f.pixels() * sizeof(uint32_t));
    f.wait();
}
} // namespace rf
