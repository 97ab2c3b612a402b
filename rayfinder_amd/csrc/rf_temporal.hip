// rf_temporal.hip -- the temporal history: the previous view's frame reprojected into the current camera and blended behind the current view's samples.  The arithmetic
// is the one include/rayfinder_amd.h writes out ("Temporal history"), one IEEE f32 operation at a time in that order (-ffp-contract=off, correctly rounded divide and
// sqrt, no denormal flushing): tests/temporal_restatement.py reproduces it bit for bit.  No atomics: every output is one lane's fixed sequence of operations.
//   kTemporalReproject<TILE_MAJOR>  one lane per pixel, 16x16-pixel workgroups of four 8x8-pixel waves as kDenoiseAtrous has them (the four taps of a wave's 64 pixels fall
//                   on few cache lines of the two history planes).  The lane forms prep's values of its pixel from the sums where they lie (tile-major: a handle's own;
//                   row-major: rf_temporal_images), its world point, the point's place in the old view, the four taps, the blend and the texel, and writes T, G and the
//                   texel: no plane makes a round trip through HBM between the steps.  No LDS: a lane's taps are its own, and a neighbour's taps are a cache's business.
#include "rf_temporal.hpp"

#include "rf_device.hpp" // tonemapTexel
#include "rf_math.hpp"
#include "rf_prep.hpp"

namespace rf
{
namespace
{
struct TemporalArgs
{
    const float4 *colorSum, *albedoCoverage, *normalDepth; // the current view's sums, all in one layout
    const float4 *histColor, *histGeometry;                // row-major T', G'; nullptr: no history
    float4 *      outColor, *outGeometry;                  // row-major T, G
    uint32_t*     outBgra;
    Camera        camera, histCamera;
    uint32_t      width, height, tilesX;
    float         nf, maxHistory, depthTolerance, minNormalDot, exposure;
};

template<bool TILE_MAJOR>
__global__ __launch_bounds__(256) void kTemporalReproject(TemporalArgs a)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
    if (x >= a.width || y >= a.height) return;
    const uint32_t p = y * a.width + x;
    const uint32_t src = TILE_MAJOR ? prepTileMajorIndex(x, y, a.tilesX) : p;
    // 1 prep
    const float    nf = a.nf;
    const float4   S = a.colorSum[src], AC = a.albedoCoverage[src], ND = a.normalDepth[src];
    const Vec3     c = prepColor(S, nf);
    float          z;
    float4         T = make_float4(c.x, c.y, c.z, nf);
    if (prepBackground(AC, ND, z))
    {
        a.outColor[p] = T;
        a.outGeometry[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        a.outBgra[p] = tonemapTexel(T, 1u, a.exposure);
        return;
    }
    const Vec3 n = prepNormal(ND, nf);
    a.outGeometry[p] = make_float4(n.x, n.y, n.z, z);
    if (a.histColor != nullptr)
    {
        // 2 world point: kRaygen's expressions at the blue-noise pair's mean, from the pinhole centre
        const float wf = static_cast<float>(a.width), hf = static_cast<float>(a.height);
        const float u = (static_cast<float>(x) + 0.5f) / wf;
        const float v = (static_cast<float>(y) + 0.5f) / hf;
        const float s = u + 0.5f / wf;
        const float t = (1.0f - v) + 0.5f / hf;
        const Vec3  dir = normalize(a.camera.lowerLeftCorner + s * a.camera.horizontal + t * a.camera.vertical - a.camera.origin);
        const Vec3  P = a.camera.origin + z * dir;
        // 3 into the old view
        const Camera& h = a.histCamera;
        const Vec3    w = P - h.origin;
        const Vec3    L = h.lowerLeftCorner - h.origin;
        const Vec3    Nn = cross(h.horizontal, h.vertical);
        const float   den = dot(Nn, w);
        const float   k = dot(Nn, L) / den;
        if (k > 0.0f) // (in front of the old camera, whichever way horizontal' x vertical' points; a NaN fails)
        {
            const Vec3  q = k * w - L;
            const float nn = dot(Nn, Nn);
            const float ca = dot(cross(q, h.vertical), Nn) / nn;
            const float cb = dot(cross(h.horizontal, q), Nn) / nn;
            const float fx = ca * wf - 1.0f;
            const float fy = (1.0f - cb) * hf;
            if (fx >= -1.0f && fx < wf && fy >= -1.0f && fy < hf) // (a NaN fails; decided before the conversion below)
            {
                const float xf = floorf(fx), yf = floorf(fy);
                const float tx = fx - xf, ty = fy - yf;
                const int   x0 = static_cast<int>(xf), y0 = static_cast<int>(yf);
                const float zOld = rf_sqrt(dot(w, w));
                const float zTol = a.depthTolerance * zOld;
                // 4 taps
                float sumB = 0.0f, sumR = 0.0f, sumG = 0.0f, sumBl = 0.0f, sumH = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j)
                {
                    const int qy = y0 + j;
                    if (qy < 0 || qy >= static_cast<int>(a.height)) continue;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                    {
                        const int qx = x0 + i;
                        if (qx < 0 || qx >= static_cast<int>(a.width)) continue;
                        const uint32_t tap = static_cast<uint32_t>(qy) * a.width + static_cast<uint32_t>(qx);
                        const float4   Gq = a.histGeometry[tap], Tq = a.histColor[tap];
                        const bool     valid = Tq.w > 0.0f && Gq.w > 0.0f && fabsf(Gq.w - zOld) <= zTol && dot(n, vec3(Gq.x, Gq.y, Gq.z)) >= a.minNormalDot;
                        if (!valid) continue;
                        const float beta = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                        sumB += beta;
                        sumR += beta * Tq.x;
                        sumG += beta * Tq.y;
                        sumBl += beta * Tq.z;
                        sumH += beta * Tq.w;
                    }
                }
                if (sumB > 0.0f)
                {
                    // 5 blend
                    const float hh = sumH / sumB;
                    const float he = hh < a.maxHistory ? hh : a.maxHistory;
                    const float wsum = nf + he;
                    T = make_float4((nf * c.x + he * (sumR / sumB)) / wsum, (nf * c.y + he * (sumG / sumB)) / wsum, (nf * c.z + he * (sumBl / sumB)) / wsum, wsum);
                }
            }
        }
    }
    a.outColor[p] = T;
    a.outBgra[p] = tonemapTexel(T, 1u, a.exposure);
}
} // namespace

void TemporalWork::reserve(uint64_t pixels, hipStream_t stream)
{
    if (bgra.count == pixels) return;
    RF_HIP(hipStreamSynchronize(stream)); // (a set of another size may still be in use by the last run)
    release();
    for (int k = 0; k < 2; ++k) color[k].alloc(pixels), geometry[k].alloc(pixels);
    bgra.alloc(pixels);
}

void TemporalWork::release()
{
    for (int k = 0; k < 2; ++k) color[k].release(), geometry[k].release();
    bgra.release();
}

void enqueueTemporal(hipStream_t stream, const FrameSums& s, const Camera& camera, const float4* histColor, const float4* histGeometry, const Camera* histCamera,
                     const TemporalParameters& params, float exposure, float4* outColor, float4* outGeometry, uint32_t* outBgra)
{
    const uint32_t     width = s.width, height = s.height;
    const bool         history = histColor != nullptr && histGeometry != nullptr && histCamera != nullptr;
    const TemporalArgs args{s.colorSum,  s.albedoCoverage, s.normalDepth, history ? histColor : nullptr, history ? histGeometry : nullptr, outColor, outGeometry, outBgra, camera,
                            history ? *histCamera : camera, width, height, s.tilesX, static_cast<float>(s.samples), params.maxHistory, params.depthTolerance, params.minNormalDot,
                            exposure};
    const dim3         grid((width + 15) / 16, (height + 15) / 16);
    hipLaunchKernelGGL(s.tilesX ? kTemporalReproject<true> : kTemporalReproject<false>, grid, dim3(256), 0, stream, args);
    RF_HIP(hipGetLastError());
}

void temporalImages(int deviceOrdinal, uint32_t width, uint32_t height, uint32_t samples, const float* colorSum, const float* albedoCoverage, const float* normalDepth,
                    const Camera& camera, const float* histColor, const float* histGeometry, const Camera* histCamera, const TemporalParameters& params, float exposure,
                    float* outColor, float* outGeometry, uint32_t* outBgra8)
{
    DeviceBuffer<float4>   hist[2], out[2]; // (all before the stage: freed after it has drained its stream)
    DeviceBuffer<uint32_t> bgra;
    StagedFrame            f(deviceOrdinal, width, height, samples, nullptr, colorSum, nullptr, albedoCoverage, normalDepth, nullptr);
    const uint64_t         n = f.pixels();
    if (histColor) f.upload(hist[0], reinterpret_cast<const float4*>(histColor), n); // (else: no history)
    if (histGeometry) f.upload(hist[1], reinterpret_cast<const float4*>(histGeometry), n);
    out[0].alloc(n), out[1].alloc(n), bgra.alloc(n);
    enqueueTemporal(f.stream.handle, f.sums, camera, hist[0].ptr, hist[1].ptr, histCamera, params, exposure, out[0].ptr, out[1].ptr, bgra.ptr);
    f.download(outColor, out[0].ptr, n * sizeof(float4));
    f.download(outGeometry, out[1].ptr, n * sizeof(float4));
    f.download(outBgra8, bgra.ptr, n * sizeof(uint32_t));
    f.wait();
}
} // namespace rf
