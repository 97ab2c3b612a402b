// rf_c_api.cpp -- the extern "C" boundary declared in include/rayfinder_amd.h.
// Exceptions never cross it: they become status codes + a thread-local message.
#include "../../include/rayfinder_amd.h"

#include "rf_bvh.hpp"
#include "rf_bvh_gpu.hpp"
#include "rf_camera.hpp"
#include "rf_checkpoint.hpp"
#include "rf_comm.hpp"
#include "rf_feature_request.hpp"
#include "rf_gltf.hpp"
#include "rf_pt_format.hpp"
#include "rf_query.hpp"
#include "rf_renderer.hpp"
#include "rf_sky.hpp"
#include "rf_wide_build.hpp"

#include <cstring>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

static_assert(sizeof(rf_camera) == sizeof(rf::Camera));
static_assert(RF_AOV_FIRST_HIT == rf::Renderer::kAovFirstHit);
static_assert(RF_AOV_TILE_COUNTS == rf::Renderer::kAovTileCounts);
static_assert(RF_DIRECT_TILE_COUNTS == rf::Renderer::kDirectTileCounts && rf::Renderer::kDirectOn == 1u);
static_assert(RF_BUCKETS_TILE_COUNTS == rf::Renderer::kBucketsTileCounts);
static_assert(RF_BUCKETS_SHARD_TILE_COUNTS == rf::Renderer::kBucketsShardTileCounts);
static_assert(RF_FEATURE_COLOR == rf::kFeatureColor && RF_FEATURE_ALBEDO == rf::kFeatureAlbedo && RF_FEATURE_NORMAL == rf::kFeatureNormal && RF_FEATURE_DEPTH == rf::kFeatureDepth &&
              RF_FEATURE_COVERAGE == rf::kFeatureCoverage && RF_FEATURE_DIRECT == rf::kFeatureDirect && RF_FEATURE_INDIRECT == rf::kFeatureIndirect &&
              RF_FEATURE_VARIANCE == rf::kFeatureVariance && RF_FEATURE_ERROR == rf::kFeatureError && RF_FEATURE_SAMPLES == rf::kFeatureSamples);
static_assert(RF_FEATURES_CHW == rf::kFeaturesChw && RF_FEATURES_HWC == rf::kFeaturesHwc && RF_FEATURES_F32 == rf::kFeaturesF32 && RF_FEATURES_F16 == rf::kFeaturesF16);

struct rf_renderer
{
    std::unique_ptr<rf::Renderer> impl;
};

struct rf_comm
{
    std::unique_ptr<rf::TileComm> impl;
};

struct rf_pt_format
{
    rf::PtFormat format;
};

namespace
{
thread_local std::string gLastError;

struct NoDevice : std::runtime_error
{
    using std::runtime_error::runtime_error;
};

template<typename F>
int guarded(F&& f)
{
    try
    {
        gLastError.clear();
        return f();
    }
    catch (const std::invalid_argument& e)
    {
        gLastError = e.what();
        return RF_ERROR_INVALID_ARGUMENT;
    }
    catch (const std::bad_alloc&)
    {
        gLastError = "out of host memory";
        return RF_ERROR_RUNTIME;
    }
    catch (const rf::CheckpointCorrupt& e)
    {
        gLastError = e.what();
        return RF_ERROR_CORRUPT;
    }
    catch (const std::exception& e)
    {
        gLastError = e.what();
        if (gLastError.find("no HIP device") != std::string::npos) return RF_ERROR_NO_DEVICE;
        if (gLastError.find("sky parameters out of range") != std::string::npos) return RF_ERROR_OUT_OF_RANGE;
        return RF_ERROR_RUNTIME;
    }
    catch (...)
    {
        gLastError = "Unknown exception occurred.";
        return RF_ERROR_RUNTIME;
    }
}

void require(bool cond, const char* what)
{
    if (!cond) throw std::invalid_argument(what);
}

// The *_tiles calls' counts, one per tile of the frame's 32 x 32 grid: each at least `minimum` (else `what`) -> the leading one
uint32_t requireTileSamples(const uint32_t* tile_samples, uint32_t width, uint32_t height, uint32_t minimum, const char* what)
{
    const uint32_t tiles = ((width + 31u) / 32u) * ((height + 31u) / 32u);
    uint32_t       leading = 0;
    for (uint32_t t = 0; t < tiles; ++t)
    {
        require(tile_samples[t] >= minimum, what);
        leading = tile_samples[t] > leading ? tile_samples[t] : leading;
    }
    return leading;
}

rf::Vec3 v3(const float* p) { return rf::vec3(p[0], p[1], p[2]); }

rf::Camera toCamera(const rf_camera& c)
{
    rf::Camera out;
    std::memcpy(&out, &c, sizeof out);
    return out;
}

rf::RenderParameters toParams(const rf_render_parameters& p)
{
    rf::RenderParameters out;
    out.width = p.width;
    out.height = p.height;
    out.camera = toCamera(p.camera);
    out.samplingParams.numSamplesPerPixel = p.num_samples_per_pixel;
    out.samplingParams.numBounces = p.num_bounces;
    out.sky.turbidity = p.sky.turbidity;
    std::memcpy(out.sky.albedo, p.sky.albedo, sizeof out.sky.albedo);
    out.sky.sunZenithDegrees = p.sky.sun_zenith_degrees;
    out.sky.sunAzimuthDegrees = p.sky.sun_azimuth_degrees;
    out.exposure = p.exposure;
    require(p.width > 0 && p.height > 0, "framebuffer size must be non-zero");
    require(p.num_samples_per_pixel > 0, "num_samples_per_pixel must be > 0");
    require(p.num_bounces > 0, "num_bounces must be > 0");
    return out;
}
// the denoiser's parameters (NULL: the defaults), checked before anything touches a device
rf::DenoiseParameters toDenoiseParams(const rf_denoise_parameters* p)
{
    rf::DenoiseParameters out;
    if (!p) return out;
    require(p->iterations <= 8, "denoise iterations must be 0 .. 8");
    for (const float s : {p->sigma_color, p->sigma_normal, p->sigma_depth})
        require(std::isfinite(s) && s > 0.0f, "denoise sigmas must be finite and > 0");
    out.iterations = p->iterations;
    out.sigmaColor = p->sigma_color, out.sigmaNormal = p->sigma_normal, out.sigmaDepth = p->sigma_depth;
    return out;
}
// the temporal history's parameters (NULL: the defaults), checked before anything touches a device
rf::TemporalParameters toTemporalParams(const rf_temporal_parameters* p)
{
    rf::TemporalParameters out;
    if (!p) return out;
    require(std::isfinite(p->max_history) && p->max_history > 0.0f, "temporal max_history must be finite and > 0");
    require(std::isfinite(p->depth_tolerance) && p->depth_tolerance > 0.0f, "temporal depth_tolerance must be finite and > 0");
    require(p->min_normal_dot >= -1.0f && p->min_normal_dot <= 1.0f, "temporal min_normal_dot must lie in [-1, 1]");
    require(p->reserved == 0u, "temporal parameters: reserved must be 0");
    out.maxHistory = p->max_history, out.depthTolerance = p->depth_tolerance, out.minNormalDot = p->min_normal_dot;
    return out;
}
// one component's parameters of the split-component denoiser (NULL: that component's default)
rf::DenoiseParameters toSplitParams(const rf_denoise_parameters* p, const rf::DenoiseParameters& fallback) { return p ? toDenoiseParams(p) : fallback; }
rf_noise_estimate toNoiseEstimate(const rf::NoiseEstimate& e)
{
    return rf_noise_estimate{e.meanError, e.maxError, e.worstTile, e.samples, e.pixels, e.nonfinitePixels};
}

// a feature request, checked before anything touches a device
rf::FeatureRequest toFeatureRequest(const rf_feature_request* req)
{
    require(req, "null argument");
    return rf::checkedFeatureRequest(req->channels, req->layout, req->dtype, req->reserved);
}

rf::AdaptiveParameters toAdaptiveParams(const rf_adaptive_parameters& p) { return rf::AdaptiveParameters{p.target_tile_error, p.check_every, p.min_samples, p.max_samples}; }

rf_adaptive_result toAdaptiveResult(const rf::AdaptiveResult& a)
{
    return rf_adaptive_result{a.estimatePasses, a.tiles, a.stoppedTiles, a.minTileSamples, a.maxTileSamples, 0u, a.pixelSamples, toNoiseEstimate(a.last)};
}
} // namespace

extern "C" {

const char* rf_last_error_message(void) { return gLastError.c_str(); }
const char* rf_version(void) { return "rayfinder_amd 0.1 (gfx950)"; }

// ---------------------------------------------------------------------------------------- renderer
int rf_renderer_create(const rf_renderer_descriptor* desc, const rf_scene* scene, rf_renderer** out)
{
    return guarded([&] {
        require(desc && scene && out, "null argument");
        require(scene->bvh_nodes && scene->num_bvh_nodes > 0, "scene has no BVH nodes");
        require(scene->num_triangles == 0 || (scene->position_attributes && scene->vertex_attributes), "null triangle arrays");
        rf::RendererDescriptor d;
        d.renderParams = toParams(desc->render_params);
        d.maxWidth = desc->max_width;
        d.maxHeight = desc->max_height;
        d.deviceOrdinal = desc->device_ordinal;
        d.maxPathsInFlight = desc->max_paths_in_flight;
        std::vector<rf::TextureView> textures;
        for (uint64_t i = 0; i < scene->num_textures; ++i)
        {
            const rf_texture& t = scene->base_color_textures[i];
            require(t.pixels && t.width && t.height, "empty texture");
            textures.push_back({t.pixels, t.width, t.height});
        }
        rf::SceneView view;
        view.bvhNodes = {static_cast<const rf::BvhNode*>(scene->bvh_nodes), static_cast<size_t>(scene->num_bvh_nodes)};
        view.positionAttributes = {static_cast<const rf::PositionAttribute*>(scene->position_attributes), static_cast<size_t>(scene->num_triangles)};
        view.vertexAttributes = {static_cast<const rf::VertexAttributes*>(scene->vertex_attributes), static_cast<size_t>(scene->num_triangles)};
        view.baseColorTextures = textures;
        auto handle = std::make_unique<rf_renderer>();
        handle->impl = std::make_unique<rf::Renderer>(d, view);
        *out = handle.release();
        return RF_OK;
    });
}

void rf_renderer_destroy(rf_renderer* r) { delete r; }

int rf_renderer_set_render_parameters(rf_renderer* r, const rf_render_parameters* params)
{
    return guarded([&] {
        require(r && params, "null argument");
        r->impl->setRenderParameters(toParams(*params));
        return RF_OK;
    });
}

int rf_renderer_render(rf_renderer* r, uint32_t num_frames)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->render(num_frames);
        return RF_OK;
    });
}

int rf_renderer_synchronize(rf_renderer* r)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->synchronize();
        return RF_OK;
    });
}

float rf_renderer_average_renderpass_duration_ms(rf_renderer* r)
{
    float v = 0.0f;
    guarded([&] {
        require(r, "null argument");
        v = r->impl->averageRenderpassDurationMs();
        return RF_OK;
    });
    return v;
}

float rf_renderer_render_progress_percentage(const rf_renderer* r) { return r ? r->impl->renderProgressPercentage() : 0.0f; }

int rf_renderer_read_accumulation(rf_renderer* r, float* dst, uint32_t* accumulated)
{
    return guarded([&] {
        require(r && dst, "null argument");
        r->impl->readAccumulation(dst);
        if (accumulated) *accumulated = r->impl->accumulatedSampleCount();
        return RF_OK;
    });
}

int rf_renderer_read_tonemapped(rf_renderer* r, uint32_t* dst)
{
    return guarded([&] {
        require(r && dst, "null argument");
        r->impl->readTonemapped(dst);
        return RF_OK;
    });
}

int rf_renderer_render_deferred(rf_renderer* r, uint32_t num_frames)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->renderDeferred(num_frames);
        return RF_OK;
    });
}

int rf_renderer_reset_deferred(rf_renderer* r)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->resetDeferred();
        return RF_OK;
    });
}

int rf_renderer_read_deferred(rf_renderer* r, float* sample_rgb, float* accumulation_rgb, uint32_t* bgra8, uint32_t* frame_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readDeferred(sample_rgb, accumulation_rgb, bgra8);
        if (frame_count) *frame_count = r->impl->deferredFrameCount();
        return RF_OK;
    });
}

int rf_renderer_set_aovs(rf_renderer* r, uint32_t flags)
{
    return guarded([&] {
        // (the flags first: a bad value is refused whatever the handle is, and is never confused with a bad handle)
        require((flags & ~(RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS)) == 0u, "unknown AOV flag bits");
        require((flags & RF_AOV_TILE_COUNTS) == 0u || (flags & RF_AOV_FIRST_HIT) != 0u, "RF_AOV_TILE_COUNTS says how the AOVs are kept: valid only together with RF_AOV_FIRST_HIT");
        require(r, "null argument");
        r->impl->setAovs(flags);
        return RF_OK;
    });
}

int rf_renderer_read_aovs(rf_renderer* r, float* albedo_coverage, float* normal_depth, uint32_t* aov_sample_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readAovs(albedo_coverage, normal_depth, aov_sample_count);
        return RF_OK;
    });
}

int rf_denoise_default_parameters(rf_denoise_parameters* out)
{
    return guarded([&] {
        require(out, "null argument");
        const rf::DenoiseParameters d;
        *out = rf_denoise_parameters{d.iterations, d.sigmaColor, d.sigmaNormal, d.sigmaDepth};
        return RF_OK;
    });
}

int rf_renderer_denoise(rf_renderer* r, const rf_denoise_parameters* params)
{
    return guarded([&] {
        const rf::DenoiseParameters p = toDenoiseParams(params);
        require(r, "null argument");
        r->impl->denoise(p);
        return RF_OK;
    });
}

int rf_renderer_read_denoised(rf_renderer* r, float* rgba, uint32_t* bgra8, uint32_t* sample_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readDenoised(rgba, bgra8, sample_count);
        return RF_OK;
    });
}

int rf_denoise_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* albedo_coverage4,
                      const float* normal_depth4, const rf_denoise_parameters* params, float exposure, float* out_rgba, uint32_t* out_bgra8)
{
    return guarded([&] {
        const rf::DenoiseParameters p = toDenoiseParams(params);
        require(color_sum4 && albedo_coverage4 && normal_depth4, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        require(samples > 0, "sample count must be > 0");
        require(std::isfinite(exposure), "exposure must be finite");
        rf::denoiseImages(device_ordinal, width, height, samples, color_sum4, albedo_coverage4, normal_depth4, p, exposure, out_rgba, out_bgra8);
        return RF_OK;
    });
}

int rf_denoise_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, const uint32_t* tile_samples, const float* color_sum4, const float* albedo_coverage4,
                     const float* normal_depth4, const rf_denoise_parameters* params, float exposure, float* out_rgba, uint32_t* out_bgra8)
{
    return guarded([&] {
        const rf::DenoiseParameters p = toDenoiseParams(params);
        require(tile_samples && color_sum4 && albedo_coverage4 && normal_depth4, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        const uint32_t leading = requireTileSamples(tile_samples, width, height, 1u, "the sample count of every tile must be > 0");
        require(std::isfinite(exposure), "exposure must be finite");
        rf::denoiseTiles(device_ordinal, width, height, tile_samples, leading, color_sum4, albedo_coverage4, normal_depth4, p, exposure, out_rgba, out_bgra8);
        return RF_OK;
    });
}

int rf_renderer_set_direct(rf_renderer* r, int enabled)
{
    return guarded([&] {
        require(r, "null argument");
        const uint32_t word = static_cast<uint32_t>(enabled);
        require((word & ~(1u | RF_DIRECT_TILE_COUNTS)) == 0u, "unknown direct flag bits: the word is 0, 1 or 1 | RF_DIRECT_TILE_COUNTS");
        require((word & RF_DIRECT_TILE_COUNTS) == 0u || (word & 1u) != 0u, "RF_DIRECT_TILE_COUNTS says how the direct sums are kept: valid only together with 1");
        r->impl->setDirect(word);
        return RF_OK;
    });
}

int rf_renderer_read_direct(rf_renderer* r, float* direct_sum4, uint32_t* direct_sample_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readDirect(direct_sum4, direct_sample_count);
        return RF_OK;
    });
}

int rf_denoise_split_default_parameters(rf_denoise_parameters* direct, rf_denoise_parameters* indirect)
{
    return guarded([&] {
        require(direct || indirect, "null argument");
        const rf::SplitDenoiseDefaults d = rf::splitDenoiseDefaults();
        if (direct) *direct = rf_denoise_parameters{d.direct.iterations, d.direct.sigmaColor, d.direct.sigmaNormal, d.direct.sigmaDepth};
        if (indirect) *indirect = rf_denoise_parameters{d.indirect.iterations, d.indirect.sigmaColor, d.indirect.sigmaNormal, d.indirect.sigmaDepth};
        return RF_OK;
    });
}

int rf_renderer_denoise_split(rf_renderer* r, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect)
{
    return guarded([&] {
        const rf::SplitDenoiseDefaults d = rf::splitDenoiseDefaults();
        const rf::DenoiseParameters    pd = toSplitParams(direct, d.direct), pi = toSplitParams(indirect, d.indirect);
        require(r, "null argument");
        r->impl->denoiseSplit(pd, pi);
        return RF_OK;
    });
}

int rf_denoise_split_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* direct_sum4,
                            const float* albedo_coverage4, const float* normal_depth4, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect,
                            float exposure, float* out_rgba, uint32_t* out_bgra8)
{
    return guarded([&] {
        const rf::SplitDenoiseDefaults d = rf::splitDenoiseDefaults();
        const rf::DenoiseParameters    pd = toSplitParams(direct, d.direct), pi = toSplitParams(indirect, d.indirect);
        require(color_sum4 && direct_sum4 && albedo_coverage4 && normal_depth4, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        require(samples > 0, "sample count must be > 0");
        require(std::isfinite(exposure), "exposure must be finite");
        rf::denoiseSplitImages(device_ordinal, width, height, samples, color_sum4, direct_sum4, albedo_coverage4, normal_depth4, pd, pi, exposure, out_rgba, out_bgra8);
        return RF_OK;
    });
}

int rf_denoise_split_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, const uint32_t* tile_samples, const float* color_sum4, const float* direct_sum4,
                           const float* albedo_coverage4, const float* normal_depth4, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect,
                           float exposure, float* out_rgba, uint32_t* out_bgra8)
{
    return guarded([&] {
        const rf::SplitDenoiseDefaults d = rf::splitDenoiseDefaults();
        const rf::DenoiseParameters    pd = toSplitParams(direct, d.direct), pi = toSplitParams(indirect, d.indirect);
        require(tile_samples && color_sum4 && direct_sum4 && albedo_coverage4 && normal_depth4, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        const uint32_t leading = requireTileSamples(tile_samples, width, height, 1u, "the sample count of every tile must be > 0");
        require(std::isfinite(exposure), "exposure must be finite");
        rf::denoiseSplitTiles(device_ordinal, width, height, tile_samples, leading, color_sum4, direct_sum4, albedo_coverage4, normal_depth4, pd, pi, exposure, out_rgba,
                              out_bgra8);
        return RF_OK;
    });
}

int rf_feature_channel_count(uint32_t channels, uint32_t* count)
{
    return guarded([&] {
        require(count, "null argument");
        rf::checkedFeatureRequest(channels, RF_FEATURES_CHW, RF_FEATURES_F32, 0u);
        *count = rf::featureChannelCount(channels);
        return RF_OK;
    });
}

int rf_renderer_export_features(rf_renderer* r, const rf_feature_request* req, void* dst_device, uint64_t dst_bytes, uint32_t* sample_count)
{
    return guarded([&] {
        require(r && req && dst_device, "null argument");
        const rf::FeatureRequest request = toFeatureRequest(req);
        const uint32_t           samples = r->impl->exportFeatures(request, dst_device, dst_bytes);
        if (sample_count) *sample_count = samples;
        return RF_OK;
    });
}

int rf_export_features_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const uint32_t* tile_samples, const float* color_sum4,
                              const float* sumsq4, const float* albedo_coverage4, const float* normal_depth4, const float* direct_sum4, const rf_feature_request* req,
                              void* out_host)
{
    return guarded([&] {
        const rf::FeatureRequest request = toFeatureRequest(req);
        const uint32_t           have = (color_sum4 ? rf::kFeatureReadsS : 0u) | (sumsq4 ? rf::kFeatureReadsQ : 0u) |
                              (albedo_coverage4 && normal_depth4 ? rf::kFeatureReadsAovs : 0u) | (direct_sum4 ? rf::kFeatureReadsD : 0u);
        rf::checkFeatureImages(width, height, samples, tile_samples, have, request, out_host);
        rf::exportFeaturesImages(device_ordinal, width, height, samples, tile_samples, color_sum4, sumsq4, albedo_coverage4, normal_depth4, direct_sum4, request, out_host);
        return RF_OK;
    });
}

int rf_renderer_set_moments(rf_renderer* r, int enabled)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->setMoments(enabled != 0);
        return RF_OK;
    });
}

int rf_renderer_read_moments(rf_renderer* r, float* sumsq4, uint32_t* moment_sample_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readMoments(sumsq4, moment_sample_count);
        return RF_OK;
    });
}

int rf_renderer_set_buckets(rf_renderer* r, uint32_t K)
{
    return guarded([&] {
        // (the low byte is K; above it RF_BUCKETS_TILE_COUNTS, only with K > 0, and RF_BUCKETS_SHARD_TILE_COUNTS, only together with it)
        const uint32_t k = K & 0xFFu;
        require((K & ~(0xFFu | RF_BUCKETS_TILE_COUNTS | RF_BUCKETS_SHARD_TILE_COUNTS)) == 0u && (k != 0u || K == 0u) && (k == 0u || (k % 2u == 1u && k >= 3u && k <= 15u)) &&
                    (!(K & RF_BUCKETS_SHARD_TILE_COUNTS) || (K & RF_BUCKETS_TILE_COUNTS)),
                "set_buckets: K must be 0 (off) or odd with 3 <= K <= 15, alone or ORed with RF_BUCKETS_TILE_COUNTS (K > 0 only), and with RF_BUCKETS_SHARD_TILE_COUNTS on top "
                "of that bit only");
        require(r, "null argument");
        r->impl->setBuckets(K);
        return RF_OK;
    });
}

int rf_renderer_read_buckets(rf_renderer* r, float* buckets, uint32_t* K, uint32_t* bucket_sample_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readBuckets(buckets, K, bucket_sample_count);
        return RF_OK;
    });
}

int rf_renderer_robust_mean(rf_renderer* r)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->robustMean();
        return RF_OK;
    });
}

int rf_renderer_read_robust_mean(rf_renderer* r, float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* sample_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readRobustMean(rgba, bgra8, trim, sample_count);
        return RF_OK;
    });
}

int rf_robust_mean_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t K, uint32_t samples, const float* buckets, float exposure, float* out_rgba,
                          uint32_t* out_bgra8, uint8_t* out_trim)
{
    return guarded([&] {
        require(buckets, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        require(K % 2u == 1u && K >= 3u && K <= 15u, "K must be odd with 3 <= K <= 15");
        require(samples >= K, "every bucket needs a sample: the sample count must be >= K");
        require(std::isfinite(exposure), "exposure must be finite");
        rf::robustMeanImages(device_ordinal, width, height, K, samples, buckets, exposure, out_rgba, out_bgra8, out_trim);
        return RF_OK;
    });
}

int rf_robust_mean_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t K, const uint32_t* tile_samples, const float* buckets, float exposure,
                         float* out_rgba, uint32_t* out_bgra8, uint8_t* out_trim)
{
    return guarded([&] {
        require(buckets && tile_samples, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        require(K % 2u == 1u && K >= 3u && K <= 15u, "K must be odd with 3 <= K <= 15");
        (void)requireTileSamples(tile_samples, width, height, K, "every bucket of every tile needs a sample: every tile count must be >= K");
        require(std::isfinite(exposure), "exposure must be finite");
        rf::robustMeanTiles(device_ordinal, width, height, K, tile_samples, buckets, exposure, out_rgba, out_bgra8, out_trim);
        return RF_OK;
    });
}

int rf_renderer_denoise_robust(rf_renderer* r, const rf_denoise_parameters* params)
{
    return guarded([&] {
        const rf::DenoiseParameters p = toDenoiseParams(params);
        require(r, "null argument");
        r->impl->denoiseRobust(p);
        return RF_OK;
    });
}

int rf_temporal_default_parameters(rf_temporal_parameters* params)
{
    return guarded([&] {
        require(params, "null argument");
        const rf::TemporalParameters d;
        *params = rf_temporal_parameters{d.maxHistory, d.depthTolerance, d.minNormalDot, 0u};
        return RF_OK;
    });
}

int rf_renderer_temporal_accumulate(rf_renderer* r, const rf_temporal_parameters* params)
{
    return guarded([&] {
        require(r, "null argument");
        const rf::TemporalParameters p = toTemporalParams(params);
        r->impl->temporalAccumulate(p);
        return RF_OK;
    });
}

int rf_renderer_temporal_commit(rf_renderer* r)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->temporalCommit();
        return RF_OK;
    });
}

int rf_renderer_temporal_reset(rf_renderer* r)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->temporalReset();
        return RF_OK;
    });
}

int rf_renderer_read_temporal(rf_renderer* r, float* rgba, uint32_t* bgra8, float* geometry, uint32_t* sample_count)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->readTemporal(rgba, bgra8, geometry, sample_count);
        return RF_OK;
    });
}

int rf_renderer_denoise_temporal(rf_renderer* r, const rf_temporal_parameters* tparams, const rf_denoise_parameters* dparams)
{
    return guarded([&] {
        require(r, "null argument");
        const rf::TemporalParameters tp = toTemporalParams(tparams);
        const rf::DenoiseParameters  dp = toDenoiseParams(dparams);
        r->impl->denoiseTemporal(tp, dp);
        return RF_OK;
    });
}

int rf_temporal_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* albedo_coverage4,
                       const float* normal_depth4, const rf_camera* camera, const float* history_color4, const float* history_geometry4, const rf_camera* history_camera,
                       const rf_temporal_parameters* params, float exposure, float* out_color4, float* out_geometry4, uint32_t* out_bgra8)
{
    return guarded([&] {
        const rf::TemporalParameters p = toTemporalParams(params);
        require(color_sum4 && albedo_coverage4 && normal_depth4 && camera, "null argument");
        const int given = (history_color4 ? 1 : 0) + (history_geometry4 ? 1 : 0) + (history_camera ? 1 : 0);
        require(given == 0 || given == 3, "the history is given whole or not at all: history_color4, history_geometry4 and history_camera are all NULL or all set");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        require(samples > 0, "sample count must be > 0");
        require(std::isfinite(exposure), "exposure must be finite");
        const rf::Camera cam = toCamera(*camera), old = history_camera ? toCamera(*history_camera) : cam;
        rf::temporalImages(device_ordinal, width, height, samples, color_sum4, albedo_coverage4, normal_depth4, cam, history_color4, history_geometry4,
                           history_camera ? &old : nullptr, p, exposure, out_color4, out_geometry4, out_bgra8);
        return RF_OK;
    });
}

int rf_renderer_noise_estimate(rf_renderer* r, rf_noise_estimate* out, float* error_map, float* tile_sum, float* tile_max)
{
    return guarded([&] {
        require(r && out, "null argument");
        *out = toNoiseEstimate(r->impl->noiseEstimate(error_map, tile_sum, tile_max));
        return RF_OK;
    });
}

int rf_noise_estimate_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* sumsq4, rf_noise_estimate* out,
                             float* error_map, float* tile_sum, float* tile_max)
{
    return guarded([&] {
        require(color_sum4 && sumsq4 && out, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        require(samples >= 2, "a variance needs a sample count >= 2");
        *out = toNoiseEstimate(rf::noiseEstimateImages(device_ordinal, width, height, samples, color_sum4, sumsq4, error_map, tile_sum, tile_max));
        return RF_OK;
    });
}

int rf_renderer_render_until(rf_renderer* r, float target_mean_error, uint32_t check_every, uint32_t max_frames, uint32_t* frames_rendered, rf_noise_estimate* last)
{
    return guarded([&] {
        require(r, "null argument");
        rf::NoiseEstimate e;
        const uint32_t    frames = r->impl->renderUntil(target_mean_error, check_every, max_frames, &e);
        if (frames_rendered) *frames_rendered = frames;
        if (last) *last = toNoiseEstimate(e);
        return RF_OK;
    });
}

int rf_renderer_render_adaptive(rf_renderer* r, const rf_adaptive_parameters* params, rf_adaptive_result* result)
{
    return guarded([&] {
        require(r && params, "null argument");
        const rf::AdaptiveResult a = r->impl->renderAdaptive(toAdaptiveParams(*params));
        if (result) *result = toAdaptiveResult(a);
        return RF_OK;
    });
}

int rf_renderer_read_tile_samples(rf_renderer* r, uint32_t* tile_samples, uint32_t* num_tiles)
{
    return guarded([&] {
        require(r && num_tiles, "null argument");
        *num_tiles = r->impl->readTileSamples(tile_samples);
        return RF_OK;
    });
}

int rf_renderer_read_mean(rf_renderer* r, float* rgba)
{
    return guarded([&] {
        require(r && rgba, "null argument");
        r->impl->readMean(rgba);
        return RF_OK;
    });
}

int rf_noise_estimate_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, const uint32_t* tile_samples, const float* color_sum4, const float* sumsq4,
                            rf_noise_estimate* out, float* error_map, float* tile_sum, float* tile_max)
{
    return guarded([&] {
        require(tile_samples && color_sum4 && sumsq4 && out, "null argument");
        require(width > 0 && height > 0, "image size must be non-zero");
        require(static_cast<uint64_t>(width) * height < (1ull << 31), "image too large");
        const uint32_t leading = requireTileSamples(tile_samples, width, height, 2u, "a variance needs a sample count >= 2 in every tile");
        *out = toNoiseEstimate(rf::noiseEstimateTiles(device_ordinal, width, height, tile_samples, leading, color_sum4, sumsq4, error_map, tile_sum, tile_max));
        return RF_OK;
    });
}

int rf_renderer_set_counting(rf_renderer* r, int enabled)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->setCounting(enabled != 0);
        return RF_OK;
    });
}

int rf_renderer_set_option(rf_renderer* r, const char* name, int64_t value)
{
    return guarded([&] {
        require(r && name, "null argument");
        r->impl->setOption(name, value);
        return RF_OK;
    });
}

int rf_renderer_set_timing(rf_renderer* r, int enabled)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->setTiming(enabled != 0);
        return RF_OK;
    });
}

int rf_renderer_reset_stats(rf_renderer* r)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->resetStats();
        return RF_OK;
    });
}

int rf_renderer_get_bounce_stats(rf_renderer* r, uint32_t capacity, uint64_t* closest_rays, uint64_t* shadow_rays, double* ms_closest,
                                 double* ms_shadow, uint32_t* num_bounces)
{
    return guarded([&] {
        require(r != nullptr, "null argument");
        const rf::RenderStats s = r->impl->stats();
        const uint32_t        n = std::min<uint32_t>(r->impl->numBounces(), rf::RenderStats::kMaxBounceStats);
        if (num_bounces) *num_bounces = n;
        for (uint32_t b = 0; b < capacity; ++b)
        {
            const bool in = b < rf::RenderStats::kMaxBounceStats;
            if (closest_rays) closest_rays[b] = in ? s.closestRaysByBounce[b] : 0;
            if (shadow_rays) shadow_rays[b] = in ? s.shadowRaysByBounce[b] : 0;
            if (ms_closest) ms_closest[b] = in ? s.msClosestByBounce[b] : 0.0;
            if (ms_shadow) ms_shadow[b] = in ? s.msShadowByBounce[b] : 0.0;
        }
        return RF_OK;
    });
}

int rf_renderer_get_stats(rf_renderer* r, rf_stats* out)
{
    return guarded([&] {
        require(r && out, "null argument");
        const rf::RenderStats s = r->impl->stats();
        std::memset(out, 0, sizeof *out);
        out->primary_rays = s.primaryRays;
        out->closest_rays = s.closestRays;
        out->shadow_rays = s.shadowRays;
        out->closest_node_visits = s.closestNodeVisits;
        out->closest_triangle_tests = s.closestTriangleTests;
        out->shadow_node_visits = s.shadowNodeVisits;
        out->shadow_triangle_tests = s.shadowTriangleTests;
        out->paths = s.paths;
        out->stack_high_water = s.stackHighWater;
        out->batch_samples_used = s.batchSamplesUsed;
        out->batches_traced = s.batchesTraced;
        out->ms_raygen = s.msRaygen;
        out->ms_closest = s.msClosest;
        out->ms_shade = s.msShade;
        out->ms_shadow = s.msShadow;
        out->ms_accumulate = s.msAccumulate;
        out->launches_raygen = s.launchesRaygen;
        out->launches_closest = s.launchesClosest;
        out->launches_shade = s.launchesShade;
        out->launches_shadow = s.launchesShadow;
        out->launches_accumulate = s.launchesAccumulate;
        out->closest_record_fetches = s.closestRecordFetches;
        out->shadow_record_fetches = s.shadowRecordFetches;
        out->abandoned_rays = s.abandonedRays;
        out->scalar_redo_rays = s.scalarRedoRays;
        out->shadow_rays_hint_answered = s.shadowRaysHintAnswered;
        out->shadow_rays_self_answered = s.shadowRaysSelfAnswered;
        out->primary_list_rays = s.primaryListRays;
        out->primary_fallback_rays = s.primaryFallbackRays;
        out->primary_fused_rays = s.primaryFusedRays;
        return RF_OK;
    });
}

int rf_renderer_set_tile_shard(rf_renderer* r, uint32_t rank, uint32_t world_size)
{
    return guarded([&] {
        require(r, "null argument");
        require(world_size > 0 && rank < world_size, "invalid rank / world size");
        r->impl->setTileShard(rank, world_size);
        return RF_OK;
    });
}

int rf_renderer_shard_tiles(rf_renderer* r, uint32_t* tile_ids, uint32_t* num_tiles)
{
    return guarded([&] {
        require(r && num_tiles, "null argument");
        const auto tiles = r->impl->shardTiles();
        *num_tiles = static_cast<uint32_t>(tiles.size());
        if (tile_ids) std::memcpy(tile_ids, tiles.data(), tiles.size() * sizeof(uint32_t));
        return RF_OK;
    });
}

int rf_renderer_accumulation_device_buffer(rf_renderer* r, void** device_ptr, uint64_t* bytes)
{
    return guarded([&] {
        require(r && device_ptr && bytes, "null argument");
        *device_ptr = r->impl->accumulationDevicePointer();
        *bytes = r->impl->accumulationBytes();
        return RF_OK;
    });
}

int rf_renderer_bind_accumulation_buffer(rf_renderer* r, void* device_ptr, uint64_t bytes)
{
    return guarded([&] {
        require(r, "null argument");
        r->impl->bindAccumulationBuffer(device_ptr, bytes);
        return RF_OK;
    });
}

// ---------------------------------------------------------------------------------------- state digest and checkpoints
int rf_renderer_state_digest(rf_renderer* r, rf_state_digest* out)
{
    return guarded([&] {
        require(r && out, "null argument");
        const rf::StateDigest d = rf::stateDigest(*r->impl);
        *out = rf_state_digest{};
        out->accumulation = d.plane[0], out->albedo_coverage = d.plane[1], out->normal_depth = d.plane[2], out->moments = d.plane[3], out->direct = d.plane[4];
        for (uint32_t b = 0; b < 15; ++b) out->bucket[b] = d.plane[5 + b];
        out->counts = d.counts;
        for (uint32_t f = 0; f < 5; ++f) out->family_on[f] = d.familyOn[f], out->family_samples[f] = d.familySamples[f];
        out->frame_count = d.frameCount, out->accumulated = d.accumulated, out->num_tiles = d.numTiles;
        out->aov_flags = d.aovFlags, out->moments_on = d.moments, out->direct_word = d.directWord, out->buckets_word = d.bucketsWord;
        out->kernel_ms = d.kernelMs;
        return RF_OK;
    });
}

int rf_renderer_save_checkpoint(rf_renderer* r, void* dst, uint64_t* bytes)
{
    return guarded([&] {
        require(r && bytes, "null argument");
        rf::saveCheckpoint(*r->impl, dst, bytes);
        return RF_OK;
    });
}

int rf_checkpoint_info(const void* blob, uint64_t bytes, struct rf_checkpoint_info* out)
{
    return guarded([&] {
        require(blob && out, "null argument");
        const rf::ckpt::View    v = rf::ckpt::parse(blob, bytes);
        const rf::ckpt::Header& h = v.header;
        std::memset(out, 0, sizeof *out);
        out->version = h.version, out->width = h.width, out->height = h.height, out->num_tiles = h.numTiles, out->frame_count = h.frameCount, out->accumulated = h.accumulated;
        out->frame_leading_samples = h.frameLeadingSamples, out->frame_min_tile_samples = h.frameMinTileSamples;
        out->aov_flags = h.aovFlags, out->moments_on = h.moments, out->direct_word = h.directWord, out->buckets_word = h.bucketsWord;
        for (uint32_t f = 0; f < 5; ++f) out->family_samples[f] = h.family[f].samples, out->family_restarted[f] = h.family[f].restarted;
        out->num_bounces = h.numBounces, out->stored_planes = v.numPlanes, out->total_bytes = h.totalBytes;
        static_assert(sizeof out->camera == sizeof h.camera && sizeof out->sky == sizeof h.sky);
        std::memcpy(&out->camera, h.camera, sizeof h.camera);
        std::memcpy(&out->sky, h.sky, sizeof h.sky);
        return RF_OK;
    });
}

int rf_renderer_load_checkpoint(rf_renderer* r, const void* const* blobs, const uint64_t* sizes, uint32_t count)
{
    return guarded([&] {
        require(r && blobs && sizes && count > 0, "null argument");
        for (uint32_t i = 0; i < count; ++i) require(blobs[i] != nullptr, "null blob");
        rf::loadCheckpoint(*r->impl, blobs, sizes, count);
        return RF_OK;
    });
}

int rf_device_count(int32_t* count_out)
{
    return guarded([&] {
        require(count_out, "null argument");
        *count_out = rf::deviceCount();
        return RF_OK;
    });
}

int rf_comm_unique_id(uint8_t id_out[RF_COMM_ID_BYTES])
{
    return guarded([&] {
        require(id_out, "null argument");
        rf::TileComm::uniqueId(id_out);
        return RF_OK;
    });
}

int rf_comm_create(const uint8_t id[RF_COMM_ID_BYTES], uint32_t rank, uint32_t world_size, int32_t device_ordinal, rf_comm** out)
{
    return guarded([&] {
        require(id && out, "null argument");
        require(world_size > 0 && rank < world_size, "invalid rank / world size");
        auto h = std::make_unique<rf_comm>();
        h->impl = std::make_unique<rf::TileComm>(id, rank, world_size, device_ordinal);
        *out = h.release();
        return RF_OK;
    });
}

void rf_comm_destroy(rf_comm* c) { delete c; }

int rf_renderer_gather_frame(rf_renderer* r, rf_comm* c, uint32_t root, uint32_t flags, void** image_device_out)
{
    return guarded([&] {
        require(r && c, "null argument");
        const void* image = rf::gatherFrame(*r->impl, *c->impl, root, flags);
        if (image_device_out) *image_device_out = const_cast<void*>(image);
        return RF_OK;
    });
}

int rf_renderer_tonemap_device_image(rf_renderer* r, const void* image_device, uint64_t num_pixels, uint32_t samples, uint32_t* dst)
{
    return guarded([&] {
        require(r && image_device && dst, "null argument");
        require(samples > 0, "samples must be > 0");
        r->impl->tonemapDeviceImage(image_device, num_pixels, samples, dst);
        return RF_OK;
    });
}

int rf_comm_read_frame(rf_comm* c, rf_renderer* r, float* dst)
{
    return guarded([&] {
        require(c && r && dst, "null argument");
        c->impl->readFrame(dst, r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_gathered_planes(const rf_comm* c, uint32_t* flags_out, uint32_t* width, uint32_t* height, uint32_t* samples)
{
    return guarded([&] {
        require(c, "null argument");
        uint32_t mask = 0, w = 0, h = 0, n = 0;
        c->impl->gatheredPlanes(mask, w, h, n);
        if (flags_out) *flags_out = ((mask & rf::kPlaneMaskAovs) == rf::kPlaneMaskAovs ? RF_GATHER_AOVS : 0u) | ((mask & rf::kPlaneMaskMoments) ? RF_GATHER_MOMENTS : 0u) |
                                        ((mask & rf::kGatherMaskTileCounts) ? RF_GATHER_TILE_COUNTS : 0u) | ((mask & rf::kPlaneMaskRobustMean) ? RF_GATHER_ROBUST_MEAN : 0u) |
                                        ((mask & rf::kPlaneMaskDirect) ? RF_GATHER_DIRECT : 0u);
        if (width) *width = w;
        if (height) *height = h;
        if (samples) *samples = n;
        return RF_OK;
    });
}

int rf_comm_read_plane(rf_comm* c, rf_renderer* r, uint32_t plane, float* dst)
{
    return guarded([&] {
        require(c && r && dst, "null argument");
        c->impl->readPlane(plane, dst, r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_plane_device(rf_comm* c, uint32_t plane, void** device_ptr)
{
    return guarded([&] {
        require(c && device_ptr, "null argument");
        *device_ptr = const_cast<void*>(c->impl->planeDevice(plane));
        return RF_OK;
    });
}

int rf_comm_denoise(rf_comm* c, rf_renderer* r, const rf_denoise_parameters* params)
{
    return guarded([&] {
        const rf::DenoiseParameters p = toDenoiseParams(params);
        require(c && r, "null argument");
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        c->impl->denoise(p, r->impl->exposure(), r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_read_denoised(rf_comm* c, rf_renderer* r, float* rgba, uint32_t* bgra8, uint32_t* sample_count)
{
    return guarded([&] {
        require(c && r, "null argument");
        c->impl->readDenoised(rgba, bgra8, sample_count, r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_noise_estimate(rf_comm* c, rf_renderer* r, rf_noise_estimate* out, float* error_map, float* tile_sum, float* tile_max)
{
    return guarded([&] {
        require(c && r && out, "null argument");
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        *out = toNoiseEstimate(c->impl->noiseEstimate(error_map, tile_sum, tile_max, r->impl->streamHandle()));
        return RF_OK;
    });
}

int rf_comm_read_tile_samples(rf_comm* c, uint32_t* tile_samples, uint32_t* num_tiles)
{
    return guarded([&] {
        require(c && num_tiles, "null argument");
        *num_tiles = c->impl->readTileSamples(tile_samples);
        return RF_OK;
    });
}

int rf_comm_read_mean(rf_comm* c, rf_renderer* r, float* rgba)
{
    return guarded([&] {
        require(c && r && rgba, "null argument");
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        c->impl->readMean(rgba, r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_read_robust_mean(rf_comm* c, rf_renderer* r, float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* K, uint32_t* sample_count)
{
    return guarded([&] {
        require(c && r, "null argument");
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        c->impl->readRobustMean(rgba, bgra8, trim, K, sample_count, r->impl->exposure(), r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_denoise_robust(rf_comm* c, rf_renderer* r, const rf_denoise_parameters* params)
{
    return guarded([&] {
        const rf::DenoiseParameters p = toDenoiseParams(params);
        require(c && r, "null argument");
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        c->impl->denoiseRobust(p, r->impl->exposure(), r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_denoise_split(rf_comm* c, rf_renderer* r, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect)
{
    return guarded([&] {
        const rf::SplitDenoiseDefaults d = rf::splitDenoiseDefaults();
        const rf::DenoiseParameters    pd = toSplitParams(direct, d.direct), pi = toSplitParams(indirect, d.indirect);
        require(c && r, "null argument");
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        c->impl->denoiseSplit(pd, pi, r->impl->exposure(), r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_read_split(rf_comm* c, rf_renderer* r, float* direct_rgba, float* indirect_rgba)
{
    return guarded([&] {
        require(c && r && (direct_rgba || indirect_rgba), "null argument");
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        c->impl->readSplit(direct_rgba, indirect_rgba, r->impl->streamHandle());
        return RF_OK;
    });
}

int rf_comm_export_features(rf_comm* c, rf_renderer* r, const rf_feature_request* req, void* dst_device, uint64_t dst_bytes, uint32_t* sample_count)
{
    return guarded([&] {
        require(c && r && req && dst_device, "null argument");
        const rf::FeatureRequest request = toFeatureRequest(req);
        require(r->impl->deviceOrdinal() == c->impl->deviceOrdinal(), "the renderer and the communicator are on different devices");
        const uint32_t samples = c->impl->exportFeatures(request, dst_device, dst_bytes, r->impl->streamHandle());
        if (sample_count) *sample_count = samples;
        return RF_OK;
    });
}

int rf_comm_render_adaptive(rf_comm* c, rf_renderer* r, const rf_adaptive_parameters* params, rf_comm_adaptive_result* result)
{
    return guarded([&] {
        require(c && r && params, "null argument");
        const rf::ShardedAdaptiveResult f = rf::renderAdaptive(*r->impl, *c->impl, toAdaptiveParams(*params));
        if (result) *result = rf_comm_adaptive_result{toAdaptiveResult(f.rank), f.frameLeadingSamples, f.frameMinTileSamples, f.maxRankPixelSamples};
        return RF_OK;
    });
}

int rf_comm_all_reduce_max(rf_comm* c, rf_renderer* r, double* value)
{
    return guarded([&] {
        require(c && value, "null argument");
        *value = c->impl->allReduceMax(*value, r ? r->impl->streamHandle() : nullptr);
        return RF_OK;
    });
}

namespace
{
rf::TriangleSpan triangleSpan(const void* positions, uint32_t stride, uint64_t count)
{
    require(stride == 36 || stride == 48, "position_stride_bytes must be 36 (Positions) or 48 (PositionAttribute)");
    require(positions != nullptr || count == 0, "null triangle array");
    return rf::TriangleSpan{static_cast<const uint8_t*>(positions), count, stride};
}
} // namespace

int rf_intersect_bvh(const float ray6[6], const void* nodes48, uint64_t num_nodes, const void* positions, uint32_t position_stride_bytes, uint64_t num_triangles,
                     float t_max, rf_intersection* out, rf_bvh_stats* stats, int* hit_out)
{
    return guarded([&] {
        require(ray6 && nodes48 && out && hit_out, "null argument");
        require(num_nodes > 0, "scene has no BVH nodes");
        static_assert(sizeof(rf_intersection) == sizeof(rf::HostIntersection) && sizeof(rf_bvh_stats) == sizeof(rf::HostBvhStats));
        rf::HostIntersection h{};
        rf::HostBvhStats     st{};
        const bool           hit = rf::intersectBvh(rf::vec3(ray6[0], ray6[1], ray6[2]), rf::vec3(ray6[3], ray6[4], ray6[5]),
                                                    std::span<const rf::BvhNode>(static_cast<const rf::BvhNode*>(nodes48), num_nodes),
                                                    triangleSpan(positions, position_stride_bytes, num_triangles), t_max, h, &st);
        std::memcpy(out, &h, sizeof h);
        if (stats) std::memcpy(stats, &st, sizeof st);
        *hit_out = hit ? 1 : 0;
        return RF_OK;
    });
}

int rf_intersect_bvh_batch(const float* rays6, uint64_t num_rays, const void* nodes48, uint64_t num_nodes, const void* positions, uint32_t position_stride_bytes,
                           uint64_t num_triangles, float t_max, uint32_t num_threads, uint8_t* hit, rf_intersection* out, rf_bvh_stats* stats)
{
    return guarded([&] {
        require((rays6 || num_rays == 0) && nodes48, "null argument");
        require(num_nodes > 0, "scene has no BVH nodes");
        rf::intersectBvhBatch(rays6, num_rays, std::span<const rf::BvhNode>(static_cast<const rf::BvhNode*>(nodes48), num_nodes),
                              triangleSpan(positions, position_stride_bytes, num_triangles), t_max, num_threads, hit, reinterpret_cast<rf::HostIntersection*>(out),
                              reinterpret_cast<rf::HostBvhStats*>(stats));
        return RF_OK;
    });
}

int rf_bvh_visualizer_pass(const rf_camera* camera, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, const void* nodes48, uint64_t num_nodes,
                           const void* positions, uint32_t position_stride_bytes, uint64_t num_triangles, uint32_t num_threads, uint32_t* nodes_visited, uint8_t* hit,
                           float* t, uint32_t* triangle_tests)
{
    return guarded([&] {
        require(camera && nodes48, "null argument");
        require(num_nodes > 0, "scene has no BVH nodes");
        require(width > 0 && height > 0, "empty image");
        rf::Camera cam;
        static_assert(sizeof(rf::Camera) == sizeof(rf_camera));
        std::memcpy(&cam, camera, sizeof cam);
        rf::bvhVisualizerPass(cam, width, height, row_begin, row_end, std::span<const rf::BvhNode>(static_cast<const rf::BvhNode*>(nodes48), num_nodes),
                              triangleSpan(positions, position_stride_bytes, num_triangles), num_threads, nodes_visited, hit, t, triangle_tests);
        return RF_OK;
    });
}

int rf_comm_info(const rf_comm* c, uint32_t* rccl_ranks, uint32_t* rccl_rank, int32_t* device_ordinal)
{
    return guarded([&] {
        require(c, "null argument");
        uint32_t count = 0, user = 0;
        int      dev = 0;
        c->impl->rcclInfo(count, user, dev);
        if (rccl_ranks) *rccl_ranks = count;
        if (rccl_rank) *rccl_rank = user;
        if (device_ordinal) *device_ordinal = dev;
        return RF_OK;
    });
}

int rf_comm_transport(const rf_comm* c, uint32_t* local_out)
{
    return guarded([&] {
        require(c && local_out, "null argument");
        *local_out = c->impl->localTransport() ? 1u : 0u;
        return RF_OK;
    });
}

int rf_comm_last_exchange_ms(rf_comm* c, double* ms_out)
{
    return guarded([&] {
        require(c && ms_out, "null argument");
        *ms_out = c->impl->lastExchangeMs();
        return RF_OK;
    });
}

int rf_gather_plan(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t root, uint32_t flags, rf_gather_op* ops, uint32_t* num_ops)
{
    return guarded([&] {
        require(width > 0 && height > 0 && world_size > 0, "empty frame or world");
        require(rank < world_size && root < world_size, "rank / root out of range");
        require(num_ops, "null argument");
        static_assert(sizeof(rf_gather_op) == sizeof(rf::GatherOp));
        const rf::GatherLayout          g = rf::gatherLayout(width, height, world_size);
        const std::vector<rf::GatherOp> plan = rf::gatherPlan(g, world_size, rank, root, (flags & RF_GATHER_LOOPBACK) != 0);
        if (ops)
        {
            require(*num_ops >= plan.size(), "ops array too small");
            std::memcpy(ops, plan.data(), plan.size() * sizeof(rf::GatherOp));
        }
        *num_ops = static_cast<uint32_t>(plan.size());
        return RF_OK;
    });
}

int rf_gather_plan_planes(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t root, uint32_t flags, rf_gather_plane_op* ops, uint32_t* num_ops)
{
    return guarded([&] {
        require(width > 0 && height > 0 && world_size > 0, "empty frame or world");
        require(rank < world_size && root < world_size, "rank / root out of range");
        require(num_ops, "null argument");
        static_assert(sizeof(rf_gather_plane_op) == sizeof(rf::GatherPlaneOp));
        const uint32_t mask = rf::kPlaneMaskImage | ((flags & RF_GATHER_AOVS) ? rf::kPlaneMaskAovs : 0u) | ((flags & RF_GATHER_MOMENTS) ? rf::kPlaneMaskMoments : 0u) |
                              ((flags & RF_GATHER_ROBUST_MEAN) ? rf::kPlaneMaskRobustMean : 0u) | ((flags & RF_GATHER_DIRECT) ? rf::kPlaneMaskDirect : 0u);
        const rf::GatherLayout               g = rf::gatherLayout(width, height, world_size);
        const std::vector<rf::GatherPlaneOp> plan = rf::gatherPlanPlanes(g, world_size, rank, root, (flags & RF_GATHER_LOOPBACK) != 0, mask);
        if (ops)
        {
            require(*num_ops >= plan.size(), "ops array too small");
            std::memcpy(ops, plan.data(), plan.size() * sizeof(rf::GatherPlaneOp));
        }
        *num_ops = static_cast<uint32_t>(plan.size());
        return RF_OK;
    });
}

int rf_gather_plan_counts(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t root, uint32_t flags, rf_gather_op* ops, uint32_t* num_ops)
{
    return guarded([&] {
        require(width > 0 && height > 0 && world_size > 0, "empty frame or world");
        require(rank < world_size && root < world_size, "rank / root out of range");
        require(num_ops, "null argument");
        const rf::GatherLayout          g = rf::gatherLayout(width, height, world_size);
        const std::vector<rf::GatherOp> plan = rf::gatherPlanCounts(g, world_size, rank, root, (flags & RF_GATHER_LOOPBACK) != 0);
        if (ops)
        {
            require(*num_ops >= plan.size(), "ops array too small");
            std::memcpy(ops, plan.data(), plan.size() * sizeof(rf::GatherOp));
        }
        *num_ops = static_cast<uint32_t>(plan.size());
        return RF_OK;
    });
}

int rf_renderer_layout_info(const rf_renderer* r, rf_layout_info* out)
{
    return guarded([&] {
        require(r && out, "null argument");
        uint32_t layouts[48], misc[4];
        float    ratio = 0.0f;
        uint64_t tree = 0;
        r->impl->layoutInfo(layouts, misc, ratio, tree);
        for (int i = 0; i < 16; ++i) out->closest_layout[i] = layouts[i], out->shadow_layout[i] = layouts[16 + i], out->shadow_cached[i] = layouts[32 + i];
        out->occluder_hint_levels = misc[0], out->shadow_first_look_from_bounce = misc[1], out->dense_leaf_min = misc[2], out->legacy_layouts_compiled = misc[3];
        out->quad_half_area_ratio = ratio, out->reserved = 0.0f, out->tree_bytes = tree;
        return RF_OK;
    });
}

int rf_renderer_launch_plan(const rf_renderer* r, uint32_t bounce, uint32_t num_samples, rf_launch_plan* out)
{
    return guarded([&] {
        require(r && out, "null argument");
        r->impl->launchPlan(bounce, num_samples, *out);
        return RF_OK;
    });
}

int rf_renderer_memory_info(const rf_renderer* r, uint64_t* path_state_bytes, uint64_t* paths_allocated, uint64_t* max_paths_per_batch, uint64_t* scene_bytes)
{
    return guarded([&] {
        require(r, "null argument");
        uint64_t a = 0, b = 0, c = 0, d = 0;
        r->impl->memoryInfo(a, b, c, d);
        if (path_state_bytes) *path_state_bytes = a;
        if (paths_allocated) *paths_allocated = b;
        if (max_paths_per_batch) *max_paths_per_batch = c;
        if (scene_bytes) *scene_bytes = d;
        return RF_OK;
    });
}

int rf_gather_layout(uint32_t width, uint32_t height, uint32_t world_size, uint32_t* rank_first_tile, uint32_t* tile_slot, uint32_t* tile_owner)
{
    return guarded([&] {
        require(width > 0 && height > 0 && world_size > 0, "empty frame or world");
        const rf::GatherLayout g = rf::gatherLayout(width, height, world_size);
        if (rank_first_tile) std::memcpy(rank_first_tile, g.rankFirstTile.data(), g.rankFirstTile.size() * sizeof(uint32_t));
        if (tile_slot) std::memcpy(tile_slot, g.tileSlot.data(), g.tileSlot.size() * sizeof(uint32_t));
        if (tile_owner) std::memcpy(tile_owner, g.tileOwner.data(), g.tileOwner.size() * sizeof(uint32_t));
        return RF_OK;
    });
}

int rf_tiles_for_rank(uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size, uint32_t* tile_ids, uint32_t* num_tiles)
{
    return guarded([&] {
        require(num_tiles, "null argument");
        require(world_size > 0 && rank < world_size, "invalid rank / world size");
        const auto tiles = rf::tilesForRank(width, height, rank, world_size);
        *num_tiles = static_cast<uint32_t>(tiles.size());
        if (tile_ids) std::memcpy(tile_ids, tiles.data(), tiles.size() * sizeof(uint32_t));
        return RF_OK;
    });
}

int rf_untile(const float* compact, const uint32_t* tile_ids, uint32_t num_tiles, uint32_t width, uint32_t height, float* image)
{
    return guarded([&] {
        require((compact && tile_ids) || num_tiles == 0, "null argument");
        require(image, "null argument");
        rf::untileHost(compact, tile_ids, num_tiles, width, height, image);
        return RF_OK;
    });
}

// ---------------------------------------------------------------------------------------- queries
int rf_renderer_trace_primary_stats(rf_renderer* r, const rf_camera* camera, uint32_t width, uint32_t height, uint32_t* nodes_visited,
                                    uint8_t* hit, float* t, uint32_t* triangle_tests)
{
    return guarded([&] {
        require(r && camera && nodes_visited, "null argument");
        require(width > 0 && height > 0, "empty image");
        r->impl->tracePrimaryStats(toCamera(*camera), width, height, nodes_visited, hit, t, triangle_tests);
        return RF_OK;
    });
}

int rf_renderer_intersect_rays(rf_renderer* r, const float* rays6, uint64_t num_rays, float t_max, uint32_t* triangle, float* t, float* uv,
                               float* p, uint32_t* nodes_visited, uint32_t* triangle_tests)
{
    return guarded([&] {
        require(r && (num_rays == 0 || (rays6 && triangle)), "null argument");
        r->impl->intersectRays(rays6, num_rays, t_max, triangle, t, uv, p, nodes_visited, triangle_tests);
        return RF_OK;
    });
}

int rf_renderer_occluded_rays(rf_renderer* r, const float* rays6, uint64_t num_rays, float t_max, float* visibility)
{
    return guarded([&] {
        require(r && (num_rays == 0 || (rays6 && visibility)), "null argument");
        r->impl->occludedRays(rays6, num_rays, t_max, visibility);
        return RF_OK;
    });
}

int rf_renderer_cast_rays(rf_renderer* r, const rf_ray_batch* batch)
{
    return guarded([&] {
        require(r && batch, "null argument");
        rf::RayQueryRequest q;
        const auto          address = [](const void* p) { return static_cast<uint64_t>(reinterpret_cast<uintptr_t>(p)); };
        q.origins = address(batch->origins), q.directions = address(batch->directions);
        q.originStride = batch->origin_stride, q.directionStride = batch->direction_stride;
        q.numRays = batch->num_rays, q.tMax = batch->t_max, q.kind = batch->kind;
        q.reserved[0] = batch->reserved[0], q.reserved[1] = batch->reserved[1];
        const void* const outputs[rf::kCastOutputs] = {batch->triangle, batch->t,        batch->bary,   batch->position, batch->geometric_normal,
                                                       batch->normal,   batch->texcoord, batch->albedo, batch->texture,  batch->visibility};
        for (uint32_t i = 0; i < rf::kCastOutputs; ++i) q.outputs[i] = address(outputs[i]);
        r->impl->castRays(q);
        return RF_OK;
    });
}

// ---------------------------------------------------------------------------------------- CPU side
int rf_build_bvh(const float* positions36, uint64_t num_triangles, void* nodes_out, uint64_t* num_nodes_out,
                 uint64_t* triangle_indices_out, int32_t* depth_out)
{
    return guarded([&] {
        require(positions36 && nodes_out && num_nodes_out && triangle_indices_out, "null argument");
        require(num_triangles > 0, "buildBvh needs at least one triangle"); // bvh.cpp:265 asserts
        const rf::Bvh bvh = rf::buildBvh({reinterpret_cast<const rf::Positions*>(positions36), static_cast<size_t>(num_triangles)});
        std::memcpy(nodes_out, bvh.nodes.data(), bvh.nodes.size() * sizeof(rf::BvhNode));
        *num_nodes_out = bvh.nodes.size();
        for (size_t i = 0; i < bvh.triangleIndices.size(); ++i) triangle_indices_out[i] = bvh.triangleIndices[i];
        if (depth_out) *depth_out = bvh.depth;
        return RF_OK;
    });
}

int rf_check_wide_layouts(const void* nodes48, uint64_t num_nodes, uint32_t* flags_out)
{
    return guarded([&] {
        require(nodes48 && flags_out, "null argument");
        std::span<const rf::BvhNode> nodes{static_cast<const rf::BvhNode*>(nodes48), static_cast<size_t>(num_nodes)};
        // (the same structural check rf_renderer_create runs first: the layout builder follows child links blindly)
        rf::validateScene(nodes, static_cast<size_t>(-1), {}, 0);
        *flags_out = rf::checkWideLayouts(nodes);
        return RF_OK;
    });
}

int rf_wide_layout_stats(const void* nodes48, uint64_t num_nodes, uint32_t* flags_out, float* quad_half_area_ratio)
{
    return guarded([&] {
        require(nodes48, "null argument");
        std::span<const rf::BvhNode> nodes{static_cast<const rf::BvhNode*>(nodes48), static_cast<size_t>(num_nodes)};
        rf::validateScene(nodes, static_cast<size_t>(-1), {}, 0);
        float          ratio = 0.0f;
        const uint32_t flags = rf::checkWideLayouts(nodes, &ratio);
        if (flags_out) *flags_out = flags;
        if (quad_half_area_ratio) *quad_half_area_ratio = ratio;
        return RF_OK;
    });
}

int rf_build_bvh_gpu(const float* positions36, uint64_t num_triangles, void* nodes_out, uint64_t* num_nodes_out, uint64_t* triangle_indices_out,
                     int32_t* depth_out, int32_t device_ordinal, float* build_ms_out)
{
    return guarded([&] {
        require(positions36 && nodes_out && num_nodes_out && triangle_indices_out, "null argument");
        require(num_triangles > 0, "buildBvh needs at least one triangle"); // bvh.cpp:265 asserts
        const rf::Bvh bvh = rf::buildBvhGpu({reinterpret_cast<const rf::Positions*>(positions36), static_cast<size_t>(num_triangles)}, device_ordinal,
                                            build_ms_out);
        std::memcpy(nodes_out, bvh.nodes.data(), bvh.nodes.size() * sizeof(rf::BvhNode));
        *num_nodes_out = bvh.nodes.size();
        for (size_t i = 0; i < bvh.triangleIndices.size(); ++i) triangle_indices_out[i] = bvh.triangleIndices[i];
        if (depth_out) *depth_out = bvh.depth;
        return RF_OK;
    });
}

int rf_create_camera(const float origin[3], const float look_at[3], float aperture, float focus_distance, float vfov_radians,
                     float aspect_ratio, rf_camera* out)
{
    return guarded([&] {
        require(origin && look_at && out, "null argument");
        const rf::Camera c = rf::createCamera(v3(origin), v3(look_at), aperture, focus_distance, vfov_radians, aspect_ratio);
        std::memcpy(out, &c, sizeof c);
        return RF_OK;
    });
}

int rf_fly_camera(const float position[3], float yaw_degrees, float pitch_degrees, float vfov_degrees, float aperture, float focus_distance,
                  float aspect_ratio, rf_camera* out)
{
    return guarded([&] {
        require(position && out, "null argument");
        const rf::Camera c = rf::flyCamera(v3(position), yaw_degrees, pitch_degrees, vfov_degrees, aperture, focus_distance, aspect_ratio);
        std::memcpy(out, &c, sizeof c);
        return RF_OK;
    });
}

int rf_bvh_visualizer_camera(const void* root_node48, float aspect_ratio, rf_camera* out)
{
    return guarded([&] {
        require(root_node48 && out, "null argument");
        const rf::Camera c = rf::bvhVisualizerCamera(static_cast<const rf::BvhNode*>(root_node48)->aabb, aspect_ratio);
        std::memcpy(out, &c, sizeof c);
        return RF_OK;
    });
}

int rf_sky_state_new(float elevation, float turbidity, const float albedo[3], float state33[33])
{
    if (!albedo || !state33) return -1;
    return static_cast<int>(rf::skyStateNew(elevation, turbidity, albedo, state33));
}

float rf_sky_state_radiance(const float state33[33], float theta, float gamma, int channel)
{
    return rf::skyStateRadiance(state33, theta, gamma, channel);
}

int rf_aligned_sky_state(const rf_sky* sky, float out40[40])
{
    return guarded([&] {
        require(sky && out40, "null argument");
        rf::Sky s;
        s.turbidity = sky->turbidity;
        std::memcpy(s.albedo, sky->albedo, sizeof s.albedo);
        s.sunZenithDegrees = sky->sun_zenith_degrees;
        s.sunAzimuthDegrees = sky->sun_azimuth_degrees;
        rf::SkyStateGpu g;
        const rf::SkyResult rc = rf::alignedSkyState(s, g);
        std::memcpy(out40, &g, sizeof g);
        if (rc != rf::SkyResult::Success)
        {
            gLastError = "sky parameters out of range";
            return static_cast<int>(RF_ERROR_OUT_OF_RANGE);
        }
        return static_cast<int>(RF_OK);
    });
}

// ---------------------------------------------------------------------------------------- .pt files
int rf_texture_from_memory(const void* data, uint64_t size, uint32_t* width, uint32_t* height, uint32_t* pixels)
{
    return guarded([&] {
        require(data && width && height, "null argument");
        const rf::Texture t = rf::textureFromMemory({static_cast<const uint8_t*>(data), static_cast<size_t>(size)});
        *width = t.width;
        *height = t.height;
        if (pixels) std::memcpy(pixels, t.pixels.data(), t.pixels.size() * sizeof(uint32_t));
        return RF_OK;
    });
}

int rf_pt_format_set_bvh_builder(int32_t gpu_device_or_minus_one)
{
    return guarded([&] {
        rf::setBakeBvhBuilder(gpu_device_or_minus_one);
        return RF_OK;
    });
}

int rf_pt_format_from_gltf(const char* gltf_path, rf_pt_format** out)
{
    return guarded([&] {
        require(gltf_path && out, "null argument");
        auto h = std::make_unique<rf_pt_format>();
        h->format = rf::ptFormatFromGltf(gltf_path);
        *out = h.release();
        return RF_OK;
    });
}

int rf_pt_format_load(const char* pt_path, rf_pt_format** out)
{
    return guarded([&] {
        require(pt_path && out, "null argument");
        auto h = std::make_unique<rf_pt_format>();
        h->format = rf::readPtFile(pt_path);
        *out = h.release();
        return RF_OK;
    });
}

int rf_pt_format_deserialize(const void* data, uint64_t size, rf_pt_format** out)
{
    return guarded([&] {
        require(data && out, "null argument");
        auto h = std::make_unique<rf_pt_format>();
        rf::deserializePt(static_cast<const uint8_t*>(data), static_cast<size_t>(size), h->format);
        *out = h.release();
        return RF_OK;
    });
}

int rf_pt_format_save(const rf_pt_format* f, const char* pt_path)
{
    return guarded([&] {
        require(f && pt_path, "null argument");
        rf::writePtFile(pt_path, f->format);
        return RF_OK;
    });
}

int rf_pt_format_serialize(const rf_pt_format* f, void* dst, uint64_t* size)
{
    return guarded([&] {
        require(f && size, "null argument");
        const std::vector<uint8_t> bytes = rf::serializePt(f->format);
        if (dst)
        {
            require(*size >= bytes.size(), "destination too small");
            std::memcpy(dst, bytes.data(), bytes.size());
        }
        *size = bytes.size();
        return RF_OK;
    });
}

int rf_pt_format_from_triangles(const float* positions36, const float* normals36, const float* tex_coords24, const uint32_t* texture_indices,
                                uint64_t num_triangles, const rf_texture* textures, uint64_t num_textures, rf_pt_format** out)
{
    return guarded([&] {
        require(positions36 && normals36 && tex_coords24 && texture_indices && out, "null argument");
        require(num_triangles > 0, "no triangles");
        const size_t n = static_cast<size_t>(num_triangles);
        std::vector<rf::Texture> tex;
        for (uint64_t i = 0; i < num_textures; ++i)
        {
            rf::Texture t;
            t.width = textures[i].width;
            t.height = textures[i].height;
            t.pixels.assign(textures[i].pixels, textures[i].pixels + static_cast<size_t>(t.width) * t.height);
            tex.push_back(std::move(t));
        }
        auto h = std::make_unique<rf_pt_format>();
        h->format = rf::ptFormatFromTriangles({reinterpret_cast<const rf::Positions*>(positions36), n},
                                              {reinterpret_cast<const rf::Normals*>(normals36), n},
                                              {reinterpret_cast<const rf::TexCoords*>(tex_coords24), n}, {texture_indices, n}, std::move(tex));
        *out = h.release();
        return RF_OK;
    });
}

int rf_pt_format_view_get(const rf_pt_format* f, rf_pt_format_view* v)
{
    return guarded([&] {
        require(f && v, "null argument");
        const rf::PtFormat& p = f->format;
        std::memset(v, 0, sizeof *v);
        v->bvh_nodes = p.bvhNodes.data();
        v->num_bvh_nodes = p.bvhNodes.size();
        v->bvh_position_attributes = p.bvhPositionAttributes.data();
        v->num_bvh_position_attributes = p.bvhPositionAttributes.size();
        v->triangle_position_attributes = p.trianglePositionAttributes.data();
        v->num_triangle_position_attributes = p.trianglePositionAttributes.size();
        v->triangle_vertex_attributes = p.triangleVertexAttributes.data();
        v->num_triangle_vertex_attributes = p.triangleVertexAttributes.size();
        v->vertex_positions = reinterpret_cast<const float*>(p.vertexPositions.data());
        v->num_vertex_positions = p.vertexPositions.size();
        v->vertex_normals = reinterpret_cast<const float*>(p.vertexNormals.data());
        v->num_vertex_normals = p.vertexNormals.size();
        v->vertex_tex_coords = reinterpret_cast<const float*>(p.vertexTexCoords.data());
        v->num_vertex_tex_coords = p.vertexTexCoords.size();
        v->vertex_indices = p.vertexIndices.data();
        v->num_vertex_indices = p.vertexIndices.size();
        static_assert(sizeof(rf::Slice) == 16);
        v->model_vertex_positions = reinterpret_cast<const uint64_t*>(p.modelVertexPositions.data());
        v->num_model_vertex_positions = p.modelVertexPositions.size();
        v->model_vertex_normals = reinterpret_cast<const uint64_t*>(p.modelVertexNormals.data());
        v->num_model_vertex_normals = p.modelVertexNormals.size();
        v->model_vertex_tex_coords = reinterpret_cast<const uint64_t*>(p.modelVertexTexCoords.data());
        v->num_model_vertex_tex_coords = p.modelVertexTexCoords.size();
        v->model_vertex_indices = reinterpret_cast<const uint64_t*>(p.modelVertexIndices.data());
        v->num_model_vertex_indices = p.modelVertexIndices.size();
        v->model_base_color_texture_indices = p.modelBaseColorTextureIndices.data();
        v->num_model_base_color_texture_indices = p.modelBaseColorTextureIndices.size();
        v->num_textures = p.baseColorTextures.size();
        return RF_OK;
    });
}

int rf_pt_format_texture(const rf_pt_format* f, uint64_t index, rf_texture* out)
{
    return guarded([&] {
        require(f && out, "null argument");
        require(index < f->format.baseColorTextures.size(), "texture index out of range");
        const rf::Texture& t = f->format.baseColorTextures[static_cast<size_t>(index)];
        out->pixels = t.pixels.data();
        out->width = t.width;
        out->height = t.height;
        return RF_OK;
    });
}

void rf_pt_format_destroy(rf_pt_format* f) { delete f; }

int rf_pt_format_scene(const rf_pt_format* f, rf_scene* scene, rf_texture* textures)
{
    return guarded([&] {
        require(f && scene, "null argument");
        const rf::PtFormat& p = f->format;
        require(textures || p.baseColorTextures.empty(), "null texture array");
        require(p.trianglePositionAttributes.size() == p.triangleVertexAttributes.size(), "attribute arrays differ in length");
        scene->bvh_nodes = p.bvhNodes.data();
        scene->num_bvh_nodes = p.bvhNodes.size();
        scene->position_attributes = p.trianglePositionAttributes.data();
        scene->vertex_attributes = p.triangleVertexAttributes.data();
        scene->num_triangles = p.trianglePositionAttributes.size();
        for (size_t i = 0; i < p.baseColorTextures.size(); ++i)
            require(p.baseColorTextures[i].pixels.size() == static_cast<size_t>(p.baseColorTextures[i].width) * p.baseColorTextures[i].height,
                    "texture pixel count differs from width * height");
        for (size_t i = 0; i < p.baseColorTextures.size(); ++i)
            textures[i] = rf_texture{p.baseColorTextures[i].pixels.data(), p.baseColorTextures[i].width, p.baseColorTextures[i].height};
        scene->base_color_textures = textures;
        scene->num_textures = p.baseColorTextures.size();
        return RF_OK;
    });
}
} // extern "C"
