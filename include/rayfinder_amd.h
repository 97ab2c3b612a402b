/*
 * rayfinder_amd.h -- C ABI of the MI355X-native path-tracing core (librayfinder_amd.so).
 *
 * This is the drop-in boundary for rayfinder's hot path.  The reference (Nelarius/rayfinder) has
 * no FFI layer; its path sits behind three C++ seams.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference repo).  Plain pointers and sizes only;
 * every call returns RF_OK (0) or an error code instead of throwing -- rf_last_error_message()
 * returns the text the reference would have put into its std::runtime_error.  One handle is used
 * from one host thread at a time (as in the reference, whose renderer lives on the GLFW thread).
 *
 * Record layouts are the reference's, byte for byte:
 *   BvhNode 48 B (src/common/bvh.hpp:14-21), Positions 36 B (src/common/triangle_attributes.hpp:7-12),
 *   PositionAttribute 48 B / VertexAttributes 80 B (src/pt-format/vertex_attributes.hpp:7-35),
 *   texture pixels u32 BGRA (src/common/texture.cpp:46), AlignedSkyState 160 B
 *   (src/pt/aligned_sky_state.hpp:34-41).
 */
#ifndef RAYFINDER_AMD_H
#define RAYFINDER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_API __attribute__((visibility("default")))

typedef enum rf_status
{
    RF_OK = 0,
    RF_ERROR_INVALID_ARGUMENT = 1,
    RF_ERROR_RUNTIME = 2,      /* what the reference reports with std::runtime_error */
    RF_ERROR_NO_DEVICE = 3,    /* no HIP device: this library has NO CPU fallback for rendering */
    RF_ERROR_OUT_OF_RANGE = 4, /* sky parameters out of range (sky_state_result != success) */
    RF_ERROR_CORRUPT = 5,      /* rf_renderer_load_checkpoint: what the copies left in device memory does not digest to what the blob stores */
} rf_status;

/* Text of the last error on the calling thread ("" if none). */
RF_API const char* rf_last_error_message(void);
RF_API const char* rf_version(void);

/* ---------------------------------------------------------------------------------------------
 * Value types
 * ------------------------------------------------------------------------------------------ */
/* nlrs::Camera, src/common/camera.hpp:10-21 (19 floats). */
typedef struct rf_camera
{
    float origin[3];
    float lower_left_corner[3];
    float horizontal[3];
    float vertical[3];
    float up[3];
    float right[3];
    float lens_radius;
} rf_camera;

/* nlrs::Sky, src/pt/aligned_sky_state.hpp:15-23. */
typedef struct rf_sky
{
    float turbidity;          /* [1, 10] */
    float albedo[3];          /* [0, 1] */
    float sun_zenith_degrees; /* [0, 90] */
    float sun_azimuth_degrees;
} rf_sky;

/* nlrs::RenderParameters + SamplingParams, src/pt/reference_path_tracer.hpp:26-43. */
typedef struct rf_render_parameters
{
    uint32_t  width, height;          /* framebufferSize */
    rf_camera camera;
    uint32_t  num_samples_per_pixel;  /* default 128 */
    uint32_t  num_bounces;            /* default 4 */
    rf_sky    sky;
    float     exposure;               /* 1 / 2^stops (src/pt/main.cpp:367) */
} rf_render_parameters;

/* nlrs::Texture as a view, src/common/texture.hpp:10-47. */
typedef struct rf_texture
{
    const uint32_t* pixels; /* width*height BGRA (b | g<<8 | r<<16 | a<<24) */
    uint32_t        width, height;
} rf_texture;

/* nlrs::Scene, src/pt/reference_path_tracer.hpp:45-51: non-owning views; rf_renderer_create
 * copies everything to device memory and keeps nothing from these pointers. */
typedef struct rf_scene
{
    const void*       bvh_nodes;           /* 48-B BvhNode records */
    uint64_t          num_bvh_nodes;
    const void*       position_attributes; /* 48-B PositionAttribute records, BVH leaf order */
    const void*       vertex_attributes;   /* 80-B VertexAttributes records, same order */
    uint64_t          num_triangles;
    const rf_texture* base_color_textures;
    uint64_t          num_textures;
} rf_scene;

/* nlrs::RendererDescriptor, src/pt/reference_path_tracer.hpp:53-57, plus device placement. */
typedef struct rf_renderer_descriptor
{
    rf_render_parameters render_params;
    uint32_t             max_width, max_height; /* maxFramebufferSize; 0 = render_params size */
    int32_t              device_ordinal;
    uint64_t             max_paths_in_flight;   /* batch depth; 0 = default (1 Gi paths).  Default or chosen, a render() call whose batches do not fit the device memory
                                                   free at that moment traces the same samples in shallower batches (same image; said on stderr; the configured depth is
                                                   used again once the memory is back).  Path state is allocated on demand: samples x pixels x 148 B */
} rf_renderer_descriptor;

typedef struct rf_stats
{
    uint64_t primary_rays, closest_rays, shadow_rays;
    uint64_t closest_node_visits, closest_triangle_tests; /* only while counting is enabled */
    uint64_t shadow_node_visits, shadow_triangle_tests;
    uint64_t paths;
    uint32_t stack_high_water;
    uint32_t batch_samples_used; /* samples per pixel traced together in the MOST RECENT batch (x the shard's padded pixel count = the batch depth in paths, see
                                  * rf_renderer_memory_info).  Less than asked for when device memory was short at that moment: same image, shallower batches, shorter launches */
    double   ms_raygen, ms_closest, ms_shade, ms_shadow, ms_accumulate; /* while timing is enabled */
    uint32_t launches_raygen, launches_closest, launches_shade, launches_shadow, launches_accumulate;
    uint32_t batches_traced; /* batches since the last reset */
    uint64_t closest_record_fetches, shadow_record_fetches; /* 64-byte BVH records fetched (counting build) */
    /* Always counted.  abandoned_rays: traversals that needed more than 96 stack entries and were cut short (the
     * reference's 32-entry stack, ray_intersection.cpp:148,194 / wgsl:327,375, is overrun long before: undefined
     * there); 0 on every scene tested.  scalar_redo_rays: rays the packed traversal handed to the reference-ordered
     * scalar one (axis-parallel / non-finite rays, origins outside the conservative records' bound, more than 48 pending
     * entries: a full 12-entry LDS stack first evicts its oldest entries to scratch) -- results are identical. */
    uint64_t abandoned_rays, scalar_redo_rays;
    /* Of shadow_rays: rays whose occluder was found by the any-hit launch's first look (kShadowFirstLook: the leaves that stopped the last shadow rays
     * from the same cell of the scene, tested with the reference's box and triangle arithmetic) and that therefore never entered the BVH walk.
     * Same visibility bit; reported so that a rays-per-second figure can be read with and without them. */
    uint64_t shadow_rays_hint_answered;
    /* Of shadow_rays: rays stopped by the very triangle they start on -- the reference pushes the hit point off the surface along the GEOMETRIC normal whatever side the
     * path came from (wgsl:511-519), so wherever the sun stands behind that normal shadowRay (wgsl:321-368) finds the surface itself.  The shading stage tests exactly that
     * (the leaf's exact box, then the triangle, with the reference's arithmetic) and such a ray is never queued for an any-hit launch.  Same visibility bit. */
    uint64_t shadow_rays_self_answered;
    /* Bounce 1 over per-pixel leaf lists (option primary_lists, default on).  Under a pinhole camera all samples of a pixel share one origin and a pixel-sized bundle of
     * directions; a batch with enough samples per pixel walks the tree ONCE per pixel (interval slab tests over the pixel's direction box, the reference's visit order) and
     * every sample then tests only the exact boxes and the triangles of the few leaves on its pixel's list -- same hits bit for bit.  primary_list_rays: bounce-1 rays of the
     * batches that did so (0: a thin-lens camera, the option off, a counting build, batches below primary_list_min_samples samples per pixel, a tree whose boxes are not
     * nested).  primary_fallback_rays: of those, rays handed on to the ordinary traversal launch (a pixel whose directions change sign on an axis, whose list would
     * exceed primary_list_capacity entries or holds a leaf of more than 7 triangles; a ray with an infinite 1 / direction component). */
    uint64_t primary_list_rays, primary_fallback_rays;
    /* Of primary_list_rays: rays of the batches whose bounce 1 ran as ONE kernel per path (option primary_fused, default on): the lane that generates the ray walks its
     * pixel's list and shades the hit from its registers, so queue entry, direction, hit record and blue-noise triple of a covered ray are never written.  0: the option
     * off, the first-hit AOVs on, or `transcendentals` 1 -- those batches keep the three launches.  Same image bit for bit. */
    uint64_t primary_fused_rays;
} rf_stats;

typedef struct rf_renderer rf_renderer;

/* ---------------------------------------------------------------------------------------------
 * Renderer  (replaces class nlrs::ReferencePathTracer, src/pt/reference_path_tracer.hpp:59-76)
 * ------------------------------------------------------------------------------------------ */
/* ReferencePathTracer(const RendererDescriptor&, const GpuContext&, Scene)
 * (reference_path_tracer.cpp:131-481).  Fails with RF_ERROR_NO_DEVICE when no GPU is present. */
RF_API int rf_renderer_create(const rf_renderer_descriptor* desc, const rf_scene* scene, rf_renderer** out);
RF_API void rf_renderer_destroy(rf_renderer* r);

/* void setRenderParameters(const RenderParameters&) (reference_path_tracer.cpp:556-563):
 * any change resets the accumulation; frameCount keeps counting. */
RF_API int rf_renderer_set_render_parameters(rf_renderer* r, const rf_render_parameters* params);

/* void render(...) called num_frames times (reference_path_tracer.cpp:565-595 + fsMain
 * wgsl:34-57): frame f uses sample index frameCount % spp, adds one sample while fewer than spp
 * are accumulated.  Work is enqueued on the handle's HIP stream; returns without waiting. */
RF_API int rf_renderer_render(rf_renderer* r, uint32_t num_frames);
RF_API int rf_renderer_synchronize(rf_renderer* r);

/* float averageRenderpassDurationMs() const (reference_path_tracer.cpp:706-716): mean GPU time per
 * sample over the last 30 samples. */
RF_API float rf_renderer_average_renderpass_duration_ms(rf_renderer* r);
/* float renderProgressPercentage() const (reference_path_tracer.cpp:718-722). */
RF_API float rf_renderer_render_progress_percentage(const rf_renderer* r);

/* The reference's `imageBuffer` (wgsl:32; never read back there): row-major width*height*4 f32,
 * SUM of samples, 16-byte stride.  This is the parity surface. */
RF_API int rf_renderer_read_accumulation(rf_renderer* r, float* dst, uint32_t* accumulated_sample_count);
/* fsMain's return value (wgsl:59-63) as the BGRA8Unorm swap-chain texel, row-major. */
RF_API int rf_renderer_read_tonemapped(rf_renderer* r, uint32_t* dst_bgra8);

/* First-hit AOVs: the auxiliary buffers a denoiser, a compositor or a debug view wants next to the noisy image (no reference counterpart in the
 * path tracer: nlrs::DeferredRenderer rasterises an albedo / normal / depth G-buffer instead, deferred_renderer_gbuffer_pass.wgsl).
 * For every sample (pixel x, y, frame f) the renderer takes the primary ray it traces anyway -- the thin-lens ray of wgsl:36-54, same blue noise,
 * same origin -- and records at its closest hit:
 *   albedo   the texel value the shading uses for that hit (textureLookup, the linear value after the sRGB table)
 *   normal   normalize(n), n = the interpolated shading normal (wgsl:396), normalize(v) = v * (1 / sqrt(dot(v, v))); (0, 0, 0) where dot(n, n) is 0
 *            or not finite
 *   depth    the hit's t: the distance from the ray's origin (lens offset included) along the unit primary direction
 *   coverage 1
 * and, where the ray leaves the scene, 0 for every value, coverage included.  Per pixel the renderer keeps SUMS in sample order in f32, exactly as the
 * radiance (wgsl:47-57): bit-reproducible whatever the batching, slot order or number of ranks.  Means are the caller's to form: albedo and normal
 * divided by the AOV sample count, depth divided by coverage (where coverage > 0).
 *
 * rf_renderer_set_aovs: flags 0 (the default: nothing is allocated or launched, image / stats / timings exactly as without), RF_AOV_FIRST_HIT, or
 * RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS.  The low byte of the flags says WHICH AOVs are kept, the bits from 8 up HOW they are kept.  RF_AOV_TILE_COUNTS: the sums
 * follow the per-tile sample counts of rf_renderer_render_adaptive (below: after that call the AOV sums of a pixel are those of its tile's first tile_samples[t]
 * samples, as S and Q are), and rf_renderer_denoise then runs in the non-uniform state.  Until rf_renderer_render_adaptive is called, a handle with the bit behaves
 * bit for bit like one with RF_AOV_FIRST_HIT alone: sums, image, stats and launches are the same.  The bit on its own is refused.
 * While on, 32 more bytes per path slot of device memory (rf_renderer_memory_info counts them; a batch that no longer fits gets shallower).
 * The AOV sums keep their own sample count -- the samples traced while the AOVs were on -- and are cleared, with the count set to 0, when the image is
 * (a change through rf_renderer_set_render_parameters, a new tile shard, a newly bound accumulation buffer) and when the flags value changes in any way
 * (RF_AOV_FIRST_HIT <-> RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS included).  Turned on partway through an accumulation, they cover only the later samples: the
 * count stays below the accumulated sample count.
 * rf_renderer_read_aovs: row-major width*height*4 floats each, {albedo.rgb, coverage} and {normal.xyz, depth} sums (the layout of
 * rf_renderer_read_accumulation; either pointer may be NULL) and the AOV sample count.  With a tile shard set, this rank's pixels and zeros elsewhere:
 * the sum of the ranks' reads is the whole frame.  (rf_renderer_gather_frame carries them with RF_GATHER_AOVS: the root then holds the whole frame's AC and ND
 * sums in device memory, rf_comm_read_plane planes 1 and 2.)  In the non-uniform state of
 * rf_renderer_render_adaptive: the sums as they are; the count reported is the AOV sample count -- the leading count L, since the sums cover the accumulation (the
 * call that made the state needs that); 0, with zero sums, once the flags were changed in that state -- and the divisor of a pixel is its tile's own count
 * (rf_renderer_read_tile_samples), as for rf_renderer_read_accumulation and rf_renderer_read_moments.
 * A NULL handle, unknown flag bits or RF_AOV_TILE_COUNTS without RF_AOV_FIRST_HIT: RF_ERROR_INVALID_ARGUMENT, the state kept. */
#define RF_AOV_FIRST_HIT 1u
#define RF_AOV_TILE_COUNTS 0x100u
RF_API int rf_renderer_set_aovs(rf_renderer* r, uint32_t flags);
RF_API int rf_renderer_read_aovs(rf_renderer* r, float* albedo_coverage, float* normal_depth, uint32_t* aov_sample_count);

/* Edge-aware a-trous denoiser (Dammertz et al. 2010, "Edge-avoiding A-Trous wavelet transform for fast global illumination filtering") guided by the
 * first-hit AOVs.  No reference counterpart.  Inputs: the per-pixel sums of one accumulation -- S (rf_renderer_read_accumulation's layout), AC = {albedo.rgb,
 * coverage} and ND = {normal.xyz, depth} (rf_renderer_read_aovs) -- and ONE sample count N that both the accumulation and the AOVs have.
 * All arithmetic is f32, one IEEE operation at a time in the order written (+ - * /, sqrt, compares and selects; no transcendentals): a numpy float32
 * restatement reproduces the result bit for bit.  Nf = float(N), εa = 2^-8, εℓ = 2^-8.
 *   prep, per pixel:  c = S.rgb / Nf per channel (kTonemap's division)
 *                     background: AC.w == 0, or z (below) not > 0 (never from the renderer: a hit's t is > 0).  Output c exactly; never a neighbour.
 *                     otherwise:  a = AC.rgb / Nf;  m = ND.xyz / Nf;  n = normalize(m) = m * (1 / sqrt(dot(m, m))), (0, 0, 0) where dot(m, m) is 0 or not finite;
 *                                 z = ND.w / AC.w;  e = c / (a + εa) per channel (demodulated irradiance);  ℓ = (e.r + e.g) + e.b
 *   iteration i = 0 .. L-1, step s = 2^i, for each non-background pixel p (background pixels keep e):
 *     the 25 taps q = p + s (dx, dy) in row-major order (dy, then dx, each -2 .. 2), skipping taps outside the frame and background taps (no clamping);
 *     h = k[dx] k[dy], k = {1/16, 1/4, 3/8, 1/4, 1/16} (exact);  centre tap: w = h = 9/64;  every other tap: w = ((h T(xc)) T(xn)) T(xz) with
 *       T(x) = x < 1 ? (1 - x)(1 - x) : 0                                     (Tukey's biweight; NaN -> 0)
 *       d = e_q - e_p;  xc = ((d.r d.r + d.g d.g) + d.b d.b) / (σc²_i (ℓ_p ℓ_p + εℓ)),  σc²_i = (σc σc) 2^-i
 *       xn = (1 - ((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)) / σn
 *       xz = |z_q - z_p| / ((σz s) z_p)
 *     in tap order: sumW += w; sumE += w e_q (per channel, both from +0);  e'_p = sumE / sumW;  ℓ'_p = (e'.r + e'.g) + e'.b
 *   finish: out = e^(L) (a + εa) per channel; background out = c;  L = 0: out = c for every pixel.  The mean is returned as {out.rgb, 1}.
 * Parameters: 0 <= iterations <= 8, each sigma finite and > 0; defaults L = 5, σc = 1, σn = 0.1, σz = 0.1 (profiles/denoise/README.md: the sweep).
 * With one sample count per 32x32 tile (a frame of rf_renderer_render_adaptive; rf_denoise_tiles) the definition changes in exactly one place: in prep, Nf of
 * pixel p is float(tile_samples[tile of p]), tile = (y >> 5) ceil(width / 32) + (x >> 5), for c, a and m alike (z = ND.w / AC.w does not involve N).  Everything
 * after prep is as written: the taps cross tile borders freely -- a tile stopped at 4 samples filters against its 32-sample neighbour -- and no term weighs a tap
 * by its count or its variance.  With all counts equal to N the result is bit for bit that of the one-count filter.
 *
 * rf_renderer_denoise: enqueued on the handle's stream over its own sums; params NULL = the defaults.  RF_ERROR_INVALID_ARGUMENT when the AOVs are off,
 * when the AOV sample count differs from the accumulated count (AOVs turned on partway through), when no sample has been accumulated, or when a tile
 * shard is set (rf_renderer_gather_frame carries them with RF_GATHER_AOVS, and rf_comm_denoise then runs this filter on the root over the gathered sums, in
 * device memory; rf_denoise_images does the same from host memory).  In the non-uniform state of
 * rf_renderer_render_adaptive it runs, with each tile's own count in prep, when the AOVs are on with RF_AOV_TILE_COUNTS and their count equals the accumulated
 * (leading) count L -- the snapshot's sample count is then L, and the call is not purely an enqueue: it first waits for the handle's stream and copies the
 * per-tile counts to the device (8 KB at 1080p), as the other per-tile reads do; otherwise it is refused with the non-uniform state's message ("different
 * sample counts"), which comes before the checks above.  Leaves the accumulation, the AOV sums, the tile counts, rf_renderer_read_tonemapped, the stats and
 * later samples untouched.  The result is a snapshot with its sample count: its device buffers (five float4
 * and one u32 per pixel) are allocated by the first call and freed with the handle; the snapshot is dropped whenever the AOV sums are cleared
 * (rf_renderer_set_render_parameters, a change of the AOV flags, a new tile shard, a newly bound accumulation buffer).
 * rf_renderer_read_denoised: row-major width*height*4 mean floats and / or the BGRA8 texels (kTonemap with accumulatedSamples = 1 and the handle's
 * exposure) and the snapshot's sample count; any pointer may be NULL.  RF_ERROR_INVALID_ARGUMENT without a snapshot.
 * rf_denoise_images: the same filter over row-major host sums (width*height*4 floats each, e.g. assembled from several ranks) on device
 * device_ordinal; out_rgba / out_bgra8 may be NULL.  Synchronous.  A NULL input, a zero size or sample count and bad parameters are refused before any
 * device call.
 * rf_denoise_tiles: rf_denoise_images with one count per 32x32 tile: tile_samples holds ceil(width / 32) * ceil(height / 32) words in the estimate's tile numbering
 * (tile_y * ceil(width / 32) + tile_x), exactly as for rf_noise_estimate_tiles.  Synchronous.  A NULL input, a zero size, any tile count of 0 and bad parameters
 * are refused before any device call. */
typedef struct rf_denoise_parameters
{
    uint32_t iterations;
    float    sigma_color, sigma_normal, sigma_depth;
} rf_denoise_parameters;
RF_API int rf_denoise_default_parameters(rf_denoise_parameters* out);
RF_API int rf_renderer_denoise(rf_renderer* r, const rf_denoise_parameters* params);
RF_API int rf_renderer_read_denoised(rf_renderer* r, float* rgba, uint32_t* bgra8, uint32_t* sample_count);
RF_API int rf_denoise_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* albedo_coverage4,
                             const float* normal_depth4, const rf_denoise_parameters* params, float exposure, float* out_rgba, uint32_t* out_bgra8);
RF_API int rf_denoise_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, const uint32_t* tile_samples, const float* color_sum4,
                            const float* albedo_coverage4, const float* normal_depth4, const rf_denoise_parameters* params, float exposure, float* out_rgba,
                            uint32_t* out_bgra8);

/* Direct radiance sums: where the light came from, next to albedo, normal and depth.  No reference counterpart as a buffer; as a value it is the reference's own:
 * what rayColor returns with numBounces = 1 (reference_path_tracer.wgsl:181-234: the primary miss's sky term, or the first hit's sun term times its visibility).
 *
 * rf_renderer_set_direct: 0 (the default: nothing is allocated or launched, image / stats / timings / launch plans exactly as without) or 1.  While on, the handle
 * keeps one more per-pixel f32 buffer next to the accumulation, D = {sum d.x, sum d.y, sum d.z, 0}, where d is the sample's radiance as it stands after bounce 1,
 * added in f32 in sample-index order, one dependent chain per channel, by the kernel that adds the image: all four floats of D are bit for bit what
 * rf_renderer_read_accumulation returns from a handle that differs only in num_bounces = 1 and has traced the same samples, whatever the batching, slot order or
 * number of ranks; on a handle whose own num_bounces is 1, D == S.  Indirect light is not stored: it is (S - D) per channel, one f32 subtraction, formed by whoever
 * needs it, and it may be negative (the reference does not clamp dot(n, l)).  One more launch per batch, behind bounce 1's shadow launch (rf_stats counts it with the
 * accumulation: ms_accumulate, launches_accumulate), and 16 bytes per pixel of device memory (rf_renderer_memory_info counts them in path_state_bytes while they are
 * allocated); S, Q, the AOV sums, the bucket sums and the ray counts are bit for bit what they are with it off.  D keeps its own sample count -- the samples traced
 * while it was on -- and is cleared, with the count set to 0, when the image is (a change through rf_renderer_set_render_parameters, a new tile shard, a newly bound
 * accumulation buffer) and when the switch changes.  Turned on partway through an accumulation, D covers only the later samples.
 * While on with plain 1, rf_renderer_render_adaptive and rf_comm_render_adaptive return RF_ERROR_INVALID_ARGUMENT (the message names the direct sums) before anything
 * is traced or exchanged, the state kept; turning D on, in either form, is refused in the non-uniform state.  rf_renderer_gather_frame carries D with RF_GATHER_DIRECT (DIRECT SUMS ACROSS RANKS, below).
 * The argument's domain is checked (until RF_DIRECT_TILE_COUNTS was added any non-zero value meant "on"): 0, 1 and 1 | RF_DIRECT_TILE_COUNTS; the bit alone and any
 * other bit are RF_ERROR_INVALID_ARGUMENT, the state kept.
 * rf_renderer_set_direct(r, 1 | RF_DIRECT_TILE_COUNTS) opts in to per-tile counts, as RF_AOV_TILE_COUNTS does for the AOV sums.  Until rf_renderer_render_adaptive or
 * rf_comm_render_adaptive is called the handle behaves bit for bit like one with plain 1: sums, image, stats, launch plans, rf_renderer_memory_info.  The adaptive calls
 * then run with D on: D of every pixel of tile t is bit for bit what rf_renderer_render(tile_samples[t]) leaves there in a fresh accumulation with D on -- equally,
 * the accumulation of a num_bounces = 1 handle after tile_samples[t] samples --, added under the call's tile list by the list-addressed radiance sum (one lane per
 * pixel for batches of at most 4 samples or a slot order that is not pixel-major, else LDS-staged; the same ordered chain either way); the direct sample count
 * advances with L; S, Q, the AOV sums, the schedule and *result are exactly what they are with D off.  The calls are still refused (the message names the direct sums
 * and says "restart the accumulation first") when D is on but does not cover the accumulation.  Any change of the argument's value clears D and drops a
 * split-denoised snapshot, 1 <-> 1 | RF_DIRECT_TILE_COUNTS included.  In the non-uniform state rf_renderer_read_direct returns the sums as they are and the leading
 * count L; a pixel's divisor is its tile's count (rf_renderer_read_tile_samples).
 * Across ranks the one bit covers rf_comm_render_adaptive too (D is shard-compact and addressed through the shard's slot list): afterwards the sum of the ranks'
 * rf_renderer_read_direct is the whole-frame handle's D, bit for bit.  The frame gather carries D with RF_GATHER_DIRECT, per tile count together with
 * RF_GATHER_TILE_COUNTS, and rf_comm_denoise_split / rf_comm_read_split then run on the root over the gathered sums (DIRECT SUMS ACROSS RANKS, below).  NOT covered:
 * `rf-render --gpus N --direct / --indirect / --denoise-split` stays refused; lifting that is the follow-up.
 * rf_renderer_read_direct: row-major width*height*4 floats (the layout of rf_renderer_read_accumulation; may be NULL) and the direct sample count.  With a tile shard
 * set, this rank's pixels and zeros elsewhere: the sum of the ranks' reads is the whole frame.
 *
 * Split-component denoiser: the a-trous filter above run on the direct and the indirect light separately, each with its own parameters, and recombined (what SVGF
 * does with its two components).  The sun's term at the first hit is nearly noise-free and carries the hard shadow edges, the bounced light carries the variance:
 * one colour sigma cannot serve both.  Inputs: S, D, AC, ND of one accumulation and ONE sample count N that all of them have; two parameter sets, direct and
 * indirect (L_D, σc_D, σn_D, σz_D and L_I, σc_I, σn_I, σz_I), each within the limits above.  f32, one IEEE operation at a time in the order written.
 *   prep, per pixel:  c, the background test, a, n, z and ae = a + εa exactly as above.
 *                     background: eD = c, eI = 0; never a neighbour; output c exactly.
 *                     otherwise:  cD = D.rgb / Nf;  cI = (S.rgb - D.rgb) / Nf (one subtraction, one division);  eD = cD / ae;  eI = cI / ae per channel;
 *                                 each component X has its own ℓ_X = (e_X.r + e_X.g) + e_X.b
 *   passes:           component X in {D, I} runs iterations i = 0 .. L_X - 1 of the pass defined above over its own e_X and ℓ_X with its own σc, σn, σz; the two
 *                     chains never read each other.  A component past its L_X keeps its value.
 *   finish:           out = (eD' + eI') ae per channel -- one add, one multiply; background out = c;  L_D = L_I = 0: out = c for every pixel.  {out.rgb, 1}.
 * With D == S and L_D >= 1 the indirect chain is exactly +0 throughout and the result is bit for bit the one filter's with the direct parameters.
 * rf_denoise_split_default_parameters: the two default sets (either pointer may be NULL, not both): direct L = 1, σc = 0.25; indirect L = 2, σc = 256; σn = σz = 0.1
 * for both (profiles/split_denoise/README.md: the sweep behind them, at 4 samples per pixel).
 * rf_renderer_denoise_split: enqueued on the handle's stream over its own sums; a NULL parameter set = that component's default.  The result is the snapshot that
 * rf_renderer_read_denoised reads, with the invalidation rules above, and it is also dropped whenever D is cleared.  RF_ERROR_INVALID_ARGUMENT in the non-uniform
 * state (that state's message, before the other checks), when the AOVs or the direct sums are off, when the AOV or the direct sample count differs from the accumulated
 * count, when no sample has been accumulated, or when a tile shard is set.  The first call allocates two more float4 per pixel next to rf_renderer_denoise's buffers.
 * rf_denoise_split_images: the same filter over row-major host sums on device device_ordinal; out_rgba / out_bgra8 may be NULL.  Synchronous.  A NULL input, a zero
 * size or sample count and bad parameters are refused before any device call.
 * ONE COUNT PER TILE.  In the non-uniform state rf_renderer_denoise_split runs when D carries RF_DIRECT_TILE_COUNTS, the AOVs carry RF_AOV_TILE_COUNTS and both cover
 * the accumulation: prep's Nf is float(tile_samples[t]) of the pixel's tile t, for c, a, m, cD and cI alike; the passes and the finish are unchanged.  The call first
 * waits for the handle's stream and copies the counts to the device, as rf_renderer_denoise does in this state; the snapshot's sample count is L.  With every count
 * equal to N the result is bit for bit the one-count filter's.  Otherwise the non-uniform state's refusal stands ("different sample counts"), before the other checks.
 * rf_denoise_split_tiles: rf_denoise_split_images with rf_denoise_tiles' tile_samples (one count > 0 per tile of the 32x32 grid, host memory) in place of the one
 * sample count.  A NULL input, a zero size, any count of 0 and bad parameters are refused before any device call.  Synchronous. */
#define RF_DIRECT_TILE_COUNTS 0x100u /* ORed into rf_renderer_set_direct's 1: keep D per tile count under rf_renderer_render_adaptive / rf_comm_render_adaptive */
RF_API int rf_renderer_set_direct(rf_renderer* r, int enabled);
RF_API int rf_renderer_read_direct(rf_renderer* r, float* direct_sum4, uint32_t* direct_sample_count);
RF_API int rf_denoise_split_default_parameters(rf_denoise_parameters* direct, rf_denoise_parameters* indirect);
RF_API int rf_renderer_denoise_split(rf_renderer* r, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect);
RF_API int rf_denoise_split_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* direct_sum4,
                                   const float* albedo_coverage4, const float* normal_depth4, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect,
                                   float exposure, float* out_rgba, uint32_t* out_bgra8);
RF_API int rf_denoise_split_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, const uint32_t* tile_samples, const float* color_sum4, const float* direct_sum4,
                                  const float* albedo_coverage4, const float* normal_depth4, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect,
                                  float exposure, float* out_rgba, uint32_t* out_bgra8);

/* Feature export: the frame's per-pixel feature channels as ONE tensor in caller-owned DEVICE memory -- what a learned denoiser, a compositor or any tensor pipeline
 * takes -- without the sums leaving the device: one kernel reads the sums where they lie (tile-major on a handle, row-major on the root of a gather), divides every
 * pixel by its own sample count and writes planar or interleaved f32 / f16.  No reference counterpart.
 *
 * A request (rf_feature_request) is a channel mask, a layout and an element type; `reserved` is 0.  The output holds, for every pixel of the width x height frame,
 * the selected channels in ascending bit order.  f32, one IEEE operation at a time in the order written, no contraction, as everywhere in this header.
 * Nf = float(count), count = N, the frame's one sample count -- or, where a count per tile is used (the non-uniform state of rf_renderer_render_adaptive, a gather
 * with RF_GATHER_TILE_COUNTS, tile_samples), count = tile_samples[(y >> 5) * ceil(width / 32) + (x >> 5)].  A pixel whose count is 0 gives +0 in every channel.
 *
 *   bit    name                  channels  value
 *   0x001  RF_FEATURE_COLOR      3         S.c / Nf  (kTonemap's division; rf_renderer_read_mean's)
 *   0x002  RF_FEATURE_ALBEDO     3         AC.c / Nf
 *   0x004  RF_FEATURE_NORMAL     3         background: 0, 0, 0; else m = ND.xyz / Nf, n = m * (1 / sqrt(dot(m, m))) with dot = (m.x m.x + m.y m.y) + m.z m.z -- the
 *                                          denoiser's guide normal, computed exactly as its prep computes it; (0, 0, 0) where dot(m, m) is 0 or not finite
 *   0x008  RF_FEATURE_DEPTH      1         background: 0; else z = ND.w / AC.w
 *   0x010  RF_FEATURE_COVERAGE   1         AC.w / Nf
 *   0x020  RF_FEATURE_DIRECT     3         D.c / Nf
 *   0x040  RF_FEATURE_INDIRECT   3         (S.c - D.c) / Nf  (one subtraction, one division: rf_comm_read_split's)
 *   0x080  RF_FEATURE_VARIANCE   3         per channel, mu and v exactly as the noise estimate forms them: mu = S.c / Nf; v = (Q.c - S.c mu) / (Nf - 1);
 *                                          v = v > 0 ? v : 0; out = v / Nf, the variance of the mean
 *   0x100  RF_FEATURE_ERROR      1         the noise estimate's per-pixel e (its error_map), 0 where e <= FLT_MAX is false
 *   0x200  RF_FEATURE_SAMPLES    1         Nf
 * Background is the denoiser's test: AC.w == 0, or z = ND.w / AC.w not > 0.
 *
 * Layouts: RF_FEATURES_CHW -- plane after plane, each row-major: element (c * height + y) * width + x; RF_FEATURES_HWC -- element (y * width + x) * C + c.
 * Element types: RF_FEATURES_F32; RF_FEATURES_F16 -- the f32 value converted with ONE round-to-nearest-even conversion (overflow to +-inf, half subnormals kept, NaN
 * stays NaN: numpy's float32 -> float16).  rf_feature_channel_count gives C; the buffer holds width * height * C elements, contiguous; the destination needs element
 * alignment only (4 or 2 bytes; a 16-byte aligned destination of a frame whose width is a multiple of 4 (f32) / 8 (f16) is written 16 bytes per lane, any other
 * element by element: the same values).
 *
 * rf_renderer_export_features: over the handle's own sums.  Enqueued on the handle's stream and then waited for: when it returns the buffer may be used from any
 * stream (torch's current one, say).  *sample_count (may be NULL): the accumulated (leading) count.  In the non-uniform state every pixel takes its tile's own count
 * (the call first waits for the stream and copies the counts to the device, as the other per-tile reads do).  READ-ONLY: every sum, count, snapshot, statistic and the
 * frame counter stay as they are.  It needs no scratch but the counts' buffer of the per-tile reads; a handle that never calls it allocates and launches nothing for it.
 * RF_ERROR_INVALID_ARGUMENT, the state kept, each before any launch: a NULL argument; unknown channel, layout or dtype bits, an empty mask or reserved != 0;
 * dst_bytes smaller than the frame needs; dst_device that hipPointerGetAttributes does not report as device memory on the handle's device (a host pointer never
 * reaches the kernel); a tile shard is set (gather the frame and call rf_comm_export_features on the root); no sample accumulated; a selected channel's family is
 * off or does not cover the accumulation (the AOVs for ALBEDO / NORMAL / DEPTH / COVERAGE, D for DIRECT / INDIRECT, the moments for VARIANCE / ERROR); in the
 * non-uniform state, a selected family that was kept without its tile-count bit (RF_AOV_TILE_COUNTS, RF_DIRECT_TILE_COUNTS); VARIANCE / ERROR with fewer than 2
 * samples.  COLOR and SAMPLES need nothing but samples.
 * rf_comm_export_features (declared with the communicator's calls, below): the same over the row-major planes gathered on the root -- planes 0 .. 3 and 5, and the
 * gathered tile counts when the gather carried them --, on the root's handle's stream, then waited for.  Bit for bit what the un-sharded handle's own export writes.
 * Refused when a selected channel's plane was not gathered, on a rank that was not the root, and as above.
 * rf_export_features_images: the same over host-assembled row-major width*height*4 sums, into HOST memory (out_host: width * height * C elements); synchronous,
 * like rf_denoise_images.  tile_samples NULL: `samples` for every pixel; else one count per tile (host memory) and `samples` is not used.  An input pointer may be
 * NULL when no selected channel reads it (COLOR / INDIRECT / VARIANCE / ERROR read color_sum4, VARIANCE / ERROR sumsq4, ALBEDO / NORMAL / DEPTH / COVERAGE both AOV
 * sums, DIRECT / INDIRECT direct_sum4).  A NULL that is needed, a zero size, samples == 0 without tile_samples, a tile count of 0 (rf_denoise_tiles' rule) and, where
 * VARIANCE / ERROR are selected, any count below 2 are refused before any device call. */
#define RF_FEATURE_COLOR 0x001u
#define RF_FEATURE_ALBEDO 0x002u
#define RF_FEATURE_NORMAL 0x004u
#define RF_FEATURE_DEPTH 0x008u
#define RF_FEATURE_COVERAGE 0x010u
#define RF_FEATURE_DIRECT 0x020u
#define RF_FEATURE_INDIRECT 0x040u
#define RF_FEATURE_VARIANCE 0x080u
#define RF_FEATURE_ERROR 0x100u
#define RF_FEATURE_SAMPLES 0x200u
#define RF_FEATURES_CHW 0u
#define RF_FEATURES_HWC 1u
#define RF_FEATURES_F32 0u
#define RF_FEATURES_F16 1u
typedef struct rf_feature_request
{
    uint32_t channels, layout, dtype, reserved;
} rf_feature_request;
RF_API int rf_feature_channel_count(uint32_t channels, uint32_t* count);
RF_API int rf_renderer_export_features(rf_renderer* r, const rf_feature_request* req, void* dst_device, uint64_t dst_bytes, uint32_t* sample_count);
RF_API int rf_export_features_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const uint32_t* tile_samples /* NULL: `samples` for all */,
                                     const float* color_sum4, const float* sumsq4, const float* albedo_coverage4, const float* normal_depth4, const float* direct_sum4,
                                     const rf_feature_request* req, void* out_host);

/* Radiance second moments and the noise estimate: how noisy the accumulation still is, per pixel, per 32x32 tile and for the frame, and a render call that stops
 * at a noise target.  No reference counterpart (the reference counts samples: renderProgressPercentage).
 *
 * rf_renderer_set_moments: 0 (the default: nothing is allocated or launched, image / stats / timings exactly as without) or 1.  While on, the handle keeps one more
 * per-pixel f32 buffer next to the accumulation, Q = {sum r.x r.x, sum r.y r.y, sum r.z r.z, 0}, where r is the radiance the accumulation adds for that sample
 * (wgsl:55-57), each square is one f32 multiply, and the squares are added in f32 in sample-index order, one dependent chain per channel -- the order of the radiance
 * sum: bit-reproducible whatever the batching, slot order or number of ranks.  16 bytes per pixel of device memory and nothing per path slot
 * (rf_renderer_memory_info's figures do not change).  The moments keep their own sample count -- the samples traced while they were on -- and are cleared, with the
 * count set to 0, when the image is (a change through rf_renderer_set_render_parameters, a new tile shard, a newly bound accumulation buffer) and when the switch
 * changes.  Turned on partway through an accumulation, they cover only the later samples: the count stays below the accumulated sample count.
 * rf_renderer_read_moments: row-major width*height*4 floats (the layout of rf_renderer_read_accumulation; may be NULL) and the moment sample count.  With a tile
 * shard set, this rank's pixels and zeros elsewhere: the sum of the ranks' reads is the whole frame.  (rf_renderer_gather_frame carries them with
 * RF_GATHER_MOMENTS: the root then holds the whole frame's Q in device memory, rf_comm_read_plane plane 3.)
 *
 * The estimate.  Inputs: the per-pixel sums S (the accumulation) and Q of one accumulation and ONE sample count N >= 2 that both have.  All arithmetic is f32, one
 * IEEE operation at a time in the order written (+ - * /, sqrt, compares and selects): a numpy float32 restatement reproduces every output bit for bit.
 * Nf = float(N).
 *   per pixel, per channel c:  mu = S_c / Nf;  v = (Q_c - S_c mu) / (Nf - 1);  v = (v > 0) ? v : 0  (NaN -> 0)
 *   per pixel:                 s2 = ((v_r + v_g) + v_b) / Nf;  l = (mu_r + mu_g) + mu_b;  e = sqrt(s2) / (l + 2^-8)
 *                              -- the standard error of the pixel's mean relative to its level.  Where e <= FLT_MAX is false (NaN, +inf) the pixel is counted as
 *                              non-finite and its e is 0.
 *   per 32x32 tile of the renderer's tile grid (tile t = tile_y * ceil(width / 32) + tile_x):  a[i] = e of the pixel at tile-local (tx, ty), i = ty 32 + tx, and 0 for
 *                              pixels outside the frame (not counted);  for h = 512, 256, ..., 1:  a[i] = a[i] + a[i + h] for every i < h;  tile_sum = a[0];
 *                              tile_max = the maximum of e over the tile's in-frame pixels (a maximum of -0 is returned as +0);  tile_pixels, tile_nonfinite: counts.
 *   frame, on the host:        mean_error = (sum over t of double(tile_sum[t]), t ascending, in f64) / pixels;  max_error = the maximum of tile_max[t], worst_tile the
 *                              first tile that attains it;  pixels, nonfinite_pixels: the counts' totals.
 *
 * rf_renderer_noise_estimate: over the handle's own sums; enqueued on the handle's stream and then waited for.  error_map (row-major width*height floats), tile_sum
 * and tile_max (ceil(width / 32) * ceil(height / 32) floats each) may be NULL.  RF_ERROR_INVALID_ARGUMENT when the moments are off, when the moment sample count
 * differs from the accumulated count (moments turned on partway through), when fewer than 2 samples are accumulated, or when a tile shard is set (gather with
 * RF_GATHER_MOMENTS and use rf_comm_noise_estimate on the root, or rf_noise_estimate_images on the sum of the ranks' reads).  Leaves the accumulation, the AOV sums, the denoise snapshot, the stats and later samples untouched; its
 * device buffers (a few words per tile, one float per pixel once a map was asked for) are allocated by the first call and freed with the moments.
 * rf_noise_estimate_images: the same kernel over row-major host sums (width*height*4 floats each, e.g. assembled from several ranks) on device device_ordinal.
 * Synchronous.  A NULL input or `out`, a zero size and samples < 2 are refused before any device call.
 * rf_renderer_render_until: rf_renderer_render in steps -- render min(check_every, frames left) frames, estimate (once 2 samples are accumulated), repeat -- until
 * mean_error <= target_mean_error, max_frames frames have been rendered or the accumulation holds num_samples_per_pixel samples (frames past that are not rendered).
 * The image it leaves is the image rf_renderer_render(*frames_rendered) leaves.  *last (may be NULL): the last estimate made; samples = 0 when none was (fewer than 2
 * samples).  RF_ERROR_INVALID_ARGUMENT when the moments are off or do not cover the whole accumulation, a tile shard is set, or check_every is 0.  Waits for the work
 * it enqueues. */
typedef struct rf_noise_estimate
{
    double   mean_error;
    float    max_error;
    uint32_t worst_tile, samples;
    uint64_t pixels, nonfinite_pixels;
} rf_noise_estimate;
RF_API int rf_renderer_set_moments(rf_renderer* r, int enabled);
RF_API int rf_renderer_read_moments(rf_renderer* r, float* sumsq4, uint32_t* moment_sample_count);
RF_API int rf_renderer_noise_estimate(rf_renderer* r, rf_noise_estimate* out, float* error_map, float* tile_sum, float* tile_max);
RF_API int rf_noise_estimate_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* sumsq4,
                                    rf_noise_estimate* out, float* error_map, float* tile_sum, float* tile_max);
RF_API int rf_renderer_render_until(rf_renderer* r, float target_mean_error, uint32_t check_every, uint32_t max_frames, uint32_t* frames_rendered,
                                    rf_noise_estimate* last);

/* Bucket sums and the robust mean: a firefly-robust estimate of the image, a median-of-means over K sums of every K-th sample whose trim follows the spread of the
 * buckets (after Buisine et al. 2021, "Firefly removal in Monte Carlo rendering with adaptive Median of meaNs"; the definition below is this library's own).  No
 * reference counterpart.  The plain mean S / N is the one estimator a single firefly ruins; this one gives it up to (K - 1) / 2 buckets to discard.
 *
 * rf_renderer_set_buckets(r, K): K = 0 (the default: nothing is allocated or launched, image / stats / timings exactly as without) or K odd with 3 <= K <= 15;
 * anything else is RF_ERROR_INVALID_ARGUMENT and the state is kept.  While on, the handle keeps K more per-pixel f32 planes next to the accumulation, one after
 * another in one allocation, each laid out like the accumulation:  B_b = {sum r.x, sum r.y, sum r.z, 0} over the samples whose ORDINAL j satisfies j mod K == b,
 * where r is the radiance the accumulation adds for that sample (wgsl:55-57) and j is the bucket sample count just before that sample -- 0 for the first sample
 * traced with the buckets on.  Each channel of each bucket is one dependent chain of f32 additions in sample order, no atomics, no contraction: bit-reproducible
 * whatever the batching, slot order or options.  (S is NOT bitwise the sum of the B_b: that is another addition order.)  K x 16 bytes per pixel of device memory and
 * nothing per path slot (rf_renderer_memory_info's figures do not change); under a tile shard the planes are shard-compact, as Q is.  S, Q, the AOV sums and the
 * ray counts are bit for bit what they are with the buckets off.  The buckets keep their own sample count -- the samples traced while they were on -- and are
 * cleared, with the count set to 0, when the image is (a change through rf_renderer_set_render_parameters, a new tile shard, a newly bound accumulation buffer) and
 * when K changes.  Turned on partway through an accumulation, they cover only the later samples.
 * The buckets and tile-adaptive sampling.  As set with K alone the buckets keep ONE sample count for the frame: while they are on, rf_renderer_render_adaptive and
 * rf_comm_render_adaptive return RF_ERROR_INVALID_ARGUMENT (the message names the buckets) before anything is traced or exchanged.
 * rf_renderer_set_buckets(r, K | RF_BUCKETS_TILE_COUNTS), K > 0 (the low byte of the argument is K, the bits from bit 8 up say how; the bit with K = 0 and any other
 * bit are RF_ERROR_INVALID_ARGUMENT), opts in to per-tile counts, as RF_AOV_TILE_COUNTS does for the AOV sums: until rf_renderer_render_adaptive is called the handle is
 * bit for bit the handle without the bit (the same kernels, the same planes, the same memory figures); rf_renderer_render_adaptive then runs -- refused, "restart the
 * accumulation first", when samples are accumulated and the bucket sample count does not cover them -- and afterwards the K planes of every pixel of tile t are bit for
 * bit what rf_renderer_render(tile_samples[t]) leaves there in a fresh accumulation with the buckets on: sample j of the tile in plane j mod K, the same chains, whatever
 * the batching, the slot order or the options (all active tiles share one count, so one bucket phase serves a batch; a batch shorter than K leaves the planes it does
 * not reach untouched).  The bucket sample count advances with the leading count L.  S, Q, the AOV sums, which tile stops when, *result and the ray counts are exactly
 * what they are with the buckets off.  A change of the bit alone clears the bucket sums, as a change of K does; rf_renderer_read_buckets reports K without the bit, and
 * in the non-uniform state the planes as they are and L.  rf_comm_render_adaptive stays refused while the buckets are on, in either of these two forms (bucket planes
 * under a tile shard then keep one count).  rf_renderer_set_buckets(K > 0), with or without the bits, is refused in the non-uniform state: the buckets could not cover
 * the accumulation.
 * rf_renderer_set_buckets(r, K | RF_BUCKETS_TILE_COUNTS | RF_BUCKETS_SHARD_TILE_COUNTS) -- the second bit is valid only on top of the first; 0x200 stays unknown and
 * refused -- says that the per-tile-count planes are also kept UNDER A TILE SHARD and may leave the handle through the frame gather; one bit serves both calls.
 * rf_comm_render_adaptive then runs with the buckets on -- refused, "restart the accumulation first", when the bucket sample count does not cover the accumulation --:
 * the bucket kernels address every plane through the shard's slot list, a rank's active tiles all sit at the frame's leading count, which is that rank's bucket sample
 * count, so one phase serves a batch, and after any sequence of calls with the same parameters on every rank the K planes of every tile (rf_renderer_read_buckets on its
 * owner) are bit for bit the whole-frame handle's after the same rf_renderer_render_adaptive calls.  S, Q, the AOV sums, the schedule, the ray counts and the result
 * structs are what they are with the buckets off.  And rf_renderer_gather_frame carries plane 4 in the non-uniform state (ROBUST MEAN ACROSS RANKS, below).  A change
 * of the bit alone clears the bucket sums and frees the plane-4 buffer, as a change of RF_BUCKETS_TILE_COUNTS does.  On a handle without a tile shard
 * rf_renderer_render_adaptive, rf_renderer_robust_mean and rf_renderer_denoise_robust behave exactly as with RF_BUCKETS_TILE_COUNTS alone, and without the bit every
 * call and every refusal is what it is without it.
 * rf_renderer_render, rf_renderer_render_until, rf_renderer_set_tile_shard and rf_renderer_gather_frame work as before; the frame gather does not carry the bucket planes
 * themselves: with RF_GATHER_ROBUST_MEAN every rank combines its own and ONE plane travels (ROBUST MEAN ACROSS RANKS, below).
 * rf_renderer_read_buckets: K x width*height*4 floats, plane after plane, each row-major (the layout of rf_renderer_read_accumulation; may be NULL), K and the bucket
 * sample count (either may be NULL).  With a tile shard set, this rank's pixels and zeros elsewhere: the sum of the ranks' reads is the whole frame.  Buckets off:
 * nothing is written to `buckets`, K = 0, count = 0.
 *
 * The robust mean.  Inputs: the K bucket sums of one accumulation and their count N >= K.  All arithmetic is f32, one IEEE operation at a time in the order written
 * (+ - * /, floor, compares and selects; no transcendentals): a numpy float32 restatement reproduces M and trim bit for bit.  Per pixel:
 *   bucket sizes and means:  n_b = N / K + (b < N mod K ? 1 : 0) in integer arithmetic;  m_b = B_b.rgb / float(n_b) per channel
 *   sort key:                l_b = (m_b.r + m_b.g) + m_b.b;  key_b = (l_b <= FLT_MAX) ? l_b : +inf   (a NaN becomes +inf)
 *   order:                   the buckets ascending by key, ties by bucket index (a stable sort): r_0 ... r_{K-1}
 *   Gini coefficient:        num = sum over i = 0 .. K-1 of float(2i - (K - 1)) key_{r_i}, each term one multiply, added in i order from +0;
 *                            den = float(K) (sum over i of key_{r_i}, in i order from +0);  G = (den > 0) ? num / den : 0
 *   trim count:              t = G (float(K) 0.5f);  c = (t >= 0) ? min(uint(floor(t)), (K - 1) / 2) : (K - 1) / 2  -- the minimum is taken before the conversion (t >=
 *                            float((K - 1) / 2) gives (K - 1) / 2), so a huge t is never converted; a NaN t compares false: a pixel with a non-finite bucket takes
 *                            the median
 *   output:                  M.rgb = (sum over i = c .. K-1-c of m_{r_i}, per channel, in i order from +0) / float(K - 2c);  M.a = 1;  trim = c (uint8)
 * All buckets equal: G = 0, c = 0, the mean of the means.  One bucket far above the rest: G approaches (K - 1) / K and c grows until the outlier is cut; c = (K - 1) / 2
 * is the median of the means.  The estimate is biased low on pixels whose samples are skewed, the more so the fewer samples a bucket holds.
 * One count per tile (the tiles combine): the same per pixel with N = tile_samples[t] >= K, t = (y / 32) ceil(width / 32) + (x / 32) the pixel's 32x32 tile, and nothing
 * else changed: no term looks at a neighbour, so a tile's result does not depend on the other tiles' counts, and with all counts equal to N it is bit for bit the
 * one-count form at N.
 *
 * rf_renderer_robust_mean: enqueued on the handle's stream over its own bucket sums.  It keeps a snapshot -- M, trim, the BGRA8 texels (kTonemap with
 * accumulatedSamples = 1 and the handle's exposure) and the count N; one float4, one byte and one u32 per pixel -- allocated by the first call and dropped whenever
 * the bucket sums are cleared.  RF_ERROR_INVALID_ARGUMENT when the buckets are off, when the bucket sample count differs from the accumulated count (turned on
 * partway through), when N < K, when a tile shard is set (use rf_robust_mean_images on the sum of the ranks' rf_renderer_read_buckets) or in the non-uniform state
 * -- unless the buckets were set with RF_BUCKETS_TILE_COUNTS: the tiles combine then runs over the handle's per-tile counts, the snapshot's count is the leading count L,
 * and the call is refused when any tile holds fewer than K samples (the message names K and the smallest count; sample with min_samples >= K); like the other per-tile
 * reads it first waits for the stream and copies the counts to the device.  When rf_renderer_render_adaptive left every tile at L the state is uniform again and the
 * one-count form runs.  Leaves every sum, the denoise snapshot, the stats and later samples untouched.
 * rf_renderer_read_robust_mean: row-major width*height*4 mean floats, the BGRA8 texels, one trim count per pixel and the snapshot's sample count; any pointer may be
 * NULL.  RF_ERROR_INVALID_ARGUMENT without a snapshot.
 * rf_robust_mean_images: the same kernel over host bucket planes (K x width*height*4 floats, each plane row-major, e.g. the sum of several ranks' reads) of `samples`
 * samples on device device_ordinal; the outputs may be NULL.  Synchronous.  A NULL input, a zero size, a K that is not odd in 3 .. 15 and samples < K are refused
 * before any device call.  Row-major and tile-major inputs give bit-identical results.
 * rf_robust_mean_tiles: rf_robust_mean_images with one count per 32x32 tile: tile_samples holds ceil(width / 32) * ceil(height / 32) words in the estimate's tile
 * numbering, exactly as for rf_denoise_tiles (e.g. rf_renderer_read_tile_samples next to rf_renderer_read_buckets).  Synchronous.  A NULL input, a zero size, a K that is
 * not odd in 3 .. 15 and any tile count below K are refused before any device call.
 * rf_renderer_denoise_robust: rf_renderer_robust_mean, then the a-trous filter of rf_renderer_denoise, whose definition changes in exactly one place: in prep,
 * c = M.rgb instead of S.rgb / Nf (a = AC.rgb / Nf and m = ND.xyz / Nf as ever, everything after prep as written; L = 0 returns M).  The result is the ordinary denoise
 * snapshot (rf_renderer_read_denoised).  Refused as rf_renderer_denoise is, and also when rf_renderer_robust_mean would be.  In the non-uniform state it runs the tiles
 * combine and then prep with Nf = float(the count of the pixel's tile) for a and m (c = M.rgb as it is; the passes unchanged): it needs the AOVs on with
 * RF_AOV_TILE_COUNTS and the buckets with RF_BUCKETS_TILE_COUNTS, both covering the accumulation.  rf_renderer_denoise itself is unchanged. */
#define RF_BUCKETS_TILE_COUNTS 0x100u /* ORed into K: keep the bucket sums per tile count under rf_renderer_render_adaptive */
#define RF_BUCKETS_SHARD_TILE_COUNTS 0x400u /* ORed into K | RF_BUCKETS_TILE_COUNTS: ... under a tile shard too (rf_comm_render_adaptive), and through the frame gather */
RF_API int rf_renderer_set_buckets(rf_renderer* r, uint32_t K);
RF_API int rf_renderer_read_buckets(rf_renderer* r, float* buckets, uint32_t* K, uint32_t* bucket_sample_count);
RF_API int rf_renderer_robust_mean(rf_renderer* r);
RF_API int rf_renderer_read_robust_mean(rf_renderer* r, float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* sample_count);
RF_API int rf_robust_mean_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t K, uint32_t samples, const float* buckets, float exposure,
                                 float* out_rgba, uint32_t* out_bgra8, uint8_t* out_trim);
RF_API int rf_robust_mean_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t K, const uint32_t* tile_samples, const float* buckets, float exposure,
                                float* out_rgba, uint32_t* out_bgra8, uint8_t* out_trim);
RF_API int rf_renderer_denoise_robust(rf_renderer* r, const rf_denoise_parameters* params);

/* Temporal history: the last view's frame reprojected into a new camera.  A camera change restarts the accumulation and the first frames of the new view are as noisy
 * as if the previous one had never been rendered; but the scene is static, so the first hit of a pixel can be looked up in the previous view's frame, and where the
 * surface is the same one the previous view's samples stand behind the new view's.  One side kernel over planes the handle keeps anyway; the trace and shading
 * kernels, every sum and every other snapshot are untouched.  No reference counterpart.
 *
 * The definition.  Inputs: the sums S, AC, ND of one accumulation with ONE count N (Nf = float(N)), the camera C of that accumulation, the frame size W x H
 * (Wf = float(W), Hf = float(H)); the history -- the previous view's camera C' and two row-major float4 planes of the same W x H, T' = {mean colour rgb, effective
 * sample count h} and G' = {unit normal xyz, depth z}, G'.w = 0 marking background -- which may be absent; and rf_temporal_parameters {max_history, depth_tolerance,
 * min_normal_dot, reserved}: max_history and depth_tolerance finite and > 0, min_normal_dot in [-1, 1], reserved = 0.  All arithmetic is f32, one IEEE operation at a
 * time in the order written, with the parentheses written (correctly rounded divide and sqrt, denormals kept, no FMA contraction; the only conversions are float(uint)
 * and one float-to-integer conversion that is guarded before it happens): a numpy float32 restatement reproduces T, G and the texels bit for bit.  dot(a, b) =
 * (a.x b.x + a.y b.y) + a.z b.z;  cross(a, b) = (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y);  a scalar times a vector and a sum of vectors work per
 * component.  Per pixel p = (x, y), y counted from the top as everywhere:
 *   1 prep:         exactly the denoiser's prep (above): c = S.rgb / Nf;  z = ND.w / AC.w;  background iff AC.w == 0 or not (z > 0);  otherwise m = ND.xyz / Nf,
 *                   d = dot(m, m), n = (d != 0 and |d| <= FLT_MAX) ? m (1 / sqrt(d)) : 0.
 *                   background:  T = {c, Nf}, G = {0, 0, 0, 0}; steps 2 .. 4 are not taken (sky pixels take no history: they carry no noise).
 *   2 world point:  kRaygen's own expressions with the blue-noise pair replaced by its mean (0.5, 0.5) and no lens offset -- a thin-lens camera is accepted and
 *                   treated as its pinhole centre `origin`; lens_radius, up and right are not read:
 *                   u = (float(x) + 0.5) / Wf;  v = (float(y) + 0.5) / Hf;  s = u + (0.5 / Wf);  t = (1 - v) + (0.5 / Hf)
 *                   e = ((llc + s horizontal) + t vertical) - origin;  dir = e (1 / sqrt(dot(e, e)));  P = origin + (z dir)
 *   3 old view:     no history given: NO HISTORY.  Otherwise, with the members of C':
 *                   w = P - origin';  L = llc' - origin';  Nn = cross(horizontal', vertical');  den = dot(Nn, w);  k = dot(Nn, L) / den
 *                   not (k > 0) -- the point lies behind or in the plane through origin' parallel to the old image plane, or k is NaN: NO HISTORY.  (k w is where the
 *                   line from origin' to P meets the old image plane.  The sign of den alone does not say "in front": it depends on the handedness of horizontal' x
 *                   vertical', and for the cameras rf_create_camera makes Nn points AWAY from the scene; the ratio k does not.)
 *                   q = (k w) - L;  nn = dot(Nn, Nn)
 *                   a = dot(cross(q, vertical'), Nn) / nn;  b = dot(cross(horizontal', q), Nn) / nn      (Cramer's rule: horizontal' and vertical' need not be
 *                   perpendicular)
 *                   fx = (a Wf) - 1;  fy = (1 - b) Hf      (the continuous pixel coordinate: step 2 inverted in real arithmetic; a pixel centre maps to an integer)
 *                   not (fx >= -1 and fx < Wf and fy >= -1 and fy < Hf): NO HISTORY -- written so that a NaN fails, and decided BEFORE any conversion to an integer.
 *                   xf = floor(fx);  yf = floor(fy);  tx = fx - xf;  ty = fy - yf;  x0 = int(xf);  y0 = int(yf)      (-1 <= x0 <= W - 1, -1 <= y0 <= H - 1)
 *                   z' = sqrt(dot(w, w))      (the depth the old view would have recorded for P)
 *   4 taps:         the four taps (x0 + i, y0 + j) in the order j = 0, 1, inside it i = 0, 1, with bx = i ? tx : (1 - tx), by = j ? ty : (1 - ty), β = bx by.
 *                   A tap is VALID iff it lies inside the frame and, with its T' and G':  T'.w > 0  and  G'.w > 0  and  |G'.w - z'| <= (depth_tolerance z')  and
 *                   dot(n, G'.xyz) >= min_normal_dot  (every comparison false for a NaN).  An invalid tap is SKIPPED, not multiplied by zero: a NaN or an
 *                   infinity in an invalid tap does not reach the output; one in a valid tap does.
 *                   From +0, in tap order over the valid taps:  sumB += β;  sumC.rgb += β T'.rgb;  sumH += β T'.w
 *                   not (sumB > 0): NO HISTORY.  Otherwise hist = sumC.rgb / sumB;  h = sumH / sumB.
 *   5 blend:        NO HISTORY:  T = {c, Nf}.  Otherwise he = (h < max_history) ? h : max_history (a NaN h gives max_history);
 *                   T.rgb = ((Nf c) + (he hist)) / (Nf + he) per channel;  T.w = Nf + he.
 *                   G = {n, z} for a foreground pixel.  The BGRA8 texel is kTonemap over T.rgb with accumulatedSamples = 1 and the exposure, as for the robust mean.
 * T.w is the weight the NEXT view gives this frame: the samples behind a pixel, capped at max_history so that an old frame's lighting fades out.
 *
 * rf_temporal_default_parameters: max_history = 64, depth_tolerance = 0.05, min_normal_dot = 0.9 (kept after the sweep of profiles/temporal/README.md:
 * over a six-view orbit of the Duck at 4 samples per view every one of the 36 triples takes the RMSE against 1024 samples from 1.70 to 1.11 - 1.16; the sweep's best
 * is 16 / 0.02 / 0.8 at 1.1075, these values give 1.1312 -- 2.1 % above it; the depth tolerance orders the table, and 0.05 is kept for surfaces at a grazing angle).
 * rf_renderer_temporal_accumulate: the definition over the handle's own sums, its current camera and its kept history, if it has one (rf_renderer_temporal_commit);
 * params NULL = the defaults.  Enqueued on the handle's stream: ONE kernel (kTemporalReproject) does prep, reprojection, blend and the texel; the tile-major sums are read
 * where they lie, and row-major and tile-major sources give identical bits.  The result is a snapshot -- T, G, the texels, the camera and the count N -- tracked as the
 * denoise snapshot is, and dropped whenever the AOV sums are cleared.  Calling it again later in the same accumulation recomputes from the SAME history: history is
 * never counted twice.  The first call allocates two pairs of float4 planes and one u32 plane, 68 bytes per pixel (rf_renderer_memory_info counts them in
 * path_state_bytes once they exist; a handle that never calls it allocates nothing).  RF_ERROR_INVALID_ARGUMENT, before any launch and with the state kept, in this
 * order: a NULL handle; bad parameters; the AOVs off; the AOV sample count different from the accumulated count; no sample accumulated; a tile shard set (use
 * rf_temporal_images on the gathered sums -- the root of a frame gather has no history of its own); the non-uniform state of rf_renderer_render_adaptive.
 * rf_renderer_temporal_commit: the current result becomes the history, by a pointer swap and no copy; the result snapshot is then gone (refused without one).  The
 * history survives a restart of the accumulation -- that is its purpose -- and is dropped when the frame size changes, when a tile shard is set, and by
 * rf_renderer_temporal_reset, which drops the result snapshot as well and keeps the buffers.
 * rf_renderer_read_temporal: row-major width*height*4 floats {T.rgb, T.w}, the BGRA8 texels, width*height*4 floats G and the snapshot's sample count N; any pointer may
 * be NULL.  RF_ERROR_INVALID_ARGUMENT without a result.
 * rf_renderer_denoise_temporal: rf_renderer_temporal_accumulate, then the a-trous filter of rf_renderer_denoise with prep's colour c = T.rgb (rf_renderer_denoise_robust's
 * one change, with T in M's place); the result is the ordinary denoise snapshot (rf_renderer_read_denoised).  Refused as either half would be.
 * rf_temporal_images: the same kernel over row-major host planes on device device_ordinal: color_sum4 / albedo_coverage4 / normal_depth4 of `samples` samples, the
 * camera, and the history (history_color4 = T', history_geometry4 = G', history_camera = C': all three NULL or all three given); out_color4 = T, out_geometry4 = G,
 * out_bgra8 may be NULL.  Synchronous.  A NULL input, a zero size, a zero sample count, a history given in part and bad parameters are refused before any device call.
 * These calls leave every sum, count and tile count, the other snapshots, rf_renderer_read_tonemapped, the stats, the frame counter and rf_renderer_state_digest exactly
 * as they were.  NOT covered, deliberately: a tile shard and the root of a gather (refused); the non-uniform state (refused); the history is not part of a checkpoint
 * or of the state digest; rf-render has no option for it; the geometry does not move -- the scene is static. */
typedef struct rf_temporal_parameters
{
    float    max_history;     /* finite, > 0: the cap on the effective sample count a pixel takes from the history */
    float    depth_tolerance; /* finite, > 0: a tap is the same surface when |z_tap - z'| <= depth_tolerance z' */
    float    min_normal_dot;  /* in [-1, 1]: ... and when dot(n, n_tap) >= min_normal_dot */
    uint32_t reserved;        /* 0 */
} rf_temporal_parameters;
RF_API int rf_temporal_default_parameters(rf_temporal_parameters* params);
RF_API int rf_renderer_temporal_accumulate(rf_renderer* r, const rf_temporal_parameters* params);
RF_API int rf_renderer_temporal_commit(rf_renderer* r);
RF_API int rf_renderer_temporal_reset(rf_renderer* r);
RF_API int rf_renderer_read_temporal(rf_renderer* r, float* rgba, uint32_t* bgra8, float* geometry, uint32_t* sample_count);
RF_API int rf_renderer_denoise_temporal(rf_renderer* r, const rf_temporal_parameters* tparams, const rf_denoise_parameters* dparams);
RF_API int rf_temporal_images(int32_t device_ordinal, uint32_t width, uint32_t height, uint32_t samples, const float* color_sum4, const float* albedo_coverage4,
                              const float* normal_depth4, const rf_camera* camera, const float* history_color4, const float* history_geometry4,
                              const rf_camera* history_camera, const rf_temporal_parameters* params, float exposure, float* out_color4, float* out_geometry4,
                              uint32_t* out_bgra8);

/* Tile-adaptive sampling: a render call that keeps sampling only the 32x32 tiles that are still noisy, and the per-tile sample count that the reads then honour.
 * No reference counterpart.  rf_renderer_render_adaptive: the whole frame only (no tile shard; across ranks: rf_comm_render_adaptive, below); needs the moments on from the first sample and the AOVs off, or on with RF_AOV_TILE_COUNTS
 * (from the first sample as well).
 *
 * The handle keeps one more word per tile, tile_samples[t], t in the estimate's tile numbering (tile_y * ceil(width / 32) + tile_x).  rf_renderer_render(n) adds n to
 * every tile (min(n, samples left), as it does to the accumulated count); the counts are cleared, to 0, whenever the image is.  L, the LEADING count, is the
 * accumulated sample count (0 at the start); no tile ever holds more.
 *
 * rf_renderer_render_adaptive(r, params, result).  cap = params->max_samples, where 0 means num_samples_per_pixel and a larger value is clamped to it.  The loop:
 *   1. the ACTIVE tiles are those with tile_samples[t] == L;
 *   2. n = min(check_every, cap - L) more samples of the active tiles only are traced and added to S and Q -- samples frameCount, frameCount + 1, ..., exactly the
 *      ones rf_renderer_render would trace next (frameCount is the handle's frame counter, which advances by n) -- and L and the active tiles' counts grow by n;
 *   3. once L >= max(2, min_samples): the estimate above over the active tiles, Nf = float(L);
 *   4. an active tile with tile_sum / float(tile_pixels) <= target_tile_error (one f32 division; tile_pixels: its in-frame pixels) STOPS: it keeps its count for the
 *      rest of the accumulation.  A NaN compares false: such a tile goes on;
 *   5. repeat from 1 until no tile is active or L == cap.  (An estimate is made after the last step as well.)
 * All active tiles share one count at all times, and a stopped tile is never sampled again.  The defining property: afterwards, S and Q of every pixel of tile t are bit
 * for bit what rf_renderer_render(tile_samples[t]) leaves there in a fresh accumulation (with the moments on) -- each pixel's sums are its first tile_samples[t] samples
 * in sample order -- whatever the batching, the slot order or the options.  rf_stats' primary_rays counts the pixel-samples traced.
 * With RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS the same holds for the AOV sums: AC = {albedo.rgb, coverage} and ND = {normal.xyz, depth} of every pixel of tile t are
 * bit for bit what rf_renderer_render(tile_samples[t]) leaves there in a fresh accumulation with the AOVs on; the AOV sample count advances with L, as the moment
 * count does; and S, Q, the schedule (which tile stops when) and *result are exactly what they are with the AOVs off.
 * With rf_renderer_set_direct(r, 1 | RF_DIRECT_TILE_COUNTS) the same holds for the direct sums D (the direct sums' block above).
 * A later call, with the same or other parameters, continues with the tiles still at the leading count only (stopped tiles are not revived, the active set is not
 * dilated to neighbouring tiles, and counts are per tile, not per pixel).  Waits for the work it enqueues.
 * RF_ERROR_INVALID_ARGUMENT: the moments are off or do not cover the accumulation, the AOVs are on without RF_AOV_TILE_COUNTS (their sums then keep ONE sample
 * count) or with it but do not cover the accumulation (turned on partway through), the bucket sums or the direct sums are on without their tile-count bit or with
 * it but do not cover the accumulation, a tile
 * shard is set (rf_comm_render_adaptive is the call for a sharded frame), check_every is 0, or target_tile_error is negative or not finite.
 * *result (may be NULL): estimate_passes made by this call; tiles and stopped_tiles (tiles below L) of the frame; the minimum and maximum tile count; pixel_samples =
 * the sum over the tiles of in-frame pixels x tile_samples[t]; last = the estimate of the call's last pass, over the tiles that were active in it (mean_error, max_error,
 * pixels and nonfinite_pixels over those tiles, worst_tile in the frame's numbering, samples = L at that pass; samples = 0 when the call made no pass).
 *
 * While some tile is below L (the NON-UNIFORM state), rf_renderer_render, rf_renderer_render_until, rf_renderer_set_tile_shard and rf_renderer_gather_frame (without RF_GATHER_TILE_COUNTS)
 * return RF_ERROR_INVALID_ARGUMENT with a message that says so: each of them assumes one count for the frame.  So does rf_renderer_denoise, unless the AOVs are on
 * with RF_AOV_TILE_COUNTS and cover the accumulation: it then filters with each tile's own count (the denoiser's block above).  rf_renderer_denoise_split
 * likewise needs both RF_AOV_TILE_COUNTS and RF_DIRECT_TILE_COUNTS.
 * rf_renderer_set_render_parameters (with a change) and a newly bound accumulation buffer clear the counts with the image.  When every tile is at L -- every tile
 * ran to the cap, a huge target stopped every tile at the first check -- the handle is in the ordinary state and none of them refuses.  (A target of 0 runs a tile to
 * the cap only while its mean error is > 0: a tile in which no pixel has shown any variance so far -- black, constant or non-finite pixels have e = 0 -- is <= 0
 * and stops at the first check, as step 4 says.  min_samples = cap puts the only check at the cap: no tile can stop.)  In the non-uniform state:
 *   rf_renderer_read_accumulation, rf_renderer_read_moments, rf_renderer_read_aovs: the sums as they are; the count they report is L, and the divisor of a pixel is
 *       its tile's own count.  (For the moments and the AOV sums that is their own sample count, as ever: it IS L while they cover the accumulation, which the call
 *       that made the state requires; a switch changed in the state clears its sums, and its count then reads 0 -- see INTERLEAVINGS below.)
 *   rf_renderer_read_tile_samples: the counts (tile_samples may be NULL) and ceil(width / 32) * ceil(height / 32).  Uniform state: every tile of the shard at the
 *       accumulated count, a tile outside the shard 0.
 *   rf_renderer_read_mean: row-major width*height*4 floats {S.rgb / float(tile_samples[t]), 1}, one f32 division per channel; {0, 0, 0, 1} in a tile without a sample.
 *       Works in the uniform state too (pixels outside a shard's tiles: four zeros).
 *   rf_renderer_read_tonemapped: kTonemap over that mean with accumulatedSamples = 1 (rf_renderer_read_denoised's display path; x / 1 is exact, so in the uniform
 *       state the texels are those of the sums divided by the accumulated count).
 *   rf_renderer_noise_estimate: Nf = float(tile_samples[t]) for the pixels of tile t (every count is >= 2: a tile stops at an estimate); out->samples = L.
 * rf_noise_estimate_tiles: rf_noise_estimate_images with one count per tile (tile_samples: ceil(width / 32) * ceil(height / 32) words); out->samples = the largest.
 * A NULL input or `out`, a zero size and any tile count below 2 are refused before any device call.
 *
 * INTERLEAVINGS.  What the paragraphs above leave open between the switches, the sums and the two states follows from two general rules -- a sum covers the
 * accumulation only if it was on from its first sample, and whatever clears the image clears every sum with its count, the per-tile counts (both states) and both
 * snapshots -- and is stated here once (tests/handle_model.py is these rules as a program; tests/test_gpu_handle_walk.py holds the handle to it over random call
 * sequences):
 *   - A refused call (RF_ERROR_INVALID_ARGUMENT) changes nothing: no sum, count, snapshot or switch, and not the frame counter.  Where several refusals apply to one
 *     call, only the order stated above holds (the non-uniform state's message comes first for rf_renderer_denoise, and so for rf_renderer_denoise_robust, which is
 *     refused as it is); otherwise which of the messages is given is not promised.
 *   - rf_renderer_set_moments and rf_renderer_set_aovs are accepted in the non-uniform state.  A change clears that family's sums and sets its count to 0, as always;
 *     the family then no longer covers the accumulation, so a further rf_renderer_render_adaptive is refused (the AOVs: unless they were turned off) and the per-tile
 *     reads that need the family (rf_renderer_noise_estimate; rf_renderer_denoise) are refused until the accumulation is restarted.
 *     rf_renderer_set_buckets(0) is accepted there too; K > 0 is refused, as said above, also when K and the bit are the ones already set.
 *   - Every accepted rf_renderer_set_tile_shard restarts the accumulation, a call with the rank and world size already set included (the tiles are dealt anew).  So does
 *     every accepted rf_renderer_bind_accumulation_buffer: binding a buffer, binding another, and unbinding (NULL: back to the handle's own buffer).  The frame counter
 *     keeps counting through all of them, as through rf_renderer_set_render_parameters; the parameters compare equal or not as a whole, and an equal set restarts nothing.
 *   - rf_renderer_render(n) into a full accumulation traces nothing and advances the frame counter by n: the next accumulation starts n frames later.
 *     rf_renderer_render_until advances it by *frames_rendered, rf_renderer_render_adaptive by the growth of L.
 *   - A restarted accumulation reads as nothing: every sum zero with count 0, every tile of the shard at 0, rf_renderer_read_mean {0, 0, 0, 1} in the shard's tiles and
 *     rf_renderer_read_tonemapped the texel of that mean (opaque black); outside the shard's tiles the mean is four zeros and the texel 0.
 *   - The snapshots: rf_renderer_read_denoised's is dropped with the AOV sums (above) and NOT by a change of the buckets, also when rf_renderer_denoise_robust made it;
 *     rf_renderer_read_robust_mean's is dropped with the bucket sums and NOT by a change of the AOV flags.  Later samples leave both as they are, with their counts. */
typedef struct rf_adaptive_parameters
{
    float    target_tile_error;
    uint32_t check_every, min_samples, max_samples;
} rf_adaptive_parameters;
typedef struct rf_adaptive_result
{
    uint32_t          estimate_passes, tiles, stopped_tiles, min_tile_samples, max_tile_samples, reserved;
    uint64_t          pixel_samples;
    rf_noise_estimate last;
} rf_adaptive_result;
RF_API int rf_renderer_render_adaptive(rf_renderer* r, const rf_adaptive_parameters* params, rf_adaptive_result* result);
RF_API int rf_renderer_read_tile_samples(rf_renderer* r, uint32_t* tile_samples, uint32_t* num_tiles);
RF_API int rf_renderer_read_mean(rf_renderer* r, float* rgba);
RF_API int rf_noise_estimate_tiles(int32_t device_ordinal, uint32_t width, uint32_t height, const uint32_t* tile_samples, const float* color_sum4, const float* sumsq4,
                                   rf_noise_estimate* out, float* error_map, float* tile_sum, float* tile_max);

/* Deferred-lighting variant (replaces nlrs::DeferredRenderer's lighting + resolve passes, src/pt/deferred_renderer.hpp,
 * deferred_renderer_lighting_pass.wgsl:96-186 -- fixed 2-bounce surfaceColor, solar disk in the sky term, the
 * 1/16384 + 1024 offset constants :498-500 -- and deferred_renderer_resolve_pass.wgsl:33-54 -- 0.1 / 0.9 exponential
 * average).  The G-buffer comes from one primary ray per pixel through the jittered pixel centre
 * (deferred_renderer.cpp:309-315) instead of the reference's raster pass.  Camera, sky and exposure are the handle's
 * render parameters; the deferred frame counter starts at 0 and is separate from rf_renderer_render's. */
RF_API int rf_renderer_render_deferred(rf_renderer* r, uint32_t num_frames);
RF_API int rf_renderer_reset_deferred(rf_renderer* r);
/* sampleBuffer and accumulationBuffer (width*height*3 f32, row-major: array<array<f32, 3>>) and the resolve pass's
 * return value as BGRA8; any pointer may be NULL. */
RF_API int rf_renderer_read_deferred(rf_renderer* r, float* sample_rgb, float* accumulation_rgb, uint32_t* bgra8, uint32_t* frame_count);

/* Statistics (replaces the ImGui perf read-out, src/pt/main.cpp:251-257). */
RF_API int rf_renderer_set_counting(rf_renderer* r, int enabled);
RF_API int rf_renderer_set_timing(rf_renderer* r, int enabled);
/* Tuning knobs for A/B measurements; none of them changes a result (every combination is covered by the -m gpu parity tests).
 *   traversal_variant 0 | 2            one-ray-per-thread kernels over the 32-byte nodes | persistent kernels over the 64-byte records (default)
 *   quad_from_bounce, quad_shadow_from_bounce         first bounce whose closest-hit / shadow launch reads the 128-byte quad records (two
 *                                      levels of the tree per dependent fetch; defaults 1 / 1; 0 = never; takes precedence over the layouts below)
 *   quad_except_mask, quad_shadow_except_mask         ... except at bounce b when bit b-1 is set (default 0)
 *   quad_half_from_bounce, quad_half_shadow_from_bounce   first bounce whose quad launch reads the 64-byte half-precision quad records
 *                                      (conservative binary16 planes, exact boxes at the leaves; 0 = never; defaults chosen per scene:
 *                                      rf_wide_layout_stats)
 *   quad_local_from_bounce, quad_local_shadow_from_bounce   the same for the 64-byte local-grid quad records (8-bit planes on a
 *                                      per-record power-of-two grid); closest-hit launches: the half-precision records take precedence; shadow launches: these do
 *   compact_from_bounce, compact_shadow_from_bounce   first bounce whose closest-hit / shadow launch reads the compact-capable records
 *                                      (three loads per descending step; defaults 3 / 2; 0 = never)
 *   hot_from_bounce, hot_shadow_from_bounce           the same for the 32-byte records (two loads per step; default 0 = never)
 *   refill_min, refill_min_deep, refill_deep_from_bounce   idle lanes at which a wave refills (40; closest-hit launches from bounce 3 on: 22 on the 64-byte and the
 *                                      half-precision quad records, 40 on the exact quad records)
 *   leaf_vote                          descending lanes below which a wave processes its parked leaves (20)
 *   chunk, chunk_early, chunk_early_bounces   queue entries per cursor claim (128; 256 at bounces 1-2)
 *   shade_sort_from_bounce             first bounce whose shading stage appends each 1024-entry tile's surviving paths in the order of
 *                                      the triangles they hit (default 2; 0 = never: input order)
 *   uniform_fetch 0 | 1 | 2 | -1       scalar-cache fetch of wave-uniform records (1), and leaf triangles (2, default); -1: bounces 1-2 only
 *   shadow_nearest_first 0 | 1         any-hit child order: the reference's split-axis order | nearer slab entry first (default)
 *   shadow_record_order 0 | 1          shadow launches on the 64-byte quad layouts: nearest-first | entries in record order (default: the
 *                                      cheaper step wins where the VALU binds)
 *   packet_bounces n                   bounces 1..n traced by lockstep wave packets (default 0)
 *   occluder_cache_bounces n           the any-hit launches of bounces 1..n first visit the leaves that stopped the last shadow rays from the
 *                                      ray's cell of the scene (default 64; 0: off).  occluder_grid_cells c: cells along the longest extent of the
 *                                      scene (default 1024); occluder_grid_log2_cells n: table of 2^n cells x 16 bytes (default 22);
 *                                      shadow_first_look_from_bounce b: from this bounce on that first look is a dense pass of its own
 *                                      (kShadowFirstLook; default 2, 0: never).  Same image with any setting.
 *   primary_lists 0 | 1                bounce 1 of a pinhole camera over per-pixel leaf lists (default 1): a batch with at least primary_list_min_samples samples per
 *                                      pixel (default 16: the crossover measured at 1080p lies at about 10) walks the tree once per pixel and gives every sample the
 *                                      exact box and triangle tests of the leaves on its pixel's list; primary_list_capacity n: entries per pixel (1 .. 64,
 *                                      default 64; 65 words of device memory per pixel of a batch, counted by rf_renderer_memory_info and the batch-depth fit; a
 *                                      pixel that needs more takes the ordinary launch).  rf_stats.primary_list_rays / primary_fallback_rays say what ran.
 *                                      Same image with any setting.
 *   primary_fused 0 | 1                where those lists run, the first-hit AOVs are off and `transcendentals` is 0: bounce 1's ray generation, list walk and shading
 *                                      in ONE kernel per path (default 1) instead of three that hand the path on through memory.  rf_stats.ms_raygen is then 0 and
 *                                      bounce 1's closest-hit time contains generation and shading; rf_stats.primary_fused_rays says what ran.  Same image.
 *   transcendentals 0 | 1              THE ONE OPTION THAT CHANGES RESULTS (round 6; default 0).  0: sin / cos / acos / exp / pow(x, 1.5) of ray generation and the sky dome are
 *                                      the f32 rounding of a specified f64 evaluation (GPU == test oracle bit for bit); 1: the device math library's f32 functions (libm-grade) --
 *                                      WGSL's own builtins are f32 with implementation-defined ulps (wgsl:247-275,568-616).  Within SURVEY 8(d)'s tolerance of the default
 *                                      (>= 99.97 % of the pixels within 1e-3 |ref| + 1e-4 spp, image mean 5e-8), +0.2 % rays/s: off.  Set it before an accumulation's first sample.
 *   refill_min, refill_min_deep, refill_deep_from_bounce, leaf_vote, chunk, chunk_early ...
 *                                      scheduling of the persistent traversal kernel (idle lanes at which a wave refills: 40 at bounce 1 and in the any-hit
 *                                      launches, 12 from bounce 2 on -- 22 in scenes with leaves of 5 triangles or more; lanes that must still descend for the
 *                                      descend loop to go on; queue entries per cursor claim).  Same image with any setting.
 *   slot_group_shift, sample_sort, accumulate_runs, shade_blocks, reserve_samples, persistent_blocks, extra_lds
 *                                      path-slot order, accumulation kernel, grid sizes, occupancy experiments
 *   query_variant 0 | 2, query_compact 0 .. 5       kernels / record layout behind rf_renderer_intersect_rays / _occluded_rays (tests)
 *   cast_chunk n                                    rf_renderer_cast_rays traces at most n rays per chunk (0 = automatic: the path depth and the free memory) */
RF_API int rf_renderer_set_option(rf_renderer* r, const char* name, int64_t value);
RF_API int rf_renderer_reset_stats(rf_renderer* r);
RF_API int rf_renderer_get_stats(rf_renderer* r, rf_stats* out);
/* Queue occupancy and traversal kernel time per bounce since the last reset (entry b = bounce b+1;
 * bounces past 32 are folded into entry 31).  Each array holds `capacity` entries (or is NULL);
 * *num_bounces receives the number of entries that are meaningful (the current numBounces, <= 32).
 * No reference counterpart: the megakernel has no queues. */
RF_API int rf_renderer_get_bounce_stats(rf_renderer* r, uint32_t capacity, uint64_t* closest_rays, uint64_t* shadow_rays,
                                        double* ms_closest, double* ms_shadow, uint32_t* num_bounces);

/* Multi-GPU tile sharding (no reference counterpart: the reference is single-device).  The image
 * is cut into 32x32 tiles dealt to ranks in a scrambled round-robin; each rank renders its tiles
 * into a compact tile-major float4 buffer; rf_renderer_gather_frame (below) brings the shards to one rank. */
RF_API int rf_renderer_set_tile_shard(rf_renderer* r, uint32_t rank, uint32_t world_size);
RF_API int rf_renderer_shard_tiles(rf_renderer* r, uint32_t* tile_ids /* may be NULL */, uint32_t* num_tiles);
RF_API int rf_renderer_accumulation_device_buffer(rf_renderer* r, void** device_ptr, uint64_t* bytes);
RF_API int rf_renderer_bind_accumulation_buffer(rf_renderer* r, void* device_ptr, uint64_t bytes);

/* State digest and checkpoints (no reference counterpart).
 *
 * Every sum of a handle is kept in sample order, and every tile's sums are what a uniform render of that tile's own count leaves: a render is a function of the scene,
 * the parameters, the frame counter and the per-tile counts.  A checkpoint stores exactly that, keyed by tile, and the digest says whether two states are the same
 * without reading a plane back.
 *
 * THE DIGEST.  All arithmetic is mod 2^64 (tests/digest_restatement.py restates it in Python integers).
 *   mix64(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31.
 *   Plane ids p follow the gather's numbering: 0 = S, 1 = AC {albedo, coverage}, 2 = ND {normal, depth}, 3 = Q, 5 = D, 16 + b = bucket plane b.
 *   For the in-frame pixel (x, y) of plane p: i = y * width + x (the FRAME's index: the digest does not depend on the tile layout), w0 .. w3 the bit patterns of the texel's
 *   four floats, k = mix64((u64(p) << 32) | i),
 *     term = mix64(k ^ (u64(w1) << 32 | w0)) + mix64((k + 0x9E3779B97F4A7C15) ^ (u64(w3) << 32 | w2)).
 *   Tile digest d[p][t] = the sum of term over the in-frame pixels of tile t (the padding texels of a ragged tile are never read); plane digest = the sum of d[p][t]
 *   over the handle's own tiles; counts digest = the sum over the handle's tiles of mix64(mix64((u64(0xC0) << 32) | t) ^ u64(tile_samples[t])).
 * Hence: the digests of the ranks of a tile-sharded frame add up (mod 2^64) to the whole-frame handle's; -0.0 and +0.0 differ; a swap of two pixels, two planes or
 * two tiles changes the digest.  The tile digests come from one kernel (kDigestTiles: one workgroup per tile and plane, integer sums, no atomics); the host adds them.
 *
 * rf_renderer_state_digest: enqueued on the handle's stream, then waited for.  A family that is off has digest 0 and family_on 0; a restarted family digests as the
 * zeros its read returns (its sums are zeroed first, as the next sample would) with family_samples 0.  Families: 0 = S, 1 = the AOVs, 2 = Q, 3 = D, 4 = the buckets.
 * Works in the uniform and the non-uniform state, with or without a tile shard (then: over the shard's tiles) and on a bound accumulation buffer.
 *
 * rf_renderer_save_checkpoint: dst NULL = size query (*bytes out); else *bytes in = the buffer's size, out = the bytes written.  Waits for the stream.  The blob holds
 * the frame counter, the counts, the switch words, a guard of the render parameters (camera, sky, numBounces, width, height -- not numSamplesPerPixel, a cap, nor the
 * exposure, display only) and of the scene (the counts of BVH nodes, triangles, textures, texels and the root box: a guard against the wrong file, not a proof), the
 * handle's tile ids and per-tile counts, one digest per stored plane and tile, and every plane of every family that is on and holds samples.  Snapshots (denoised,
 * robust mean), statistics and the deferred variant are not saved.  The byte layout: INTEGRATION.md 3.
 * rf_checkpoint_info: host only (no device needed): the header of a blob, after the same checks of every length and count against `bytes` that a load makes.
 * rf_renderer_load_checkpoint: the blobs together must hold every tile of the handle's shard exactly once among the tiles the handle owns; tiles it does not own are
 * ignored -- one whole-frame blob feeds any shard, N shard blobs feed a whole-frame handle, N feed M.  RF_ERROR_INVALID_ARGUMENT, the handle unchanged and the message
 * naming the cause, before anything touches the device: bad magic or version, a length or count that does not fit the blob, blobs that disagree on anything but
 * their tiles, another frame size, camera, sky, numBounces or scene than the handle's, switch words that differ from the handle's (set them first: rf_checkpoint_info),
 * accumulated > the handle's numSamplesPerPixel, an own tile missing or given twice.  Then the accumulation is restarted, the planes are copied in, and kDigestTiles
 * runs over what lies in device memory: a tile whose digest differs from the blob's -> the accumulation restarted again, the frame counter as before the call,
 * RF_ERROR_CORRUPT, the handle usable.  Else the handle is indistinguishable -- through every read, every later render call and rf_renderer_state_digest -- from the
 * handle that saved, whatever process, handle history or shard layout that was.  Under a tile shard the accumulated count becomes the largest count among the handle's
 * own tiles (a rank without a tile: 0, as rf_comm_render_adaptive leaves it) and the frame's leading and smallest counts come from the blobs. */
typedef struct rf_state_digest
{
    uint64_t accumulation, albedo_coverage, normal_depth, moments, direct, bucket[15], counts;
    uint32_t family_on[5], family_samples[5];
    uint32_t frame_count, accumulated, num_tiles;
    uint32_t aov_flags, moments_on, direct_word, buckets_word;
    float    kernel_ms; /* kDigestTiles' own time in this call (two events on the handle's stream); not part of the state: two equal states report different times */
} rf_state_digest;
/* (the struct shares its name with the call, so it has no typedef: write `struct rf_checkpoint_info`) */
struct rf_checkpoint_info
{
    uint32_t   version, width, height, num_tiles, frame_count, accumulated, frame_leading_samples, frame_min_tile_samples;
    uint32_t   aov_flags, moments_on, direct_word, buckets_word;
    uint32_t   family_samples[5], family_restarted[5];
    uint32_t   num_bounces, stored_planes;
    uint64_t   total_bytes;
    rf_camera  camera;
    rf_sky     sky;
};
RF_API int rf_renderer_state_digest(rf_renderer* r, rf_state_digest* out);
RF_API int rf_renderer_save_checkpoint(rf_renderer* r, void* dst /* NULL = size query */, uint64_t* bytes);
RF_API int rf_checkpoint_info(const void* blob, uint64_t bytes, struct rf_checkpoint_info* out);
RF_API int rf_renderer_load_checkpoint(rf_renderer* r, const void* const* blobs, const uint64_t* sizes, uint32_t count);

/* Frame-end exchange behind the C ABI (no reference counterpart): one RCCL communicator per rank
 * (one process or host thread per GPU).  Rank 0 calls rf_comm_unique_id and hands the 128 bytes to the other ranks
 * through the host application's own channel; then every rank calls rf_comm_create (collective).
 * rf_renderer_gather_frame (collective, enqueued on the handle's stream behind the frame's kernels): every rank
 * ncclSend()s its compact tile buffer to `root`, the root posts all ncclRecv()s in one group (all xGMI ingress
 * links at once; no reduction, no ring) and un-tiles the shards into a row-major width*height float4 image in
 * device memory (*image_device_out on the root, NULL elsewhere; owned by the comm, valid until the next gather).
 * The renderer's tile shard must be (rank, world_size) of the comm.  SIDE EFFECT: what is sent is the accumulation of the
 * current parameters; if nothing has been rendered since the accumulation was last restarted (set_render_parameters, a new shard,
 * a newly bound buffer) the accumulation buffer is ZEROED on the handle's stream first (wgsl:47-49: a restarted frame starts from
 * zero), and that includes a caller-owned buffer bound with rf_renderer_bind_accumulation_buffer (its first
 * rf_renderer_accumulation_device_buffer() bytes).  RF_GATHER_LOOPBACK: the root's own shard also
 * goes through ncclSend/ncclRecv instead of being read in place (self-test of the RCCL path at world size 1).
 *
 * PLANES.  The exchange can carry every per-pixel sum the handle keeps, in the same single group of sends and receives.  The sums are numbered in a fixed order:
 * plane 0 = S (the image, always carried), 1 = AC = {albedo.rgb, coverage}, 2 = ND = {normal.xyz, depth} (both with RF_GATHER_AOVS), 3 = Q, the radiance second
 * moments (RF_GATHER_MOMENTS), 4 = {M.rgb, float(c)}, the robust mean of the rank's own pixels (RF_GATHER_ROBUST_MEAN; no sum: ROBUST MEAN ACROSS RANKS, below), 5 = D, the direct radiance sums (RF_GATHER_DIRECT: DIRECT SUMS ACROSS RANKS, below).  The sum planes are 0, 1, 2, 3 and 5.  A gather carries plane 0 and the planes its flags ask for, in that order: the plan is the one-plane plan once per carried plane
 * (rf_gather_plan_planes) -- on the root, for each plane in order, the receives of that plane in rank order; on a sender, its sends in plane order; per (source,
 * destination) pair the k-th send meets the k-th receive.  On the root every plane has its own staging area (rf_gather_layout; the areas lie one after another in one
 * allocation) and its own row-major width*height float4 image, and ONE kernel un-tiles all carried sum planes, D included (plane 4 has a launch of its own behind it, which
 * splits it into M and the trim image).  With neither flag a gather enqueues exactly what it
 * always did, and without RF_GATHER_ROBUST_MEAN or RF_GATHER_DIRECT exactly what it did before that flag existed, and rf_comm_last_exchange_ms brackets the whole exchange, the un-tile included, either way.
 * RF_GATHER_AOVS is refused with RF_ERROR_INVALID_ARGUMENT -- the state kept, nothing enqueued on this rank -- when the AOVs are off, when the AOV sample count
 * differs from the accumulated count (AOVs turned on partway through) or when no sample has been accumulated; RF_GATHER_MOMENTS likewise for the moments.  (A rank
 * whose shard holds no tile -- more ranks than tiles -- sends nothing, and only the switch is checked on it.)  The refusal of the non-uniform state of
 * rf_renderer_render_adaptive / rf_comm_render_adaptive comes first, with its own message: without RF_GATHER_TILE_COUNTS the gather carries no per-tile counts.  The ranks must run in step, as for the image: a rank that
 * is refused leaves its peers waiting for it.
 * The communicator records what the last gather left on the root: the carried planes, the frame size and the sample count N = the root handle's accumulated count
 * (0 on a root whose shard holds no tile).  A later gather replaces all of it (a plain gather drops the extra planes) and drops the denoised snapshot.
 *
 * DEFINING PROPERTY.  After the same samples, the gathered planes 0 .. 3 are bit for bit what a handle WITHOUT a tile shard reads through
 * rf_renderer_read_accumulation, rf_renderer_read_aovs (AC, ND) and rf_renderer_read_moments; rf_comm_read_denoised and rf_comm_noise_estimate are bit for bit that
 * handle's rf_renderer_read_denoised (after rf_renderer_denoise with the same parameters) and rf_renderer_noise_estimate: the same filter and estimate definitions
 * (above), over row-major instead of tile-major sums.
 * After the same samples, rf_comm_read_robust_mean on the root (mean, texels, trim, count) is bit for bit rf_renderer_read_robust_mean of one handle without a tile
 * shard after rf_renderer_robust_mean.  rf_comm_read_denoised after rf_comm_denoise_robust is bit for bit that handle's rf_renderer_read_denoised after
 * rf_renderer_denoise_robust with the same parameters.  Planes 0 to 3, rf_comm_denoise and rf_comm_noise_estimate of the same gather are what they are without the flag.
 *
 * ROBUST MEAN ACROSS RANKS.  The robust mean (the definition above) is per pixel -- no term looks at a neighbour -- so a sharded frame needs no bucket plane on the
 * root: with RF_GATHER_ROBUST_MEAN every rank that owns tiles first runs the combine over its own shard-compact bucket planes, on the handle's stream, with the one
 * count N = its accumulated count, into a shard-compact tile-major float4 buffer {M.rgb, float(c)} owned by the handle (allocated by the first such gather, freed
 * where the bucket planes are freed: a change of K, of the bit, or the buckets switched off; NOT the snapshot of rf_renderer_read_robust_mean, which a sharded handle cannot have).  That buffer travels as plane 4, in the same one
 * group, behind planes 0 .. 3 and in front of the counts: ONE plane on the wire instead of K, no K row-major images on the root, and the same bits by construction.
 * The trim count c <= 7 is exact in an f32 and M.a is the constant 1, so c rides in .w and no byte plane is exchanged.  The padding pixels of ragged tiles hold zero
 * sums, combine to M = 0, c = 0 and are never un-tiled.  On the root the un-tile of plane 4 leaves a row-major {M.rgb, 1} image and a row-major uint8 trim image in
 * device memory owned by the comm; the root's own shard is read in place at gather time, as the other planes are, so the root-side calls see the state AT THE GATHER
 * whatever is rendered afterwards.  The flag combines with every other flag, RF_GATHER_LOOPBACK included.
 * Refused with RF_ERROR_INVALID_ARGUMENT -- every check of the handle's state before anything is enqueued, the state kept, as for RF_GATHER_AOVS, the non-uniform
 * state's refusal first (the communicator's own checks -- an aborted transport -- follow the combine, which writes the handle's plane-4 buffer and nothing else) --
 * in the NON-UNIFORM state whatever the other flags are, unless the buckets carry RF_BUCKETS_SHARD_TILE_COUNTS (ONE COUNT PER TILE, below; RF_GATHER_TILE_COUNTS alone
 * does not lift it: plane 4 is combined with ONE count, and a whole-frame handle at
 * world size 1 may hold bucket planes per tile count after rf_renderer_render_adaptive -- rf_renderer_robust_mean is the call for that handle), when the buckets are off, when nothing has been accumulated, when the bucket sample count differs from the accumulated count (the message names both) or when
 * N < K (the message names K and N).  A rank whose shard holds no tile checks only the switch and sends nothing.  Under a tile shard the buckets keep ONE
 * count unless they carry RF_BUCKETS_SHARD_TILE_COUNTS: RF_BUCKETS_TILE_COUNTS alone makes no difference there, rf_comm_render_adaptive stays refused while such
 * buckets are on, and with RF_GATHER_TILE_COUNTS in the ordinary state the combine is unchanged, with or without either bit.
 * ONE COUNT PER TILE.  When the buckets carry RF_BUCKETS_SHARD_TILE_COUNTS, the handle is in the non-uniform state and the gather carries RF_GATHER_ROBUST_MEAN |
 * RF_GATHER_TILE_COUNTS, the rank's combine is the tiles combine (above) over its shard: pixel i of the shard-compact planes with the count of its slot, i / 1024 --
 * the device array the gather sends as counts, which also covers a rank whose own tiles share one count below the frame's leading count.  Plane 4 travels as ever; the
 * root's un-tile, rf_comm_read_robust_mean (sample_count = the largest count) and rf_comm_denoise_robust (each tile's count) are the same kernels.  After the same
 * rf_comm_render_adaptive / rf_renderer_render_adaptive calls M, the texels, the trim image, the counts and the robust-denoised frame on the root are bit for bit one
 * whole-frame handle's (rf_renderer_robust_mean, rf_renderer_read_tile_samples, rf_renderer_denoise_robust); planes 0 .. 3, rf_comm_denoise and rf_comm_noise_estimate
 * are what they are without the flag.  Refused, before anything is enqueued and the state kept: without RF_GATHER_TILE_COUNTS (the non-uniform state's own refusal,
 * first); without the bit (the refusal above, word for word); when the buckets do not cover the accumulation; when the smallest count known to the rank is below K
 * (the message names K and that count) -- after rf_comm_render_adaptive that is the FRAME's smallest count, which every rank holds, so all ranks are refused alike and
 * no peer waits; otherwise the smallest of the rank's own tiles (a whole-frame handle at world size 1 after rf_renderer_render_adaptive).
 * rf_comm_gathered_planes reports the flag.  rf_comm_read_plane and rf_comm_plane_device serve the sum planes alone (0 .. 3 and 5): plane 4 is read through
 * rf_comm_read_robust_mean(c, r, rgba, bgra8, trim, K, sample_count): row-major width*height*4 floats {M.rgb, 1}, BGRA8 texels (kTonemap over M with
 * accumulatedSamples = 1 and the exposure of the handle passed in, enqueued on that handle's stream and waited for), one trim byte per pixel, the K of the combine and
 * sample_count = the N the gather recorded (rf_comm_gathered_planes' N: 0 on a root whose shard holds no tile, unless the counts travelled).  Any pointer may be NULL.
 * rf_comm_denoise_robust(c, r, params): rf_comm_denoise with prep's colour c = the gathered M (rf_renderer_denoise_robust's filter), per tile count when the gather
 * carried counts; needs RF_GATHER_AOVS | RF_GATHER_ROBUST_MEAN; refused as rf_comm_denoise is (N = 0, a tile without a sample, bad parameters).  The result is the
 * comm's ordinary denoise snapshot, read with rf_comm_read_denoised, and is dropped by the next gather.
 * Out of scope: `rf-render --gpus N --buckets` and `rf-render --gpus N --adaptive` stay refused; raw bucket planes are not gathered (every rank's
 * rf_renderer_read_buckets is still the way to them).
 *
 * DIRECT SUMS ACROSS RANKS.  With RF_GATHER_DIRECT the gather carries D (rf_renderer_set_direct) as plane 5: a sum plane like planes 0 .. 3, the rank's
 * shard-compact tile-major float4 buffer on the wire, in the same one group, behind plane 4 when both travel and in front of the counts.  On the root it has its own
 * staging area and its own row-major image, un-tiled by the sum planes' one launch as one more plane of it.  The flag combines with every other flag,
 * RF_GATHER_LOOPBACK included; without it a gather posts and enqueues exactly what it did before the flag existed.
 * DEFINING PROPERTY.  After the same samples, plane 5 on the root is bit for bit what one handle without a tile shard reads through rf_renderer_read_direct;
 * rf_comm_read_denoised after rf_comm_denoise_split is bit for bit that handle's rf_renderer_read_denoised after rf_renderer_denoise_split with the same parameters;
 * planes 0 .. 4 and every other root-side call of the same gather are what they are without the flag.
 * Refused with RF_ERROR_INVALID_ARGUMENT -- every check before anything is enqueued or cleared, the state kept, as for RF_GATHER_AOVS: when the direct sums are
 * off; when no sample has been accumulated; when the direct sample count differs from the accumulated count (D turned on partway through; the message names both).  A
 * rank whose shard holds no tile checks only the switch and sends nothing.  In the NON-UNIFORM state the refusal of a gather without RF_GATHER_TILE_COUNTS comes
 * first, as ever; with the counts, D must carry RF_DIRECT_TILE_COUNTS (the message names the bit) -- the adaptive calls refuse plain 1 in the first place.
 * On the root, after such a gather:
 *   rf_comm_read_plane / rf_comm_plane_device serve plane 5 (plane 4 stays "plane out of range": it is read through rf_comm_read_robust_mean; planes >= 6 do not
 *   exist); after a gather without the flag plane 5 is refused with a message that names RF_GATHER_DIRECT.  rf_comm_gathered_planes reports the flag.
 *   rf_comm_denoise_split(c, r, direct, indirect): the split-component denoiser (the definition above) enqueued on the handle's stream over the gathered S, D, AC and
 *   ND where they lie; needs RF_GATHER_AOVS | RF_GATHER_DIRECT (the message names what is missing); a NULL parameter set = that component's default; each tile with
 *   its own count when the gather carried RF_GATHER_TILE_COUNTS (rf_denoise_split_tiles' filter); refused as rf_comm_denoise is (N = 0, a tile without a sample, bad
 *   parameters).  The result is the comm's one denoise snapshot, read with rf_comm_read_denoised: of rf_comm_denoise, rf_comm_denoise_robust and this call the last
 *   one wins, and the next gather drops it.
 *   rf_comm_read_split(c, r, direct_rgba, indirect_rgba): the two components as means, row-major width*height*4 floats each (either pointer may be NULL, not both):
 *   direct = {D.rgb / float(n), 1}, indirect = {(S.rgb - D.rgb) / float(n), 1} -- per channel one f32 subtraction, then one IEEE division -- with n = N, or the
 *   pixel's tile's count when the gather carried counts.  A tile with count 0 is handled as rf_comm_read_mean handles it: {0, 0, 0, 1} in both images; without the
 *   counts N = 0 (a root whose shard holds no tile) is refused.  One kernel over the gathered planes, enqueued on the handle's stream, then waited for, as
 *   rf_comm_read_mean.  Needs RF_GATHER_DIRECT.  These are the expressions `rf-render --direct / --indirect` evaluates on the host.
 * Out of scope: `rf-render --gpus N --direct / --indirect / --denoise-split` stays refused.
 *
 * The root-side calls below take the communicator and the ROOT's handle, whose stream, device and exposure they use.  Each returns RF_ERROR_INVALID_ARGUMENT, with a
 * message that says which case applies, when this rank was not the root of the last gather, when no gather has been made, or when the last gather did not carry the
 * planes the call needs (the AOVs for the denoiser, the moments for the estimate, the plane asked for).
 * rf_comm_gathered_planes: RF_GATHER_AOVS / RF_GATHER_MOMENTS / RF_GATHER_TILE_COUNTS / RF_GATHER_ROBUST_MEAN / RF_GATHER_DIRECT as carried by the last gather, its frame size and N; any pointer may be NULL.
 * rf_comm_read_plane: waits for the handle's stream and copies a sum plane (0 .. 3, 5) to the host (width*height*4 floats, row-major).  rf_comm_plane_device: the plane's
 * image in device memory (owned by the comm, valid until the next gather; work on it belongs on the handle's stream).
 * rf_comm_denoise: the a-trous denoiser (the definition above, one count N) enqueued on the handle's stream over the gathered planes 0, 1, 2 where they lie: the
 * sums never leave the device.  params NULL = the defaults; bad parameters are refused as everywhere else.  The snapshot is owned by the comm (its buffers are
 * allocated by the first call) and is dropped by the next gather.  rf_comm_read_denoised: as rf_renderer_read_denoised; RF_ERROR_INVALID_ARGUMENT without a snapshot.
 * rf_comm_noise_estimate: the noise estimate (the definition above) over the gathered planes 0 and 3; enqueued on the handle's stream, then waited for, as
 * rf_renderer_noise_estimate.  Also refused when N < 2.  error_map, tile_sum and tile_max may be NULL.
 *
 * TILE-ADAPTIVE SAMPLING ACROSS RANKS.  rf_comm_render_adaptive(c, r, params, result) is rf_renderer_render_adaptive for a frame whose tiles are dealt to the ranks of a
 * communicator: COLLECTIVE, every rank calls it with the same parameters (the caller's duty, as the frame size is).  r's tile shard must be (rank, world_size) of c.
 * The frame's leading count L is the largest accumulated count of any rank (one all-reduce at the start of the call).  A rank's active tiles are those of its shard
 * at L -- it may have none, and a rank without an active tile, or without a tile, traces nothing but takes part in the exchanges -- and from there the loop is
 * rf_renderer_render_adaptive's own, over the rank's tiles, with no further exchange: a tile stops on its own estimate, which reads that tile's S and Q alone, at the
 * same checks as on one GPU.  At the end three all-reduces give the frame's figures, and every rank's frame counter stands where the leading tiles' ranks left
 * theirs: whatever is traced next, after a restart of the accumulation too, is the sample a handle without a tile shard would trace.
 * DEFINING PROPERTY.  For any sequence of calls with the same parameters on every rank, the count and S, Q, AC, ND of every tile are bit for bit what ONE handle
 * without a tile shard holds after the same sequence of rf_renderer_render_adaptive calls.  That includes continuation: a tile below the frame's L is never revived,
 * also on a rank whose tiles all share one lower count.
 * Every argument and precondition is checked BEFORE the first exchange, so that a refusal (RF_ERROR_INVALID_ARGUMENT; the state kept) leaves no peer waiting when
 * all ranks are refused alike: rf_renderer_render_adaptive's checks of the moments, the AOV flags, check_every and the target, then the communicator's rank and
 * world size against the shard.
 * *result (may be NULL): rank = rf_adaptive_result over this rank's tiles (stopped_tiles: those below the FRAME's leading count; pixel_samples: in-frame pixels x
 * count over this rank's tiles; last: over this rank's tiles active in the last pass); frame_leading_samples and frame_min_tile_samples: the largest and the smallest
 * tile count of the frame afterwards; max_rank_pixel_samples: the pixel-samples the busiest rank traced in this call (what the call's duration follows).
 * Every rank keeps the two frame counts.  While they differ the handle is in the NON-UNIFORM state on every rank, also on one whose own tiles share one count:
 * rf_renderer_render, rf_renderer_render_until, rf_renderer_set_tile_shard and a gather without RF_GATHER_TILE_COUNTS refuse as above.  The reads behave as they do
 * under a tile shard: this rank's pixels, each tile with its own divisor, zeros elsewhere; rf_renderer_read_accumulation reports the rank's own leading count.  When
 * the two are equal every rank is in the ordinary state.  A restart of the accumulation clears it all.
 * RF_GATHER_TILE_COUNTS: in the same one group, behind its planes, every sender also sends the counts of its shard's tiles from device memory (one uint32 per tile,
 * in the order of rf_renderer_shard_tiles); the root stages them rank after rank (rf_gather_plan_counts lists the operations, in words) and one small kernel leaves
 * one count per tile of the frame in device memory.  Allowed in the ordinary state (every tile then carries the accumulated count); required in the non-uniform one.
 * The root waits for such an exchange.  rf_comm_gathered_planes reports the flag, and N is the largest count.  After such a gather, on the root:
 *   rf_comm_denoise: each tile with its own count (rf_denoise_tiles' filter; every count must be >= 1); rf_comm_read_denoised reports the largest count.
 *   rf_comm_noise_estimate: Nf = float(the tile's count) (rf_noise_estimate_tiles' estimate; every count must be >= 2); out->samples = the largest count.
 *   rf_comm_read_tile_samples: the counts (tile_samples may be NULL) and the number of tiles.
 *   rf_comm_read_mean: row-major width*height*4 floats {S.rgb / float(the tile's count), 1}; {0, 0, 0, 1} in a tile without a sample.
 * The gathered planes, counts, mean, denoised frame and estimate are bit for bit the un-sharded handle's reads (rf_renderer_read_tile_samples, rf_renderer_read_mean,
 * rf_renderer_denoise in the non-uniform state, rf_renderer_noise_estimate). */
/* MI355X devices this process sees (hipGetDeviceCount; 0 without a GPU).  No reference counterpart (the reference asks Dawn for one adapter,
 * gpu_context.cpp); what a host application sizes `--gpus N` against. */
RF_API int rf_device_count(int32_t* count_out);
typedef struct rf_comm rf_comm;
#define RF_COMM_ID_BYTES 128
#define RF_GATHER_LOOPBACK 1u
#define RF_GATHER_AOVS    2u  /* with the image: AC = {albedo.rgb, coverage} and ND = {normal.xyz, depth} */
#define RF_GATHER_MOMENTS 4u  /* with the image: Q */
#define RF_GATHER_TILE_COUNTS 8u /* with the image: one sample count per tile (tile-adaptive sampling across ranks, below) */
#define RF_GATHER_ROBUST_MEAN 16u /* with the image: the robust mean of every rank's own pixels, combined before the exchange: plane 4 = {M.rgb, float(c)} */
#define RF_GATHER_DIRECT 32u /* with the image: D, the direct radiance sums (rf_renderer_set_direct): plane 5 */
RF_API int  rf_comm_unique_id(uint8_t id_out[RF_COMM_ID_BYTES]);
RF_API int  rf_comm_create(const uint8_t id[RF_COMM_ID_BYTES], uint32_t rank, uint32_t world_size, int32_t device_ordinal, rf_comm** out);
RF_API void rf_comm_destroy(rf_comm* c);
RF_API int  rf_renderer_gather_frame(rf_renderer* r, rf_comm* c, uint32_t root, uint32_t flags, void** image_device_out /* NULL ok */);
/* fsMain's display transform (wgsl:59-63) for a row-major float4 SUM image in device memory -- the frame
 * rf_renderer_gather_frame left on the root: num_pixels BGRA8 texels to the host, with the handle's exposure. */
RF_API int  rf_renderer_tonemap_device_image(rf_renderer* r, const void* image_device, uint64_t num_pixels, uint32_t samples, uint32_t* dst_bgra8);
/* Root: wait for the exchange and copy the gathered image to the host (width*height*4 floats, row-major, the
 * layout of rf_renderer_read_accumulation). */
RF_API int  rf_comm_read_frame(rf_comm* c, rf_renderer* r, float* dst);
RF_API int  rf_comm_gathered_planes(const rf_comm* c, uint32_t* flags_out, uint32_t* width, uint32_t* height, uint32_t* samples);
RF_API int  rf_comm_read_plane(rf_comm* c, rf_renderer* r, uint32_t plane /* 0..3, 5 */, float* dst);   /* width*height*4 floats, row-major */
RF_API int  rf_comm_plane_device(rf_comm* c, uint32_t plane, void** device_ptr);
RF_API int  rf_comm_denoise(rf_comm* c, rf_renderer* r, const rf_denoise_parameters* params);          /* NULL = defaults */
RF_API int  rf_comm_read_denoised(rf_comm* c, rf_renderer* r, float* rgba, uint32_t* bgra8, uint32_t* sample_count);
RF_API int  rf_comm_noise_estimate(rf_comm* c, rf_renderer* r, rf_noise_estimate* out, float* error_map, float* tile_sum, float* tile_max);
typedef struct rf_comm_adaptive_result
{
    rf_adaptive_result rank;          /* this rank's tiles only; "stopped" = below the FRAME's leading count */
    uint32_t frame_leading_samples;   /* max tile count over all ranks */
    uint32_t frame_min_tile_samples;  /* min tile count over all ranks (tiles that exist) */
    uint64_t max_rank_pixel_samples;  /* the busiest rank's pixel-samples traced by this call */
} rf_comm_adaptive_result;
RF_API int  rf_comm_render_adaptive(rf_comm* c, rf_renderer* r, const rf_adaptive_parameters* params, rf_comm_adaptive_result* result);
RF_API int  rf_comm_read_tile_samples(rf_comm* c, uint32_t* tile_samples /* may be NULL */, uint32_t* num_tiles);
RF_API int  rf_comm_read_mean(rf_comm* c, rf_renderer* r, float* rgba);
/* After a gather with RF_GATHER_ROBUST_MEAN, on the root (ROBUST MEAN ACROSS RANKS, above); any out pointer may be NULL */
RF_API int  rf_comm_read_robust_mean(rf_comm* c, rf_renderer* r, float* rgba, uint32_t* bgra8, uint8_t* trim, uint32_t* K, uint32_t* sample_count);
RF_API int  rf_comm_denoise_robust(rf_comm* c, rf_renderer* r, const rf_denoise_parameters* params);   /* NULL = defaults; needs RF_GATHER_AOVS | RF_GATHER_ROBUST_MEAN */
/* After a gather with RF_GATHER_DIRECT, on the root (DIRECT SUMS ACROSS RANKS, above) */
RF_API int  rf_comm_denoise_split(rf_comm* c, rf_renderer* r, const rf_denoise_parameters* direct, const rf_denoise_parameters* indirect); /* NULL = that component's default; needs RF_GATHER_AOVS | RF_GATHER_DIRECT */
RF_API int  rf_comm_read_split(rf_comm* c, rf_renderer* r, float* direct_rgba, float* indirect_rgba);  /* either may be NULL, not both */
/* The feature export (above) over the gathered planes, on the root: into caller-owned device memory on the root's device; sample_count (may be NULL): N */
RF_API int  rf_comm_export_features(rf_comm* c, rf_renderer* r, const rf_feature_request* req, void* dst_device, uint64_t dst_bytes, uint32_t* sample_count);
/* Max over ranks of *value (timing plumbing for hosts without another collective layer; also a barrier). */
RF_API int  rf_comm_all_reduce_max(rf_comm* c, rf_renderer* r /* NULL: default stream */, double* value);
/* What RCCL reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice); any pointer may be NULL.
 * A scaling line that says N GPUs carries rccl_ranks == N from here. */
RF_API int  rf_comm_info(const rf_comm* c, uint32_t* rccl_ranks, uint32_t* rccl_rank, int32_t* device_ordinal);
/* *local_out = 1: the communicator runs on the LOCAL TEST TRANSPORT, not on RCCL.  With RF_COMM_TRANSPORT=local in the environment rf_comm_unique_id makes an
 * id that rf_comm_create recognises: N communicators of ONE process (one host thread per rank, any number of them on one GPU) then execute the very plan
 * rf_gather_plan lists -- same staging offsets, same un-tile kernel -- with each ncclSend / ncclRecv pair replaced by a device-to-device copy between the ranks'
 * buffers.  It exists so that the multi-owner exchange runs on single-GPU boxes (RCCL refuses two ranks per device); rf_comm_info then reports the world the
 * caller asked for, and THIS call is how a measurement proves it did not come from such a communicator.  No reference counterpart
 * (single-device: reference_path_tracer.cpp:565-595). */
RF_API int  rf_comm_transport(const rf_comm* c, uint32_t* local_out);
/* Device time of this rank's LAST rf_renderer_gather_frame (HIP events on the handle's stream around the sends / receives and, on the root, the un-tile):
 * what the one exchange of the multi-GPU path costs once the rank's own frame has drained.  Waits for that exchange; -1 before the first.  (No reference
 * counterpart: the reference is single-device, reference_path_tracer.cpp:565-595.) */
RF_API int  rf_comm_last_exchange_ms(rf_comm* c, double* ms_out);
/* Device memory held by a handle: path state + queues (148 B per path slot: eight packed xyz streams, two float4 streams, five u32 queues / lists; 180 B while the first-hit
 * AOVs are on; allocated on demand for the largest batch traced; the radiance second moments add 16 B per pixel of the shard's tiles and nothing per path slot, so
 * they are not part of these figures),
 * the batch depth in use (lowered automatically when the device has less free memory than the default wants: same image,
 * more batches) and the resident scene.  Any pointer may be NULL. */
RF_API int  rf_renderer_memory_info(const rf_renderer* r, uint64_t* path_state_bytes, uint64_t* paths_allocated, uint64_t* max_paths_per_batch, uint64_t* scene_bytes);
/* Which BVH record layout the handle reads in the closest-hit / any-hit launch of each bounce -- what it picked BY ITSELF for this scene at upload (from the
 * binary16 surface-area ratio of the boxes, the tree's size against the Infinity Cache, the median leaf size against the sun disc) plus any option set since.
 * No reference counterpart (the reference has one node layout, bvh.hpp:14-21); lets a caller -- and the parity tests -- see that a result was produced by the
 * layouts the renderer would use on its own.  Layout codes: RF_LAYOUT_*. */
enum { RF_LAYOUT_BINARY = 0, RF_LAYOUT_COMPACT = 1, RF_LAYOUT_HOT = 2, RF_LAYOUT_QUAD = 3, RF_LAYOUT_QUAD_HALF = 4, RF_LAYOUT_QUAD_LOCAL = 5, RF_LAYOUT_OCT = 6,
       RF_LAYOUT_SCALAR = 7, RF_LAYOUT_PACKET = 8 };
typedef struct rf_layout_info
{
    uint32_t closest_layout[16];      /* bounce 1..16 */
    uint32_t shadow_layout[16];
    uint32_t shadow_cached[16];       /* 1: the any-hit launch of that bounce starts at the occluder cache's entries */
    uint32_t occluder_hint_levels;    /* 0: the cache remembers leaves; n: a record n quad levels above the leaf */
    uint32_t shadow_first_look_from_bounce;
    uint32_t dense_leaf_min;          /* leaf phases with a leaf of this many triangles or more run over dense (lane, triangle) pairs; 0: never */
    uint32_t legacy_layouts_compiled; /* 1: a build with RF_EXP_LEGACY_LAYOUTS (the compact-capable / 32-byte records and the packet kernel exist) */
    float    quad_half_area_ratio;
    float    reserved;
    uint64_t tree_bytes;              /* quad records + triangle records */
} rf_layout_info;
RF_API int  rf_renderer_layout_info(const rf_renderer* r, rf_layout_info* out);
/* The launches of bounce `bounce` (1 .. the handle's bounce count) of the handle's NEXT batch of num_samples samples, as the host driver would enqueue them in its
 * present state (scene, options, camera, AOV / moment switches, counting, and whether an earlier batch has warmed the occluder grid): read from the very plans the
 * render path enqueues from; nothing is enqueued.  No reference counterpart (the reference has one kernel per pass).  None of this shows in the image -- the
 * contract is "same image with any setting" -- so this is where a test can pin which kernel instantiation runs, at which refill threshold, claim size and exit
 * vote, and which words of the device counters each launch reads.  Every field is one uint32_t; *_word: offset in 32-bit words from the start of the batch's counter
 * block; kernels: 0 = one ray per thread, 1 = packet (RF_EXP_LEGACY_LAYOUTS builds), 2 = kTraceWide; layouts: RF_LAYOUT_*.  RF_ERROR_INVALID_ARGUMENT for a bounce
 * outside 1 .. the bounce count or num_samples == 0. */
typedef struct rf_launch_plan
{
    /* the batch */
    uint32_t num_samples, num_bounces;
    uint32_t sample_perm;         /* 1: the samples of a pixel are traced in the order of their direction key */
    uint32_t dense_raygen;        /* 1: kRaygen computes its queue positions (no atomic) */
    uint32_t const_origin;        /* 1: the primary launch takes the pinhole camera's origin as an argument, kRaygen writes no origins */
    uint32_t primary_layout;
    uint32_t occluder_grid, occluder_scale_bits, occluder_mask; /* the occluder grid's cells: scale (the bits of a float) and mask; 0: no grid */
    uint32_t runs;                /* 1: the sums run in the LDS-staged kernels */
    uint32_t tile_list;           /* 1: the tile-list kernel adds the image and the moments (rf_renderer_render_adaptive's batches; never through this call) */
    uint32_t accumulate_kernel;   /* 0 = one thread per pixel, 1 = runs, 2 = tile list */
    uint32_t accumulate_pixels, aov_pixels, moment_pixels; /* pixels per workgroup of each sum's launch; 0: not launched */
    uint32_t raygen_count_word;
    /* the closest-hit launch */
    uint32_t closest_kernel, closest_layout, closest_counting, closest_nearest, closest_dense, closest_refill_min, closest_chunk, closest_leaf_vote, closest_flags, closest_extra_lds;
    uint32_t closest_count_word, closest_cursor_word;
    /* kShade */
    uint32_t shade_sorted, shade_aov, shade_flags, shade_sort_scale, shade_grid_cap;
    /* the any-hit launch */
    uint32_t shadow_kernel, shadow_layout, shadow_counting, shadow_nearest, shadow_dense, shadow_refill_min, shadow_chunk, shadow_leaf_vote, shadow_flags, shadow_extra_lds;
    uint32_t shadow_count_word, shadow_cursor_word;
    uint32_t shadow_cached;       /* it starts at the occluder cache's entries */
    uint32_t shadow_first_look;   /* it runs behind kShadowFirstLook */
    uint32_t shadow_self;         /* kShade settles the shadow rays that their own triangle answers and lists the rest */
    uint32_t shadow_source;       /* whose count and list it reads: 0 = kShade's output queue, 1 = kShade's list of unsettled shadow rays, 2 = kShadowFirstLook's list */
    uint32_t look_flags, look_count_word, look_list_word; /* kShadowFirstLook's flags, the count it reads, the length of the list it leaves; 0 without a first look */
} rf_launch_plan;
RF_API int  rf_renderer_launch_plan(const rf_renderer* r, uint32_t bounce, uint32_t num_samples, rf_launch_plan* out);
/* Host helpers (no GPU needed). */
/* The point-to-point operations rank `rank` posts (one RCCL group) for a gather to `root`: exactly the list
 * rf_renderer_gather_frame executes.  Offsets / counts in tiles (1024 float4): a receive lands at offset_tiles of the root's
 * staging area (rf_gather_layout), a send starts at offset_tiles of the rank's own compact buffer.  ops == NULL: count query. */
typedef struct rf_gather_op
{
    uint32_t is_send, peer, offset_tiles, count_tiles;
} rf_gather_op;
RF_API int rf_gather_plan(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t root, uint32_t flags, rf_gather_op* ops, uint32_t* num_ops);
/* The operations a gather with RF_GATHER_TILE_COUNTS posts for the counts, behind those of its planes: {is_send, peer, offset_words, count_words} -- the fields of
 * rf_gather_op read as uint32 words (one per tile) of the root's count staging area (receive) or of the rank's own counts (send).  Host arithmetic. */
RF_API int rf_gather_plan_counts(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t root, uint32_t flags, rf_gather_op* ops, uint32_t* num_ops);
/* The same for a gather with RF_GATHER_AOVS / RF_GATHER_MOMENTS / RF_GATHER_ROBUST_MEAN / RF_GATHER_DIRECT in `flags`: the one-plane list once per carried plane (plane 0 = S, 1 = AC, 2 = ND, 3 = Q, 4 = the robust mean, 5 = D), the
 * receives of planes 0 .. 4 first (plane after plane, each in rank order), then their sends in plane order.  offset_tiles counts from the start of THAT plane's own staging
 * area (a receive) or compact buffer (a send).  With neither flag the list is rf_gather_plan's with plane = 0.  With RF_GATHER_DIRECT the list is the list without the
 * flag followed by rf_gather_plan's tagged plane 5 (its receives, then its send).  ops == NULL: count query. */
typedef struct rf_gather_plane_op
{
    uint32_t is_send, peer, plane, offset_tiles, count_tiles;
} rf_gather_plane_op;
RF_API int rf_gather_plan_planes(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t root, uint32_t flags, rf_gather_plane_op* ops,
                                 uint32_t* num_ops);
/* The staging layout the gather uses: shards rank after rank, each rank's tiles in ascending tile id.
 * rank_first_tile[world_size + 1], tile_slot[tiles] (staging position of a tile, in tiles), tile_owner[tiles]. */
RF_API int rf_gather_layout(uint32_t width, uint32_t height, uint32_t world_size, uint32_t* rank_first_tile, uint32_t* tile_slot, uint32_t* tile_owner);
RF_API int rf_tiles_for_rank(uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size, uint32_t* tile_ids, uint32_t* num_tiles);
RF_API int rf_untile(const float* compact, const uint32_t* tile_ids, uint32_t num_tiles, uint32_t width, uint32_t height, float* image);

/* ---------------------------------------------------------------------------------------------
 * BVH queries on the GPU
 * ------------------------------------------------------------------------------------------ */
/* The bvh-visualizer pixel loop (src/bvh-visualizer/main.cpp:60-78): pinhole camera
 * (generateCameraRay, src/common/camera.cpp:44-52), u = j/W, v = 1-(i+1)/H, tMax = FLT_MAX.
 * nodes_visited[W*H] row-major is bit-exact with the CPU reference's BvhStats::nodesVisited. */
RF_API int rf_renderer_trace_primary_stats(rf_renderer* r, const rf_camera* camera, uint32_t width, uint32_t height,
                                           uint32_t* nodes_visited, uint8_t* hit /* NULL ok */, float* t /* NULL ok */,
                                           uint32_t* triangle_tests /* NULL ok */);
/* bool rayIntersectBvh(const Ray&, span<BvhNode>, span<Positions>, float tMax, Intersection&,
 * BvhStats*) (src/common/ray_intersection.hpp:43-49) for a batch of rays (6 floats each: origin,
 * direction).  triangle[i] = 0xFFFFFFFF on a miss. */
RF_API int rf_renderer_intersect_rays(rf_renderer* r, const float* rays6, uint64_t num_rays, float t_max, uint32_t* triangle,
                                      float* t, float* uv, float* p, uint32_t* nodes_visited, uint32_t* triangle_tests);
/* shadowRay (wgsl:321-368): visibility[i] = 1.0 if nothing is hit, else 0.0. */
RF_API int rf_renderer_occluded_rays(rf_renderer* r, const float* rays6, uint64_t num_rays, float t_max, float* visibility);

/* Cast rays from device memory: what do these rays hit, and what is the surface there?  The rays are read from caller-owned device memory, traced by the renderer's
 * production traversal (kTraceWide, with the record layout and parameters the launch policy picks for an incoherent closest-hit / any-hit launch of this scene; the
 * reference-order scalar traversal where the scene's wide records are unusable), and the hit and the chosen surface attributes are written into caller-owned device
 * memory -- any number of rays, in chunks of one path-state allocation (option cast_chunk caps the chunk; 0 = automatic).
 * Values.  triangle, t, bary and position are bit for bit rf_intersect_bvh_batch's for the same ray; on a miss every float output is +0 and the two index outputs are
 * 0xFFFFFFFF.  The attributes come from the shading stage's own device functions in its order of operations (f32, one IEEE operation at a time, no contraction): the
 * first-hit AOVs of a 1-sample render are this call's albedo, normal and t on that sample's primary rays, bit for bit up to the sign of a zero: the AOVs are SUMS,
 * +0 + value after one sample, so a component this call gives as -0 reads +0 there.  visibility is bit for bit rf_renderer_occluded_rays'.
 * Rays that start far outside the scene are answered correctly but, on the conservative record layouts, one by one by the reference-order traversal inside the
 * kernel (rf_ray_query.hip's header): slower, by an amount that has not been measured.
 * Stream rule.  The call is enqueued on the handle's stream and then waited for: when it returns the outputs may be used from any stream.  The caller makes sure the
 * inputs are complete before the call.
 * Read-only for the handle: every sum, count, snapshot and the frame counter, rf_renderer_state_digest, the image a later render produces, rf_stats and
 * rf_renderer_get_bounce_stats are unchanged by it (the query's rays are not render rays: they count into a counter block of their own, no field of rf_stats sees
 * them).  The path state is scratch between render calls and is used; a call with more rays per chunk than the path state holds grows it, as a render call does.
 * The occluder cache and the first-look bookkeeping are neither used nor disturbed.  A tile shard does not matter: every handle holds the whole scene.
 * num_rays == 0 returns 0 and reads, checks and touches nothing else.  RF_ERROR_INVALID_ARGUMENT, decided before any launch and with the state kept: a NULL batch, NULL
 * origins or directions; a stride below 3; an unknown kind; a non-zero reserved word; no output given; a CLOSEST output with RF_RAYS_ANY, or visibility with
 * RF_RAYS_CLOSEST; t_max NaN; an input or output that hipPointerGetAttributes does not report as device memory of the handle's device for its whole byte range (host,
 * registered and managed memory are refused); an output range that overlaps another output or an input. */
#define RF_RAYS_CLOSEST 0u   /* rayIntersectBvh's answer, plus the attributes at the hit */
#define RF_RAYS_ANY     1u   /* shadowRay's answer */
typedef struct rf_ray_batch
{
    const float* origins;      /* device; ray i at origins + i * origin_stride (floats), 3 floats */
    const float* directions;   /* device; likewise with direction_stride */
    uint32_t     origin_stride, direction_stride;   /* in floats, >= 3 */
    uint64_t     num_rays;
    float        t_max;
    uint32_t     kind;         /* RF_RAYS_CLOSEST | RF_RAYS_ANY */
    uint32_t     reserved[2];  /* 0 */
    /* outputs: device, contiguous, 4-byte aligned, NULL = not wanted; at least one is given */
    uint32_t* triangle;         /* N     CLOSEST  leaf-order index, 0xFFFFFFFF on a miss */
    float*    t;                /* N     CLOSEST */
    float*    bary;             /* N x 2 CLOSEST  u, v (weights 1-u-v, u, v) */
    float*    position;         /* N x 3 CLOSEST  the OFFSET hit point (offsetRay): the origin a bounce or shadow ray starts from */
    float*    geometric_normal; /* N x 3 CLOSEST  normalize(cross(e1, e2)), the normal offsetRay pushes along */
    float*    normal;           /* N x 3 CLOSEST  unit shading normal: n = (b0 n0 + b1 n1) + b2 n2 (wgsl:396), then exactly the first-hit AOV's rule: (0,0,0) where dot(n,n) is 0 or not finite, else normalize(n) */
    float*    texcoord;         /* N x 2 CLOSEST  (b0 uv0 + b1 uv1) + b2 uv2, not wrapped */
    float*    albedo;           /* N x 3 CLOSEST  evalTexture at that texcoord: the value kShade multiplies the throughput by */
    uint32_t* texture;          /* N     CLOSEST  texture descriptor index, 0xFFFFFFFF on a miss */
    float*    visibility;       /* N     ANY      1.0 if nothing is hit in (1e-5, t_max), else 0.0 */
} rf_ray_batch;
RF_API int rf_renderer_cast_rays(rf_renderer* r, const rf_ray_batch* batch);

/* ---------------------------------------------------------------------------------------------
 * BVH queries on the HOST (no GPU needed; re-entrant pure functions)
 * ------------------------------------------------------------------------------------------ */
/* nlrs::Intersection {p, t} (src/common/ray_intersection.hpp:15-19) plus the triangle hit and its barycentrics. */
typedef struct rf_intersection
{
    float    p[3];     /* offset hit point (offsetRay, ray_intersection.cpp:17-35) */
    float    t;
    uint32_t triangle; /* index into the triangle array (BVH leaf order); 0xFFFFFFFF on a miss */
    float    u, v;
} rf_intersection;
/* nlrs::BvhStats (ray_intersection.hpp:38-41) plus triangle tests and the high-water mark of the pending-node list. */
typedef struct rf_bvh_stats
{
    uint32_t nodes_visited, triangle_tests, stack_high_water;
} rf_bvh_stats;
/* bool rayIntersectBvh(const Ray&, span<const BvhNode>, span<const Positions>, float tMax, Intersection&, BvhStats* = nullptr)
 * (src/common/ray_intersection.hpp:43-49, .cpp:138-213): the reference's CPU query -- focus picking (src/pt/main.cpp:214-225),
 * bvh-visualizer (src/bvh-visualizer/main.cpp:60-78) -- on the host, bit-identical hit / t / p / nodesVisited.
 * positions: num_triangles records of position_stride_bytes = 36 (Positions, the .pt file's bvhPositionAttributes) or
 * 48 (PositionAttribute).  *hit_out = 1 / 0 replaces the bool; stats may be NULL.  Pending far children are kept in a list
 * that grows on demand (the reference's 32-entry array is overrun past depth 32).  Malformed links -> RF_ERROR_RUNTIME. */
RF_API int rf_intersect_bvh(const float ray6[6], const void* nodes48, uint64_t num_nodes, const void* positions, uint32_t position_stride_bytes,
                            uint64_t num_triangles, float t_max, rf_intersection* out, rf_bvh_stats* stats /* NULL ok */, int* hit_out);
/* The same for num_rays rays on num_threads host threads (0 = all hardware threads; static blocks of rays).
 * hit[i] = 1 / 0; any output array may be NULL. */
RF_API int rf_intersect_bvh_batch(const float* rays6, uint64_t num_rays, const void* nodes48, uint64_t num_nodes, const void* positions,
                                  uint32_t position_stride_bytes, uint64_t num_triangles, float t_max, uint32_t num_threads, uint8_t* hit,
                                  rf_intersection* out, rf_bvh_stats* stats);
/* The bvh-visualizer pixel loop on the host (src/bvh-visualizer/main.cpp:60-78; the CPU twin of
 * rf_renderer_trace_primary_stats): rows [row_begin, row_end) of a width x height grid, u = j/W, v = 1-(i+1)/H, tMax = FLT_MAX,
 * static blocks of scanlines over num_threads threads (0 = all; 1 = what the reference does).  Outputs are indexed
 * i*width + j over the whole grid; any of them may be NULL. */
RF_API int rf_bvh_visualizer_pass(const rf_camera* camera, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, const void* nodes48,
                                  uint64_t num_nodes, const void* positions, uint32_t position_stride_bytes, uint64_t num_triangles, uint32_t num_threads,
                                  uint32_t* nodes_visited, uint8_t* hit, float* t, uint32_t* triangle_tests);

/* ---------------------------------------------------------------------------------------------
 * CPU-side scene preparation (host code, runs without a GPU)
 * ------------------------------------------------------------------------------------------ */
/* Bvh buildBvh(std::span<const Positions>) (src/common/bvh.hpp:33, bvh.cpp:263-291).
 * nodes_out: room for 2*num_triangles 48-B nodes; triangle_indices_out[src] = leaf-order index.
 * RF_ERROR_INVALID_ARGUMENT, nothing written, when a position is NaN or infinite (the message names the first such triangle);
 * so do rf_build_bvh_gpu, decided on the host before the device is touched, and the bakes (rf_pt_format_from_gltf /
 * _from_triangles) with either builder. */
RF_API int rf_build_bvh(const float* positions36, uint64_t num_triangles, void* nodes_out, uint64_t* num_nodes_out,
                        uint64_t* triangle_indices_out, int32_t* depth_out /* NULL ok */);

/* The same build on the GPU (device_ordinal): identical node bytes -- except the sign of a zero box coordinate where a
 * node holds both -0 and +0 at that extreme (rf_bvh_gpu.hip header), which no ray can see -- and identical triangle_indices_out
 * (the order inside multi-triangle leaves decides closest-hit ties between coincident triangles; the
 * reference's is whatever its standard library's std::partition leaves -- rf_build_bvh uses libstdc++'s,
 * and the GPU builder reproduces that permutation).  Replaces the
 * single-threaded recursion of src/common/bvh.cpp:81-260 for large scenes.
 * build_ms_out (NULL ok): device time of the build, triangles already resident.  Fails without a
 * GPU (no CPU fallback: call rf_build_bvh). */
RF_API int rf_build_bvh_gpu(const float* positions36, uint64_t num_triangles, void* nodes_out, uint64_t* num_nodes_out,
                            uint64_t* triangle_indices_out, int32_t* depth_out /* NULL ok */, int32_t device_ordinal,
                            float* build_ms_out /* NULL ok */);

/* Host-only self-check of the render path's BVH record layouts for a flattened tree of 48-B nodes: the 64-byte
 * "children in the parent" records, the compact-capable records and the 32-byte records are built as rf_renderer_create builds
 * them and every variant must decode to the same child planes and child words.  Also checked: the leaf boxes and the occluder-cache
 * entries written into the triangle records (every entry is 0 or the index of a quad record that really lies above its leaf, 1 to 3 levels).  *flags_out: bit 0 = boxes regular (wide
 * layout usable), bit 1 = compact-capable records usable, bit 2 = 32-byte records usable.  No reference counterpart. */
RF_API int rf_check_wide_layouts(const void* nodes48, uint64_t num_nodes, uint32_t* flags_out);
/* The same check, plus (bit 3 = quad records usable, bit 4 = half-precision quad records usable) the figure the renderer's default
 * layout choice rests on: the surface area of the half-precision (binary16, conservative) child boxes relative to the exact ones,
 * summed over the tree -- the closest-hit launches read the half-precision records where it is <= 1.075 and the local-grid records
 * (bit 5, from bounce 2) beyond; the shadow launches the local-grid records from bounce 2 where it is <= 1.10 (bounce 1: the half-precision
 * records where they suit) and the exact quad records otherwise.  Either output may be NULL. */
RF_API int rf_wide_layout_stats(const void* nodes48, uint64_t num_nodes, uint32_t* flags_out, float* quad_half_area_ratio);

/* Camera createCamera(origin, lookAt, aperture, focusDistance, vfov, aspectRatio)
 * (src/common/camera.cpp:7-42); vfov in radians (Angle::asRadians). */
RF_API int rf_create_camera(const float origin[3], const float look_at[3], float aperture, float focus_distance,
                            float vfov_radians, float aspect_ratio, rf_camera* out);
/* FlyCameraController::getCamera (src/pt/fly_camera_controller.cpp:12-22,138-148). */
RF_API int rf_fly_camera(const float position[3], float yaw_degrees, float pitch_degrees, float vfov_degrees, float aperture,
                         float focus_distance, float aspect_ratio, rf_camera* out);
/* The camera lambda of src/bvh-visualizer/main.cpp:36-55 for a 48-B root node. */
RF_API int rf_bvh_visualizer_camera(const void* root_node48, float aspect_ratio, rf_camera* out);

/* sky_state_new / sky_state_radiance (src/hw-skymodel/hw_skymodel.h:35,44); state33 = params[27],
 * sky_radiances[3], solar_radiances[3].  Returns the reference's sky_state_result value. */
RF_API int   rf_sky_state_new(float elevation, float turbidity, const float albedo[3], float state33[33]);
RF_API float rf_sky_state_radiance(const float state33[33], float theta, float gamma, int channel);
/* AlignedSkyState(const Sky&) (src/pt/aligned_sky_state.hpp:44-70): 40 floats. */
RF_API int rf_aligned_sky_state(const rf_sky* sky, float out40[40]);

/* ---------------------------------------------------------------------------------------------
 * .pt scene files  (replaces nlrs::PtFormat + serialize/deserialize, src/pt-format/pt_format.hpp:18-43)
 * ------------------------------------------------------------------------------------------ */
typedef struct rf_pt_format rf_pt_format;

typedef struct rf_pt_format_view
{
    const void*     bvh_nodes;                    uint64_t num_bvh_nodes;
    const void*     bvh_position_attributes;      uint64_t num_bvh_position_attributes;      /* 36 B */
    const void*     triangle_position_attributes; uint64_t num_triangle_position_attributes; /* 48 B */
    const void*     triangle_vertex_attributes;   uint64_t num_triangle_vertex_attributes;   /* 80 B */
    const float*    vertex_positions;             uint64_t num_vertex_positions;             /* vec4 */
    const float*    vertex_normals;               uint64_t num_vertex_normals;               /* vec4 */
    const float*    vertex_tex_coords;            uint64_t num_vertex_tex_coords;            /* vec2 */
    const uint32_t* vertex_indices;               uint64_t num_vertex_indices;
    const uint64_t* model_vertex_positions;       uint64_t num_model_vertex_positions;       /* {offset,count} pairs */
    const uint64_t* model_vertex_normals;         uint64_t num_model_vertex_normals;
    const uint64_t* model_vertex_tex_coords;      uint64_t num_model_vertex_tex_coords;
    const uint64_t* model_vertex_indices;         uint64_t num_model_vertex_indices;
    const uint32_t* model_base_color_texture_indices; uint64_t num_model_base_color_texture_indices;
    uint64_t        num_textures;
} rf_pt_format_view;

/* PtFormat(std::filesystem::path gltfPath) (pt_format.cpp:20-151): glTF/GLB -> BVH + GPU arrays. */
/* BVH builder used by rf_pt_format_from_gltf / _from_triangles: -1 = host (default), >= 0 = rf_build_bvh_gpu on that device. */
RF_API int rf_pt_format_set_bvh_builder(int32_t gpu_device_or_minus_one);
RF_API int rf_pt_format_from_gltf(const char* gltf_path, rf_pt_format** out);
/* deserialize(InputStream&, PtFormat&) (pt_format.cpp:271-321) from a file / from memory.
 * Wrong magic -> RF_ERROR_RUNTIME with the reference's exact messages (src/tests/pt_format.cpp:192-210). */
RF_API int rf_pt_format_load(const char* pt_path, rf_pt_format** out);
RF_API int rf_pt_format_deserialize(const void* data, uint64_t size, rf_pt_format** out);
/* serialize(OutputStream&, const PtFormat&) (pt_format.cpp:240-269). */
RF_API int rf_pt_format_save(const rf_pt_format* f, const char* pt_path);
RF_API int rf_pt_format_serialize(const rf_pt_format* f, void* dst /* NULL = size query */, uint64_t* size);
/* Build a PtFormat from caller arrays (triangle soup in source order + textures): runs buildBvh +
 * reorderAttributes + the GPU-layout packing of pt_format.cpp:40-79.  Raster-mesh arrays are left
 * empty.  Used by the synthetic-scene generator. */
RF_API int rf_pt_format_from_triangles(const float* positions36, const float* normals36, const float* tex_coords24,
                                       const uint32_t* texture_indices, uint64_t num_triangles, const rf_texture* textures,
                                       uint64_t num_textures, rf_pt_format** out);
/* Texture::fromMemory (src/common/texture.hpp:41, texture.cpp:12-54): PNG or JPEG bytes -> width*height
 * BGRA8 texels packed as u32 (b | g<<8 | r<<16 | 255<<24).  pixels == NULL: size query. */
RF_API int  rf_texture_from_memory(const void* data, uint64_t size, uint32_t* width, uint32_t* height, uint32_t* pixels);
RF_API int  rf_pt_format_view_get(const rf_pt_format* f, rf_pt_format_view* out);
RF_API int  rf_pt_format_texture(const rf_pt_format* f, uint64_t index, rf_texture* out);
RF_API void rf_pt_format_destroy(rf_pt_format* f);
/* Fill an rf_scene (the four spans of nlrs::Scene, src/pt/main.cpp:150-157) from a PtFormat.
 * textures_out must hold num_textures entries. */
RF_API int rf_pt_format_scene(const rf_pt_format* f, rf_scene* scene_out, rf_texture* textures_out);

#ifdef __cplusplus
}
#endif
#endif /* RAYFINDER_AMD_H */
