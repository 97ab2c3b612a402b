// rf-render <scene.pt|scene.glb> [--width W] [--height H] [--spp N] [--bounces B] [--vfov deg]
//           [--zenith deg] [--azimuth deg] [--turbidity t] [--exposure-stops s] [--out image.png]
//           [--pfm image.pfm] [--aov-albedo a.pfm] [--aov-normal n.pfm] [--aov-depth d.pfm] [--denoise d.png] [--denoise-pfm d.pfm]
//           [--denoise-iterations L] [--denoise-sigma-color s] [--denoise-sigma-normal s] [--denoise-sigma-depth s]
//           [--noise-map m.pfm] [--noise-target t] [--noise-check-every k] [--gpus N]
//           [--adaptive T] [--adaptive-min n] [--adaptive-every n] [--sample-map s.pfm]
//           [--buckets K] [--buckets-tile-counts] [--robust-mean out.pfm|out.png] [--trim-map t.pfm] [--denoise-robust d.png]
//           [--direct d.pfm] [--indirect i.pfm] [--denoise-split out.png]
// Offline counterpart of the interactive `pt` app (src/pt/main.cpp): same default camera pose,
// sky and exposure; renders all samples and writes the tonemapped image (and optionally the
// mean radiance as PFM).  --gpus N: one host thread per GPU, the image tile-sharded across them, one RCCL
// gather to GPU 0 at frame end (rf_renderer_gather_frame), which also carries the AOV sums and the second moments when an option below needs them
// (RF_GATHER_AOVS / RF_GATHER_MOMENTS: the same one group of sends and receives, one un-tile kernel on rank 0).
// --aov-*: the means of the first-hit AOVs (rf_renderer_set_aovs): albedo and normal over the samples, depth over the samples that hit
// something (a one-channel PFM, 0 where none did).  With --gpus N > 1 they are read from the planes gathered on rank 0 (rf_comm_read_plane).
// --denoise / --denoise-pfm: the edge-aware a-trous denoiser (rf_renderer_denoise) over the frame, guided by the AOVs (any --denoise* option turns them on
// from the first sample).  With --gpus N > 1 it runs once, on rank 0, over the gathered sums where they lie in device memory (rf_comm_denoise):
// the same inputs, the same kernels, the same bytes whatever N.
// --noise-map: the per-pixel relative standard error of the frame (rf_renderer_noise_estimate's error map, a one-channel PFM) from the radiance second moments
// (rf_renderer_set_moments, on from the first sample).  With --gpus N > 1 the estimate runs once, on rank 0, over the gathered accumulation and moments
// (rf_comm_noise_estimate): the same map whatever N.
// --adaptive T [--adaptive-min n] [--adaptive-every n]: tile-adaptive sampling (rf_renderer_render_adaptive): every 32x32 tile is sampled until its mean error is <= T,
// checked every n samples (default 8) from --adaptive-min samples on, --spp at the latest; the image is the per-tile mean.  --gpus 1 only, and not with --noise-target.
// With --aov-* / --denoise* the AOVs are kept per tile count (RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS): the AOV PFMs are divided by each pixel's tile count, and the
// denoiser (rf_renderer_denoise) divides every pixel by its own tile's count before it filters.
// --sample-map s.pfm: the sample count of every pixel's tile (a one-channel PFM)
// --buckets K: keep K bucket sums (rf_renderer_set_buckets; K odd, 3 .. 15) from the first sample.  --robust-mean: the firefly-robust mean of the frame
// (rf_renderer_robust_mean) as a PFM, or tonemapped as a PNG; --trim-map: how many buckets the combine cut from each end, per pixel (a one-channel PFM);
// --denoise-robust: the robust mean through the denoiser (rf_renderer_denoise_robust; turns the AOVs on, takes the --denoise-* parameters) as a PNG.  These three need
// --buckets.  --gpus 1 only and not with --adaptive: the bucket planes are not carried by the frame gather and keep one sample count for the frame.
// --buckets-tile-counts (a switch, no value): keep the bucket sums per tile count (K | RF_BUCKETS_TILE_COUNTS).  With it --buckets K --adaptive T runs on --gpus 1, and
// --robust-mean, --trim-map and --denoise-robust write the adaptive frame's images, every pixel combined with its own tile's count (--adaptive-min >= K, or a tile
// may stop with an empty bucket and the combine is refused).
// --direct d.pfm / --indirect i.pfm: the light split of the frame from the direct radiance sums (rf_renderer_set_direct, on from the first sample): D / N, the mean
// of each sample's radiance after bounce 1 (sky on a primary miss, the first hit's sun term), and (S - D) / N per channel (it may be negative).  --denoise-split out.png:
// the two components denoised separately and recombined (rf_renderer_denoise_split at its defaults; turns the AOVs on).  --gpus 1 only: the frame gather does not
// carry D.  With --adaptive T the direct sums and the AOVs are kept per tile count (1 | RF_DIRECT_TILE_COUNTS, RF_AOV_FIRST_HIT | RF_AOV_TILE_COUNTS): the two PFMs
// divide every pixel by its own tile's count, and the split denoiser divides every pixel by its tile's count before it filters.
// --noise-target t [--noise-check-every k]: stop as soon as the frame's mean error is <= t, checked every k samples (default 8), at --spp at the latest
// (rf_renderer_render_until).  One GPU only: stopping several ranks in step is not implemented.
// --checkpoint FILE [--checkpoint-every N]: rf_renderer_save_checkpoint into FILE (a temporary file, then a rename) after every N samples and at the end; with
// --adaptive / --noise-target after the call.  --resume FILE: the four switches from rf_checkpoint_info, rf_renderer_load_checkpoint, then the render continues to
// --spp: the images are those of an uninterrupted run.  --gpus 1 only.
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>

int main(int argc, char** argv)
{
    if (argc < 2)
    {
        std::printf("Usage: rf-render <scene.pt|scene.glb> [--width W] [--height H] [--spp N] [--bounces B] [--vfov deg]\n"
                    "                 [--zenith deg] [--azimuth deg] [--turbidity t] [--exposure-stops s] [--out image.png] [--pfm image.pfm]\n"
                    "                 [--aov-albedo a.pfm] [--aov-normal n.pfm] [--aov-depth d.pfm] [--gpus N]\n"
                    "  --aov-albedo / --aov-normal / --aov-depth: mean first-hit albedo, shading normal (3-channel PFM) and depth (1-channel PFM, 0 where\n"
                    "  no sample hit) -- the auxiliary inputs of a denoiser\n"
                    "                 [--denoise d.png] [--denoise-pfm d.pfm] [--denoise-iterations L] [--denoise-sigma-color s] [--denoise-sigma-normal s]\n"
                    "                 [--denoise-sigma-depth s]\n"
                    "  --denoise / --denoise-pfm: the frame through the edge-aware a-trous denoiser guided by the AOVs (defaults: L 5, sigmas 1, 0.1, 0.1)\n"
                    "                 [--adaptive T] [--adaptive-min n] [--adaptive-every n] [--sample-map s.pfm]\n"
                    "  --adaptive: sample every 32x32 tile until its mean error is <= T (checked every n samples, default 8; --spp at the latest); --sample-map: the\n"
                    "  tiles' sample counts (1-channel PFM).  --gpus 1 only, not with --noise-target; with --aov-* / --denoise* the AOVs and the denoiser use each\n"
                    "  tile's own sample count\n"
                    "                 [--buckets K] [--buckets-tile-counts] [--robust-mean out.pfm|out.png] [--trim-map t.pfm] [--denoise-robust d.png]\n"
                    "  --buckets: keep K bucket sums (K odd, 3 .. 15); --robust-mean: the firefly-robust median-of-means image (PFM, or PNG tonemapped); --trim-map: the\n"
                    "  buckets cut from each end per pixel (1-channel PFM); --denoise-robust: the robust mean through the denoiser.  --gpus 1 only, not with --adaptive\n"
                    "  unless --buckets-tile-counts (no value) is given: the bucket sums then follow the tiles' sample counts, and the three images are the adaptive frame's\n"
                    "                 [--direct d.pfm] [--indirect i.pfm] [--denoise-split out.png]\n"
                    "  --direct / --indirect: the mean direct light (after bounce 1) and the rest, (S - D) / N (3-channel PFMs); --denoise-split: the two denoised\n"
                    "  separately and recombined, at the split defaults.  --gpus 1 only; with --adaptive the direct sums follow the tiles' sample counts and the\n"
                    "  three images are the adaptive frame's\n"
                    "                 [--noise-map m.pfm] [--noise-target t] [--noise-check-every k]\n"
                    "  --noise-map: the per-pixel relative standard error of the frame (1-channel PFM); --noise-target: stop once the frame's mean error is <= t,\n"
                    "  checked every k samples (default 8), at --spp at the latest (one GPU only)\n"
                    "                 [--checkpoint FILE] [--checkpoint-every N] [--resume FILE]\n"
                    "  --checkpoint: save the render's state at the end, and after every N samples with --checkpoint-every (with --adaptive / --noise-target: after the\n"
                    "  call); --resume: set the sums' switches as the file says, load it and continue to --spp.  --gpus 1 only\n");
        return 0;
    }
    uint32_t    W = 1920, H = 1080, spp = 64, bounces = 2; // UI defaults src/pt/main.cpp:46-60
    uint32_t    gpus = 1;
    float       vfov = 70.0f, zenith = 30.0f, azimuth = 0.0f, turbidity = 1.0f;
    int         stops = 2;
    std::string out = "render.png", pfm, aovAlbedo, aovNormal, aovDepth, denoisePng, denoisePfm;
    rf_denoise_parameters denoiseParams{};
    rf_denoise_default_parameters(&denoiseParams);
    bool denoising = false;
    std::string noiseMap;
    float       noiseTarget = 0.0f;
    bool        noiseTargetSet = false;
    uint32_t    noiseCheckEvery = 8;
    std::string sampleMap;
    bool        adaptive = false;
    rf_adaptive_parameters adaptiveParams{0.0f, 8u, 0u, 0u};
    rf_adaptive_result     adaptiveResult{};
    uint32_t    buckets = 0;
    bool        bucketsTileCounts = false;
    std::string robustMean, trimMap, denoiseRobust;
    std::string directPfm, indirectPfm, denoiseSplit;
    std::string checkpointPath, resumePath;
    uint32_t    checkpointEvery = 0;
    for (int i = 2; i < argc; i += 2)
    {
        // (the one switch without a value)
        if (std::string(argv[i]) == "--buckets-tile-counts")
        {
            bucketsTileCounts = true;
            --i;
            continue;
        }
        if (i + 1 >= argc) break;
        const std::string k = argv[i];
        const char*       val = argv[i + 1];
        if (k == "--width") W = static_cast<uint32_t>(std::atoi(val));
        else if (k == "--height") H = static_cast<uint32_t>(std::atoi(val));
        else if (k == "--spp") spp = static_cast<uint32_t>(std::atoi(val));
        else if (k == "--bounces") bounces = static_cast<uint32_t>(std::atoi(val));
        else if (k == "--vfov") vfov = static_cast<float>(std::atof(val));
        else if (k == "--zenith") zenith = static_cast<float>(std::atof(val));
        else if (k == "--azimuth") azimuth = static_cast<float>(std::atof(val));
        else if (k == "--turbidity") turbidity = static_cast<float>(std::atof(val));
        else if (k == "--exposure-stops") stops = std::atoi(val);
        else if (k == "--gpus") gpus = static_cast<uint32_t>(std::max(1, std::atoi(val)));
        else if (k == "--out") out = val;
        else if (k == "--pfm") pfm = val;
        else if (k == "--aov-albedo") aovAlbedo = val;
        else if (k == "--aov-normal") aovNormal = val;
        else if (k == "--aov-depth") aovDepth = val;
        else if (k == "--denoise") denoisePng = val, denoising = true;
        else if (k == "--denoise-pfm") denoisePfm = val, denoising = true;
        else if (k == "--denoise-iterations") denoiseParams.iterations = static_cast<uint32_t>(std::atoi(val)), denoising = true;
        else if (k == "--denoise-sigma-color") denoiseParams.sigma_color = static_cast<float>(std::atof(val)), denoising = true;
        else if (k == "--denoise-sigma-normal") denoiseParams.sigma_normal = static_cast<float>(std::atof(val)), denoising = true;
        else if (k == "--denoise-sigma-depth") denoiseParams.sigma_depth = static_cast<float>(std::atof(val)), denoising = true;
        else if (k == "--noise-map") noiseMap = val;
        else if (k == "--noise-target") noiseTarget = static_cast<float>(std::atof(val)), noiseTargetSet = true;
        else if (k == "--noise-check-every") noiseCheckEvery = static_cast<uint32_t>(std::max(1, std::atoi(val)));
        else if (k == "--adaptive") adaptiveParams.target_tile_error = static_cast<float>(std::atof(val)), adaptive = true;
        else if (k == "--adaptive-min") adaptiveParams.min_samples = static_cast<uint32_t>(std::max(0, std::atoi(val)));
        else if (k == "--adaptive-every") adaptiveParams.check_every = static_cast<uint32_t>(std::max(1, std::atoi(val)));
        else if (k == "--sample-map") sampleMap = val;
        else if (k == "--buckets") buckets = static_cast<uint32_t>(std::max(0, std::atoi(val)));
        else if (k == "--robust-mean") robustMean = val;
        else if (k == "--trim-map") trimMap = val;
        else if (k == "--denoise-robust") denoiseRobust = val;
        else if (k == "--direct") directPfm = val;
        else if (k == "--indirect") indirectPfm = val;
        else if (k == "--denoise-split") denoiseSplit = val;
        else if (k == "--checkpoint") checkpointPath = val;
        else if (k == "--checkpoint-every") checkpointEvery = static_cast<uint32_t>(std::max(0, std::atoi(val)));
        else if (k == "--resume") resumePath = val;
        else
        {
            std::fprintf(stderr, "unknown option %s\n", k.c_str());
            return 1;
        }
    }
    if (noiseTargetSet && gpus > 1)
    {
        std::fprintf(stderr, "--noise-target needs --gpus 1: stopping several ranks in step at a noise target is not implemented (render a fixed --spp and use --noise-map)\n");
        return 1;
    }
    if (adaptive && (gpus > 1 || noiseTargetSet))
    {
        std::fprintf(stderr, "--adaptive needs --gpus 1 and does not go with --noise-target (the per-tile counts are carried neither by the frame gather nor by render_until)\n");
        return 1;
    }
    const bool robust = !robustMean.empty() || !trimMap.empty() || !denoiseRobust.empty();
    if (bucketsTileCounts && buckets == 0u)
    {
        std::fprintf(stderr, "--buckets-tile-counts needs --buckets K (K odd, 3 .. 15)\n");
        return 1;
    }
    if ((buckets != 0u || robust) && (gpus > 1 || (adaptive && !bucketsTileCounts)))
    {
        std::fprintf(stderr, "--buckets / --robust-mean / --trim-map / --denoise-robust need --gpus 1 and do not go with --adaptive (the bucket sums are not carried by the "
                             "frame gather and keep one sample count for the frame)\n");
        return 1;
    }
    if (robust && buckets == 0u)
    {
        std::fprintf(stderr, "--robust-mean / --trim-map / --denoise-robust need --buckets K (K odd, 3 .. 15)\n");
        return 1;
    }
    const bool direct = !directPfm.empty() || !indirectPfm.empty() || !denoiseSplit.empty();
    if (direct && gpus > 1)
    {
        std::fprintf(stderr, "--direct / --indirect / --denoise-split need --gpus 1 (the direct sums are not carried by the frame gather)\n");
        return 1;
    }
    if ((!checkpointPath.empty() || !resumePath.empty()) && gpus > 1)
    {
        std::fprintf(stderr, "--checkpoint / --resume need --gpus 1 (saving and loading one blob per rank is not wired into this tool; rf_renderer_save_checkpoint and "
                             "rf_renderer_load_checkpoint work on tile-sharded handles)\n");
        return 1;
    }
    if (checkpointEvery != 0u && checkpointPath.empty())
    {
        std::fprintf(stderr, "--checkpoint-every needs --checkpoint FILE\n");
        return 1;
    }
    // --resume: the file is read and its header checked before the scene is loaded
    std::vector<unsigned char> resumeBlob;
    struct rf_checkpoint_info  resumeInfo{};
    if (!resumePath.empty())
    {
        std::FILE* f = std::fopen(resumePath.c_str(), "rb");
        if (!f)
        {
            std::fprintf(stderr, "cannot open %s\n", resumePath.c_str());
            return 1;
        }
        unsigned char chunk[1 << 16];
        for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) != 0u;) resumeBlob.insert(resumeBlob.end(), chunk, chunk + got);
        std::fclose(f);
        rfCheck(rf_checkpoint_info(resumeBlob.data(), resumeBlob.size(), &resumeInfo), "checkpoint info");
    }
    rf_pt_format*     pt = loadScene(argv[1]);
    rf_pt_format_view v;
    rf_pt_format_view_get(pt, &v);
    std::vector<rf_texture> textures(std::max<uint64_t>(v.num_textures, 1));
    rf_scene                scene;
    rfCheck(rf_pt_format_scene(pt, &scene, textures.data()), "scene");

    rf_renderer_descriptor desc{};
    desc.render_params.width = W;
    desc.render_params.height = H;
    const float position[3] = {1.22f, 1.25f, -1.25f};
    rfCheck(rf_fly_camera(position, 129.64f, -13.73f, vfov, 0.0f, 10.0f, static_cast<float>(W) / static_cast<float>(H), &desc.render_params.camera), "camera");
    desc.render_params.num_samples_per_pixel = spp;
    desc.render_params.num_bounces = bounces;
    desc.render_params.sky = rf_sky{turbidity, {1.0f, 1.0f, 1.0f}, zenith, azimuth};
    desc.render_params.exposure = 1.0f / std::exp2(static_cast<float>(stops));
    // One host thread per GPU (gpus > 1: the image is tile-sharded; one RCCL gather to rank 0 at frame end).
    uint8_t commId[RF_COMM_ID_BYTES] = {};
    if (gpus > 1) rfCheck(rf_comm_unique_id(commId), "RCCL unique id");
    std::atomic<unsigned long long> closestRays{0}, shadowRays{0};
    std::vector<uint32_t>           bgra(static_cast<size_t>(W) * H);
    std::vector<float>              acc;
    // the error map, and the samples actually rendered
    const bool         noise = !noiseMap.empty() || noiseTargetSet || adaptive;
    std::vector<uint32_t> tileSamples;
    std::vector<float> errorMap;
    rf_noise_estimate  estimate{};
    uint32_t           sppReached = spp;
    if (!noiseMap.empty()) errorMap.resize(static_cast<size_t>(W) * H);
    if (!pfm.empty()) acc.resize(static_cast<size_t>(W) * H * 4);
    // first-hit AOV sums of the whole frame ({albedo, coverage}, {normal, depth}), read on rank 0 when a file is made from them: from the handle, or (several ranks)
    // from the planes the gather left there
    const bool         aovFiles = !aovAlbedo.empty() || !aovNormal.empty() || !aovDepth.empty();
    const bool         aovs = aovFiles || denoising || !denoiseRobust.empty() || !denoiseSplit.empty();
    // the direct sums and, next to them, the accumulation (rank 0; one GPU), and the split-denoised frame's texels
    std::vector<float>    directSum, directAcc;
    std::vector<uint32_t> splitBgra;
    uint32_t              directSamples = 0;
    if (!directPfm.empty() || !indirectPfm.empty()) directSum.resize(static_cast<size_t>(W) * H * 4), directAcc.resize(static_cast<size_t>(W) * H * 4);
    if (!denoiseSplit.empty()) splitBgra.resize(static_cast<size_t>(W) * H);
    // the robust mean's snapshot (rank 0; one GPU): the mean, its display texels, the trim counts, and the robust mean through the denoiser
    std::vector<float>    robustRgba;
    std::vector<uint32_t> robustBgra, robustDenoisedBgra;
    std::vector<uint8_t>  robustTrim;
    if (robust) robustRgba.resize(static_cast<size_t>(W) * H * 4), robustBgra.resize(static_cast<size_t>(W) * H), robustTrim.resize(static_cast<size_t>(W) * H);
    if (!denoiseRobust.empty()) robustDenoisedBgra.resize(static_cast<size_t>(W) * H);
    std::vector<float>    denoisedRgba;
    std::vector<uint32_t> denoisedBgra;
    if (denoising) denoisedRgba.resize(static_cast<size_t>(W) * H * 4), denoisedBgra.resize(static_cast<size_t>(W) * H);
    std::vector<float> aovAc, aovNd;
    uint32_t           aovSamples = 0;
    if (aovFiles) aovAc.resize(static_cast<size_t>(W) * H * 4), aovNd.resize(static_cast<size_t>(W) * H * 4);
    double       seconds = 0.0;
    // rank r runs on device r -- modulo the devices there are: with more ranks than GPUs RCCL refuses the communicator (two ranks on one device), the local TEST transport
    // (RF_COMM_TRANSPORT=local in the environment: rf_comm.hip) runs them all on what is there -- how the exchange is exercised with many owners on a single-GPU box
    int32_t deviceCount = 0;
    rfCheck(rf_device_count(&deviceCount), "device count");
    const auto   worker = [&](uint32_t rank) {
        rf_renderer_descriptor d = desc;
        d.device_ordinal = static_cast<int32_t>(deviceCount > 0 ? rank % static_cast<uint32_t>(deviceCount) : rank);
        rf_renderer* renderer = nullptr;
        rfCheck(rf_renderer_create(&d, &scene, &renderer), "create renderer");
        rf_comm* comm = nullptr;
        if (gpus > 1)
        {
            rfCheck(rf_renderer_set_tile_shard(renderer, rank, gpus), "tile shard");
            rfCheck(rf_comm_create(commId, rank, gpus, d.device_ordinal, &comm), "RCCL communicator");
        }
        // (--adaptive: the AOV sums follow the per-tile counts)
        if (aovs) rfCheck(rf_renderer_set_aovs(renderer, RF_AOV_FIRST_HIT | (adaptive ? RF_AOV_TILE_COUNTS : 0u)), "AOVs");
        if (noise) rfCheck(rf_renderer_set_moments(renderer, 1), "moments");
        if (buckets != 0u) rfCheck(rf_renderer_set_buckets(renderer, buckets | (bucketsTileCounts ? RF_BUCKETS_TILE_COUNTS : 0u)), "buckets");
        // (--adaptive: the direct sums follow the per-tile counts too)
        if (direct) rfCheck(rf_renderer_set_direct(renderer, static_cast<int>(1u | (adaptive ? RF_DIRECT_TILE_COUNTS : 0u))), "direct sums");
        // --resume: the four switches as the checkpoint's header has them, then the load; the render continues to --spp
        uint32_t resumed = 0;
        if (!resumeBlob.empty())
        {
            rfCheck(rf_renderer_set_aovs(renderer, resumeInfo.aov_flags), "AOVs of the checkpoint");
            rfCheck(rf_renderer_set_moments(renderer, static_cast<int>(resumeInfo.moments_on)), "moments of the checkpoint");
            rfCheck(rf_renderer_set_direct(renderer, static_cast<int>(resumeInfo.direct_word)), "direct sums of the checkpoint");
            rfCheck(rf_renderer_set_buckets(renderer, resumeInfo.buckets_word), "buckets of the checkpoint");
            const void* const blobs[1] = {resumeBlob.data()};
            const uint64_t    sizes[1] = {resumeBlob.size()};
            rfCheck(rf_renderer_load_checkpoint(renderer, blobs, sizes, 1), "load checkpoint");
            resumed = resumeInfo.accumulated;
        }
        // --checkpoint: the blob to a temporary file beside the target, then renamed over it
        const auto saveCheckpoint = [&] {
            if (checkpointPath.empty()) return;
            uint64_t bytes = 0;
            rfCheck(rf_renderer_save_checkpoint(renderer, nullptr, &bytes), "checkpoint size");
            std::vector<unsigned char> blob(bytes);
            rfCheck(rf_renderer_save_checkpoint(renderer, blob.data(), &bytes), "save checkpoint");
            const std::string tmp = checkpointPath + ".tmp";
            std::FILE*        f = std::fopen(tmp.c_str(), "wb");
            const bool        ok = f && std::fwrite(blob.data(), 1, bytes, f) == bytes;
            if (f) std::fclose(f);
            if (!ok || std::rename(tmp.c_str(), checkpointPath.c_str()) != 0)
            {
                std::fprintf(stderr, "cannot write %s\n", checkpointPath.c_str());
                std::exit(1);
            }
        };
        const auto t0 = std::chrono::steady_clock::now();
        if (adaptive) rfCheck(rf_renderer_render_adaptive(renderer, &adaptiveParams, &adaptiveResult), "adaptive render");
        else if (noiseTargetSet)
        {
            rfCheck(rf_renderer_render_until(renderer, noiseTarget, noiseCheckEvery, spp - std::min(spp, resumed), &sppReached, &estimate), "render to the noise target");
            sppReached += resumed;
        }
        else
        {
            // (in steps of --checkpoint-every samples, a checkpoint after each: the samples and their order are those of one call)
            uint32_t todo = spp - std::min(spp, resumed);
            while (todo != 0u)
            {
                const uint32_t n = checkpointEvery != 0u ? std::min(checkpointEvery, todo) : todo;
                rfCheck(rf_renderer_render(renderer, n), "render");
                todo -= n;
                if (checkpointEvery != 0u && todo != 0u) saveCheckpoint();
            }
        }
        saveCheckpoint();
        // (several ranks: the sums the outputs need travel with the image, in the one exchange)
        void* gathered = nullptr;
        if (comm) rfCheck(rf_renderer_gather_frame(renderer, comm, 0, (aovs ? RF_GATHER_AOVS : 0u) | (!noiseMap.empty() ? RF_GATHER_MOMENTS : 0u), &gathered), "gather");
        rfCheck(rf_renderer_synchronize(renderer), "synchronize");
        if (rank == 0) seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        rf_stats stats;
        rfCheck(rf_renderer_get_stats(renderer, &stats), "stats");
        closestRays += stats.closest_rays;
        shadowRays += stats.shadow_rays;
        if (rank == 0)
        {
            uint32_t n = 0;
            if (comm)
            {
                // the gathered frame lies un-tiled in device memory here: tonemap, denoise and estimate it where it is
                rfCheck(rf_renderer_tonemap_device_image(renderer, gathered, static_cast<uint64_t>(W) * H, spp, bgra.data()), "tonemap");
                if (!acc.empty()) rfCheck(rf_comm_read_frame(comm, renderer, acc.data()), "read frame");
                rfCheck(rf_comm_gathered_planes(comm, nullptr, nullptr, nullptr, &aovSamples), "gathered planes");
                if (aovFiles)
                {
                    rfCheck(rf_comm_read_plane(comm, renderer, 1, aovAc.data()), "read AOVs");
                    rfCheck(rf_comm_read_plane(comm, renderer, 2, aovNd.data()), "read AOVs");
                }
                if (denoising)
                {
                    rfCheck(rf_comm_denoise(comm, renderer, &denoiseParams), "denoise");
                    rfCheck(rf_comm_read_denoised(comm, renderer, denoisedRgba.data(), denoisedBgra.data(), &n), "read denoised");
                }
                if (!noiseMap.empty()) rfCheck(rf_comm_noise_estimate(comm, renderer, &estimate, errorMap.data(), nullptr, nullptr), "noise estimate");
            }
            else
            {
                if (aovFiles) rfCheck(rf_renderer_read_aovs(renderer, aovAc.data(), aovNd.data(), &aovSamples), "read AOVs");
                if (!noiseMap.empty()) rfCheck(rf_renderer_noise_estimate(renderer, &estimate, errorMap.data(), nullptr, nullptr), "noise estimate");
                rfCheck(rf_renderer_read_tonemapped(renderer, bgra.data()), "tonemap");
                if (!acc.empty()) rfCheck(adaptive ? rf_renderer_read_mean(renderer, acc.data()) : rf_renderer_read_accumulation(renderer, acc.data(), &n), "read accumulation");
                if (!sampleMap.empty() || (adaptive && (aovs || direct)))
                {
                    uint32_t numTiles = 0;
                    rfCheck(rf_renderer_read_tile_samples(renderer, nullptr, &numTiles), "tile samples");
                    tileSamples.resize(numTiles);
                    rfCheck(rf_renderer_read_tile_samples(renderer, tileSamples.data(), &numTiles), "tile samples");
                }
                if (denoising)
                {
                    rfCheck(rf_renderer_denoise(renderer, &denoiseParams), "denoise");
                    rfCheck(rf_renderer_read_denoised(renderer, denoisedRgba.data(), denoisedBgra.data(), &n), "read denoised");
                }
                if (robust)
                {
                    rfCheck(rf_renderer_robust_mean(renderer), "robust mean");
                    rfCheck(rf_renderer_read_robust_mean(renderer, robustRgba.data(), robustBgra.data(), robustTrim.data(), &n), "read robust mean");
                }
                if (!directSum.empty())
                {
                    rfCheck(rf_renderer_read_direct(renderer, directSum.data(), &directSamples), "read direct sums");
                    rfCheck(rf_renderer_read_accumulation(renderer, directAcc.data(), &n), "read accumulation");
                }
                if (!denoiseSplit.empty())
                {
                    rfCheck(rf_renderer_denoise_split(renderer, nullptr, nullptr), "denoise split");
                    rfCheck(rf_renderer_read_denoised(renderer, nullptr, splitBgra.data(), &n), "read denoised");
                }
                if (!denoiseRobust.empty())
                {
                    rfCheck(rf_renderer_denoise_robust(renderer, &denoiseParams), "denoise robust");
                    rfCheck(rf_renderer_read_denoised(renderer, nullptr, robustDenoisedBgra.data(), &n), "read denoised");
                }
            }
        }
        if (comm) rf_comm_destroy(comm);
        rf_renderer_destroy(renderer);
    };
    std::vector<std::thread> threads;
    for (uint32_t rank = 1; rank < gpus; ++rank) threads.emplace_back(worker, rank);
    worker(0);
    for (std::thread& t : threads) t.join();
    const double rays = static_cast<double>(closestRays.load() + shadowRays.load());
    std::printf("%ux%u, %u spp, %u bounces on %u GPU(s): %.3f s, %.1f Mrays/s (%llu closest + %llu shadow rays)\n", W, H, sppReached, bounces, gpus, seconds,
                rays / seconds * 1e-6, closestRays.load(), shadowRays.load());
    if (noiseTargetSet)
        std::printf("noise target %g: stopped at %u of %u spp, mean error %.6g (estimated at %u spp)\n", noiseTarget, sppReached, spp, estimate.mean_error, estimate.samples);
    if (adaptive)
        std::printf("adaptive target %g: %u of %u tiles stopped early, %u .. %u spp per tile, %llu of %llu pixel-samples, %u estimate pass(es)\n", adaptiveParams.target_tile_error,
                    adaptiveResult.stopped_tiles, adaptiveResult.tiles, adaptiveResult.min_tile_samples, adaptiveResult.max_tile_samples,
                    static_cast<unsigned long long>(adaptiveResult.pixel_samples), static_cast<unsigned long long>(W) * H * spp, adaptiveResult.estimate_passes);
    if (!noiseMap.empty())
        std::printf("noise at %u spp: mean error %.6g, max error %.6g in tile %u, %llu non-finite pixel(s)\n", estimate.samples, estimate.mean_error, estimate.max_error,
                    estimate.worst_tile, static_cast<unsigned long long>(estimate.nonfinite_pixels));

    const auto writeBgraPng = [&](const std::string& path, const std::vector<uint32_t>& texels) {
        std::vector<uint8_t> px(texels.size() * 4);
        for (size_t i = 0; i < texels.size(); ++i)
        {
            px[4 * i] = static_cast<uint8_t>(texels[i] >> 16);
            px[4 * i + 1] = static_cast<uint8_t>(texels[i] >> 8);
            px[4 * i + 2] = static_cast<uint8_t>(texels[i]);
            px[4 * i + 3] = 255;
        }
        return writePngRgba(path, px.data(), W, H);
    };
    if (!writeBgraPng(out, bgra)) return 1;
    if (!robustMean.empty() && !(endsWith(robustMean, ".png") ? writeBgraPng(robustMean, robustBgra) : writePfm(robustMean, robustRgba.data(), W, H, 1.0f))) return 1;
    if (!denoiseRobust.empty() && !writeBgraPng(denoiseRobust, robustDenoisedBgra)) return 1;
    if (!denoiseSplit.empty() && !writeBgraPng(denoiseSplit, splitBgra)) return 1;
    if (!pfm.empty()) writePfm(pfm, acc.data(), W, H, adaptive ? 1.0f : 1.0f / static_cast<float>(std::max(sppReached, 1u))); // (--adaptive: acc holds the per-tile mean)
    if (denoising)
    {
        std::vector<uint8_t> d(denoisedBgra.size() * 4);
        for (size_t i = 0; i < denoisedBgra.size(); ++i)
        {
            d[4 * i] = static_cast<uint8_t>(denoisedBgra[i] >> 16);
            d[4 * i + 1] = static_cast<uint8_t>(denoisedBgra[i] >> 8);
            d[4 * i + 2] = static_cast<uint8_t>(denoisedBgra[i]);
            d[4 * i + 3] = 255;
        }
        if (!denoisePng.empty() && !writePngRgba(denoisePng, d.data(), W, H)) return 1;
        if (!denoisePfm.empty() && !writePfm(denoisePfm, denoisedRgba.data(), W, H, 1.0f)) return 1;
    }
    // a 3- or 1-channel PFM of value(4 * pixel index, channel)
    const auto write = [&](const std::string& path, uint32_t channels, auto&& value) {
        if (path.empty()) return true;
        FILE* fp = std::fopen(path.c_str(), "wb");
        if (!fp) return false;
        std::fprintf(fp, "%s\n%u %u\n-1.0\n", channels == 3 ? "PF" : "Pf", W, H);
        std::vector<float> row(static_cast<size_t>(channels) * W);
        for (uint32_t y = 0; y < H; ++y) // (bottom row first)
        {
            for (uint32_t x = 0; x < W; ++x)
                for (uint32_t c = 0; c < channels; ++c) row[channels * x + c] = value(4 * (static_cast<size_t>(H - 1 - y) * W + x), c);
            std::fwrite(row.data(), sizeof(float), row.size(), fp);
        }
        std::fclose(fp);
        return true;
    };
    // (f32 divisions by the direct sample count -- with --adaptive the pixel's tile's own count --, as a caller of rf_renderer_read_direct forms them; indirect: one
    // f32 subtraction first)
    const auto directN = [&](size_t i) {
        const uint32_t count = adaptive ? tileSamples[((i / 4) / W / 32) * ((W + 31) / 32) + ((i / 4) % W) / 32] : directSamples;
        return static_cast<float>(std::max(count, 1u));
    };
    if (!write(directPfm, 3, [&](size_t i, uint32_t c) { return directSum[i + c] / directN(i); })) return 1;
    if (!write(indirectPfm, 3, [&](size_t i, uint32_t c) { return (directAcc[i + c] - directSum[i + c]) / directN(i); })) return 1;
    if (!write(noiseMap, 1, [&](size_t i, uint32_t) { return errorMap[i / 4]; })) return 1;
    if (!write(trimMap, 1, [&](size_t i, uint32_t) { return static_cast<float>(robustTrim[i / 4]); })) return 1;
    if (!sampleMap.empty() && tileSamples.empty()) tileSamples.assign(static_cast<size_t>((W + 31) / 32) * ((H + 31) / 32), sppReached); // (several ranks: one count)
    if (!write(sampleMap, 1, [&](size_t i, uint32_t) { return static_cast<float>(tileSamples[((i / 4) / W / 32) * ((W + 31) / 32) + ((i / 4) % W) / 32]); })) return 1;
    if (aovFiles)
    {
        // means (f32 divisions, as ReferencePathTracer.aov_means): albedo / normal over the AOV samples -- with --adaptive the pixel's tile's own count --, depth over the coverage
        const auto n = [&](size_t i) {
            const uint32_t count = adaptive ? tileSamples[((i / 4) / W / 32) * ((W + 31) / 32) + ((i / 4) % W) / 32] : aovSamples;
            return static_cast<float>(std::max(count, 1u));
        };
        const bool ok = write(aovAlbedo, 3, [&](size_t i, uint32_t c) { return aovAc[i + c] / n(i); }) && write(aovNormal, 3, [&](size_t i, uint32_t c) { return aovNd[i + c] / n(i); }) &&
                        write(aovDepth, 1, [&](size_t i, uint32_t) { return aovAc[i + 3] > 0.0f ? aovNd[i + 3] / aovAc[i + 3] : 0.0f; });
        if (!ok) return 1;
    }
    rf_pt_format_destroy(pt);
    return 0;
}
