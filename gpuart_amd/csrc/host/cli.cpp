// cli.cpp — headless command-line driver: what the reference's GUI main loop does
// (src/main.cpp:549-623: scene set-up, camera, direct lighting or progressive path tracing with
// pathsPerPass / pathsPerPixel), without a window. Writes PFM (float RGB, bottom-up like our rows) and/or
// an 8-bit PPM (what the reference's default framebuffer would show: clamped to [0,1]), prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include <unistd.h>

#include "renderer.h"
#include "scenes.h"

using gpuart::Vec3f;

static void usage() {
    std::cerr << "usage: gpuart_cli [--scene box|ply:<file>|cluster|tree] [--width W] [--height H] [--mode direct|pt]\n"
                 "                  [--spp N] [--per-pass K] [--max-segments M] [--seed S] [--tile x0,y0,w,h]\n"
                 "                  [--camera px,py,pz] [--sun az,alt[,off]] [--user-sphere x,y,z,r,em[,specular[,fuzzy]]]\n"
                 "                  [--device D] [--gpus N] [--resume ck] [--checkpoint ck] [--pfm out.pfm] [--ppm out.ppm] [--nearest-first]\n"
                 "                  [--adaptive T [--adaptive-min N] [--until-batch N] [--until-floor F] [--samples-pfm out.pfm] [--refine]]\n"
                 "                  [--denoise] [--edge-resolve] [--firefly-clamp [--firefly-k K] [--firefly-rank R]]\n"
                 "                  [--until T [--until-share S] [--until-floor F] [--until-batch N] [--error-pfm out.pfm] [--refine]]\n"
                 "                  [--display out.ppm [--tonemap clamp|reinhard|aces] [--white W] [--exposure-ev E] [--auto-exposure] [--key K]\n"
                 "                   [--srgb] [--dither] [--upscale S]]\n"
                 "  --until T: render until the relative standard error of every pixel's luminance is at most T (Renderer::RenderUntil; path\n"
                 "             tracing on one GPU), --spp being the cap; --until-share S: the share of pixels that may stay above T (default 0);\n"
                 "             --until-floor F: luminance below which the error is taken relative to F (default 1/256, one step of the 8-bit\n"
                 "             output); --until-batch N: paths per pixel between two measurements; --error-pfm: the error per pixel (PFM, grey).\n"
                 "             With --resume the checkpoint's paths are the first batch; one already at --spp renders nothing and is not measured\n"
                 "             (its line says 0 batches, converged false)\n"
                 "  --adaptive T: adaptive sampling (Renderer::RenderAdaptive; path tracing on one GPU): like --until, but every 8x8 block stops by\n"
                 "             itself as soon as all its pixels are at most T and it holds --adaptive-min paths (default 8) and two batches; the\n"
                 "             passes that follow render the remaining blocks only. --spp is the cap, --until-batch and --until-floor as for --until;\n"
                 "             --samples-pfm: the paths per pixel (PFM, grey). Not together with --until, --denoise, --checkpoint or --gpus above 1\n"
                 "  --refine: with --until or --adaptive, write the frame filtered by its own error estimate (Renderer::ReadRefined, with --until-floor as its\n"
                 "             floor) instead of the raw one; not together with --denoise. A run that never reached two batches writes the raw frame\n"
                 "  --display F: write the frame --pfm would hold (raw, --denoise or --refine) as an 8-bit PPM encoded on the device\n"
                 "             (Renderer::ReadDisplay, include/gpuart_display.h), top-down as --ppm; without further options the bytes of --ppm.\n"
                 "             --tonemap: the curve (default clamp); --white W: reinhard's white point (default 4); --exposure-ev E: gain 2^E;\n"
                 "             --auto-exposure: adapt the gain to the frame's histogram, --key K: the luminance its log-average is brought to\n"
                 "             (default 0.18); --srgb: the sRGB transfer function (default linear); --dither: 8x8 ordered dither. One GPU only\n"
                 "  --upscale S: with --display, write the frame S (2..4) times larger in each direction: the same source upsampled under the\n"
                 "             guidance of a G-buffer of the larger frame (Renderer::ReadUpscaledDisplay, include/gpuart_upscale.h, its defaults).\n"
                 "             One GPU only\n"
                 "  --denoise: write the denoised preview of the frame (Renderer::ReadDenoised; path tracing on one GPU)\n"
                 "  --edge-resolve: with --denoise or --refine, resolve geometric edges in the filtered frame from a sub-pixel G-buffer\n"
                 "             (Renderer::SetEdgeResolve, include/gpuart_edges.h, its defaults)\n"
                 "  --firefly-clamp: with --denoise or --refine, clamp fireflies ahead of the filter (Renderer::SetFireflyClamp,\n"
                 "             include/gpuart_despeckle.h; biased: it removes energy); --firefly-k K: the cap's factor (default 2);\n"
                 "             --firefly-rank R: which of the largest neighbours the cap stands on (1..4, default 3). One GPU only\n"
                 "  --nearest-first: opt in to the nearer-child-first BVH walk (~10 % faster; soak-verified, not proven to be the reference's image)\n"
                 "  --gpus N: path tracing of ONE frame on devices D..D+N-1 (8-row bands dealt round-robin, gathered over RCCL)\n";
}

static bool parse_floats(const char *s, float *out, int minN, int maxN, int &n) {
    n = 0;
    while (*s && n < maxN) {
        char *end;
        out[n++] = strtof(s, &end);
        if (end == s) return false;
        s = *end == ',' ? end + 1 : end;
    }
    return n >= minN;
}

int main(int argc, char **argv) {
    std::string scene = "box", mode = "pt", pfm, ppm, resume, checkpoint;
    unsigned W = 640, H = 480, spp = 16, perPass = 1, maxSeg = 5, device = 0, gpus = 1;
    long seed = -1;
    bool nearestFirst = false, denoise = false, refine = false, edgeResolve = false, fireflyClamp = false, haveFireflyOption = false;
    gpuart_despeckle_params firefly;
    gpuart_despeckle_defaults(&firefly);
    std::string errorPfm;
    float until = -1, untilShare = 0, untilFloor = 1.0f / 256;
    unsigned untilBatch = GPUART_CONVERGE_DEFAULT_BATCH;
    bool haveUntil = false, haveAdaptive = false;
    float adaptive = -1;
    unsigned adaptiveMin = GPUART_ADAPTIVE_DEFAULT_MIN_PATHS;
    std::string samplesPfm;
    std::string display, tonemap = "clamp";
    bool displayOption = false;  // one of --display's own options was given
    unsigned upscale = 0;        // --upscale S (0: not given)
    bool haveUpscale = false;
    gpuart_display_params dp;
    gpuart_display_defaults(&dp);
    float tile[4] = {0, 0, 0, 0}, campos[3] = {0.1f, -3.05f, 1.0f}, sun[3] = {0, 0, 0}, us[7] = {-0.4f, 0, 0.2f, 0, 0, 0, 0};
    int nTile = 0, nSun = 0, nUs = 0, n;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](const char *what) -> const char * {
            if (i + 1 >= argc) { std::cerr << what << " needs a value\n"; usage(); exit(2); }
            return argv[++i];
        };
        if (a == "--scene") scene = need("--scene");
        else if (a == "--width") W = (unsigned)atoi(need("--width"));
        else if (a == "--height") H = (unsigned)atoi(need("--height"));
        else if (a == "--mode") mode = need("--mode");
        else if (a == "--spp") spp = (unsigned)atoi(need("--spp"));
        else if (a == "--per-pass") perPass = (unsigned)atoi(need("--per-pass"));
        else if (a == "--max-segments") maxSeg = (unsigned)atoi(need("--max-segments"));
        else if (a == "--seed") seed = atol(need("--seed"));
        else if (a == "--device") device = (unsigned)atoi(need("--device"));
        else if (a == "--gpus") gpus = (unsigned)atoi(need("--gpus"));
        else if (a == "--tile") { if (!parse_floats(need("--tile"), tile, 4, 4, nTile)) { usage(); return 2; } }
        else if (a == "--camera") { if (!parse_floats(need("--camera"), campos, 3, 3, n)) { usage(); return 2; } }
        else if (a == "--sun") { if (!parse_floats(need("--sun"), sun, 2, 3, nSun)) { usage(); return 2; } }
        else if (a == "--user-sphere") { if (!parse_floats(need("--user-sphere"), us, 5, 7, nUs)) { usage(); return 2; } }
        else if (a == "--pfm") pfm = need("--pfm");
        else if (a == "--ppm") ppm = need("--ppm");
        else if (a == "--resume") resume = need("--resume");
        else if (a == "--checkpoint") checkpoint = need("--checkpoint");
        else if (a == "--nearest-first") nearestFirst = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--refine") refine = true;
        else if (a == "--edge-resolve") edgeResolve = true;
        else if (a == "--firefly-clamp") fireflyClamp = true;
        else if (a == "--firefly-k") { firefly.k = strtof(need("--firefly-k"), nullptr); haveFireflyOption = true; }
        else if (a == "--firefly-rank") { firefly.rank = (uint32_t)strtoul(need("--firefly-rank"), nullptr, 10); haveFireflyOption = true; }
        else if (a == "--until") { until = strtof(need("--until"), nullptr); haveUntil = true; }
        else if (a == "--until-share") untilShare = strtof(need("--until-share"), nullptr);
        else if (a == "--until-floor") untilFloor = strtof(need("--until-floor"), nullptr);
        else if (a == "--until-batch") untilBatch = (unsigned)atoi(need("--until-batch"));
        else if (a == "--error-pfm") errorPfm = need("--error-pfm");
        else if (a == "--adaptive") { adaptive = strtof(need("--adaptive"), nullptr); haveAdaptive = true; }
        else if (a == "--adaptive-min") adaptiveMin = (unsigned)atoi(need("--adaptive-min"));
        else if (a == "--samples-pfm") samplesPfm = need("--samples-pfm");
        else if (a == "--display") display = need("--display");
        else if (a == "--tonemap") { tonemap = need("--tonemap"); displayOption = true; }
        else if (a == "--white") { dp.white = strtof(need("--white"), nullptr); displayOption = true; }
        else if (a == "--exposure-ev") { dp.gain = std::exp2(strtof(need("--exposure-ev"), nullptr)); displayOption = true; }
        else if (a == "--auto-exposure") { dp.auto_exposure = 1; displayOption = true; }
        else if (a == "--key") { dp.key = strtof(need("--key"), nullptr); displayOption = true; }
        else if (a == "--srgb") { dp.transfer = GPUART_DISPLAY_SRGB; displayOption = true; }
        else if (a == "--dither") { dp.dither = 1; displayOption = true; }
        else if (a == "--upscale") { upscale = (unsigned)atoi(need("--upscale")); haveUpscale = true; }
        else { usage(); return 2; }
    }
    if (W == 0 || H == 0 || (mode != "direct" && mode != "pt")) { usage(); return 2; }
    if (denoise && (mode != "pt" || gpus != 1)) { usage(); return 2; }
    if (haveUntil && gpus > 1) {
        std::cerr << "gpuart_cli: --until needs --gpus 1: the ranks of a sharded frame would stop at different path counts\n";
        return 2;
    }
    if (haveAdaptive && haveUntil) {
        std::cerr << "gpuart_cli: --adaptive and --until are two stop rules: give one of them\n";
        return 2;
    }
    if (haveAdaptive && denoise) {
        std::cerr << "gpuart_cli: --adaptive writes the frame normalised by every block's own path count (or --refine's): not together with --denoise\n";
        return 2;
    }
    if (haveAdaptive && !checkpoint.empty()) {
        std::cerr << "gpuart_cli: --adaptive leaves blocks at different path counts: a checkpoint holds one, so not together with --checkpoint\n";
        return 2;
    }
    if (haveAdaptive && gpus > 1) {
        std::cerr << "gpuart_cli: --adaptive needs --gpus 1: the frame gather divides by one path count\n";
        return 2;
    }
    if (refine && !haveUntil && !haveAdaptive) {
        std::cerr << "gpuart_cli: --refine needs --until: it filters with the error estimate of that render\n";
        return 2;
    }
    if (edgeResolve && !denoise && !refine) {
        std::cerr << "gpuart_cli: --edge-resolve mends a filtered frame: give --denoise or --refine\n";
        return 2;
    }
    if (haveFireflyOption && !fireflyClamp) {
        std::cerr << "gpuart_cli: --firefly-k and --firefly-rank shape --firefly-clamp: give --firefly-clamp\n";
        return 2;
    }
    if (fireflyClamp && !denoise && !refine) {
        std::cerr << "gpuart_cli: --firefly-clamp acts ahead of a filter: give --denoise or --refine\n";
        return 2;
    }
    if (fireflyClamp && gpus > 1) {
        std::cerr << "gpuart_cli: --firefly-clamp needs --gpus 1: the clamp is not in the frame gather\n";
        return 2;
    }
    if (refine && denoise) {
        std::cerr << "gpuart_cli: --refine and --denoise both replace the frame that is written: give one of them\n";
        return 2;
    }
    if ((haveUntil && mode != "pt") || (!haveUntil && !errorPfm.empty())) { usage(); return 2; }
    if (displayOption && display.empty()) {
        std::cerr << "gpuart_cli: --tonemap, --white, --exposure-ev, --auto-exposure, --key, --srgb and --dither shape --display's frame: give --display\n";
        return 2;
    }
    if (haveUpscale && display.empty()) {
        std::cerr << "gpuart_cli: --upscale enlarges --display's frame: give --display\n";
        return 2;
    }
    if (haveUpscale && (upscale < GPUART_UPSCALE_MIN_SCALE || upscale > GPUART_UPSCALE_MAX_SCALE)) {
        std::cerr << "gpuart_cli: --upscale takes 2, 3 or 4\n";
        return 2;
    }
    if (haveUpscale && gpus > 1) {
        std::cerr << "gpuart_cli: --upscale needs --gpus 1: a share's larger frame is no rectangle\n";
        return 2;
    }
    if (!display.empty() && gpus > 1) {
        std::cerr << "gpuart_cli: --display needs --gpus 1: the display stage is not in the frame gather\n";
        return 2;
    }
    if (tonemap == "clamp") dp.curve = GPUART_DISPLAY_CLAMP;
    else if (tonemap == "reinhard") dp.curve = GPUART_DISPLAY_REINHARD;
    else if (tonemap == "aces") dp.curve = GPUART_DISPLAY_ACES;
    else { usage(); return 2; }
    if ((haveAdaptive && mode != "pt") || (!haveAdaptive && !samplesPfm.empty())) { usage(); return 2; }

    // the reference's start-up camera (src/main.cpp:609-613), looking at (0,0,0.95)
    gpuart::Camera cam;
    cam.Pos = Vec3f(campos[0], campos[1], campos[2]);
    cam.Up = Vec3f(0, 0, 1);
    cam.Dir = Vec3f(0, 0, 0.95f) - cam.Pos;
    cam.FovY = 60;
    cam.ScreenDist = 0.2f;

    // One Renderer per GPU; with --gpus N every one is set up identically (same scene, camera, lighting, seed: all draw the
    // same RandSeed sequence) and renders its share of the frame.
    if (gpus < 1 || gpus > 64 || (gpus > 1 && (mode != "pt" || nTile == 4 || !resume.empty() || !checkpoint.empty()))) { usage(); return 2; }
    std::vector<std::unique_ptr<gpuart::Renderer>> rs;
    bool ok = true;
    for (unsigned g = 0; g < gpus && ok; g++) {
        // (GPUART_CLI_SHARED_DEVICE: every rank on --device — only an in-process RCCL stand-in accepts that: tests/test_gather_inprocess.py)
        const unsigned dev = getenv("GPUART_CLI_SHARED_DEVICE") ? device : device + g;
        rs.emplace_back(new gpuart::Renderer(W, H, cam, (int)dev));
        gpuart::Renderer &r = *rs.back();
        if (!r.GetIsOK()) { std::cerr << "Renderer initialization failed on device " << dev << "\n"; return 1; }
        r.SetUserSphere(Vec3f(us[0], us[1], us[2]), us[3], us[4]);
        if (nUs >= 6) r.SetUserSphereSpecular(us[5] != 0);
        if (nUs >= 7) r.SetUserSphereFuzzy(us[6] != 0);
        if (nSun >= 2) { r.SetSunAzimuth(sun[0]); r.SetSunAltitude(sun[1]); if (nSun == 3) r.SetSunDirectLighting(sun[2] == 0); }
        r.SetMaxPathSegments(maxSeg);
        if (seed >= 0) r.SetSeed((uint32_t)seed);
        if (nearestFirst && !r.SetNearestFirst(1024)) return 1;
        if (scene == "box") InitBox(r);
        else if (scene.compare(0, 4, "ply:") == 0) ok = InitDragon(r, scene.c_str() + 4);
        else if (scene.compare(0, 8, "cluster:") == 0) ok = InitCluster(r, scene.c_str() + 8);
        else if (scene.compare(0, 5, "tree:") == 0) ok = InitTree(r, scene.c_str() + 5);
        else if (scene == "cluster") ok = InitCluster(r);
        else if (scene == "tree") ok = InitTree(r);
        else { usage(); return 2; }
        if (!ok || !r.GetIsOK()) { std::cerr << "scene set-up failed\n"; return 1; }
        if (gpus > 1 && !r.SetShare((int)g, (int)gpus)) return 1;
    }
    gpuart::Renderer &r = *rs[0];
    if (edgeResolve && !r.SetEdgeResolve(true)) return 1;
    if (fireflyClamp && !r.SetFireflyClamp(true, &firefly)) return 1;
    if (nTile == 4 && !r.SetTile((unsigned)tile[0], (unsigned)tile[1], (unsigned)tile[2], (unsigned)tile[3])) return 1;
    const unsigned tw = gpus > 1 ? W : r.GetTileWidth(), th = gpus > 1 ? H : r.GetTileHeight();

    std::vector<float> img((size_t)tw * th * 4);
    const auto t0 = std::chrono::high_resolution_clock::now();
    unsigned done = 0, passes = 0, untilBatches = 0;
    if (mode == "direct") {
        r.RenderDirectLighting();
        ok = r.ReadDirectLighting(img.data());
    } else {
        for (auto &q : rs) q->RestartPathTracing(perPass, spp);
        if (!resume.empty()) {
            if (!r.LoadCheckpoint(resume.c_str())) return 1;
            // the checkpoint restores the run's own target (normally already reached); the command line's --spp /
            // --per-pass say how far to go on from there
            r.ExtendPathTracing(perPass, spp);
        }
        if (haveUntil) {
            // the same passes, in batches, until the frame's error estimate is below the threshold or --spp is reached
            const unsigned start = r.GetNumPathsRendered();
            gpuart_converge_summary cs{};
            const int rc = r.RenderUntil(until, untilShare, untilBatch, untilFloor, &cs);
            if (rc < 0) return 1;
            done = r.GetNumPathsRendered();
            untilBatches = cs.batches;
            passes = (done - start + std::max(1u, perPass) - 1) / std::max(1u, perPass);
            printf("{\"until\": %.9g, \"paths_rendered\": %u, \"batches\": %u, \"above\": %llu, \"pixels\": %llu, \"max_error\": %.9g, "
                   "\"converged\": %s}\n", until, done, cs.batches, (unsigned long long)cs.above, (unsigned long long)cs.pixels, cs.max_error,
                   rc == 1 ? "true" : "false");
            if (!errorPfm.empty()) {
                std::vector<float> e((size_t)tw * th);
                if (!r.ReadErrorMap(e.data(), untilFloor)) { std::cerr << "gpuart_cli: no error map (fewer than two batches were rendered)\n"; return 1; }
                FILE *f = fopen(errorPfm.c_str(), "wb");
                if (!f) return 1;
                fprintf(f, "Pf\n%u %u\n-1.0\n", tw, th);
                fwrite(e.data(), sizeof(float), e.size(), f);
                fclose(f);
            }
        } else if (haveAdaptive) {
            // the same passes, in batches, every block until its own error estimate is below the threshold or --spp is reached
            const unsigned start = r.GetNumPathsRendered();
            gpuart_adaptive_summary as{};
            const int rc = r.RenderAdaptive(adaptive, adaptiveMin, untilBatch, untilFloor, &as);
            if (rc < 0) return 1;
            done = r.GetNumPathsRendered();
            untilBatches = as.blocks ? 2 : 0;  // (a select ran: the estimate has its two batches)
            passes = (done - start + std::max(1u, perPass) - 1) / std::max(1u, perPass);
            printf("{\"adaptive\": %.9g, \"paths_issued\": %u, \"paths_min\": %u, \"paths_max\": %u, \"paths_mean\": %.9g, \"active_blocks\": %u, "
                   "\"blocks\": %u, \"max_error\": %.9g, \"converged\": %s}\n", adaptive, done, as.paths_min, as.paths_max,
                   as.pixels ? (double)as.paths_sum / (double)as.pixels : 0.0, as.active_blocks, as.blocks, as.max_error, rc == 1 ? "true" : "false");
            if (!samplesPfm.empty()) {
                std::vector<uint32_t> cnt((size_t)tw * th);
                if (!r.ReadSampleCounts(cnt.data())) return 1;
                std::vector<float> cf(cnt.begin(), cnt.end());
                FILE *f = fopen(samplesPfm.c_str(), "wb");
                if (!f) return 1;
                fprintf(f, "Pf\n%u %u\n-1.0\n", tw, th);
                fwrite(cf.data(), sizeof(float), cf.size(), f);
                fclose(f);
            }
        } else {
            // the reference's draw loop: one pass per frame until pathsPerPixel is reached (src/main.cpp:554-582)
            // (every GPU's pass is only enqueued: the devices work at the same time)
            for (;;) {
                for (auto &q : rs) done = q->RenderPathTracingPass();
                passes++;
                if (done >= r.GetPathsPerPixel()) break;
            }
        }
        for (auto &q : rs) q->Finish();
        if (!checkpoint.empty() && !r.SaveCheckpoint(checkpoint.c_str())) return 1;
        if (gpus > 1 || getenv("GPUART_CLI_FORCE_GATHER")) {  // (the variable: the RCCL path with a single rank, for tests)
            std::vector<gpuart::Renderer *> ranks;
            for (auto &q : rs) ranks.push_back(q.get());
            ok = gpuart::Renderer::GatherRadiance(ranks.data(), (int)gpus, 0, true, img.data());
            // The communicator goes in a phase of its own, not in the destructors at exit. A read-out that gave up (a bounded wait
            // of the library ran out: a message above says which) leaves streams and possibly a parked RCCL thread behind:
            // nothing of that is waited for again — no destructors, no atexit handlers.
            if (ok) ok = gpuart::Renderer::ReleaseCommunicator(ranks.data(), (int)gpus);
            if (!ok) {
                std::cerr << "gpuart_cli: the multi-GPU read-out failed" << (gpuart_hip_comm_stuck() ? " (an RCCL call never returned)" : "")
                          << "; ending without unwinding." << std::endl;
                fflush(nullptr);
                _exit(1);
            }
        } else
            if (refine && untilBatches >= 2) ok = r.ReadRefined(img.data(), untilFloor);
            else {
                if (refine) std::cerr << "gpuart_cli: --refine: the estimate never reached two batches; writing the raw frame\n";
                ok = denoise ? r.ReadDenoised(img.data()) : r.ReadRadiance(img.data(), true);
            }
    }
    const double secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    if (!ok) return 1;

    if (!pfm.empty()) {  // PFM rows run bottom-to-top, as ours do
        FILE *f = fopen(pfm.c_str(), "wb");
        if (!f) return 1;
        fprintf(f, "PF\n%u %u\n-1.0\n", tw, th);
        for (size_t i = 0; i < (size_t)tw * th; i++) fwrite(&img[4 * i], sizeof(float), 3, f);
        fclose(f);
    }
    if (!ppm.empty()) {  // top-down, clamped to [0,1] like the GL default framebuffer
        FILE *f = fopen(ppm.c_str(), "wb");
        if (!f) return 1;
        fprintf(f, "P6\n%u %u\n255\n", tw, th);
        for (unsigned y = th; y-- > 0;)
            for (unsigned x = 0; x < tw; x++)
                for (int c = 0; c < 3; c++) {
                    float v = img[4 * ((size_t)y * tw + x) + c];
                    v = v != v ? 0.0f : (v < 0 ? 0.0f : (v > 1 ? 1.0f : v));
                    fputc((int)std::lround(v * 255.0f), f);
                }
        fclose(f);
    }
    std::string displayKeys;
    if (!display.empty()) {  // the same frame, encoded on the device; top-down like --ppm
        const gpuart_display_source src = mode == "direct" ? GPUART_DISPLAY_DIRECT
                                          : refine && untilBatches >= 2 ? GPUART_DISPLAY_REFINED
                                          : denoise ? GPUART_DISPLAY_DENOISED : GPUART_DISPLAY_RADIANCE;
        const unsigned k = haveUpscale ? upscale : 1u, dw = k * tw, dh = k * th;
        std::vector<uint8_t> img8((size_t)dw * dh * 4);
        if (!(haveUpscale ? r.ReadUpscaledDisplay(img8.data(), src, upscale, &dp, untilFloor) : r.ReadDisplay(img8.data(), src, &dp, untilFloor))) return 1;
        FILE *f = fopen(display.c_str(), "wb");
        if (!f) return 1;
        fprintf(f, "P6\n%u %u\n255\n", dw, dh);
        for (unsigned y = dh; y-- > 0;)
            for (unsigned x = 0; x < dw; x++) fwrite(&img8[4 * ((size_t)y * dw + x)], 1, 3, f);
        fclose(f);
        char buf[256];
        snprintf(buf, sizeof buf, ", \"display\": {\"tonemap\": \"%s\", \"transfer\": \"%s\", \"gain\": %.9g, \"auto_exposure\": %s, \"dither\": %s}",
                 tonemap.c_str(), dp.transfer ? "srgb" : "linear", dp.gain, dp.auto_exposure ? "true" : "false", dp.dither ? "true" : "false");
        displayKeys = buf;
    }
    printf("{\"scene\": \"%s\", \"mode\": \"%s\", \"frame\": [%u, %u], \"tile\": [%u, %u], \"gpus\": %u, \"paths_per_pixel\": %u, "
           "\"passes\": %u, \"seconds\": %.6f, \"mpaths_per_s\": %.3f%s}\n",
           scene.c_str(), mode.c_str(), W, H, tw, th, gpus, done, passes, secs,
           mode == "pt" ? (double)tw * th * done / secs / 1e6 : (double)tw * th / secs / 1e6, displayKeys.c_str());
    return 0;
}
