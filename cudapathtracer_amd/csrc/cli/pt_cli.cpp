// pt_cli -- the reference's program (kernel.cu:565-790 `main`) as a command-line tool over the
// C-ABI of include/pt/pt.h: load OBJ models (loadOBJ, kernel.cu:589-599), build the BVH
// (:601, depth guard :627-631), render (:702-737), report rates (:753-757, in 64-bit), tone-map
// on the GPU and write the PPM (:763-778), optionally a PFM float dump.
//
//   pt_cli --obj models/CornellBox-Original.obj --obj models/teapot.obj@0.35,0.6,0.3@0.75 \
//          --width 512 --height 512 --spp 99 --bounces 3 --out image.ppm [--pfm image.pfm]
//
// --obj PATH[@ox,oy,oz[@scale[@flip]]]   loadOBJ(path, mtl dir, origin, scale, flipNormals)
// --num-samples N                         the reference's NUM_SAMPLES (renders N-1 samples);
//                                         --spp gives the sample count directly
// --gpus N                                shard image tiles over devices 0..N-1 (pt_render_multi:
//                                         one context per device, one RCCL reduce of the shards)
// --morton                                render into the reference's Morton-indexed framebuffer
//                                         (square power-of-two sizes); --tile WxH sets the shard tile
// --tri-counts out.csv                    per-triangle test counts (the reference's out.csv,
//                                         kernel.cu:742-750); --reference-walk makes them the
//                                         reference's own (its exact trace() sequence)
// --checkpoint FILE                       render through an accumulator (pt_accum_*) and write its state
//                                         (per-pixel XORWOW + f64 mean) to FILE after rendering
// --resume FILE                           continue the render FILE holds: every fixed parameter and the
//                                         camera come from the file, --spp is the samples to ADD; an
//                                         option that contradicts the file is an error
// --session FILE                          as --checkpoint, but a session file (pt_session_save): the accumulator, the
//                                         frozen pixels' counts and the noise estimator with its window; allowed with
//                                         --until-error and --adaptive
// --resume-session FILE                   continue the render a session file holds, as --resume does a checkpoint; the
//                                         estimator continues the saved window when the file has one, so a resumed
//                                         --until-error / --adaptive run equals the uninterrupted one
// --pass-spp K                            render in passes of K samples (the reference's progressive
//                                         loop, kernel.cu:709-736), rewriting --out / --pfm /
//                                         --checkpoint / --session after each and printing its "sample %d" line
// --until-error TOL                       with --pass-spp K: attach a noise estimator (pt_noise_*) and stop as soon as
//   [--error-quantile Q] [--min-batches B]  the fraction Q (default 0.95) of the pixels has a relative standard error
//                                         of its mean luminance <= TOL, after at least B (default 2) passes; --spp
//                                         (with --resume / --resume-session: the samples done plus --spp) is the cap.
//                                         After --resume a fresh estimator window starts at the resumed state; after
//                                         --resume-session the saved window continues
// --error-map FILE.pfm                    with --pass-spp K: write the squared relative standard error of every
//                                         pixel ((float)rel2 of pt_noise_map) as a grey PFM
// --adaptive                              with --until-error: freeze every pixel once its error is <= TOL (after at least
//                                         B passes) and sample only the others from then on (pt_noise_freeze; the
//                                         loop of pt_accum_add_adaptive).  Not with --checkpoint: format version 1
//                                         holds a single sample count (--session holds them all)
// --count-map FILE.pfm                    with --pass-spp K: write every pixel's sample count (pt_accum_counts) as a
//                                         grey PFM
// --denoise [ITERS]                       filter the image with the edge-avoiding a-trous denoiser (pt_denoise,
//                                         ITERS iterations, default 5) before the PPM / PFM is written -- also
//                                         after every --pass-spp pass, after --resume and after the multi-GPU
//                                         reduce (features and filter then run for the whole frame on GPU 0)
// --denoise-guided [ITERS]                with an estimator (--until-error, with or without --adaptive; --error-map and
//   [--sigma-luma S]                      --variance-map attach one too): filter the FINAL image with the
//                                         variance-guided denoiser (pt_denoise_guided, sigma_luma S, default 2) and the
//                                         estimator's variance map; the files written after earlier passes are unfiltered
// --variance-map FILE.pfm                 with --pass-spp K: write the variance of every pixel's mean luminance
//                                         (pt_noise_variance) as a grey PFM
// --look-at X,Y,Z [--up X,Y,Z]            aim the camera (pt_view_look_at from --cam towards X,Y,Z; up defaults to 0,1,0).  With
//   [--vfov DEG | --film W,H]             every mode that renders.  --vfov sizes the film for a vertical field of view and
//                                         square pixels (pt_view_set_fov), --film sets its extent directly (1,1 = the
//                                         reference's unit square, the default); without --look-at they apply to a camera
//                                         looking down -z.  --session writes the view (format version 3); after
//                                         --resume-session the view is the file's, and a command-line view that differs is
//                                         an error; --checkpoint cannot hold a view (the library's message says so)
// --jitter box|tent                       sub-pixel jitter (PT_FLAG_JITTER; tent: PT_FLAG_JITTER_TENT as well): every sample's
//                                         camera ray goes through its own point of the film, so edges are anti-aliased.
//                                         With every mode that renders; with --aov the feature rays go through the pixels'
//                                         centres.  After --resume / --resume-session the flags are the file's, and a
//                                         --jitter that differs is an error
// --camera-path FILE --temporal           a moving camera: FILE has one pose per line, "px py pz tx ty tz" (position, target;
//   [--temporal-max N]                    blank lines and lines starting with # are skipped).  Each line is one frame through
//                                         pt_view_look_at with --up / --vfov / --film as above, rendered at --spp with seed
//                                         --seed + frame (frames are independent) and pushed with its feature buffers through
//                                         a temporal history (pt_temporal_*, history length capped at N, default 32), which
//                                         reprojects what it holds into every new frame.  The image files hold the last
//                                         frame's temporal image; --denoise-guided filters it with the temporal variance (no
//                                         estimator needed), --variance-map writes that variance.  --gpus 1 only; not with the
//                                         accumulating modes, --look-at or --cam (the poses place and aim the camera)
// --rays FILE                             render along the caller's rays instead of a camera's (pt_render_rays): FILE is raw
//                                         little-endian float32, 6 * W * H values {o.xyz, d.xyz} in scanline order, with
//                                         --width / --height / --spp and the usual output options (--morton permutes the
//                                         rays into the Morton-indexed buffer's order).  --denoise and --aov take their
//                                         features from the ray file (pt_render_features_rays).  Not with the camera, view,
//                                         jitter, checkpoint, session, temporal, pass, adaptive or --denoise-guided options,
//                                         --tri-counts or --gpus above 1: an error.  A ray far outside the scene or with an
//                                         unnormalised direction sends the whole render to the slow exact walk (pt.h)
// --irradiance FILE                       an irradiance render at the caller's points (pt_render_irradiance): FILE has
//                                         --rays' format with the second triple a unit normal, {p.xyz, n.xyz}; every sample
//                                         leaves p along a fresh cosine-weighted direction about n.  --rays' exclusions, and
//                                         not with --rays, --denoise or --aov (there are no features over points): an error
// --aov PREFIX                            write the primary-hit feature buffers as PREFIX_albedo.pfm,
//                                         PREFIX_normal.pfm, PREFIX_position.pfm and PREFIX_depth.pfm (depth
//                                         replicated to 3 channels)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt/pt.h"

namespace {

struct Obj {
    std::string path;
    pt_vec3 origin{0, 0, 0};
    float scale = 1.0f;
    int flip = 0;
};

[[noreturn]] void usage(const char* msg)
{
    if (msg) fprintf(stderr, "pt_cli: %s\n", msg);
    fprintf(stderr,
            "usage: pt_cli --obj PATH[@ox,oy,oz[@scale[@flip]]] [--obj ...] [--mtl-dir DIR]\n"
            "              [--width W] [--height H] [--spp N | --num-samples N] [--bounces D]\n"
            "              [--integrator unidir|head] [--seed S] [--cam X,Y,Z] [--dist D] [--focal F]\n"
            "              [--radius R] [--gpus N] [--out image.ppm] [--pfm image.pfm] [--quiet]\n"
            "              [--look-at X,Y,Z] [--up X,Y,Z] [--vfov DEG | --film W,H] [--jitter box|tent]\n"
            "              [--tri-counts out.csv [--reference-walk]] [--morton] [--tile WxH]\n"
            "              [--checkpoint FILE] [--resume FILE] [--pass-spp K]\n"
            "              [--session FILE] [--resume-session FILE]\n"
            "              [--denoise [ITERS]] [--aov PREFIX]\n"
            "              [--camera-path FILE --temporal [--temporal-max N]] [--rays FILE | --irradiance FILE]\n"
            "              [--until-error TOL [--error-quantile Q] [--min-batches B] [--adaptive]] [--error-map FILE.pfm]\n"
            "              [--count-map FILE.pfm] [--denoise-guided [ITERS] [--sigma-luma S]] [--variance-map FILE.pfm]\n"
            "  --until-error TOL  with --pass-spp: stop once the fraction Q (default 0.95) of the pixels has a relative\n"
            "                     standard error <= TOL after at least B (default 2) passes; --spp is the cap\n"
            "  --adaptive         with --until-error: freeze each pixel once its error is <= TOL and sample only the rest\n"
            "  --count-map FILE   with --pass-spp: write the per-pixel sample counts as a grey PFM\n"
            "  --error-map FILE   with --pass-spp: write the per-pixel squared relative standard error as a grey PFM\n"
            "  --denoise [ITERS]  filter the image (edge-avoiding a-trous, ITERS iterations, default 5) before it is written\n"
            "  --denoise-guided [ITERS]  with --until-error: filter the final image guided by the estimator's variance map\n"
            "  --sigma-luma S     the guided filter's luminance tolerance in standard errors (default 2)\n"
            "  --variance-map FILE  with --pass-spp: write the variance of every pixel's mean luminance as a grey PFM\n"
            "  --session FILE     write the whole progressive state (accumulator, frozen pixels, estimator) after each pass\n"
            "  --resume-session FILE  continue the render FILE holds; its estimator window continues; --spp is the samples to add\n"
            "  --look-at X,Y,Z    aim the camera at a point (--up X,Y,Z, default 0,1,0); --vfov DEG: the vertical field of view\n"
            "                     with square pixels; --film W,H: the film's extent (1,1 = the reference's unit square)\n"
            "  --jitter box|tent  anti-alias: every sample's camera ray through its own point of the pixel's footprint (box), or\n"
            "                     of the tent of half-width 1 pixel about its centre (tent)\n"
            "  --camera-path FILE --temporal  one frame per line of FILE (px py pz tx ty tz: position, target), each rendered at\n"
            "                     --spp with seed --seed + frame and pushed through a temporal history (--temporal-max N caps its\n"
            "                     length, default 32); the files hold the last frame's temporal image; --denoise-guided and\n"
            "                     --variance-map use the temporal variance\n"
            "  --rays FILE        render along the rays of FILE (raw float32, 6*W*H values {o.xyz, d.xyz}, scanline order) instead\n"
            "                     of a camera's; --denoise and --aov take their features from FILE; not with the camera, view,\n"
            "                     jitter, accumulating, temporal or --denoise-guided options\n"
            "  --irradiance FILE  an irradiance render at the points of FILE (--rays' format, {p.xyz, n.xyz} with n a unit normal):\n"
            "                     every sample leaves p along a cosine-weighted direction about n; --rays' exclusions, and not with\n"
            "                     --rays, --denoise or --aov\n"
            "  --aov PREFIX       write PREFIX_albedo.pfm, PREFIX_normal.pfm, PREFIX_position.pfm, PREFIX_depth.pfm\n");
    exit(2);
}

bool parse_vec3(const std::string& s, pt_vec3* v)
{
    return sscanf(s.c_str(), "%f,%f,%f", &v->x, &v->y, &v->z) == 3;
}

// (strict: every component present and nothing after the last)
bool parse_vec3_strict(const std::string& s, pt_vec3* v)
{
    char tail = 0;
    return sscanf(s.c_str(), "%f,%f,%f%c", &v->x, &v->y, &v->z, &tail) == 3;
}

Obj parse_obj(const std::string& arg)
{
    Obj o;
    std::vector<std::string> parts;
    size_t b = 0;
    for (size_t e; (e = arg.find('@', b)) != std::string::npos; b = e + 1) parts.push_back(arg.substr(b, e - b));
    parts.push_back(arg.substr(b));
    o.path = parts[0];
    if (parts.size() > 1 && !parse_vec3(parts[1], &o.origin)) usage("bad --obj origin");
    if (parts.size() > 2) o.scale = strtof(parts[2].c_str(), nullptr);
    if (parts.size() > 3) o.flip = atoi(parts[3].c_str());
    return o;
}

std::string dir_of(const std::string& p)
{
    const size_t k = p.find_last_of('/');
    return k == std::string::npos ? std::string("./") : p.substr(0, k + 1);
}

struct Pose {
    pt_vec3 pos, target;
};

// The poses of a --camera-path file; false with a message on stderr.
bool read_camera_path(const std::string& path, std::vector<Pose>* poses)
{
    FILE* f = fopen(path.c_str(), "r");
    if (!f) { fprintf(stderr, "pt_cli: --camera-path: cannot read %s\n", path.c_str()); return false; }
    char line[512];
    for (int no = 1; fgets(line, sizeof line, f); ++no) {
        const char* c = line;
        while (*c == ' ' || *c == '\t' || *c == '\r' || *c == '\n') ++c;
        if (!*c || *c == '#') continue;
        Pose q;
        char tail = 0;
        if (sscanf(c, "%f %f %f %f %f %f %c", &q.pos.x, &q.pos.y, &q.pos.z, &q.target.x, &q.target.y, &q.target.z, &tail) != 6) {
            fprintf(stderr, "pt_cli: --camera-path: %s line %d is not \"px py pz tx ty tz\"\n", path.c_str(), no);
            fclose(f);
            return false;
        }
        poses->push_back(q);
    }
    fclose(f);
    if (poses->empty()) { fprintf(stderr, "pt_cli: --camera-path: %s holds no pose\n", path.c_str()); return false; }
    return true;
}

int die(const char* what)
{
    fprintf(stderr, "pt_cli: %s: %s\n", what, pt_last_error());
    return 1;
}

}  // namespace

int main(int argc, char** argv)
{
    std::vector<Obj> objs;
    std::string mtl_dir, out = "image.ppm", pfm;
    pt_params p{};
    p.width = 512; p.height = 512; p.spp = 99; p.bounces = 3;   // kernel.cu:29-33 defaults
    p.integrator = PT_INTEGRATOR_UNIDIR; p.seed = 1234; p.shard_index = 0; p.shard_count = 1;
    pt_camera cam{{0, 1, 3}, 1, 3, 0, 0, 0};                      // kernel.cu:642-648
    int gpus = 1;
    bool quiet = false, ref_walk = false;
    std::string tri_csv, checkpoint, resume, session, resume_session;
    uint32_t jitter_flags = 0;   // --jitter: PT_FLAG_JITTER, with PT_FLAG_JITTER_TENT for tent
    int pass_spp = 0;
    bool denoise = false;
    pt_denoise_params dparams;
    pt_denoise_defaults(&dparams);
    bool guided = false;
    pt_denoise_guided_params gparams;
    pt_denoise_guided_defaults(&gparams);
    std::string variance_map;
    std::string aov;
    std::string rays_path;     // --rays FILE
    std::string irr_path;      // --irradiance FILE
    std::string camera_path;   // --camera-path FILE --temporal [--temporal-max N]
    bool temporal = false;
    pt_temporal_params tparams;
    pt_temporal_defaults(&tparams);
    bool until_error = false, adaptive = false;
    std::string error_map, count_map;
    pt_converge_params conv{};
    conv.min_batches = 2; conv.quantile = 0.95f;
    pt_noise_defaults(&conv.noise);
    // the oriented camera: --look-at / --up / --vfov / --film (any of them makes a view)
    bool have_target = false, have_vfov = false, have_film = false, have_up = false;
    pt_vec3 target{0, 0, 0}, up{0, 1, 0};
    float vfov = 0.0f, film_w = 1.0f, film_h = 1.0f;
    std::vector<std::string> given;   // the options on the command line (a resumed file may contradict them)
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        given.push_back(a);
        auto next = [&]() -> std::string {
            if (i + 1 >= argc) usage(("missing value for " + a).c_str());
            return argv[++i];
        };
        if (a == "--obj") objs.push_back(parse_obj(next()));
        else if (a == "--mtl-dir") mtl_dir = next();
        else if (a == "--width") p.width = atoi(next().c_str());
        else if (a == "--height") p.height = atoi(next().c_str());
        else if (a == "--spp") p.spp = atoi(next().c_str());
        else if (a == "--num-samples") p.spp = atoi(next().c_str()) - 1;   // kernel.cu:709-710
        else if (a == "--bounces") p.bounces = atoi(next().c_str());
        else if (a == "--integrator") {
            const std::string v = next();
            if (v == "unidir") p.integrator = PT_INTEGRATOR_UNIDIR;
            else if (v == "head") p.integrator = PT_INTEGRATOR_HEAD;
            else usage("--integrator is unidir or head");
        } else if (a == "--seed") p.seed = strtoull(next().c_str(), nullptr, 10);
        else if (a == "--cam") { if (!parse_vec3(next(), &cam.pos)) usage("bad --cam"); }
        else if (a == "--dist") cam.dist_from_film = strtof(next().c_str(), nullptr);
        else if (a == "--focal") cam.focal_length = strtof(next().c_str(), nullptr);
        else if (a == "--radius") cam.radius = strtof(next().c_str(), nullptr);
        else if (a == "--gpus") gpus = atoi(next().c_str());
        else if (a == "--out") out = next();
        else if (a == "--pfm") pfm = next();
        else if (a == "--quiet") quiet = true;
        else if (a == "--tri-counts") tri_csv = next();
        else if (a == "--reference-walk") ref_walk = true;
        else if (a == "--morton") p.pixel_order = PT_ORDER_MORTON;   // the reference's imgBuff order
        else if (a == "--tile") {
            if (sscanf(next().c_str(), "%dx%d", &p.tile_w, &p.tile_h) != 2) usage("--tile is WxH");
        }
        else if (a == "--checkpoint") checkpoint = next();
        else if (a == "--resume") resume = next();
        else if (a == "--session") session = next();
        else if (a == "--resume-session") resume_session = next();
        else if (a == "--pass-spp") { pass_spp = atoi(next().c_str()); if (pass_spp < 1) usage("--pass-spp must be >= 1"); }
        else if (a == "--denoise") {
            denoise = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dparams.iterations = atoi(argv[++i]);
            if (dparams.iterations > 8) usage("--denoise takes 0..8 iterations");
        }
        else if (a == "--denoise-guided") {
            guided = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') gparams.base.iterations = atoi(argv[++i]);
            if (gparams.base.iterations > 8) usage("--denoise-guided takes 0..8 iterations");
        }
        else if (a == "--sigma-luma") gparams.sigma_luma = strtof(next().c_str(), nullptr);
        else if (a == "--variance-map") variance_map = next();
        else if (a == "--aov") aov = next();
        else if (a == "--rays") rays_path = next();
        else if (a == "--irradiance") irr_path = next();
        else if (a == "--camera-path") camera_path = next();
        else if (a == "--temporal") temporal = true;
        else if (a == "--temporal-max") { tparams.max_history = atoi(next().c_str()); if (tparams.max_history < 1) usage("--temporal-max must be >= 1"); }
        else if (a == "--jitter") {
            const std::string v = next();
            if (v == "box") jitter_flags = PT_FLAG_JITTER;
            else if (v == "tent") jitter_flags = PT_FLAG_JITTER | PT_FLAG_JITTER_TENT;
            else usage("--jitter is box or tent");
        }
        else if (a == "--until-error") { until_error = true; conv.noise.tol = strtof(next().c_str(), nullptr); }
        else if (a == "--error-quantile") conv.quantile = strtof(next().c_str(), nullptr);
        else if (a == "--min-batches") conv.min_batches = atoi(next().c_str());
        else if (a == "--error-map") error_map = next();
        else if (a == "--adaptive") adaptive = true;
        else if (a == "--count-map") count_map = next();
        else if (a == "--look-at") { have_target = true; if (!parse_vec3_strict(next(), &target)) usage("bad --look-at (X,Y,Z)"); }
        else if (a == "--up") { have_up = true; if (!parse_vec3_strict(next(), &up)) usage("bad --up (X,Y,Z)"); }
        else if (a == "--vfov") {
            have_vfov = true;
            vfov = strtof(next().c_str(), nullptr);
            if (!(vfov > 0.0f && vfov < 180.0f)) usage("--vfov is in (0, 180) degrees");
        }
        else if (a == "--film") {
            have_film = true;
            char tail = 0;
            if (sscanf(next().c_str(), "%f,%f%c", &film_w, &film_h, &tail) != 2 || !(film_w > 0.0f) || !(film_h > 0.0f) ||
                !std::isfinite(film_w) || !std::isfinite(film_h))
                usage("--film is W,H, both > 0");
        }
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown option " + a).c_str());
    }
    if (objs.empty()) usage("at least one --obj is required");
    if (gpus < 1) usage("--gpus must be >= 1");
    std::vector<float> rays;   // --rays / --irradiance: the buffer in the render's pixel order
    const bool irradiance = !irr_path.empty();
    if (irradiance && !rays_path.empty()) usage("--irradiance cannot be combined with --rays");
    if (irradiance) {   // (no features over a point buffer, pt.h)
        for (const std::string& g : given)
            for (const char* o : {"--denoise", "--aov"})
                if (g == o) usage(("--irradiance cannot be combined with " + g).c_str());
        rays_path = irr_path;
    }
    const std::string rays_opt = irradiance ? "--irradiance" : "--rays";
    if (!rays_path.empty()) {
        // a render along rays takes no camera, and its passes are not driven from here: every option of those is an error.
        // (--denoise and --aov work: the features then come from the ray file, pt_render_features_rays)
        for (const std::string& g : given)
            for (const char* o : {"--cam", "--dist", "--focal", "--radius", "--look-at", "--up", "--vfov", "--film", "--jitter",
                                  "--checkpoint", "--resume", "--session", "--resume-session", "--pass-spp", "--camera-path",
                                  "--temporal", "--temporal-max", "--until-error", "--error-quantile", "--min-batches", "--error-map",
                                  "--adaptive", "--count-map", "--denoise-guided", "--sigma-luma", "--variance-map",
                                  "--tri-counts"})
                if (g == o) usage((rays_opt + " cannot be combined with " + g).c_str());
        if (gpus != 1) usage((rays_opt + " needs --gpus 1").c_str());
        if (p.width <= 0 || p.height <= 0 || p.width > 65535 || p.height > 65535) usage((rays_opt + ": bad --width / --height").c_str());
        const size_t npx = (size_t)p.width * p.height;
        FILE* f = fopen(rays_path.c_str(), "rb");
        if (!f) { fprintf(stderr, "pt_cli: %s: cannot read %s\n", rays_opt.c_str(), rays_path.c_str()); return 2; }
        std::vector<float> scan(npx * 6);
        const size_t got = fread(scan.data(), sizeof(float), scan.size(), f);
        const bool more = got == scan.size() && fgetc(f) != EOF;
        fclose(f);
        if (got != scan.size() || more) {
            fprintf(stderr, "pt_cli: %s: %s does not hold %zu float32 values (6 per pixel of %dx%d)\n", rays_opt.c_str(),
                    rays_path.c_str(), scan.size(), p.width, p.height);
            return 2;
        }
        if (p.pixel_order == PT_ORDER_MORTON) {
            rays.assign(scan.size(), 0.0f);   // (a size the library refuses leaves the zeros: its message is the error)
            const bool square = p.width == p.height && (p.width & (p.width - 1)) == 0;
            for (int y = 0; square && y < p.height; ++y)
                for (int x = 0; x < p.width; ++x)
                    memcpy(&rays[(size_t)pt_morton_pxl_to_i(x, y) * 6], &scan[((size_t)y * p.width + x) * 6], 24);
        } else {
            rays.swap(scan);
        }
    }
    if (!tri_csv.empty() && gpus != 1) usage("--tri-counts needs --gpus 1");
    if (!tri_csv.empty()) p.flags |= PT_FLAG_COUNT | PT_FLAG_TRI_COUNTS;
    // --reference-walk: the reference's own trace() sequence for every sample (its node order, the
    // camera ray traced per sample, dead paths traced), so --tri-counts reproduces its out.csv
    if (ref_walk) p.flags |= PT_FLAG_REFERENCE_TRAVERSAL | PT_FLAG_NO_PRIMARY_CACHE | PT_FLAG_NO_DEAD_PATH_SKIP;
    p.flags |= jitter_flags;
    cam.pxl_width = p.width;
    cam.pxl_height = p.height;
    if (temporal && camera_path.empty()) usage("--temporal needs --camera-path FILE (the poses of the frames)");
    if (!camera_path.empty() && !temporal) usage("--camera-path needs --temporal");
    if (temporal && (until_error || !error_map.empty())) usage("--temporal has no estimator: not with --until-error / --error-map");
    // (with --temporal the variance map is the history's, and needs no estimator)
    const bool estimate = !temporal && (until_error || !error_map.empty() || !variance_map.empty());
    if (guided && !estimate && !temporal) usage("--denoise-guided needs an estimator: --until-error TOL with --pass-spp K");
    if (guided && denoise) usage("--denoise and --denoise-guided: choose one");
    if (!(gparams.sigma_luma > 0.0f) || !std::isfinite(gparams.sigma_luma)) usage("--sigma-luma must be finite and > 0");
    if (estimate && gpus != 1) usage("--until-error / --error-map / --variance-map need --gpus 1 (one estimator per accumulator)");
    if (estimate && pass_spp < 1) usage("--until-error / --error-map / --variance-map need --pass-spp K (the passes are the batches)");
    if (!(conv.noise.tol > 0.0f)) usage("--until-error takes a tolerance > 0");
    if (!(conv.quantile > 0.0f && conv.quantile <= 1.0f)) usage("--error-quantile is in (0, 1]");
    if (conv.min_batches < 2) usage("--min-batches must be >= 2");
    if (adaptive && !until_error) usage("--adaptive needs --until-error TOL (the tolerance pixels are frozen at)");
    if (adaptive && !checkpoint.empty()) usage("--adaptive cannot write a --checkpoint (format version 1 holds a single sample count)");
    if (!count_map.empty() && pass_spp < 1) usage("--count-map needs --pass-spp K");
    if (!resume.empty() && !resume_session.empty()) usage("--resume and --resume-session: choose one");
    if (have_vfov && have_film) usage("--vfov and --film: choose one");
    const bool view_given = have_target || have_up || have_vfov || have_film;
    pt_view file_view{};
    int file_has_view = 0;
    const bool accumulate = !checkpoint.empty() || !resume.empty() || !session.empty() || !resume_session.empty() || pass_spp > 0;
    if (accumulate && gpus != 1)
        usage("--checkpoint / --resume / --session / --resume-session / --pass-spp need --gpus 1 (one accumulator per shard)");
    if (accumulate && (!tri_csv.empty() || ref_walk)) usage("--tri-counts and --reference-walk do not accumulate");
    std::vector<Pose> poses;
    if (temporal) {
        if (accumulate) usage("--temporal renders independent frames: not with --checkpoint / --resume / --session / --resume-session / --pass-spp");
        if (gpus != 1) usage("--temporal needs --gpus 1 (one history per context)");
        if (!tri_csv.empty()) usage("--temporal: not with --tri-counts");
        if (have_target) usage("--temporal: the poses of --camera-path aim the camera, not --look-at");
        for (const std::string& g : given) if (g == "--cam") usage("--temporal: the poses of --camera-path place the camera, not --cam");
        if (!read_camera_path(camera_path, &poses)) return 2;
    }
    const std::string& resumed = resume.empty() ? resume_session : resume;   // the file a render continues, if any
    if (!resumed.empty()) {
        // the file fixes the render; what the command line says as well must say the same
        pt_params fp;
        pt_camera fc;
        int64_t done = 0;
        if (!resume.empty()) {
            if (pt_accum_file_info(resume.c_str(), &fp, &fc, &done, nullptr) != PT_OK) return die("--resume");
        } else {
            pt_session_info si;
            if (pt_session_file_info(resume_session.c_str(), &si) != PT_OK) return die("--resume-session");
            fp = si.params; fc = si.cam; done = si.samples;
            if (pt_session_file_view(resume_session.c_str(), &file_view, &file_has_view) != PT_OK) return die("--resume-session");
        }
        auto has = [&](const char* o) { for (const std::string& g : given) if (g == o) return true; return false; };
        auto conflict = [&](const char* o, bool differs) {
            if (has(o) && differs) {
                fprintf(stderr, "pt_cli: %s contradicts the resumed file %s\n", o, resumed.c_str());
                exit(2);
            }
        };
        conflict("--width", p.width != fp.width);
        conflict("--height", p.height != fp.height);
        conflict("--bounces", p.bounces != fp.bounces);
        conflict("--integrator", p.integrator != fp.integrator);
        conflict("--seed", p.seed != fp.seed);
        conflict("--morton", p.pixel_order != fp.pixel_order);
        conflict("--tile", p.tile_w != fp.tile_w || p.tile_h != fp.tile_h);
        conflict("--cam", memcmp(&cam.pos, &fc.pos, sizeof(pt_vec3)) != 0);
        conflict("--dist", cam.dist_from_film != fc.dist_from_film);
        conflict("--focal", cam.focal_length != fc.focal_length);
        conflict("--radius", cam.radius != fc.radius);
        conflict("--jitter", ((p.flags ^ fp.flags) & (PT_FLAG_JITTER | PT_FLAG_JITTER_TENT)) != 0);
        const int add = p.spp;
        p = fp;
        p.spp = add;
        cam = fc;
        if (!quiet) printf("resuming %s: %dx%d, %lld samples done, adding %d\n", resumed.c_str(), p.width, p.height, (long long)done, add);
    }

    // the view: the command line's (from the camera as it stands now: after a resume, the file's), or the resumed
    // file's; a command-line view that is not the file's is a conflict, like --dist and --focal above
    pt_view view_store{};
    const pt_view* cam_view = nullptr;
    if (view_given) {
        const pt_vec3 at = have_target ? target : pt_vec3{cam.pos.x, cam.pos.y, cam.pos.z - 1.0f};   // (else down -z)
        if (pt_view_look_at(cam.pos, at, up, &view_store) != PT_OK) return die(have_target ? "--look-at" : "--up");
        if (have_vfov && pt_view_set_fov(&view_store, &cam, vfov, p.width, p.height) != PT_OK) return die("--vfov");
        if (have_film) { view_store.film_w = film_w; view_store.film_h = film_h; }
        cam_view = &view_store;
    }
    if (!resumed.empty()) {
        if (view_given && (!file_has_view || memcmp(&view_store, &file_view, sizeof(pt_view)) != 0)) {
            fprintf(stderr, "pt_cli: --look-at / --up / --vfov / --film contradict the resumed file %s (%s)\n", resumed.c_str(),
                    file_has_view ? "its view differs" : "it has no view");
            return 2;
        }
        cam_view = file_has_view ? &file_view : nullptr;
    }

    const auto t0 = std::chrono::steady_clock::now();
    pt_host_scene* s = pt_scene_new();
    for (const Obj& o : objs) {
        const std::string md = mtl_dir.empty() ? dir_of(o.path) : mtl_dir;
        if (pt_scene_load_obj(s, o.path.c_str(), md.c_str(), o.origin, o.scale, o.flip) != PT_OK) return die("loadOBJ");
        const char* warn = pt_scene_last_warning(s);
        if (warn && *warn && !quiet) fprintf(stderr, "%s", warn);
    }
    if (pt_scene_build_bvh(s) != PT_OK) return die("buildBVH");
    pt_scene view;
    pt_scene_view(s, &view);
    const double t_load = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!quiet)
        printf("scene: %u triangles, %u lights, BVH depth %d (load + build %.3f s)\n", view.num_tris, view.num_lights,
               view.bvh_depth, t_load);

    const size_t n = (size_t)p.width * p.height * 3;
    std::vector<pt_ctx*> ctx(gpus, nullptr);
    for (int g = 0; g < gpus; ++g) {
        int err = 0;
        ctx[g] = pt_create(&view, g, &err);
        if (!ctx[g]) return die("pt_create");
    }
    std::vector<float> img(n, 0.0f);
    // --denoise / --aov: the whole frame's primary-hit features, once, on the first context
    std::vector<pt_feature> feat;
    std::vector<float> var;   // --denoise-guided / --variance-map: the estimator's variance map, once the passes are done
    auto features = [&]() -> bool {
        if (!feat.empty()) return true;
        feat.resize((size_t)p.width * p.height);
        pt_params fp = p;
        fp.shard_index = 0; fp.shard_count = 1;
        if (!rays.empty()) return pt_render_features_rays(ctx[0], &fp, rays.data(), feat.data()) == PT_OK;
        return pt_render_features_view(ctx[0], &fp, &cam, cam_view, feat.data()) == PT_OK;
    };
    // the image files of the current `img` (after the render; with --pass-spp after every pass)
    auto write_images = [&]() -> const char* {
        if (denoise) {
            if (!features()) return "pt_render_features";
            if (pt_denoise(ctx[0], &dparams, p.width, p.height, p.pixel_order, img.data(), feat.data(), img.data()) != PT_OK)
                return "pt_denoise";
        }
        if (guided && !var.empty()) {
            if (!features()) return "pt_render_features";
            if (pt_denoise_guided(ctx[0], &gparams, p.width, p.height, p.pixel_order, img.data(), feat.data(), var.data(), img.data()) !=
                PT_OK)
                return "pt_denoise_guided";
        }
        if (p.pixel_order == PT_ORDER_MORTON) {
            // the buffer as the reference holds it (imgBuff[mortonPxltoI(x,y)]): the PPM loop of
            // kernel.cu:763-778 reads it through the Morton map
            if (pt_write_ppm_order(out.c_str(), img.data(), p.width, p.height, PT_ORDER_MORTON) != PT_OK) return "write PPM";
            if (!pfm.empty()) {
                std::vector<float> scan(n);
                for (int y = 0; y < p.height; ++y)
                    for (int x = 0; x < p.width; ++x)
                        memcpy(&scan[((size_t)y * p.width + x) * 3], &img[(size_t)pt_morton_pxl_to_i(x, y) * 3], 12);
                if (pt_write_pfm(pfm.c_str(), scan.data(), p.width, p.height) != PT_OK) return "write PFM";
            }
        } else {
            std::vector<int32_t> codes(n);
            if (pt_tonemap(ctx[0], img.data(), p.width, p.height, codes.data()) != PT_OK) return "tone map";
            if (pt_write_ppm_codes(out.c_str(), codes.data(), p.width, p.height) != PT_OK) return "write PPM";
            if (!pfm.empty() && pt_write_pfm(pfm.c_str(), img.data(), p.width, p.height) != PT_OK) return "write PFM";
        }
        return nullptr;
    };
    pt_stats st{};
    const auto t1 = std::chrono::steady_clock::now();
    if (accumulate) {
        // the reference's progressive loop (kernel.cu:709-736) as passes of an accumulator
        int err = 0;
        pt_accum* acc = nullptr;
        pt_noise* noise = nullptr;
        if (!resume_session.empty()) {
            // the estimator of the file continues its window (it is skipped when this run estimates nothing)
            if (pt_session_load(ctx[0], resume_session.c_str(), &acc, estimate ? &noise : nullptr, nullptr) != PT_OK)
                return die("--resume-session");
            if (noise && !quiet)
                printf("noise estimate: the window saved in %s continues (%lld samples)\n", resume_session.c_str(),
                       (long long)pt_accum_samples(acc));
        } else {
            acc = resume.empty() ? pt_accum_create_view(ctx[0], &p, &cam, cam_view, &err) : pt_accum_load(ctx[0], resume.c_str(), &err);
            if (!acc) return die(resume.empty() ? "pt_accum_create" : "--resume");
        }
        const int step = pass_spp > 0 ? pass_spp : (p.spp > 0 ? p.spp : 1);
        if (estimate && !noise) {
            noise = pt_noise_create(acc, &err);
            if (!noise) return die("pt_noise_create");
            if (!resumed.empty() && !quiet)
                printf("noise estimate: a fresh window starts at the resumed state (%lld samples)\n", (long long)pt_accum_samples(acc));
        }
        bool converged = false;
        for (int left = p.spp; left > 0 && !converged; left -= step) {
            pt_stats ps{};
            if (pt_accum_add(acc, left < step ? left : step, nullptr, nullptr, &ps) != PT_OK) return die("pt_accum_add");
            st.samples += ps.samples; st.rays_traced += ps.rays_traced; st.rays_reference += ps.rays_reference;
            st.rays_nominal += ps.rays_nominal;
            if (pass_spp > 0 && !quiet) printf("sample %lld\n", (long long)pt_accum_samples(acc));   // kernel.cu:731
            if (noise) {
                // pt_accum_add_until's loop, spelled out here for the per-pass stats, lines and files: fold the pass,
                // then its stop rule
                pt_noise_summary ns;
                if (pt_noise_update(noise, &conv.noise, nullptr, &ns) != PT_OK) return die("pt_noise_update");
                converged = until_error && ns.batches >= conv.min_batches &&
                            ns.converged >= (uint64_t)ceil((double)conv.quantile * (double)ns.pixels);
                if (!quiet)
                    printf("converged %llu of %llu pixels (%.4f) at tolerance %g after %d batches\n", (unsigned long long)ns.converged,
                           (unsigned long long)ns.pixels, ns.pixels ? (double)ns.converged / (double)ns.pixels : 0.0,
                           (double)conv.noise.tol, ns.batches);
                if (adaptive && ns.batches >= conv.min_batches) {   // pt_accum_add_adaptive's step: freeze what converged
                    uint64_t newly = 0, active = 0;
                    if (pt_noise_freeze(noise, &conv.noise, nullptr, &newly, &active) != PT_OK) return die("pt_noise_freeze");
                    if (!quiet) printf("froze %llu pixels, %llu still sampled\n", (unsigned long long)newly, (unsigned long long)active);
                    if (active == 0) converged = true;
                }
            }
            if (pass_spp > 0 && left > step && !converged) {   // (the last pass's files are written below)
                if (pt_accum_read(acc, img.data(), nullptr) != PT_OK) return die("pt_accum_read");
                if (const char* what = write_images()) return die(what);
                if (!checkpoint.empty() && pt_accum_save(acc, checkpoint.c_str()) != PT_OK) return die("--checkpoint");
                if (!session.empty() && pt_session_save(acc, noise, session.c_str()) != PT_OK) return die("--session");
            }
        }
        if (pt_accum_read(acc, img.data(), nullptr) != PT_OK) return die("pt_accum_read");
        if (!checkpoint.empty() && pt_accum_save(acc, checkpoint.c_str()) != PT_OK) return die("--checkpoint");
        if (!session.empty() && pt_session_save(acc, noise, session.c_str()) != PT_OK) return die("--session");
        if (until_error)   // (printed with --quiet too: it is the run's result)
            printf("stopped at %lld samples: %s\n", (long long)pt_accum_samples(acc),
                   converged ? "converged" : "not converged (the sample cap)");
        if (!count_map.empty()) {
            const size_t npix = (size_t)p.width * p.height;
            std::vector<uint32_t> cnt(npix);
            std::vector<float> grey(npix * 3);
            if (pt_accum_counts(acc, cnt.data()) != PT_OK) return die("pt_accum_counts");
            for (int y = 0; y < p.height; ++y)
                for (int x = 0; x < p.width; ++x) {
                    const uint32_t v = cnt[p.pixel_order == PT_ORDER_MORTON ? (size_t)pt_morton_pxl_to_i(x, y) : (size_t)y * p.width + x];
                    for (int k = 0; k < 3; ++k) grey[((size_t)y * p.width + x) * 3 + k] = (float)v;
                }
            if (pt_write_pfm(count_map.c_str(), grey.data(), p.width, p.height) != PT_OK) return die("--count-map");
        }
        if (!error_map.empty()) {
            const size_t npix = (size_t)p.width * p.height;
            std::vector<float> rel2(npix), grey(npix * 3);
            if (pt_noise_map(noise, &conv.noise, rel2.data()) != PT_OK) return die("pt_noise_map");
            for (int y = 0; y < p.height; ++y)
                for (int x = 0; x < p.width; ++x) {
                    const float v = rel2[p.pixel_order == PT_ORDER_MORTON ? (size_t)pt_morton_pxl_to_i(x, y) : (size_t)y * p.width + x];
                    for (int k = 0; k < 3; ++k) grey[((size_t)y * p.width + x) * 3 + k] = v;
                }
            if (pt_write_pfm(error_map.c_str(), grey.data(), p.width, p.height) != PT_OK) return die("--error-map");
        }
        if (guided || !variance_map.empty()) {
            const size_t npix = (size_t)p.width * p.height;
            var.resize(npix);
            if (pt_noise_variance(noise, var.data()) != PT_OK) return die("pt_noise_variance");
            if (!variance_map.empty()) {
                std::vector<float> grey(npix * 3);
                for (int y = 0; y < p.height; ++y)
                    for (int x = 0; x < p.width; ++x) {
                        const float v = var[p.pixel_order == PT_ORDER_MORTON ? (size_t)pt_morton_pxl_to_i(x, y) : (size_t)y * p.width + x];
                        for (int k = 0; k < 3; ++k) grey[((size_t)y * p.width + x) * 3 + k] = v;
                    }
                if (pt_write_pfm(variance_map.c_str(), grey.data(), p.width, p.height) != PT_OK) return die("--variance-map");
            }
        }
        pt_noise_destroy(noise);
        pt_accum_destroy(acc);
    } else if (temporal) {
        // one frame per pose: render, features, push; `img` and `var` end as the last frame's temporal image and variance
        int err = 0;
        pt_temporal* hist = pt_temporal_create(ctx[0], &tparams, p.width, p.height, p.pixel_order, &err);
        if (!hist) return die("pt_temporal_create");
        const size_t npix = (size_t)p.width * p.height;
        std::vector<float> frame(n);
        feat.resize(npix);
        var.resize(npix);
        for (size_t k = 0; k < poses.size(); ++k) {
            cam.pos = poses[k].pos;
            if (pt_view_look_at(cam.pos, poses[k].target, up, &view_store) != PT_OK) return die("--camera-path");
            if (have_vfov && pt_view_set_fov(&view_store, &cam, vfov, p.width, p.height) != PT_OK) return die("--vfov");
            if (have_film) { view_store.film_w = film_w; view_store.film_h = film_h; }
            cam_view = &view_store;
            pt_params fp = p;
            fp.seed = p.seed + k;
            pt_stats ps{};
            if (pt_render_view(ctx[0], &fp, &cam, cam_view, frame.data(), &ps) != PT_OK) return die("pt_render");
            st.samples += ps.samples; st.rays_traced += ps.rays_traced; st.rays_reference += ps.rays_reference;
            st.rays_nominal += ps.rays_nominal;
            if (pt_render_features_view(ctx[0], &fp, &cam, cam_view, feat.data()) != PT_OK) return die("pt_render_features");
            if (pt_temporal_push(hist, &cam, cam_view, p.flags, frame.data(), feat.data(), img.data(), var.data()) != PT_OK)
                return die("pt_temporal_push");
            if (!quiet) printf("frame %zu of %zu\n", k + 1, poses.size());
        }
        pt_temporal_destroy(hist);
        if (!variance_map.empty()) {
            std::vector<float> grey(npix * 3);
            for (int y = 0; y < p.height; ++y)
                for (int x = 0; x < p.width; ++x) {
                    const float v = var[p.pixel_order == PT_ORDER_MORTON ? (size_t)pt_morton_pxl_to_i(x, y) : (size_t)y * p.width + x];
                    for (int k = 0; k < 3; ++k) grey[((size_t)y * p.width + x) * 3 + k] = v;
                }
            if (pt_write_pfm(variance_map.c_str(), grey.data(), p.width, p.height) != PT_OK) return die("--variance-map");
        }
    } else if (!rays.empty() && irradiance) {
        if (pt_render_irradiance(ctx[0], &p, rays.data(), img.data(), &st) != PT_OK) return die("pt_render_irradiance");
    } else if (!rays.empty()) {
        if (pt_render_rays(ctx[0], &p, rays.data(), img.data(), &st) != PT_OK) return die("pt_render_rays");
    } else {
        // one GPU: pt_render; N GPUs: image-tile shards on devices 0..N-1 summed by one RCCL reduce
        const int rc = (gpus == 1) ? pt_render_view(ctx[0], &p, &cam, cam_view, img.data(), &st)
                                   : pt_render_multi_view(ctx.data(), gpus, &p, &cam, cam_view, img.data(), &st);
        if (rc != PT_OK) return die("pt_render");
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    const uint64_t samples = st.samples, traced = st.rays_traced, reference = st.rays_reference;
    const uint64_t nominal = st.rays_nominal;   // (summed over the shards)
    if (!tri_csv.empty()) {
        // kernel.cu:742-750: one "count,\n" line per entry of the reference's test[] buffer, which
        // has bvh.size = numTris-1 entries (kernel.cu:696)
        std::vector<uint32_t> counts(view.num_tris);
        if (pt_tri_counts(ctx[0], counts.data(), view.num_tris) != PT_OK) return die("pt_tri_counts");
        FILE* f = fopen(tri_csv.c_str(), "w");
        if (!f) { fprintf(stderr, "pt_cli: cannot write %s\n", tri_csv.c_str()); return 1; }
        for (uint32_t k = 0; k + 1 < view.num_tris; ++k) fprintf(f, "%u,\n", counts[k]);
        fclose(f);
    }
    if (!quiet) {
        printf("%d GPU(s): %.3f s, %.1f Msamples/s, %.1f Mrays/s traced, %.1f Mrays/s reference-equivalent, "
               "%.1f Mrays/s nominal (kernel.cu:757)\n",
               gpus, secs, samples / secs / 1e6, traced / secs / 1e6, reference / secs / 1e6, nominal / secs / 1e6);
    }
    if (const char* what = write_images()) return die(what);
    if (!aov.empty()) {
        if (!features()) return die("pt_render_features");
        std::vector<float> plane(n);
        const char* names[4] = {"albedo", "normal", "position", "depth"};
        for (int which = 0; which < 4; ++which) {
            for (int y = 0; y < p.height; ++y)
                for (int x = 0; x < p.width; ++x) {
                    const pt_feature& f = feat[p.pixel_order == PT_ORDER_MORTON ? (size_t)pt_morton_pxl_to_i(x, y) : (size_t)y * p.width + x];
                    const float* v = which == 0 ? f.albedo : which == 1 ? f.normal : f.position;
                    for (int k = 0; k < 3; ++k) plane[((size_t)y * p.width + x) * 3 + k] = which == 3 ? f.depth : v[k];
                }
            const std::string path = aov + "_" + names[which] + ".pfm";
            if (pt_write_pfm(path.c_str(), plane.data(), p.width, p.height) != PT_OK) return die("--aov");
        }
    }
    for (pt_ctx* c : ctx) pt_destroy(c);
    pt_scene_free(s);
    return 0;
}
