// rusty_sr -- host CLI with the argv surface of millardjn/rusty_sr v1
// (reference src/main.rs:33-178), driving the MI355X engine through libsrhip's C ABI.
//
//   rusty_sr <INPUT_FILE> <OUTPUT_FILE> [-p imagenet|imagenetlinear|anime|bilinear] [-c FILE] [-d]
//   rusty_sr validate [-p imagenet|imagenetlinear|anime | -c FILE] [-l] [-r] [-m N] <VALIDATION_FOLDER>
//
// `validate` is the validation pass of the reference's `train` sub-command alone (main.rs:220-247, options of main.rs:83-114): the
// PSNR a parameter set reaches on a folder of HR images.  A first argument that is literally `validate` selects it (as `train` is
// reserved); every other argv is the upscale surface, unchanged.
//
// Differences from the reference, all outside the hot path: own codecs (PNG over zlib, baseline + progressive JPEG, GIF,
// TIFF, TGA, ICO, PPM/PGM/PBM, BMP in; PNG, JPEG, BMP, PPM out by extension -- of what the reference's `image` crate reads
// only WebP is missing), the `train` sub-command
// is not part of this build (its validation pass is, as `validate`), and three extra options that cannot collide with the
// reference's (-p -c -d): --device N, --precision f32|split_f16, --timing.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cctype>
#include <cstring>
#include <charconv>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <filesystem>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/srhip.h"
#include "png.hpp"

// The three parameter sets the reference embeds with include_bytes! (main.rs:26-28)
#define EMBED(sym, path)                                                                    \
    asm(".section .rodata\n.global " #sym "_begin\n" #sym "_begin:\n.incbin \"" path "\"\n" \
        ".global " #sym "_end\n" #sym "_end:\n.byte 0\n.previous\n");                      \
    extern "C" const unsigned char sym##_begin[], sym##_end[];
EMBED(imagenet_rsr, SR_RES_DIR "/imagenet.rsr")
EMBED(imagenetlinear_rsr, SR_RES_DIR "/imagenetlinear.rsr")
EMBED(anime_rsr, SR_RES_DIR "/anime.rsr")

namespace {

const char* kUsage =
    "Rusty SR v0.1.1 (MI355X engine)\n"
    "A convolutional neural network trained to upscale images\n\n"
    "USAGE:\n    rusty_sr [FLAGS] [OPTIONS] <INPUT_FILE> <OUTPUT_FILE>\n    rusty_sr validate [FLAGS] [OPTIONS] <VALIDATION_FOLDER>\n"
    "    rusty_sr train ...   (not part of this build)\n\n"
    "FLAGS:\n    -d, --downsample    Perform downscaling rather than upscaling\n    -h, --help          Prints help information\n"
    "    -V, --version       Prints version information\n        --timing        Print device / transfer times on stderr\n\n"
    "OPTIONS:\n    -c, --custom <PARAMETER_FILE>    Sets a custom parameter file (.rsr) to use with the neural net\n"
    "    -p, --parameters <PARAMETERS>    Sets which built-in parameters to use with the neural net [values: imagenet,\n"
    "                                     imagenetlinear, anime, bilinear]\n"
    "        --device <N>                 HIP device index [default: 0]\n"
    "        --devices <N,N,...>          spread one image over several GPUs (row shares, halo rows from the image)\n"
    "        --precision <MODE>           f32 (exact) or split_f16 (2x faster, same 1e-4 parity bar) [default: f32]\n\n"
    "ARGS:\n    <INPUT_FILE>     Sets the input image to upscale\n    <OUTPUT_FILE>    Sets the output file to write/overwrite (.png recommended)\n\n"
    "SUBCOMMANDS:\n    validate    The validation pass of `train`: PSNR of the parameters on a folder of HR images\n"
    "                (rusty_sr validate --help)\n";

const char* kValidateUsage =
    "rusty_sr validate\nPSNR of a parameter set on a folder of HR images: each image is mean-pooled f x f in linear RGB, upscaled\n"
    "by the network and compared with itself (the validation pass of the reference's `train`)\n\n"
    "USAGE:\n    rusty_sr validate [FLAGS] [OPTIONS] <VALIDATION_FOLDER>\n\n"
    "FLAGS:\n    -l, --linearLoss    Apply MSE loss to a linearised RGB output rather than sRGB values\n"
    "    -r, --recurse       Recurse into subfolders of the validation folder looking for files\n"
    "    -h, --help          Prints help information\n        --timing        Print images/s and GPU ms per image on stderr\n\n"
    "OPTIONS:\n    -c, --custom <PARAMETER_FILE>    Sets a custom parameter file (.rsr); its size selects the factor (2, 3 or 4)\n"
    "    -p, --parameters <PARAMETERS>    Sets which built-in parameters to use [values: imagenet, imagenetlinear, anime]\n"
    "    -m, --val_max <N>                Set upper limit on number of images used for the validation pass\n"
    "        --devices <N,N,...>          HIP devices; images are dealt round-robin [default: 0]\n"
    "        --precision <MODE>           f32 (exact) or split_f16 [default: f32]\n\n"
    "ARGS:\n    <VALIDATION_FOLDER>    Images from this folder (or sub-folders with -r) are scored, in path order\n";

[[noreturn]] void die(const std::string& msg, int code = 1) {
    fprintf(stderr, "error: %s\n", msg.c_str());
    exit(code);
}
[[noreturn]] void usage_error(const std::string& msg) {
    fprintf(stderr, "error: %s\n\nUSAGE:\n    rusty_sr [FLAGS] [OPTIONS] <INPUT_FILE> <OUTPUT_FILE>\n\nFor more information try --help\n", msg.c_str());
    exit(2);
}

std::vector<float> decode_rsr(const unsigned char* blob, size_t len) {
    size_t n = 0;
    if (sr_rsr_decode(blob, len, nullptr, 0, &n) != SR_OK) die("ByteVec conversion failed");  // main.rs:138
    std::vector<float> p(n);
    if (sr_rsr_decode(blob, len, p.data(), n, &n) != SR_OK) die("ByteVec conversion failed");
    return p;
}

[[noreturn]] void validate_usage_error(const std::string& msg) {
    fprintf(stderr, "error: %s\n\nUSAGE:\n    rusty_sr validate [FLAGS] [OPTIONS] <VALIDATION_FOLDER>\n\nFor more information try --help\n", msg.c_str());
    exit(2);
}

// Rust's `{}` of an f32: the shortest digits that read back as the same float, never an exponent; inf / NaN as Rust spells them
std::string rust_f32(float v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[128];
    const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

// the containers decode_image_file reads (png.hpp), by extension, case-insensitive
bool decodable(const std::filesystem::path& p) {
    std::string ext = p.extension().string();
    for (auto& ch : ext) ch = (char)tolower((unsigned char)ch);
    static const char* const kExt[] = {".png", ".jpg", ".jpeg", ".gif", ".tif", ".tiff", ".bmp", ".ico", ".tga", ".ppm", ".pgm", ".pbm", ".pnm"};
    for (const char* e : kExt) if (ext == e) return true;
    return false;
}

// rusty_sr validate: the validation pass of the reference's `train` (main.rs:220-247) on its own.  Files are decoded on up to 16 host
// threads (OMP_NUM_THREADS if set) ahead of the GPU, which scores them in path order; with --devices image i goes to context i mod n.
// The sums are taken in image order, so the printed value does not depend on the number of devices.
int run_validate(int argc, char** argv) {
    std::string parameters, custom, precision = "f32", folder;
    bool has_p = false, has_c = false, linear = false, recurse = false, timing = false, has_folder = false;
    long val_max = -1;
    std::vector<int> devices;
    for (int k = 2; k < argc; ++k) {
        const std::string a = argv[k];
        auto value = [&](const char* name) -> std::string {
            if (k + 1 >= argc) validate_usage_error(std::string("The argument '") + name + "' requires a value but none was supplied");
            return argv[++k];
        };
        if (a == "-h" || a == "--help") { fputs(kValidateUsage, stdout); return 0; }
        else if (a == "-l" || a == "--linearLoss") linear = true;
        else if (a == "-r" || a == "--recurse") recurse = true;
        else if (a == "--timing") timing = true;
        else if (a == "-d" || a == "--downsample") validate_usage_error("The argument '--downsample' cannot be used with 'validate'");
        else if (a == "-p" || a == "--parameters") { parameters = value("--parameters <PARAMETERS>"); has_p = true; }
        else if (a.rfind("--parameters=", 0) == 0) { parameters = a.substr(13); has_p = true; }
        else if (a == "-c" || a == "--custom") { custom = value("--custom <PARAMETER_FILE>"); has_c = true; }
        else if (a.rfind("--custom=", 0) == 0) { custom = a.substr(9); has_c = true; }
        else if (a == "-m" || a == "--val_max" || a.rfind("--val_max=", 0) == 0) {
            const std::string v = a.rfind("--val_max=", 0) == 0 ? a.substr(10) : value("--val_max <N>");
            long n = 0;
            const auto r = std::from_chars(v.data(), v.data() + v.size(), n);
            if (v.empty() || r.ec != std::errc() || r.ptr != v.data() + v.size() || n <= 0)
                validate_usage_error("-val_max N must be a positive integer");  // main.rs:225
            val_max = n;
        }
        else if (a == "--devices") {
            const std::string list = value("--devices <N,N,...>");
            for (size_t pos0 = 0; pos0 <= list.size();) {
                const size_t comma = std::min(list.find(',', pos0), list.size());
                if (comma == pos0 || !isdigit((unsigned char)list[pos0])) validate_usage_error("'" + list + "' isn't a valid value for '--devices <N,N,...>'");
                devices.push_back(atoi(list.substr(pos0, comma - pos0).c_str()));
                pos0 = comma + 1;
            }
        }
        else if (a == "--precision") precision = value("--precision <MODE>");
        else if (a.size() > 1 && a[0] == '-') validate_usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else if (has_folder) validate_usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else { folder = a; has_folder = true; }
    }
    if (has_p && parameters != "imagenet" && parameters != "imagenetlinear" && parameters != "anime")
        validate_usage_error("'" + parameters + "' isn't a valid value for '--parameters <PARAMETERS>'\n\t[values: anime, imagenet, imagenetlinear]");
    if (has_c && has_p) validate_usage_error("The argument '--custom <PARAMETER_FILE>' cannot be used with '--parameters <PARAMETERS>'");
    if (!has_folder) validate_usage_error("The following required arguments were not provided:\n    <VALIDATION_FOLDER>");
    if (precision != "f32" && precision != "split_f16") validate_usage_error("'" + precision + "' isn't a valid value for '--precision <MODE>'");
    if (devices.empty()) devices.push_back(0);

    // ---- the files: decodable extensions, sorted by path bytes, the first N with -m
    namespace fs = std::filesystem;
    std::vector<std::string> files;
    {
        std::error_code ec;
        if (!fs::is_directory(folder, ec)) validate_usage_error("'" + folder + "' is not a folder");
        auto take = [&](const fs::directory_entry& e) {
            std::error_code ec2;
            if (e.is_regular_file(ec2) && decodable(e.path())) files.push_back(e.path().string());
        };
        if (recurse) {
            for (fs::recursive_directory_iterator it(folder, ec), end; !ec && it != end; it.increment(ec)) take(*it);
        } else {
            for (fs::directory_iterator it(folder, ec), end; !ec && it != end; it.increment(ec)) take(*it);
        }
        if (ec) die("could not read the validation folder (" + ec.message() + ")");
        std::sort(files.begin(), files.end());
        if (val_max > 0 && (size_t)val_max < files.size()) files.resize((size_t)val_max);
        if (files.empty()) validate_usage_error("no image files in '" + folder + "'" + (recurse ? "" : " (-r recurses into subfolders)"));
    }

    // ---- parameters; a custom file's length selects the factor it was trained for
    std::vector<float> params;
    if (has_c) {
        FILE* f = fopen(custom.c_str(), "rb");
        if (!f) die("Error opening parameter file");  // main.rs:134
        std::vector<unsigned char> data;
        unsigned char tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + n);
        fclose(f);
        printf("Validating using custom neural net parameters...");
        params = decode_rsr(data.data(), data.size());
    } else if (!has_p || parameters == "imagenet") {
        printf("Validating using imagenet neural net parameters...");
        params = decode_rsr(imagenet_rsr_begin, imagenet_rsr_end - imagenet_rsr_begin);
    } else if (parameters == "imagenetlinear") {
        printf("Validating using linear loss imagenet neural net parameters...");
        params = decode_rsr(imagenetlinear_rsr_begin, imagenetlinear_rsr_end - imagenetlinear_rsr_begin);
    } else {
        printf("Validating using anime neural net parameters...");
        params = decode_rsr(anime_rsr_begin, anime_rsr_end - anime_rsr_begin);
    }
    printf(" %zu image%s%s\n", files.size(), files.size() == 1 ? "" : "s", linear ? ", linear loss" : "");
    fflush(stdout);
    int factor = SR_FACTOR;
    for (int f : {3, 2, 4})
        if (params.size() == (size_t)sr_num_params_factor(f)) { factor = f; break; }

    // ---- decoding ahead of the GPU: worker threads take the next file; at most 2 x threads decoded images wait for the GPU
    const size_t nfile = files.size();
    unsigned threads = 16;
    if (const char* e = getenv("OMP_NUM_THREADS")) { const int v = atoi(e); if (v > 0) threads = (unsigned)std::min(v, 16); }
    threads = (unsigned)std::min<size_t>(threads, nfile);
    struct Slot { srpng::Image img; std::string err; int state = 0; };  // 0 pending, 1 decoded, 2 failed, 3 scored
    std::vector<Slot> slots(nfile);
    std::mutex mu;
    std::condition_variable cv;
    size_t next = 0, scored = 0;
    bool stop = false;
    const size_t window = 2 * (size_t)threads + devices.size();
    std::vector<std::thread> decoders;
    for (unsigned t = 0; t < threads; ++t)
        decoders.emplace_back([&] {
            for (;;) {
                size_t i;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return stop || next >= nfile || next < scored + window; });
                    if (stop || next >= nfile) return;
                    i = next++;
                }
                srpng::Image img;
                std::string err;
                const bool ok = srpng::decode_image_file(files[i], img, err);
                std::lock_guard<std::mutex> lk(mu);
                slots[i].img = std::move(img);
                slots[i].err = err;
                slots[i].state = ok ? 1 : 2;
                cv.notify_all();
            }
        });

    // ---- contexts, one scoring thread per context
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    std::vector<sr_ctx*> ctxs(devices.size(), nullptr);
    int rc = SR_OK;
    for (size_t k = 0; k < devices.size() && rc == SR_OK; ++k) {
        rc = sr_create(&ctxs[k], params.data(), params.size(), factor, devices[k]);
        if (rc == SR_OK) rc = sr_set_precision(ctxs[k], precision == "f32" ? SR_PRECISION_F32 : SR_PRECISION_SPLIT_F16);
        if (rc == SR_OK && timing) rc = sr_set_profiling(ctxs[k], 1);
    }
    std::vector<double> err(nfile, 0.0), gpu_ms(nfile, 0.0);
    std::vector<size_t> cnt(nfile, 0);
    std::string failure;
    int fail_code = 0;
    std::vector<std::thread> scorers;
    if (rc != SR_OK) {
        failure = sr_strerror(rc);
        fail_code = 1;
    } else {
        for (size_t k = 0; k < ctxs.size(); ++k)
            scorers.emplace_back([&, k] {
                for (size_t i = k; i < nfile; i += ctxs.size()) {
                    srpng::Image img;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return stop || slots[i].state != 0; });
                        if (stop) return;
                        if (slots[i].state == 2) {
                            if (failure.empty() || fail_code == 0) { failure = "Error opening validation image file " + files[i] + " (" + slots[i].err + ")"; fail_code = 1; }
                            stop = true;
                            cv.notify_all();
                            return;
                        }
                        img = std::move(slots[i].img);
                        slots[i].state = 3;
                    }
                    const int r = sr_validation_error_rgba8(ctxs[k], img.rgba.data(), 4, img.h, img.w, linear ? 1 : 0, &err[i], &cnt[i]);
                    if (r == SR_OK && timing) { double tot = 0; sr_last_timing(ctxs[k], &tot, nullptr, nullptr, nullptr); gpu_ms[i] = tot; }
                    std::lock_guard<std::mutex> lk(mu);
                    if (r != SR_OK) {
                        if (failure.empty()) {
                            failure = files[i] + ": " + sr_strerror(r) + (r == SR_E_INVALID ? " (smaller than one pooling block?)" : "");
                            fail_code = 1;
                        }
                        stop = true;
                    }
                    ++scored;
                    cv.notify_all();
                }
            });
    }
    for (auto& t : scorers) t.join();
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
        cv.notify_all();
    }
    for (auto& t : decoders) t.join();
    for (sr_ctx* c : ctxs) sr_destroy(c);
    if (fail_code) die(failure, fail_code);
    double err_sum = 0, n_sum = 0, ms_sum = 0;
    for (size_t i = 0; i < nfile; ++i) { err_sum += err[i]; n_sum += (double)cnt[i]; ms_sum += gpu_ms[i]; }
    const float psnr = err_sum == 0.0 ? INFINITY : (float)(-10.0 * std::log10(err_sum / n_sum));
    printf("Validation PSNR:\t%s\n", rust_f32(psnr).c_str());  // main.rs:246
    if (timing) {
        const double s = std::chrono::duration<double>(clk::now() - t0).count();
        fprintf(stderr, "[timing] %zu images in %.3f s: %.2f images/s; GPU %.3f ms per image (whole validation call)\n", nfile, s, nfile / s,
                ms_sum / nfile);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<std::string> pos;
    std::string parameters, custom, precision = "f32";
    bool has_p = false, has_c = false, downsample = false, timing = false;
    int device = 0;
    std::vector<int> devices;
    if (argc >= 2 && !strcmp(argv[1], "train"))  // main.rs:119-121
        die("the `train` sub-command is not part of this build (the MI355X engine covers the upscale path only)", 2);
    if (argc >= 2 && !strcmp(argv[1], "validate")) return run_validate(argc, argv);
    for (int k = 1; k < argc; ++k) {
        const std::string a = argv[k];
        auto value = [&](const char* name) -> std::string {
            if (k + 1 >= argc) usage_error(std::string("The argument '") + name + "' requires a value but none was supplied");
            return argv[++k];
        };
        if (a == "-h" || a == "--help") { fputs(kUsage, stdout); return 0; }
        else if (a == "-V" || a == "--version") { puts("Rusty SR v0.1.1"); return 0; }
        else if (a == "-d" || a == "--downsample") downsample = true;
        else if (a == "--timing") timing = true;
        else if (a == "-p" || a == "--parameters") { parameters = value("--parameters <PARAMETERS>"); has_p = true; }
        else if (a.rfind("--parameters=", 0) == 0) { parameters = a.substr(13); has_p = true; }
        else if (a == "-c" || a == "--custom") { custom = value("--custom <PARAMETER_FILE>"); has_c = true; }
        else if (a.rfind("--custom=", 0) == 0) { custom = a.substr(9); has_c = true; }
        else if (a == "--device") device = atoi(value("--device <N>").c_str());
        else if (a == "--devices") {
            const std::string list = value("--devices <N,N,...>");
            for (size_t pos0 = 0; pos0 <= list.size();) {
                const size_t comma = std::min(list.find(',', pos0), list.size());
                if (comma == pos0 || !isdigit((unsigned char)list[pos0])) usage_error("'" + list + "' isn't a valid value for '--devices <N,N,...>'");
                devices.push_back(atoi(list.substr(pos0, comma - pos0).c_str()));
                pos0 = comma + 1;
            }
        }
        else if (a == "--precision") precision = value("--precision <MODE>");
        else if (a.size() > 1 && a[0] == '-') usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else pos.push_back(a);
    }
    // clap rules of the reference: possible_values (main.rs:54), conflicts (main.rs:58,66), required positionals
    if (has_p && parameters != "imagenet" && parameters != "imagenetlinear" && parameters != "anime" && parameters != "bilinear")
        usage_error("'" + parameters + "' isn't a valid value for '--parameters <PARAMETERS>'\n\t[values: anime, bilinear, imagenet, imagenetlinear]");
    if (has_c && has_p) usage_error("The argument '--custom <PARAMETER_FILE>' cannot be used with '--parameters <PARAMETERS>'");
    if (downsample && (has_p || has_c)) usage_error("The argument '--downsample' cannot be used with '--parameters <PARAMETERS>' or '--custom <PARAMETER_FILE>'");
    if (pos.size() < 2) usage_error("The following required arguments were not provided:\n    <INPUT_FILE>\n    <OUTPUT_FILE>");
    if (pos.size() > 2) usage_error("Found argument '" + pos[2] + "' which wasn't expected, or isn't valid in this context");
    if (precision != "f32" && precision != "split_f16") usage_error("'" + precision + "' isn't a valid value for '--precision <MODE>'");

    // ---- parameters + graph (main.rs:133-158), same progress text
    std::vector<float> params;
    int graph = SR_GRAPH_SR_NET;
    if (has_c) {
        FILE* f = fopen(custom.c_str(), "rb");
        if (!f) die("Error opening parameter file");  // main.rs:134
        std::vector<unsigned char> data;
        unsigned char tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + n);
        fclose(f);
        printf("Upscaling using custom neural net parameters...");
        params = decode_rsr(data.data(), data.size());
    } else if (downsample) {
        printf("Downsampling using average pooling of linear RGB values...");
        graph = SR_GRAPH_DOWNSAMPLE;
    } else if (!has_p || parameters == "imagenet") {
        printf("Upscaling using imagenet neural net parameters...");
        params = decode_rsr(imagenet_rsr_begin, imagenet_rsr_end - imagenet_rsr_begin);
    } else if (parameters == "imagenetlinear") {
        printf("Upscaling using linear loss imagenet neural net parameters...");
        params = decode_rsr(imagenetlinear_rsr_begin, imagenetlinear_rsr_end - imagenetlinear_rsr_begin);
    } else if (parameters == "anime") {
        printf("Upscaling using anime neural net parameters...");
        params = decode_rsr(anime_rsr_begin, anime_rsr_end - anime_rsr_begin);
    } else {
        printf("Upscaling using bilinear interpolation...");
        graph = SR_GRAPH_BILINEAR;
    }
    fflush(stdout);

    if (devices.empty() || graph != SR_GRAPH_SR_NET) devices.assign(1, devices.empty() ? device : devices[0]);
    {   // `.save()` picks the container from the extension (main.rs:175): refuse an unknown one before any work is spent on the picture
        const size_t dot = pos[1].find_last_of('.');
        std::string ext = dot == std::string::npos ? "" : pos[1].substr(dot + 1);
        for (auto& ch : ext) ch = (char)tolower((unsigned char)ch);
        if (ext != "png" && ext != "jpg" && ext != "jpeg" && ext != "bmp" && ext != "ppm")
            die("Could not write output file (this build writes .png, .jpg, .bmp and .ppm)");
    }
    // The input file decodes on a second thread while this one brings up the device and the contexts (HIP start-up
    // and the weight upload take longer than a 1080p PNG); failures are then reported in the reference's order --
    // the graph first (main.rs:160-162), the image after it (main.rs:164).
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    const clk::time_point t_start = clk::now();
    srpng::Image in;
    std::string err;
    bool decoded = false;
    double t_decode = 0;
    std::thread decoder([&] {
        const clk::time_point t = clk::now();
        decoded = srpng::decode_image_file(pos[0], in, err);
        t_decode = ms_since(t);
    });
    // The file's header already says how large the output is (probe_image_size): a third thread page-locks it -- 15 ms at
    // 1080p, 60 ms at 4K, and independent of the context -- while this one creates the context, lets the library allocate and
    // warm what the call will need (sr_reserve_rgba8), and the decoder is still busy.
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    int pw = 0, ph = 0;
    const bool sized = srpng::probe_image_size(pos[0], pw, ph) && !(graph == SR_GRAPH_DOWNSAMPLE && (pw < 3 || ph < 3));
    std::thread pinner([&] {
        if (!sized) return;
        const size_t bytes = graph == SR_GRAPH_DOWNSAMPLE ? (size_t)(pw / 3) * (ph / 3) * 4 : (size_t)pw * 3 * ph * 3 * 4;
        if (sr_host_alloc(&pinned, bytes) == SR_OK) pinned_bytes = bytes; else pinned = nullptr;
    });
    std::vector<sr_ctx*> ctxs(devices.size(), nullptr);
    int rc = SR_OK;
    for (size_t k = 0; k < devices.size() && rc == SR_OK; ++k) {
        rc = sr_create_graph(&ctxs[k], graph, params.empty() ? nullptr : params.data(), params.size(), SR_FACTOR, devices[k]);
        if (rc == SR_OK && graph == SR_GRAPH_SR_NET) rc = sr_set_precision(ctxs[k], precision == "f32" ? SR_PRECISION_F32 : SR_PRECISION_SPLIT_F16);
    }
    const double t_create = ms_since(t_start);
    double t_prep = 0;
    {
        const clk::time_point t = clk::now();
        if (rc == SR_OK && sized && ctxs.size() == 1) (void)sr_reserve_rgba8(ctxs[0], 4, 1, ph, pw);  // best effort: the real call reports errors
        pinner.join();
        t_prep = ms_since(t);
    }
    decoder.join();
    if (rc != SR_OK) die(sr_strerror(rc));  // SR_E_PARAM_COUNT carries the text of main.rs:162
    sr_ctx* ctx = ctxs[0];
    if (!decoded) die("Error opening input image file. (" + err + ")");  // main.rs:164
    const double t_ready = ms_since(t_start);
    if (graph == SR_GRAPH_DOWNSAMPLE && (in.w < 3 || in.h < 3)) die("input image is smaller than one 3x3 pooling block");

    const int ow = graph == SR_GRAPH_DOWNSAMPLE ? in.w / 3 : in.w * 3, oh = graph == SR_GRAPH_DOWNSAMPLE ? in.h / 3 : in.h * 3;
    // page-locked output pixels: the download then runs at PCIe rate under the kernels of the next band
    const size_t out_bytes = (size_t)ow * oh * 4;
    const clk::time_point t_al = clk::now();
    std::vector<uint8_t> pageable;
    if (pinned && pinned_bytes != out_bytes) { sr_host_free(pinned); pinned = nullptr; }  // the header lied
    if (!pinned && sr_host_alloc(&pinned, out_bytes) != SR_OK) { pinned = nullptr; pageable.resize(out_bytes); }
    uint8_t* out = pinned ? (uint8_t*)pinned : pageable.data();
    // img_to_data + graph.forward + data_to_img(..).to_rgba(), fused on the device (main.rs:168-175)
    const double t_alloc = ms_since(t_al);
    const clk::time_point t_up = clk::now();
    rc = ctxs.size() > 1 ? sr_upscale_rgba8_multi(ctxs.data(), (int)ctxs.size(), in.rgba.data(), 4, in.h, in.w, out)
                         : sr_upscale_rgba8(ctx, in.rgba.data(), 4, 1, in.h, in.w, out);
    if (rc != SR_OK) die(std::string(sr_strerror(rc)) + (rc == SR_E_HIP ? " (hipError " + std::to_string(sr_last_hip_error(ctx)) + ")" : ""));
    const double t_upscale = ms_since(t_up);
    if (timing) {
        double tot = 0, h2d = 0, d2h = 0;
        sr_last_timing(ctx, &tot, nullptr, &h2d, &d2h);
        fprintf(stderr, "\n[timing] %dx%d -> %dx%d: kernels %.3f ms, h2d %.3f ms, d2h %.3f ms\n", in.w, in.h, ow, oh, tot, h2d, d2h);
    }
    printf(" Writing file...");
    fflush(stdout);
    const clk::time_point t_enc = clk::now();
    if (!srpng::encode_image_file(pos[1], out, ow, oh, err)) die("Could not write output file (" + err + ")");  // main.rs:175
    const double t_encode = ms_since(t_enc);
    puts(" Done");
    if (timing)  // t_cli of SURVEY.md 8(d): everything this process did, by phase (decode and device start-up overlap)
        fprintf(stderr, "[timing] wall: decode %.1f ms || device + contexts %.1f ms, reserve (|| page-locking the output) %.1f ms -> ready at %.1f ms; "
                        "late allocations %.1f ms; upscale call %.1f ms; encode + write %.1f ms; total %.1f ms\n", t_decode, t_create, t_prep, t_ready,
                t_alloc, t_upscale, t_encode, ms_since(t_start));
    sr_host_free(pinned);
    for (sr_ctx* c : ctxs) sr_destroy(c);
    return 0;
}
