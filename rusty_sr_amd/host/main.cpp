// rusty_sr -- host CLI with the argv surface of millardjn/rusty_sr v1
// (reference src/main.rs:33-258), driving the MI355X engine through libsrhip's C ABI.
//
//   rusty_sr <INPUT_FILE> <OUTPUT_FILE> [-p imagenet|imagenetlinear|anime|bilinear] [-c FILE] [-d]
//   rusty_sr train [-l] [-r] [-s START] [-f 2|3|4] [-v VAL_FOLDER] [-m N] [--lr_folder DIR] [--val_lr_folder DIR] [--augment] [--degrade SPEC] [--loss LOSS] <PARAMETER_FILE> <TRAINING_FOLDER>
//   rusty_sr validate [-p imagenet|imagenetlinear|anime | -c FILE] [-l] [-r] [-m N] [--lr_folder DIR] [--metrics [--shave N]] [--degrade SPEC [--seed N]] <VALIDATION_FOLDER>
//   rusty_sr video [-p ..|-c FILE] [--precision ..] [--device N] [--ensemble N] [--matrix bt601|bt709|bt2020] [--depth 8|auto] [--siting center|left] [--slots N] [--reuse] [--size WxH|--scale S [--filter F] [--resize-space linear|srgb]] [--timing] <IN|-> <OUT|->
//
// `validate` is the validation pass of the reference's `train` sub-command alone (main.rs:220-247, options of main.rs:83-114): the
// PSNR a parameter set reaches on a folder of HR images.  `video` upscales a YUV4MPEG2 stream frame by frame (y4m.hpp; the reference has
// no counterpart).  A first argument that is literally `train`, `validate` or `video` selects it; every other argv is the upscale
// surface, unchanged.
//
// Differences from the reference, all outside the hot path: own codecs (PNG over zlib, baseline + progressive JPEG, GIF,
// TIFF, TGA, ICO, PPM/PGM/PBM, BMP in; PNG, JPEG, BMP, PPM out by extension -- of what the reference's `image` crate reads
// only WebP is missing), and extra options that cannot collide with the reference's: --device N, --precision f32|split_f16,
// --timing, --ensemble 2|4|8 (upscale and validate: the network averaged over flips / rotations), --alpha [--bleed N] (upscale: the alpha
// channel is kept -- colours bled under the transparent pixels, alpha interpolated; PNG output only), --size WxH | --scale S [--filter F]
// [--resize-space linear|srgb] (upscale: the network's f32 output resampled to that size on the GPU, quantised once), --border
// wrap|replicate|mirror [--border-pad N] (upscale: the image is continued that way beyond its edges instead of the network's zero padding
// -- wrap makes a tileable texture come back seamless); for `train` --seed N (initial
// parameters, shuffles and crops are seeded; the reference's are random), --augment (each crop under a random one of the 8 flips and
// rotations, applied by the crop kernel), --degrade SPEC (train and validate: the network's input is the HR crop or image blurred, pooled,
// noised and JPEG-compressed on the GPU, each draw with its own values: degrade_spec.hpp), --loss mse|l1|charbonnier[:EPS] (the
// objective of every step, sr_set_loss; the reference's is the squared one) and --steps N (stop
// early; when that ends the run between two checkpoints the parameter file is also written at the last step -- the reference only
// writes it after step 1 and every 100 steps).
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cctype>
#include <cstring>
#include <charconv>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <filesystem>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/srhip.h"
#include "degrade_spec.hpp"
#include "png.hpp"
#include "train_state.hpp"
#include "y4m.hpp"

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
    "    rusty_sr train [FLAGS] [OPTIONS] <PARAMETER_FILE> <TRAINING_FOLDER>\n\n"
    "FLAGS:\n    -d, --downsample    Perform downscaling rather than upscaling\n    -h, --help          Prints help information\n"
    "    -V, --version       Prints version information\n        --timing        Print device / transfer times on stderr\n"
    "        --alpha         Keep transparency: bleed the visible colours under the transparent pixels, upscale, and\n"
    "                        write the interpolated alpha channel (.png output only)\n\n"
    "OPTIONS:\n    -c, --custom <PARAMETER_FILE>    Sets a custom parameter file (.rsr) to use with the neural net\n"
    "    -p, --parameters <PARAMETERS>    Sets which built-in parameters to use with the neural net [values: imagenet,\n"
    "                                     imagenetlinear, anime, bilinear]\n"
    "        --device <N>                 HIP device index [default: 0]\n"
    "        --devices <N,N,...>          spread one image over several GPUs (row shares, halo rows from the image)\n"
    "        --precision <MODE>           f32 (exact) or split_f16 (2x faster, same 1e-4 parity bar) [default: f32]\n"
    "        --ensemble <N>               average the network over N flips / rotations of the image: 2 (mirror), 4 (flips)\n"
    "                                     or 8 (flips and rotations); N passes for slightly better pixels\n"
    "        --bleed <N>                  with --alpha: how many pixels the colours are bled outward, 0..16 [default: 8]\n"
    "        --size <WxH>                 write exactly W x H pixels: the network's output is resampled on the GPU before it\n"
    "                                     is quantised (each axis 1..16384)\n"
    "        --scale <S>                  the same with W x H = the INPUT's size times S, rounded (a positive decimal: 1.5, 2,\n"
    "                                     0.5), whatever the factor of the weights\n"
    "        --filter <FILTER>            with --size / --scale: the resampling filter [values: box, triangle, catrom,\n"
    "                                     lanczos3] [default: lanczos3]\n"
    "        --resize-space <SPACE>       with --size / --scale: resample in linear light or on the sRGB values [values:\n"
    "                                     linear, srgb] [default: linear]\n"
    "        --border <MODE>              what lies beyond the image's edges: wrap (a tileable texture stays seamless),\n"
    "                                     replicate or mirror [values: wrap, replicate, mirror] [default: the network's\n"
    "                                     own zero padding]\n"
    "        --border-pad <N>             with --border: how many pixels the image is continued by, 7..32 [default: 8]\n"
    "        --depth <BITS>               bits a sample, in and out: 16 keeps both bytes of a 16-bit PNG / PNM / TIFF and writes\n"
    "                                     a 16-bit .png (grey stays grey) or .ppm; auto is 16 for such a file and output, else\n"
    "                                     8 [values: 8, 16, auto] [default: 8]\n\n"
    "ARGS:\n    <INPUT_FILE>     Sets the input image to upscale\n    <OUTPUT_FILE>    Sets the output file to write/overwrite (.png recommended)\n\n"
    "SUBCOMMANDS:\n    train       Trains a new set of neural network parameters on the GPU (rusty_sr train --help)\n"
    "    validate    The validation pass of `train`: PSNR of the parameters on a folder of HR images\n"
    "                (rusty_sr validate --help)\n";

const char* kValidateUsage =
    "rusty_sr validate\nPSNR of a parameter set on a folder of HR images: each image is mean-pooled f x f in linear RGB, upscaled\n"
    "by the network and compared with itself (the validation pass of the reference's `train`)\n\n"
    "USAGE:\n    rusty_sr validate [FLAGS] [OPTIONS] <VALIDATION_FOLDER>\n\n"
    "FLAGS:\n    -l, --linearLoss    Apply MSE loss to a linearised RGB output rather than sRGB values\n"
    "    -r, --recurse       Recurse into subfolders of the validation folder looking for files\n"
    "    -h, --help          Prints help information\n        --timing        Print images/s and GPU ms per image on stderr\n"
    "        --metrics       Also print Y-PSNR and SSIM: the 8-bit luma of the saved image, border shaved, averaged per image\n\n"
    "OPTIONS:\n    -c, --custom <PARAMETER_FILE>    Sets a custom parameter file (.rsr); its size selects the factor (2, 3 or 4)\n"
    "    -p, --parameters <PARAMETERS>    Sets which built-in parameters to use [values: imagenet, imagenetlinear, anime]\n"
    "    -m, --val_max <N>                Set upper limit on number of images used for the validation pass\n"
    "        --lr_folder <DIR>            Score LR / HR pairs: the network's input is the file of DIR with the same relative\n"
    "                                     path (extension ignored), exactly 1/f the size, instead of the pooled HR image\n"
    "        --devices <N,N,...>          HIP devices; images are dealt round-robin [default: 0]\n"
    "        --precision <MODE>           f32 (exact) or split_f16 [default: f32]\n"
    "        --ensemble <N>               score the network averaged over N flips / rotations of its input [values: 2, 4, 8]\n"
    "        --shave <N>                  with --metrics: pixels removed from each border before scoring [default: the factor]\n"
    "        --degrade <SPEC>             Score LR / HR pairs whose LR image is made from the HR image on the GPU: SPEC is\n"
    "                                     blur=A[:B],noise=A[:B],jpeg=A[:B] (Gaussian sigma 0..4 HR pixels, noise 0..64 levels, JPEG\n"
    "                                     quality 1..100; a key left out is off); image i takes draw i of the ranges\n"
    "        --seed <N>                   with --degrade: seed of the draws [default: 0]\n\n"
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

// --ensemble 2|4|8 -> the member mask of sr_upscale_ensemble_* (0: not a valid value)
unsigned ensemble_mask(const std::string& v) {
    return v == "2" ? SR_ENSEMBLE_HFLIP : v == "4" ? SR_ENSEMBLE_FLIPS : v == "8" ? SR_ENSEMBLE_ALL : 0u;
}

// ---- --size <WxH> / --scale <S>: the output size of the resampled call (sr_upscale_rgba8_sized)
constexpr int kMaxOutputAxis = 16384;

// "WxH", two whole numbers 1 .. kMaxOutputAxis
bool parse_size(const std::string& v, int& w, int& h) {
    const size_t x = v.find_first_of("xX");
    if (x == std::string::npos || x == 0 || x + 1 >= v.size()) return false;
    const char* b = v.data();
    const auto rw = std::from_chars(b, b + x, w), rh = std::from_chars(b + x + 1, b + v.size(), h);
    return rw.ec == std::errc() && rw.ptr == b + x && rh.ec == std::errc() && rh.ptr == b + v.size() && w >= 1 && h >= 1 &&
           w <= kMaxOutputAxis && h <= kMaxOutputAxis;
}

// a positive decimal: digits with at most one point, no sign, no exponent
bool parse_scale(const std::string& v, double& s) {
    if (v.empty() || v.size() > 32) return false;
    int digits = 0, points = 0;
    for (const char ch : v) {
        if (isdigit((unsigned char)ch)) ++digits;
        else if (ch == '.') ++points;
        else return false;
    }
    if (!digits || points > 1) return false;
    s = strtod(v.c_str(), nullptr);
    return std::isfinite(s) && s > 0;
}

// one axis of --scale: max(1, floor(in S + 0.5)); false above kMaxOutputAxis
bool scaled_axis(int in, double s, int& out) {
    const double v = std::max(1.0, std::floor((double)in * s + 0.5));
    if (v > kMaxOutputAxis) return false;
    out = (int)v;
    return true;
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

// Decoding ahead of the GPU (validate, train): up to 16 host threads (OMP_NUM_THREADS if set) decode queued files; at most `window`
// decoded images wait to be taken.  Jobs are numbered in push order; take(j) blocks until job j is decoded.  stop() wakes every waiter.
class DecoderPool {
public:
    DecoderPool(const std::vector<std::string>& files, size_t most_jobs, size_t extra_window = 0) : files_(files) {
        unsigned threads = 16;
        if (const char* e = getenv("OMP_NUM_THREADS")) { const int v = atoi(e); if (v > 0) threads = (unsigned)std::min(v, 16); }
        threads = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, most_jobs));
        window_ = 2 * (size_t)threads + extra_window;
        for (unsigned t = 0; t < threads; ++t) workers_.emplace_back([this] { work(); });
    }
    ~DecoderPool() {
        stop();
        for (auto& t : workers_) t.join();
    }
    size_t push(size_t file) {
        std::lock_guard<std::mutex> lk(mu_);
        jobs_.push_back(Slot{file, {}, {}, 0});
        cv_.notify_all();
        return base_ + jobs_.size() - 1;
    }
    // false: the file did not decode (err says why) or the pool was stopped (err empty)
    bool take(size_t job, srpng::Image& img, std::string& err) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || jobs_[job - base_].state != 0; });
        if (stop_) { err.clear(); return false; }
        Slot& sl = jobs_[job - base_];
        const bool ok = sl.state == 1;
        img = std::move(sl.img);
        err = std::move(sl.err);
        sl.state = 3;
        while (!jobs_.empty() && jobs_.front().state == 3) { jobs_.pop_front(); ++base_; }
        cv_.notify_all();
        return ok;
    }
    void stop() {
        std::lock_guard<std::mutex> lk(mu_);
        stop_ = true;
        cv_.notify_all();
    }
    size_t file_of(size_t job) {
        std::lock_guard<std::mutex> lk(mu_);
        return jobs_[job - base_].file;
    }

private:
    struct Slot { size_t file; srpng::Image img; std::string err; int state; };  // 0 pending, 1 decoded, 2 failed, 3 taken
    void work() {
        for (;;) {
            size_t j, file;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || (next_ < base_ + jobs_.size() && next_ < base_ + window_); });
                if (stop_) return;
                j = next_++;
                file = jobs_[j - base_].file;
            }
            srpng::Image img;
            std::string err;
            const bool ok = srpng::decode_image_file(files_[file], img, err);
            std::lock_guard<std::mutex> lk(mu_);
            Slot& sl = jobs_[j - base_];
            sl.img = std::move(img);
            sl.err = err;
            sl.state = ok ? 1 : 2;
            cv_.notify_all();
        }
    }
    const std::vector<std::string>& files_;
    std::deque<Slot> jobs_;
    size_t base_ = 0, next_ = 0, window_ = 32;
    bool stop_ = false;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<std::thread> workers_;
};

// The decodable files of a folder (with recurse: of its subfolders too), sorted by path bytes.  false: the folder could not be read.
bool list_images(const std::string& folder, bool recurse, std::vector<std::string>& files, std::string& err) {
    namespace fs = std::filesystem;
    std::error_code ec;
    auto take = [&](const fs::directory_entry& e) {
        std::error_code ec2;
        if (e.is_regular_file(ec2) && decodable(e.path())) files.push_back(e.path().string());
    };
    if (recurse) {
        for (fs::recursive_directory_iterator it(folder, ec), end; !ec && it != end; it.increment(ec)) take(*it);
    } else {
        for (fs::directory_iterator it(folder, ec), end; !ec && it != end; it.increment(ec)) take(*it);
    }
    if (ec) { err = ec.message(); return false; }
    std::sort(files.begin(), files.end());
    return true;
}

// --lr_folder: the LR partner of every HR file -- the file of lr_folder with the same path relative to its folder, extension ignored.
// An HR file without one ends the run (the message names it); LR files without an HR partner are ignored.
std::vector<std::string> pair_files(const std::string& hr_folder, const std::vector<std::string>& hr_files, const std::string& lr_folder,
                                    bool recurse) {
    namespace fs = std::filesystem;
    std::vector<std::string> lr_files;
    std::string err;
    if (!list_images(lr_folder, recurse, lr_files, err)) die("could not read the LR folder (" + err + ")");
    auto key = [](const std::string& folder, const std::string& file) {
        return fs::path(file).lexically_relative(folder).replace_extension().generic_string();
    };
    std::map<std::string, std::string> by_key;
    for (const std::string& f : lr_files) by_key.emplace(key(lr_folder, f), f);  // (sorted: of two extensions the first in path order)
    std::vector<std::string> out;
    for (const std::string& f : hr_files) {
        const auto it = by_key.find(key(hr_folder, f));
        if (it == by_key.end()) die(f + " has no LR partner in '" + lr_folder + "'");
        out.push_back(it->second);
    }
    return out;
}

// A pair whose HR size is not exactly f x its LR size ends the run.
void check_pair_sizes(const std::string& hr_file, const srpng::Image& hr, const std::string& lr_file, const srpng::Image& lr, int f) {
    if (hr.h == f * lr.h && hr.w == f * lr.w) return;
    die(hr_file + " is " + std::to_string(hr.w) + "x" + std::to_string(hr.h) + " but its LR partner " + lr_file + " is " +
        std::to_string(lr.w) + "x" + std::to_string(lr.h) + ": the HR size must be exactly " + std::to_string(f) + " x the LR size");
}

// --degrade in `validate` and in `train -v`: the HR image is cropped in place to a multiple of f (the pooled call's crop rule: the
// top-left f floor(h / f) x f floor(w / f)) and degraded whole -- frame = the cropped image, member 0 -- into lr (3 bytes a pixel).
int degrade_whole(sr_ctx* ctx, srpng::Image& hr, int factor, const srdegrade::Draw& d, srpng::Image& lr) {
    const int h = hr.h / factor * factor, w = hr.w / factor * factor;
    if (h < factor || w < factor) return SR_E_INVALID;
    if (w != hr.w)
        for (int y = 1; y < h; ++y) memmove(&hr.rgba[(size_t)y * w * 4], &hr.rgba[(size_t)y * hr.w * 4], (size_t)w * 4);
    hr.h = h; hr.w = w;
    hr.rgba.resize((size_t)h * w * 4);
    lr.h = h / factor; lr.w = w / factor;
    lr.rgba.resize((size_t)lr.h * lr.w * 3);
    const sr_degrade g{d.sigma, d.noise, d.quality, d.seed};
    return sr_degrade_rgba8(ctx, hr.rgba.data(), 4, h, w, factor, 0, 0, h, w, 0, &g, lr.rgba.data());
}

// rusty_sr validate: the validation pass of the reference's `train` (main.rs:220-247) on its own.  Files are decoded on up to 16 host
// threads (OMP_NUM_THREADS if set) ahead of the GPU, which scores them in path order; with --devices image i goes to context i mod n.
// The sums are taken in image order, so the printed value does not depend on the number of devices.
int run_validate(int argc, char** argv) {
    std::string parameters, custom, precision = "f32", folder, lr_folder;
    bool has_p = false, has_c = false, linear = false, recurse = false, timing = false, has_folder = false, has_lr = false;
    bool metrics = false, has_shave = false, has_deg = false, has_seed = false;
    srdegrade::Spec deg_spec;
    uint64_t seed = 0;
    long val_max = -1;
    int shave = -1;         // --metrics: -1 = the factor
    unsigned ensemble = 0;  // 0: the plain validation pass
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
        else if (a == "--lr_folder") { lr_folder = value("--lr_folder <DIR>"); has_lr = true; }
        else if (a == "--ensemble") {
            const std::string v = value("--ensemble <N>");
            if (!(ensemble = ensemble_mask(v))) validate_usage_error("'" + v + "' isn't a valid value for '--ensemble <N>'\n\t[values: 2, 4, 8]");
        }
        else if (a == "--metrics") metrics = true;
        else if (a == "--shave" || a.rfind("--shave=", 0) == 0) {
            const std::string v = a == "--shave" ? value("--shave <N>") : a.substr(8);
            const auto r = std::from_chars(v.data(), v.data() + v.size(), shave);
            if (v.empty() || r.ec != std::errc() || r.ptr != v.data() + v.size() || shave < 0)
                validate_usage_error("'" + v + "' isn't a valid value for '--shave <N>'");
            has_shave = true;
        }
        else if (a == "--augment") validate_usage_error("The argument '--augment' can only be used with the 'train' subcommand");
        else if (a == "--loss") validate_usage_error("The argument '--loss' can only be used with the 'train' subcommand");
        else if (a == "--lr" || a == "--lr-schedule" || a == "--warmup" || a == "--clip" || a == "--ema" || a == "--resume") validate_usage_error("The argument '" + a + "' can only be used with the 'train' subcommand");
        else if (a == "--degrade") {
            const std::string v = value("--degrade <SPEC>");
            std::string perr;
            if (!srdegrade::parse(v, deg_spec, perr)) validate_usage_error("'" + v + "' isn't a valid value for '--degrade <SPEC>': " + perr);
            has_deg = true;
        }
        else if (a == "--seed") {
            const std::string v = value("--seed <N>");
            const auto r = std::from_chars(v.data(), v.data() + v.size(), seed);
            if (v.empty() || r.ec != std::errc() || r.ptr != v.data() + v.size()) validate_usage_error("'" + v + "' isn't a valid value for '--seed <N>'");
            has_seed = true;
        }
        else if (a == "--reuse") validate_usage_error("The argument '--reuse' can only be used with the 'video' subcommand");
        else if (a.size() > 1 && a[0] == '-') validate_usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else if (has_folder) validate_usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else { folder = a; has_folder = true; }
    }
    if (has_p && parameters != "imagenet" && parameters != "imagenetlinear" && parameters != "anime")
        validate_usage_error("'" + parameters + "' isn't a valid value for '--parameters <PARAMETERS>'\n\t[values: anime, imagenet, imagenetlinear]");
    if (has_c && has_p) validate_usage_error("The argument '--custom <PARAMETER_FILE>' cannot be used with '--parameters <PARAMETERS>'");
    if (!has_folder) validate_usage_error("The following required arguments were not provided:\n    <VALIDATION_FOLDER>");
    if (precision != "f32" && precision != "split_f16") validate_usage_error("'" + precision + "' isn't a valid value for '--precision <MODE>'");
    if (ensemble && devices.size() > 1)
        validate_usage_error("The argument '--ensemble <N>' cannot be used with more than one device: the ensemble has no multi-GPU form");
    if (has_shave && !metrics) validate_usage_error("The following required arguments were not provided:\n    --metrics");
    if (has_deg && has_lr) validate_usage_error("The argument '--degrade <SPEC>' cannot be used with '--lr_folder <DIR>': the LR images are made from the HR images");
    if (has_seed && !has_deg) validate_usage_error("The following required arguments were not provided:\n    --degrade <SPEC>");
    if (devices.empty()) devices.push_back(0);

    // ---- the files: decodable extensions, sorted by path bytes, the first N with -m
    std::vector<std::string> files;
    {
        std::error_code ec;
        if (!std::filesystem::is_directory(folder, ec)) validate_usage_error("'" + folder + "' is not a folder");
        std::string err;
        if (!list_images(folder, recurse, files, err)) die("could not read the validation folder (" + err + ")");
        if (val_max > 0 && (size_t)val_max < files.size()) files.resize((size_t)val_max);
        if (files.empty()) validate_usage_error("no image files in '" + folder + "'" + (recurse ? "" : " (-r recurses into subfolders)"));
        if (has_lr && !std::filesystem::is_directory(lr_folder, ec)) validate_usage_error("'" + lr_folder + "' is not a folder");
    }
    std::vector<std::string> lr_files;
    if (has_lr) lr_files = pair_files(folder, files, lr_folder, recurse);

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

    // ---- decoding ahead of the GPU, in path order
    const size_t nfile = files.size();
    DecoderPool decoders(files, nfile, devices.size());
    for (size_t i = 0; i < nfile; ++i) decoders.push(i);
    DecoderPool lr_decoders(lr_files, std::max<size_t>(1, lr_files.size()), devices.size());
    for (size_t i = 0; i < lr_files.size(); ++i) lr_decoders.push(i);
    std::mutex mu;

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
    std::vector<sr_metrics> scores(metrics ? nfile : 0);
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
                    std::string derr;
                    if (!decoders.take(i, img, derr)) {
                        std::lock_guard<std::mutex> lk(mu);
                        if (!derr.empty() && fail_code == 0) { failure = "Error opening validation image file " + files[i] + " (" + derr + ")"; fail_code = 1; }
                        decoders.stop();
                        lr_decoders.stop();
                        return;
                    }
                    srpng::Image lr;
                    if (has_lr && !lr_decoders.take(i, lr, derr)) {
                        std::lock_guard<std::mutex> lk(mu);
                        if (!derr.empty() && fail_code == 0) { failure = "Error opening validation image file " + lr_files[i] + " (" + derr + ")"; fail_code = 1; }
                        decoders.stop();
                        lr_decoders.stop();
                        return;
                    }
                    if (has_lr) {
                        std::lock_guard<std::mutex> lk(mu);  // (a mismatch ends the run from here: one thread at a time)
                        check_pair_sizes(files[i], img, lr_files[i], lr, factor);
                    }
                    // --degrade: the HR image cropped to a multiple of f and its LR partner made from it, whole, with draw i; then a pair
                    int r = has_deg ? degrade_whole(ctxs[k], img, factor, srdegrade::draw(deg_spec, seed, i), lr) : SR_OK;
                    const bool pair = has_lr || has_deg;
                    const int lr_ch = has_deg ? 3 : 4;
                    if (r != SR_OK) {
                    } else if (metrics)  // (members 0: the plain pass)
                        r = pair ? sr_pair_validation_metrics_rgba8(ctxs[k], lr.rgba.data(), lr_ch, img.rgba.data(), 4, lr.h, lr.w, linear ? 1 : 0,
                                                                    ensemble, shave, &err[i], &cnt[i], &scores[i])
                                 : sr_pool_validation_metrics_rgba8(ctxs[k], img.rgba.data(), 4, img.h, img.w, linear ? 1 : 0, ensemble, shave,
                                                                    &err[i], &cnt[i], &scores[i]);
                    else if (ensemble)
                        r = pair ? sr_pair_validation_error_ensemble_rgba8(ctxs[k], lr.rgba.data(), lr_ch, img.rgba.data(), 4, lr.h, lr.w,
                                                                           linear ? 1 : 0, ensemble, &err[i], &cnt[i])
                                 : sr_pool_validation_error_ensemble_rgba8(ctxs[k], img.rgba.data(), 4, img.h, img.w, linear ? 1 : 0, ensemble,
                                                                           &err[i], &cnt[i]);
                    else
                        r = pair ? sr_pair_validation_error_rgba8(ctxs[k], lr.rgba.data(), lr_ch, img.rgba.data(), 4, lr.h, lr.w, linear ? 1 : 0,
                                                                  &err[i], &cnt[i])
                                 : sr_validation_error_rgba8(ctxs[k], img.rgba.data(), 4, img.h, img.w, linear ? 1 : 0, &err[i], &cnt[i]);
                    if (r == SR_OK && timing) { double tot = 0; sr_last_timing(ctxs[k], &tot, nullptr, nullptr, nullptr); gpu_ms[i] = tot; }
                    if (r != SR_OK) {
                        std::lock_guard<std::mutex> lk(mu);
                        if (fail_code == 0) {
                            failure = files[i] + ": " + sr_strerror(r) + (r == SR_E_INVALID ? " (smaller than one pooling block?)" : "");
                            fail_code = 1;
                        }
                        decoders.stop();
                        lr_decoders.stop();
                        return;
                    }
                }
            });
    }
    for (auto& t : scorers) t.join();
    decoders.stop();
    lr_decoders.stop();
    for (sr_ctx* c : ctxs) sr_destroy(c);
    if (fail_code) die(failure, fail_code);
    double err_sum = 0, n_sum = 0, ms_sum = 0;
    for (size_t i = 0; i < nfile; ++i) { err_sum += err[i]; n_sum += (double)cnt[i]; ms_sum += gpu_ms[i]; }
    const float psnr = err_sum == 0.0 ? INFINITY : (float)(-10.0 * std::log10(err_sum / n_sum));
    printf("Validation PSNR:\t%s\n", rust_f32(psnr).c_str());  // main.rs:246
    if (metrics) {
        // per-image means, in image order; an image whose shaved region is empty (or holds no 11 x 11 window) is left out and named
        double y_sum = 0, s_sum = 0;
        size_t y_n = 0, s_n = 0;
        for (size_t i = 0; i < nfile; ++i) {
            const sr_metrics& m = scores[i];
            if (m.y_count) { y_sum += m.y_sq_err ? 10.0 * std::log10(65025.0 * (double)m.y_count / (double)m.y_sq_err) : INFINITY; ++y_n; }
            else fprintf(stderr, "%s: nothing left after the shave, left out of Y-PSNR\n", files[i].c_str());
            if (m.ssim_count) { s_sum += m.ssim_sum / (double)m.ssim_count; ++s_n; }
            else fprintf(stderr, "%s: too small for an 11x11 window after the shave, left out of SSIM\n", files[i].c_str());
        }
        printf("Y-PSNR:\t%s\n", rust_f32(y_n ? (float)(y_sum / (double)y_n) : NAN).c_str());
        printf("SSIM:\t%s\n", rust_f32(s_n ? (float)(s_sum / (double)s_n) : NAN).c_str());
    }
    if (timing) {
        const double s = std::chrono::duration<double>(clk::now() - t0).count();
        fprintf(stderr, "[timing] %zu images in %.3f s: %.2f images/s; GPU %.3f ms per image (whole validation call)\n", nfile, s, nfile / s,
                ms_sum / nfile);
    }
    return 0;
}


const char* kTrainUsage =
    "rusty_sr train\nTrains a new set of neural network parameters on the GPU (the reference's `train`): random 192x192 crops of the\n"
    "training images, batch 4, Adam; the parameter file is written after the first step and every 100 steps\n\n"
    "USAGE:\n    rusty_sr train [FLAGS] [OPTIONS] <PARAMETER_FILE> <TRAINING_FOLDER>\n\n"
    "FLAGS:\n    -l, --linearLoss    Apply MSE loss to a linearised RGB output rather than sRGB values\n"
    "    -r, --recurse       Recurse into subfolders of training and validation folders looking for files\n"
    "    -h, --help          Prints help information\n"
    "        --timing        Print steps/s, the share of resident draws and the decode time on stderr\n"
    "        --augment       Cut each crop under a random one of the 8 flips and rotations (the transforms of --ensemble 8)\n\n"
    "OPTIONS:\n    -s, --start <START_PARAMETERS>    Start training from known parameters loaded from this .rsr file; its size\n"
    "                                      selects the factor (2, 3 or 4) [default: random parameters at factor 3]\n"
    "    -v, --val_folder <VAL_FOLDER>     Images from this folder (or sub-folders with -r) are used to report the validation\n"
    "                                      PSNR after the first step and every 100 steps\n"
    "    -m, --val_max <N>                 Set upper limit on number of images used for each validation pass\n"
    "    -f, --factor <2|3|4>              The up-scaling factor when there is no -s [default: 3]\n"
    "        --lr_folder <DIR>             Train on LR / HR pairs: TRAINING_FOLDER holds the HR images, DIR their LR partners (the\n"
    "                                      same relative path, extension ignored, exactly 1/f the size); crops are 192/f LR pixels\n"
    "        --val_lr_folder <DIR>         The LR partners of the validation images: the validation PSNR is then the paired score\n"
    "        --device <N>                  HIP device index [default: 0]\n"
    "        --seed <N>                    Seed of the initial parameters, the shuffles and the crops [default: random]\n"
    "        --degrade <SPEC>              Train for real-world degradations: the network's input is each HR crop blurred, pooled,\n"
    "                                      noised and JPEG-compressed on the GPU, every draw with its own values from the ranges of\n"
    "                                      SPEC = blur=A[:B],noise=A[:B],jpeg=A[:B] (sigma 0..4 HR pixels, noise 0..64 levels, quality\n"
    "                                      1..100; a key left out is off).  With -v the validation images are degraded the same way\n"
    "        --loss <LOSS>                 The training objective: mse (the reference's sum of squares), l1, or charbonnier[:EPS]\n"
    "                                      (sqrt(e^2 + EPS^2) - EPS, 0 < EPS <= 1, EPS 0.001 without one); with -l it is taken of the\n"
    "                                      linearised values.  The validation lines stay PSNR [default: mse]\n"
    "        --steps <N>                   Stop after N steps [default: 2500000, the reference's 10 000 000 evaluations]\n"
    "        --lr <LR>                     The base learning rate [default: 0.002, the reference's]\n"
    "        --lr-schedule <SCHEDULE>      constant, step:EVERY:GAMMA (LR x GAMMA every EVERY steps) or cosine:TOTAL[:MIN] (half a\n"
    "                                      cosine from LR to MIN over TOTAL steps, MIN afterwards) [default: constant]\n"
    "        --warmup <N>                  Scale the rate by min(1, step / N) [default: 0, none]\n"
    "        --clip <NORM>                 Scale a gradient whose L2 norm exceeds NORM down to it; a step whose gradient is not\n"
    "                                      finite is skipped [default: 0, off]\n"
    "        --ema <DECAY>                 Keep an average of the parameters, e <- DECAY e + (1 - DECAY) p after every step, written to\n"
    "                                      <PARAMETER_FILE stem>.ema.rsr and scored on a second validation line [default: 0, off]\n"
    "        --resume                      Continue the run that wrote PARAMETER_FILE and PARAMETER_FILE.state, with the same options,\n"
    "                                      up to --steps in all: the same bits as the run that was never interrupted\n"
    "        --store <BYTES>               Device memory for resident training images; 0 decodes every draw again\n"
    "                                      [default: the device's free memory less max(8 GiB, 1/8 of it)]\n\n"
    "ARGS:\n    <PARAMETER_FILE>     Learned network parameters will be (over)written to this parameter file (.rsr)\n"
    "    <TRAINING_FOLDER>    Images from this folder (or sub-folders with -r) are used for training\n";

[[noreturn]] void train_usage_error(const std::string& msg) {
    fprintf(stderr, "error: %s\n\nUSAGE:\n    rusty_sr train [FLAGS] [OPTIONS] <PARAMETER_FILE> <TRAINING_FOLDER>\n\nFor more information try --help\n",
            msg.c_str());
    exit(2);
}

// SplitMix64: the shuffles and crop origins of `train` (the initial parameters use the library's own, sr_init_params), one stream
// seeded with seed ^ 0x5eed5eed5eed5eed.  --augment draws the members from a SECOND stream, seeded with seed ^ 0x6175676d656e7421
// ("augment!"): one value per draw, in draw order, member = next() >> 61 (its top three bits, uniform over 0..7).  The first stream is
// the same with and without the flag, so a seed's shuffles and origins are too; without the flag the second stream is never drawn from.
struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return next() % n; }  // (the bias of the modulo is below 2^-40 for any image size)
};

bool parse_count(const std::string& v, long& n) {
    const auto r = std::from_chars(v.data(), v.data() + v.size(), n);
    return !v.empty() && r.ec == std::errc() && r.ptr == v.data() + v.size();
}

// A plain decimal, [+]digits[.digits][e[+-]digits] of at most 64 characters, as a double
bool parse_plain_decimal(const std::string& t, double& out) {
    size_t i = 0, digits = 0;
    auto run = [&] { size_t n = 0; while (i < t.size() && isdigit((unsigned char)t[i])) { ++i; ++n; } return n; };
    if (i < t.size() && t[i] == '+') ++i;
    digits = run();
    if (i < t.size() && t[i] == '.') { ++i; digits += run(); }
    bool ok = digits > 0;
    if (ok && i < t.size() && (t[i] == 'e' || t[i] == 'E')) {
        ++i;
        if (i < t.size() && (t[i] == '+' || t[i] == '-')) ++i;
        ok = run() > 0;
    }
    if (!ok || i != t.size() || t.size() > 64) return false;
    out = strtod(t.c_str(), nullptr);
    return true;
}

// --loss mse|l1|charbonnier[:EPS] -> the arguments of sr_set_loss.  EPS: a plain decimal ([+]digits[.digits][e[+-]digits], as
// parse_loss_spec of the Python package takes it) that is, as an f32, above 0 and at most 1; 1e-3 where there is none.
bool parse_loss(const std::string& v, int& kind, float& eps, std::string& err) {
    const size_t colon = v.find(':');
    const std::string name = v.substr(0, colon);
    kind = name == "mse" ? SR_LOSS_MSE : name == "l1" ? SR_LOSS_L1 : name == "charbonnier" ? SR_LOSS_CHARBONNIER : -1;
    eps = 1e-3f;
    if (kind < 0) { err = "unknown kind '" + name + "'"; return false; }
    if (colon == std::string::npos) return true;
    if (kind != SR_LOSS_CHARBONNIER) { err = "'" + name + "' takes no EPS"; return false; }
    const std::string t = v.substr(colon + 1);
    double d = 0;
    if (!parse_plain_decimal(t, d)) { err = "malformed EPS '" + t.substr(0, 64) + "'"; return false; }
    const float e = (float)d;
    if (!(e > 0.0f && e <= 1.0f)) { err = "EPS '" + t + "' outside 0 < EPS <= 1"; return false; }
    eps = e;
    return true;
}

// --lr-schedule constant|step:EVERY:GAMMA|cosine:TOTAL[:MIN] -> the kind's fields of an sr_lr_schedule whose base and warmup are set
// (parse_lr_schedule of the Python package takes the same texts); sr_lr_at is the judge of the ranges.
bool parse_schedule(const std::string& v, sr_lr_schedule& s, std::string& err) {
    std::vector<std::string> parts;
    for (size_t a = 0;;) {
        const size_t b = v.find(':', a);
        parts.push_back(v.substr(a, b == std::string::npos ? b : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
    auto whole = [](const std::string& t, long long& n) {
        long tmp = 0;
        if (t.size() > 18 || !parse_count(t[0] == '+' ? t.substr(1) : t, tmp) || tmp < 1) return false;
        n = tmp;
        return true;
    };
    double d = 0;
    if (parts.size() == 1 && parts[0] == "constant") s.kind = SR_LR_CONSTANT;
    else if (parts[0] == "step" && parts.size() == 3) {
        s.kind = SR_LR_STEP;
        if (parts[1].empty() || !whole(parts[1], s.every)) { err = "EVERY must be a whole number >= 1"; return false; }
        if (!parse_plain_decimal(parts[2], d) || !(d > 0.0 && d <= 1.0)) { err = "GAMMA must be a number with 0 < GAMMA <= 1"; return false; }
        s.gamma = d;
    } else if (parts[0] == "cosine" && (parts.size() == 2 || parts.size() == 3)) {
        s.kind = SR_LR_COSINE;
        if (parts[1].empty() || !whole(parts[1], s.total)) { err = "TOTAL must be a whole number >= 1"; return false; }
        s.min_lr = 0.0f;
        if (parts.size() == 3) {
            if (!parse_plain_decimal(parts[2], d) || !((float)d >= 0.0f && (float)d <= s.base)) { err = "MIN must be a number with 0 <= MIN <= the base rate"; return false; }
            s.min_lr = (float)d;
        }
    } else {
        err = "expected constant, step:EVERY:GAMMA or cosine:TOTAL[:MIN]";
        return false;
    }
    float probe = 0;
    if (sr_lr_at(&s, 1, &probe) != SR_OK) { err = "a field is out of range"; return false; }
    return true;
}

// OUT.rsr -> OUT.ema.rsr (a name without the extension: OUT.ema.rsr too)
std::string ema_file_name(const std::string& param_file) {
    const std::string ext = ".rsr";
    const bool has = param_file.size() > ext.size() && param_file.compare(param_file.size() - ext.size(), ext.size(), ext) == 0;
    return (has ? param_file.substr(0, param_file.size() - ext.size()) : param_file) + ".ema.rsr";
}

// A parameter file, through a temporary file renamed into place: a run ended while it writes leaves the earlier file whole.  *hash: the
// checksum of the file's bytes, which the state file written beside it records (train_state.hpp).
bool write_rsr(const std::string& path, const std::vector<float>& p, uint64_t* hash = nullptr) {
    size_t len = 0;
    if (sr_rsr_encode(p.data(), p.size(), nullptr, 0, &len) != SR_OK) return false;
    std::vector<uint8_t> blob(len);
    if (sr_rsr_encode(p.data(), p.size(), blob.data(), blob.size(), &len) != SR_OK) return false;
    if (hash) *hash = srstate::checksum(blob.data(), len);
    return srstate::write_bytes(path, blob.data(), len);
}

// RGB copy of a decoded RGBA image (the store keeps 3 bytes a pixel)
std::vector<uint8_t> to_rgb(const srpng::Image& img) {
    std::vector<uint8_t> rgb((size_t)img.w * img.h * 3);
    for (size_t i = 0, n = (size_t)img.w * img.h; i < n; ++i) memcpy(&rgb[3 * i], &img.rgba[4 * i], 3);
    return rgb;
}

// rusty_sr train: the reference's `train` (main.rs:181-257).  sr_net(f, Some((1e-6, linear_loss))), Adam (lr 2e-3, beta1 0.95, beta2
// 0.995, eps 1e-7), batches of 4 random 192 x 192 crops, each draw one crop of the next image of a per-epoch shuffle of the training files.
// Every training image is decoded once, up front, and kept in the device's image store while it has room; the others are decoded again
// each time they are drawn (ahead of the GPU, on the decoder pool).  After step 1 and every 100th step the parameter file is written and,
// with -v, the PSNR of the next min(#files, N) validation images (sorted, wrapping round) at the current parameters is printed.
int run_train(int argc, char** argv) {
    std::string start, val_folder, lr_folder, val_lr_folder;
    std::vector<std::string> pos;
    bool has_s = false, has_v = false, linear = false, recurse = false, timing = false, has_lr = false, has_vlr = false, has_f = false;
    bool augment = false, has_deg = false;
    srdegrade::Spec deg_spec;
    int loss_kind = SR_LOSS_MSE;
    float loss_eps = 1e-3f;
    long factor_arg = SR_FACTOR;
    long val_max = -1, steps = 2500000, device = 0, store = -1;
    uint64_t seed = 0;
    bool has_seed = false;
    bool resume = false;
    std::string schedule_arg = "constant", degrade_arg;
    float lr_base = 2e-3f, clip = 0.0f, ema = 0.0f;
    long warmup = 0;
    for (int k = 2; k < argc; ++k) {
        const std::string a = argv[k];
        auto value = [&](const char* name) -> std::string {
            if (k + 1 >= argc) train_usage_error(std::string("The argument '") + name + "' requires a value but none was supplied");
            return argv[++k];
        };
        // --lr, --clip, --ema are f32 in the library: a nonzero value that rounds to 0 there would quietly mean "off", so it is refused
        auto vanishes = [](double d) { return d != 0.0 && (float)d == 0.0f; };
        if (a == "-h" || a == "--help") { fputs(kTrainUsage, stdout); return 0; }
        else if (a == "-l" || a == "--linearLoss") linear = true;
        else if (a == "-r" || a == "--recurse") recurse = true;
        else if (a == "--timing") timing = true;
        else if (a == "--augment") augment = true;
        else if (a == "-s" || a == "--start") { start = value("--start <START_PARAMETERS>"); has_s = true; }
        else if (a == "-v" || a == "--val_folder") { val_folder = value("--val_folder <VAL_FOLDER>"); has_v = true; }
        else if (a == "-m" || a == "--val_max") {
            const std::string v = value("--val_max <N>");
            if (!parse_count(v, val_max) || val_max <= 0) train_usage_error("-val_max N must be a positive integer");  // main.rs:225
        }
        else if (a == "--lr_folder") { lr_folder = value("--lr_folder <DIR>"); has_lr = true; }
        else if (a == "--val_lr_folder") { val_lr_folder = value("--val_lr_folder <DIR>"); has_vlr = true; }
        else if (a == "-f" || a == "--factor") {
            const std::string v = value("--factor <2|3|4>");
            if (!parse_count(v, factor_arg) || factor_arg < 2 || factor_arg > 4)
                train_usage_error("'" + v + "' isn't a valid value for '--factor <2|3|4>'\n\t[values: 2, 3, 4]");
            has_f = true;
        }
        else if (a == "--device") {
            const std::string v = value("--device <N>");
            if (!parse_count(v, device) || device < 0) train_usage_error("'" + v + "' isn't a valid value for '--device <N>'");
        }
        else if (a == "--steps") {
            const std::string v = value("--steps <N>");
            if (!parse_count(v, steps) || steps <= 0) train_usage_error("'" + v + "' isn't a valid value for '--steps <N>'");
        }
        else if (a == "--store") {
            const std::string v = value("--store <BYTES>");
            if (!parse_count(v, store) || store < 0) train_usage_error("'" + v + "' isn't a valid value for '--store <BYTES>'");
        }
        else if (a == "--seed") {
            const std::string v = value("--seed <N>");
            const auto r = std::from_chars(v.data(), v.data() + v.size(), seed);
            if (v.empty() || r.ec != std::errc() || r.ptr != v.data() + v.size()) train_usage_error("'" + v + "' isn't a valid value for '--seed <N>'");
            has_seed = true;
        }
        else if (a == "--degrade") {
            const std::string v = value("--degrade <SPEC>");
            std::string perr;
            if (!srdegrade::parse(v, deg_spec, perr)) train_usage_error("'" + v + "' isn't a valid value for '--degrade <SPEC>': " + perr);
            has_deg = true;
            degrade_arg = v;
        }
        else if (a == "--loss") {
            const std::string v = value("--loss <LOSS>");
            std::string perr;
            if (!parse_loss(v, loss_kind, loss_eps, perr))
                train_usage_error("'" + v + "' isn't a valid value for '--loss <LOSS>': " + perr + "\n\t[values: mse, l1, charbonnier[:EPS] with 0 < EPS <= 1]");
        }
        else if (a == "--lr") {
            const std::string v = value("--lr <LR>");
            double d = 0;
            if (!parse_plain_decimal(v, d) || !std::isfinite((float)d) || vanishes(d)) train_usage_error("'" + v + "' isn't a valid value for '--lr <LR>': a finite number >= 0 (0 itself, or one that f32 can hold)");
            lr_base = (float)d;
        }
        else if (a == "--lr-schedule") schedule_arg = value("--lr-schedule <SCHEDULE>");
        else if (a == "--warmup") {
            const std::string v = value("--warmup <N>");
            if (!parse_count(v, warmup) || warmup < 0) train_usage_error("'" + v + "' isn't a valid value for '--warmup <N>': a whole number of steps >= 0");
        }
        else if (a == "--clip") {
            const std::string v = value("--clip <NORM>");
            double d = 0;
            if (!parse_plain_decimal(v, d) || !std::isfinite((float)d) || vanishes(d)) train_usage_error("'" + v + "' isn't a valid value for '--clip <NORM>': 0 (off) or a finite number above 0 (one that f32 can hold: a value that rounds to 0 would turn clipping off)");
            clip = (float)d;
        }
        else if (a == "--ema") {
            const std::string v = value("--ema <DECAY>");
            double d = 0;
            if (!parse_plain_decimal(v, d) || !((float)d >= 0.0f && (float)d < 1.0f) || vanishes(d)) train_usage_error("'" + v + "' isn't a valid value for '--ema <DECAY>': 0 (off) or a number strictly between 0 and 1");
            ema = (float)d;
        }
        else if (a == "--resume") resume = true;
        else if (a == "--metrics" || a == "--shave" || a.rfind("--shave=", 0) == 0)
            train_usage_error("The argument '" + a.substr(0, a.find('=')) + "' can only be used with the 'validate' subcommand");
        else if (a == "--reuse") train_usage_error("The argument '--reuse' can only be used with the 'video' subcommand");
        else if (a.size() > 1 && a[0] == '-') train_usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else if (pos.size() == 2) train_usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else pos.push_back(a);
    }
    if (val_max > 0 && !has_v)  // clap: -m requires -v (main.rs:104)
        train_usage_error("The following required arguments were not provided:\n    --val_folder <VAL_FOLDER>");
    if (has_vlr && !has_v)
        train_usage_error("The following required arguments were not provided:\n    --val_folder <VAL_FOLDER>");
    if (has_deg && has_lr)
        train_usage_error("The argument '--degrade <SPEC>' cannot be used with '--lr_folder <DIR>': the LR crops are made from the HR crops");
    if (has_deg && has_vlr)
        train_usage_error("The argument '--degrade <SPEC>' cannot be used with '--val_lr_folder <DIR>': the validation images are degraded the same way");
    if (pos.size() < 2) train_usage_error("The following required arguments were not provided:\n    <PARAMETER_FILE>\n    <TRAINING_FOLDER>");
    sr_lr_schedule sched{};
    sched.kind = SR_LR_CONSTANT; sched.base = lr_base; sched.warmup = warmup;
    {
        std::string perr;
        if (!parse_schedule(schedule_arg, sched, perr))
            train_usage_error("'" + schedule_arg + "' isn't a valid value for '--lr-schedule <SCHEDULE>': " + perr);
    }
    const bool scheduled = sched.kind != SR_LR_CONSTANT || warmup > 0;
    if (resume && has_s) train_usage_error("The argument '--resume' cannot be used with '--start <START_PARAMETERS>': it continues from <PARAMETER_FILE>");
    if (degrade_arg.size() >= srstate::kDegradeText) train_usage_error("the '--degrade <SPEC>' text is too long for the state file");
    // --resume: the state file, before anything else is read (its seed is the run's when none is given)
    const std::string state_file = pos[0] + ".state";
    srstate::State resumed;
    if (resume) {
        std::string perr;
        std::error_code ec;
        if (!std::filesystem::is_regular_file(pos[0], ec)) train_usage_error("--resume: could not open the parameter file " + pos[0]);
        if (!std::filesystem::is_regular_file(state_file, ec)) train_usage_error("--resume: could not open the state file " + state_file);
        if (!srstate::read_file(state_file, resumed, perr)) train_usage_error("--resume: " + state_file + ": " + perr);
        if (!has_seed) { seed = resumed.set.seed; has_seed = true; }
        start = pos[0];
        has_s = true;
    }
    if (!has_seed) seed = ((uint64_t)std::random_device{}() << 32) ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
    const std::string param_file = pos[0], train_folder = pos[1];

    // ---- the folders, before the GPU is touched
    std::vector<std::string> files, vfiles;
    {
        std::error_code ec;
        std::string err;
        if (!std::filesystem::is_directory(train_folder, ec)) train_usage_error("'" + train_folder + "' is not a folder");
        if (!list_images(train_folder, recurse, files, err)) die("could not read the training folder (" + err + ")");
        if (files.empty()) train_usage_error("no image files in '" + train_folder + "'" + (recurse ? "" : " (-r recurses into subfolders)"));
        if (has_v) {
            if (!std::filesystem::is_directory(val_folder, ec)) train_usage_error("'" + val_folder + "' is not a folder");
            if (!list_images(val_folder, recurse, vfiles, err)) die("could not read the validation folder (" + err + ")");
            if (vfiles.empty()) train_usage_error("no image files in '" + val_folder + "'" + (recurse ? "" : " (-r recurses into subfolders)"));
        }
        if (has_lr && !std::filesystem::is_directory(lr_folder, ec)) train_usage_error("'" + lr_folder + "' is not a folder");
        if (has_vlr && !std::filesystem::is_directory(val_lr_folder, ec)) train_usage_error("'" + val_lr_folder + "' is not a folder");
    }
    std::vector<std::string> lr_files, vlr_files;
    if (has_lr) lr_files = pair_files(train_folder, files, lr_folder, recurse);
    if (has_vlr) vlr_files = pair_files(val_folder, vfiles, val_lr_folder, recurse);
    // ---- parameters: the start file (its length selects the factor) or g.init_params() at the factor of -f (3 without it)
    std::vector<float> params;
    int factor = (int)factor_arg;
    uint64_t start_hash = 0;  // --resume: of the parameter file's bytes, which the state file must name
    if (has_s) {
        FILE* f = fopen(start.c_str(), "rb");
        if (!f) die("Error opening start parameter file");  // main.rs:192
        std::vector<unsigned char> data;
        unsigned char tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + n);
        fclose(f);
        start_hash = srstate::checksum(data.data(), data.size());
        params = decode_rsr(data.data(), data.size());
        int file_factor = SR_FACTOR;
        for (int fc : {3, 2, 4})
            if (params.size() == (size_t)sr_num_params_factor(fc)) { file_factor = fc; break; }
        if (has_f && file_factor != factor && params.size() == (size_t)sr_num_params_factor(file_factor))
            train_usage_error("The argument '--factor " + std::to_string(factor) + "' cannot be used with start parameters of factor " +
                              std::to_string(file_factor));
        factor = file_factor;
    } else {
        params.resize((size_t)sr_num_params_factor(factor));
        if (sr_init_params(factor, seed, params.data(), params.size()) != SR_OK) die("could not initialise the parameters");
    }

    srstate::Settings settings;
    settings.factor = factor; settings.linear = linear; settings.augment = augment; settings.pairs = has_lr; settings.degrade = has_deg;
    settings.seed = seed; settings.n_files = files.size(); settings.loss_kind = loss_kind; settings.loss_eps = loss_eps; settings.lr = lr_base;
    settings.sched_kind = sched.kind; settings.warmup = warmup; settings.every = sched.kind == SR_LR_STEP ? sched.every : 0;
    settings.gamma = sched.kind == SR_LR_STEP ? sched.gamma : 0.0; settings.total = sched.kind == SR_LR_COSINE ? sched.total : 0;
    settings.min_lr = sched.kind == SR_LR_COSINE ? sched.min_lr : 0.0f; settings.clip = clip; settings.ema = ema; settings.degrade_spec = degrade_arg;
    if (resume) {  // still before the device is touched
        const std::string d = srstate::differing(resumed.set, settings);
        if (!d.empty()) train_usage_error("--resume: the option '" + d + "' differs from the run that wrote " + state_file);
        // the two files are written one after the other: a run ended between them, or a parameter file replaced since, leaves a pair that
        // would train on from moments, counts and generators of another step
        if (resumed.n_params != params.size() || resumed.params_hash != start_hash)
            train_usage_error("--resume: the parameter file " + param_file + " is not the one written with the state file " + state_file +
                              " (its checksum differs): the run was interrupted between the two, or the file was replaced");
        if (resumed.step >= steps)
            train_usage_error("--resume: '--steps " + std::to_string(steps) + "' is the total and must exceed the " + std::to_string(resumed.step) + " steps already taken");
    }

    // ---- the device: a context (its inference path scores the validation images) and the training session on it
    sr_ctx* ctx = nullptr;
    int rc = sr_create(&ctx, params.data(), params.size(), factor, (int)device);
    if (rc != SR_OK) die(sr_strerror(rc));  // SR_E_PARAM_COUNT carries the text of main.rs:162; SR_E_NO_DEVICE: no CPU fallback
    if ((rc = sr_set_loss(ctx, loss_kind, loss_eps)) != SR_OK) die(sr_strerror(rc));  // --loss: every step's objective; the validation lines stay PSNR
    sr_train* tr = nullptr;
    rc = sr_train_create(&tr, ctx, params.data(), params.size(), linear ? 1 : 0, 1e-6f, lr_base, 0.95f, 0.995f, 1e-7f,
                         store < 0 ? SR_TRAIN_STORE_AUTO : (size_t)store);
    if (rc != SR_OK) die(sr_strerror(rc));
    if (clip > 0.0f || ema > 0.0f) {  // (neither: the session stays the default one, launch for launch)
        if ((rc = sr_train_set_optim(tr, clip, ema)) != SR_OK) die(std::string("--clip / --ema: ") + sr_strerror(rc));
    }
    if (resume) {
        rc = sr_train_set_state(tr, resumed.m.data(), resumed.v.data(), ema > 0.0f ? resumed.e.data() : nullptr, resumed.m.size(), resumed.step,
                                resumed.skipped);
        if (rc != SR_OK) die(std::string("--resume: ") + sr_strerror(rc));
    }
    using clk = std::chrono::steady_clock;
    const clk::time_point t_load = clk::now();

    // ---- every training image decoded once: into the store while it has room; the rest are transient (their sizes are kept)
    const size_t nfile = files.size();
    struct TrainImage { int id = -1, h = 0, w = 0; bool ok = false; };  // (h, w: of the HR image)
    std::vector<TrainImage> timg(nfile);
    double decode_ms = 0;
    {
        DecoderPool pool(files, nfile), lr_pool(lr_files, std::max<size_t>(1, lr_files.size()));
        for (size_t i = 0; i < nfile; ++i) pool.push(i);
        for (size_t i = 0; i < lr_files.size(); ++i) lr_pool.push(i);
        for (size_t i = 0; i < nfile; ++i) {
            srpng::Image img, lr;
            std::string err;
            const bool ok = pool.take(i, img, err);
            if (!ok) fprintf(stderr, "warning: skipping training image %s (%s)\n", files[i].c_str(), err.c_str());
            if (has_lr && !lr_pool.take(i, lr, err)) die("Error opening training image file " + lr_files[i] + " (" + err + ")");
            if (!ok) continue;
            timg[i].h = img.h; timg[i].w = img.w; timg[i].ok = true;
            const std::vector<uint8_t> rgb = to_rgb(img);
            if (has_lr) {
                check_pair_sizes(files[i], img, lr_files[i], lr, factor);
                const std::vector<uint8_t> lr_rgb = to_rgb(lr);
                rc = sr_train_add_pair(tr, lr_rgb.data(), 3, rgb.data(), 3, lr.h, lr.w, &timg[i].id);
            } else {
                rc = sr_train_add_image(tr, rgb.data(), 3, img.h, img.w, &timg[i].id);
            }
            if (rc != SR_OK) die(std::string("could not store a training image: ") + sr_strerror(rc));
        }
    }
    decode_ms += std::chrono::duration<double, std::milli>(clk::now() - t_load).count();
    std::vector<size_t> usable;
    for (size_t i = 0; i < nfile; ++i) if (timg[i].ok) usable.push_back(i);
    if (usable.empty()) train_usage_error("no decodable image in '" + train_folder + "'");
    // ---- validation images: decoded once, kept on the host
    std::vector<srpng::Image> vimg, vlr;
    if (has_v) {
        DecoderPool pool(vfiles, vfiles.size()), lr_pool(vlr_files, std::max<size_t>(1, vlr_files.size()));
        for (size_t i = 0; i < vfiles.size(); ++i) pool.push(i);
        for (size_t i = 0; i < vlr_files.size(); ++i) lr_pool.push(i);
        vimg.resize(vfiles.size());
        vlr.resize(vlr_files.size());
        for (size_t i = 0; i < vfiles.size(); ++i) {
            std::string err;
            if (!pool.take(i, vimg[i], err)) die("Error opening validation image file " + vfiles[i] + " (" + err + ")");
            if (!has_vlr) continue;
            if (!lr_pool.take(i, vlr[i], err)) die("Error opening validation image file " + vlr_files[i] + " (" + err + ")");
            check_pair_sizes(vfiles[i], vimg[i], vlr_files[i], vlr[i], factor);
        }
    }
    const size_t val_n = has_v ? std::min(vimg.size(), val_max > 0 ? (size_t)val_max : vimg.size()) : 0;
    size_t val_next = resume && !vimg.empty() ? (size_t)(resumed.val_next % vimg.size()) : 0;

    // ---- the draws: a fresh shuffle of the usable files each epoch, one crop of each drawn image
    // (pairs: one crop of 192 / f LR pixels per draw, its origin in LR pixels, uniform over the positions inside the LR image)
    constexpr int kBatch = 4, kCropHr = 192;
    const int unit = has_lr ? factor : 1, kCrop = kCropHr / unit;
    Rng rng{seed ^ 0x5eed5eed5eed5eedull};
    Rng aug_rng{seed ^ 0x6175676d656e7421ull};  // --augment: the members, a stream of their own
    std::vector<size_t> perm;
    size_t perm_pos = 0;
    // The generators as they are BEFORE a draw: what the state file records for the first draw the GPU has not consumed, so that a resumed
    // run makes that draw again.  The epoch's shuffle is not stored: epoch_rng is the crop stream before it, and the shuffle is made anew.
    struct Snap { uint64_t rng, aug_rng, epoch_rng, perm_pos, deg_drawn; bool epoch_valid; };
    struct Draw { size_t file; int y0, x0; uint8_t member; sr_degrade deg; Snap snap; };
    uint64_t deg_drawn = 0;  // --degrade: the draws of its own stream (degrade_spec.hpp), one per crop, in draw order
    uint64_t epoch_rng = 0;
    bool epoch_valid = false;
    auto shuffle = [&]() {
        epoch_rng = rng.s;
        epoch_valid = true;
        perm = usable;
        for (size_t i = perm.size(); i > 1; --i) std::swap(perm[i - 1], perm[rng.below(i)]);
    };
    auto snap_now = [&]() -> Snap { return {rng.s, aug_rng.s, epoch_rng, (uint64_t)perm_pos, deg_drawn, epoch_valid}; };
    if (resume) {
        if (resumed.epoch_valid) {
            rng.s = resumed.epoch_rng;
            shuffle();
        }
        // The one refusal of --resume that needs the images decoded, so it comes after the device is up and ends with status 1: the state
        // file counts the files listed (n_files, checked above), and a file that decoded then and no longer does shortens the shuffle.
        if (resumed.perm_pos > perm.size()) die("--resume: the training folder does not hold the images of the run that wrote " + state_file);
        perm_pos = (size_t)resumed.perm_pos;
        rng.s = resumed.rng;
        aug_rng.s = resumed.aug_rng;
        deg_drawn = resumed.deg_drawn;
    }
    auto draw = [&]() -> Draw {
        const Snap before = snap_now();
        if (perm_pos == perm.size()) {
            shuffle();
            perm_pos = 0;
        }
        const size_t fi = perm[perm_pos++];
        const TrainImage& im = timg[fi];
        // the crop origin: uniform over the positions inside the image; 0 on an axis shorter than the crop (the rest is zero padding)
        const int h = im.h / unit, w = im.w / unit;
        const int y0 = h > kCrop ? (int)rng.below((uint64_t)(h - kCrop + 1)) : 0;
        const int x0 = w > kCrop ? (int)rng.below((uint64_t)(w - kCrop + 1)) : 0;
        // (the crop is square: the window of a member that swaps the axes has the same origins to choose from)
        sr_degrade deg{0.0f, 0.0f, 0, 0};
        if (has_deg) {
            const srdegrade::Draw g = srdegrade::draw(deg_spec, seed, deg_drawn++);
            deg = {g.sigma, g.noise, g.quality, g.seed};
        }
        return {fi, y0, x0, augment ? (uint8_t)(aug_rng.next() >> 61) : (uint8_t)0, deg, before};
    };
    // draws are made a window of steps ahead, so that transient images decode while the GPU works
    DecoderPool pool(files, 16 * kBatch), lr_pool(lr_files, 16 * kBatch);
    std::deque<std::pair<Draw, long>> ahead;  // (draw, decoder job or -1; a transient pair's LR file has the same job number in lr_pool)
    const long lookahead = 8 * kBatch;
    const long first_step = resume ? (long)resumed.step + 1 : 1;
    long drawn = (first_step - 1) * kBatch;
    auto fill = [&]() {
        while ((long)ahead.size() < lookahead && drawn < steps * kBatch) {
            const Draw d = draw();
            ++drawn;
            const long job = timg[d.file].id >= 0 ? -1 : (long)pool.push(d.file);
            if (job >= 0 && has_lr) lr_pool.push(d.file);
            ahead.emplace_back(d, job);
        }
    };

    // The PSNR line of parameters p over the next val_n validation images from the cursor on
    auto score = [&](const std::vector<float>& p, const char* label) {
        int r = sr_set_params(ctx, p.data(), p.size());
        if (r != SR_OK) die(sr_strerror(r));
        double err_sum = 0, n_sum = 0;
        for (size_t k = 0; k < val_n; ++k) {
            srpng::Image& im = vimg[val_next];
            val_next = (val_next + 1) % vimg.size();
            double e = 0;
            size_t ne = 0;
            if (has_deg) {  // the k-th image of this pass takes draw k: every pass restarts the stream, so successive PSNR lines compare
                srpng::Image lr;
                r = degrade_whole(ctx, im, factor, srdegrade::draw(deg_spec, seed, k), lr);
                if (r == SR_OK) r = sr_pair_validation_error_rgba8(ctx, lr.rgba.data(), 3, im.rgba.data(), 4, lr.h, lr.w, linear ? 1 : 0, &e, &ne);
            } else if (has_vlr) {
                const srpng::Image& lr = vlr[(val_next + vimg.size() - 1) % vimg.size()];
                r = sr_pair_validation_error_rgba8(ctx, lr.rgba.data(), 4, im.rgba.data(), 4, lr.h, lr.w, linear ? 1 : 0, &e, &ne);
            } else {
                r = sr_validation_error_rgba8(ctx, im.rgba.data(), 4, im.h, im.w, linear ? 1 : 0, &e, &ne);
            }
            if (r != SR_OK) die(std::string("validation: ") + sr_strerror(r) + (r == SR_E_INVALID ? " (an image smaller than one pooling block?)" : ""));
            err_sum += e;
            n_sum += (double)ne;
        }
        const float psnr = err_sum == 0.0 ? INFINITY : (float)(-10.0 * std::log10(err_sum / n_sum));
        printf("Validation PSNR%s:\t%s\n", label, rust_f32(psnr).c_str());  // main.rs:246
        fflush(stdout);
    };
    // The parameter file, with --ema the averaged one beside it, the state file (the generators at the first draw the GPU has not
    // consumed, the cursor after the pass), and then the validation lines (the averaged parameters are scored on the same images as the raw ones).
    const std::string ema_file = ema_file_name(param_file);
    auto checkpoint = [&](bool validate) {
        srstate::State st;
        st.set = settings;
        st.n_params = params.size();
        st.m.resize(params.size());
        st.v.resize(params.size());
        if (ema > 0.0f) st.e.resize(params.size());
        long long at = 0, skipped = 0;
        std::vector<float> p(params.size());
        int r = sr_train_params(tr, p.data(), p.size());
        if (r == SR_OK) r = sr_train_get_state(tr, st.m.data(), st.v.data(), ema > 0.0f ? st.e.data() : nullptr, st.m.size(), &at, &skipped);
        if (r != SR_OK) die(sr_strerror(r));
        const Snap sn = ahead.empty() ? snap_now() : ahead.front().first.snap;
        st.step = at; st.skipped = skipped;
        st.rng = sn.rng; st.aug_rng = sn.aug_rng; st.epoch_rng = sn.epoch_rng; st.perm_pos = sn.perm_pos; st.deg_drawn = sn.deg_drawn;
        st.epoch_valid = sn.epoch_valid;
        const bool scoring = validate && has_v;
        st.val_next = scoring ? (val_next + val_n) % vimg.size() : val_next;  // where the pass below leaves the cursor
        // The files one right after the other, each through a temporary file and a rename, and the validation pass only then: the time in
        // which a run that is ended leaves a parameter file without its state is that of two renames, and --resume tells such a pair by
        // the checksum.  (A parameter file that could not be written leaves the state file as it was: the earlier pair stays whole.)
        const bool wrote = write_rsr(param_file, p, &st.params_hash);
        if (!wrote) fprintf(stderr, "Could not make parameter file\n");
        if (ema > 0.0f && !write_rsr(ema_file, st.e)) fprintf(stderr, "Could not make parameter file\n");
        std::string werr;
        if (wrote && !srstate::write_file(state_file, st, werr)) fprintf(stderr, "Could not make state file (%s)\n", werr.c_str());
        if (scoring) {
            const size_t cursor = val_next;
            score(p, "");
            if (ema > 0.0f) {
                val_next = cursor;
                score(st.e, " (EMA)");
            }
        }
    };
    // the steps' statistics: --timing reports the share of clipped and of skipped steps, and the norms seen
    long clipped_steps = 0, skipped_steps = 0;
    std::vector<double> norms;
    std::vector<sr_train_stat> stat_buf(1000 + SR_TRAIN_RING);
    auto collect = [&]() {
        size_t n = 0;
        const int r = sr_train_sync_stats(tr, stat_buf.data(), stat_buf.size(), &n);
        if (r != SR_OK) die(sr_strerror(r));
        if (!(clip > 0.0f)) return;
        for (size_t i = 0; i < std::min(n, stat_buf.size()); ++i) {
            if (!std::isfinite(stat_buf[i].grad_norm)) { ++skipped_steps; continue; }
            if (stat_buf[i].scale < 1.0f) ++clipped_steps;
            if (timing) norms.push_back(stat_buf[i].grad_norm);
        }
    };

    printf("Beginning Training\n");
    fflush(stdout);
    const clk::time_point t0 = clk::now();
    long resident_draws = 0;
    double wait_ms = 0;
    std::vector<std::vector<uint8_t>> held(kBatch), held_lr(kBatch);  // transient pixels of the step being queued
    for (long step = first_step; step <= steps; ++step) {
        fill();
        sr_train_crop items[kBatch];
        sr_train_pair_crop pairs[kBatch];
        uint8_t members[kBatch];
        sr_degrade degs[kBatch];
        for (int i = 0; i < kBatch; ++i) {
            const auto [d, job] = ahead.front();
            ahead.pop_front();
            items[i].y0 = pairs[i].y0 = d.y0;
            items[i].x0 = pairs[i].x0 = d.x0;
            members[i] = d.member;
            degs[i] = d.deg;
            if (job < 0) {
                items[i].image = pairs[i].pair = timg[d.file].id;
                items[i].px = pairs[i].lr_px = pairs[i].hr_px = nullptr;
                items[i].in_channels = 3; items[i].h = timg[d.file].h; items[i].w = timg[d.file].w;
                pairs[i].lr_channels = pairs[i].hr_channels = 3; pairs[i].lh = timg[d.file].h / unit; pairs[i].lw = timg[d.file].w / unit;
                ++resident_draws;
                continue;
            }
            srpng::Image img, lr;
            std::string err;
            const clk::time_point tw = clk::now();
            if (!pool.take((size_t)job, img, err)) die("Error opening training image file " + files[d.file] + " (" + err + ")");
            if (has_lr && !lr_pool.take((size_t)job, lr, err)) die("Error opening training image file " + lr_files[d.file] + " (" + err + ")");
            wait_ms += std::chrono::duration<double, std::milli>(clk::now() - tw).count();
            if (has_lr) check_pair_sizes(files[d.file], img, lr_files[d.file], lr, factor);
            held[i] = std::move(img.rgba);
            held_lr[i] = std::move(lr.rgba);
            items[i].image = pairs[i].pair = -1;
            items[i].px = pairs[i].hr_px = held[i].data();
            items[i].in_channels = 4; items[i].h = img.h; items[i].w = img.w;
            pairs[i].lr_px = held_lr[i].data();
            pairs[i].lr_channels = pairs[i].hr_channels = 4; pairs[i].lh = lr.h; pairs[i].lw = lr.w;
        }
        if (scheduled) {  // (a constant rate without warm-up stays the one the session was created with)
            float lr = 0;
            if ((rc = sr_lr_at(&sched, step, &lr)) != SR_OK || (rc = sr_train_set_lr(tr, lr)) != SR_OK) die(std::string("--lr-schedule: ") + sr_strerror(rc));
        }
        if (has_deg) rc = sr_train_step_degrade(tr, items, augment ? members : nullptr, degs, kBatch, kCrop, kCrop);
        else if (augment) rc = has_lr ? sr_train_step_pairs_aug(tr, pairs, members, kBatch, kCrop, kCrop) : sr_train_step_aug(tr, items, members, kBatch, kCrop, kCrop);
        else rc = has_lr ? sr_train_step_pairs(tr, pairs, kBatch, kCrop, kCrop) : sr_train_step(tr, items, kBatch, kCrop, kCrop);
        if (rc != SR_OK) die(std::string("training step: ") + sr_strerror(rc));
        if (step % 1000 == 0) collect();  // keeps the session's list of finished steps short
        if (step == 1 || step % 100 == 0) checkpoint(true);
        else if (step == steps) checkpoint(false);  // --steps ended the run between two checkpoints: the file holds the last step
    }
    collect();
    const long steps_run = steps - first_step + 1;
    if (timing) {
        const double s = std::chrono::duration<double>(clk::now() - t0).count();
        fprintf(stderr, "[timing] %ld steps in %.3f s: %.1f steps/s (checkpoints and validation included); resident draws %.1f %%; "
                        "decode: %.1f ms up front (%zu images, %d resident), %.1f ms waited for transient images\n",
                steps_run, s, steps_run / s, 100.0 * resident_draws / ((double)steps_run * kBatch), decode_ms, nfile,
                (int)std::count_if(timg.begin(), timg.end(), [](const TrainImage& t) { return t.id >= 0; }), wait_ms);
        if (clip > 0.0f) {
            std::sort(norms.begin(), norms.end());
            fprintf(stderr, "[timing] clipped steps %.1f %%, skipped steps %.1f %%; gradient norm min %.9g, median %.9g, max %.9g\n",
                    100.0 * clipped_steps / (double)steps_run, 100.0 * skipped_steps / (double)steps_run, norms.empty() ? 0.0 : norms.front(),
                    norms.empty() ? 0.0 : norms[norms.size() / 2], norms.empty() ? 0.0 : norms.back());
        }
    }
    pool.stop();
    lr_pool.stop();
    sr_train_destroy(tr);
    sr_destroy(ctx);
    printf("Done\n");
    return 0;
}

// ---- rusty_sr video: a YUV4MPEG2 stream through the frame stream of the library (sr_video_*), stdin / stdout as "-" ----
[[noreturn]] void video_usage_error(const std::string& msg) {
    fprintf(stderr, "error: %s\n\nUSAGE:\n    rusty_sr video [OPTIONS] <INPUT|-> <OUTPUT|->\n\nFor more information try --help\n", msg.c_str());
    exit(2);
}

const char kVideoHelp[] =
    "USAGE:\n    rusty_sr video [OPTIONS] <INPUT|-> <OUTPUT|->\n\n"
    "Upscales a YUV4MPEG2 stream frame by frame: colour conversion and chroma resampling run on the GPU, the network's\n"
    "output is quantised once, straight to YCbCr, and the copies of successive frames overlap the kernels.  Frames are\n"
    "independent.  `-` is stdin / stdout:  ffmpeg -i in.mp4 -f yuv4mpegpipe - | rusty_sr video - - | ffmpeg -i - out.mp4\n"
    "Streams: 8-bit progressive C420jpeg, C420, C420mpeg2, C444; XCOLORRANGE=FULL selects full range.\n"
    "With --depth auto also the deep streams C420p<d>, C422p<d>, C444p<d> (d = 9, 10, 12, 14, 16; 16-bit little-endian\n"
    "samples), written out at the depth they came in:  ffmpeg -i in.mkv -pix_fmt yuv420p10le -strict -1 -f yuv4mpegpipe - |\n"
    "rusty_sr video --depth auto - - | ffmpeg -i - out.mkv\n\n"
    "OPTIONS:\n"
    "    -p, --parameters <PARAMETERS>    [values: anime, bilinear, imagenet, imagenetlinear]\n"
    "    -c, --custom <PARAMETER_FILE>\n"
    "        --precision <MODE>           [values: f32, split_f16]\n"
    "        --device <N>\n"
    "        --ensemble <N>               [values: 2, 4, 8]\n"
    "        --matrix <MATRIX>            [values: bt601, bt709]  default: bt709 from 1280 columns or above 576 rows, else bt601;\n"
    "                                     bt2020 (non-constant luminance) on a deep stream only, never chosen by default\n"
    "        --depth <BITS>               [values: 8, auto]  8 (default): 8-bit streams only; auto: the stream's own depth\n"
    "        --siting <SITING>            [values: center, left]  chroma siting of a deep 4:2:0 / 4:2:2 stream (default: left)\n"
    "        --slots <N>                  frames in flight [1..8], default 3\n"
    "        --reuse                      compute only the rows that changed since the last frame (letterbox bars, held\n"
    "                                     frames, screen recordings); the output is byte for byte the same\n"
    "        --size <WxH>                 write frames of exactly this size: the network's f32 output is resampled on the GPU\n"
    "                                     and quantised once, straight to YCbCr (each axis 1..16384)\n"
    "        --scale <S>                  the same, S times the INPUT size (--scale 2 with the x3 weights writes 2x frames)\n"
    "        --filter <FILTER>            with --size / --scale: the resampling filter [values: box, triangle, catrom,\n"
    "                                     lanczos3]  default: lanczos3\n"
    "        --resize-space <SPACE>       with --size / --scale: resample in linear light or on the sRGB values [values:\n"
    "                                     linear, srgb]  default: linear\n"
    "        --timing                     print frames and ms/frame to stderr\n";

int run_video(int argc, char** argv) {
    std::vector<std::string> pos;
    std::string parameters, custom, precision = "f32", matrix, depth_arg = "8", siting;
    bool has_p = false, has_c = false, timing = false, reuse = false;
    long device = 0, slots = 3;
    unsigned ensemble = 0;
    // --size / --scale: the frames are resampled to a size of the user's choosing (sr_video_create*_sized)
    bool has_size = false, has_scale = false, has_filter = false, has_space = false;
    std::string size_arg, scale_arg;
    int size_w = 0, size_h = 0, filter = SR_FILTER_LANCZOS3;
    double scale = 0;
    unsigned resize_flags = 0;
    for (int k = 2; k < argc; ++k) {
        const std::string a = argv[k];
        auto value = [&](const char* name) -> std::string {
            if (k + 1 >= argc) video_usage_error(std::string("The argument '") + name + "' requires a value but none was supplied");
            return argv[++k];
        };
        if (a == "-h" || a == "--help") { fputs(kVideoHelp, stderr); return 0; }
        else if (a == "-p" || a == "--parameters") { parameters = value("--parameters <PARAMETERS>"); has_p = true; }
        else if (a == "-c" || a == "--custom") { custom = value("--custom <PARAMETER_FILE>"); has_c = true; }
        else if (a == "--precision") precision = value("--precision <MODE>");
        else if (a == "--timing") timing = true;
        else if (a == "--reuse") reuse = true;
        else if (a == "--device") {
            const std::string v = value("--device <N>");
            if (!parse_count(v, device) || device < 0) video_usage_error("'" + v + "' isn't a valid value for '--device <N>'");
        }
        else if (a == "--slots") {
            const std::string v = value("--slots <N>");
            if (!parse_count(v, slots) || slots < 1 || slots > 8) video_usage_error("'" + v + "' isn't a valid value for '--slots <N>'\n\t[values: 1..8]");
        }
        else if (a == "--ensemble") {
            const std::string v = value("--ensemble <N>");
            if (!(ensemble = ensemble_mask(v))) video_usage_error("'" + v + "' isn't a valid value for '--ensemble <N>'\n\t[values: 2, 4, 8]");
        }
        else if (a == "--matrix") {
            matrix = value("--matrix <MATRIX>");
            if (matrix != "bt601" && matrix != "bt709" && matrix != "bt2020") video_usage_error("'" + matrix + "' isn't a valid value for '--matrix <MATRIX>'\n\t[values: bt601, bt709]");
        }
        else if (a == "--depth" || a.rfind("--depth=", 0) == 0) {
            depth_arg = a == "--depth" ? value("--depth <BITS>") : a.substr(8);
            if (depth_arg != "8" && depth_arg != "auto") video_usage_error("'" + depth_arg + "' isn't a valid value for '--depth <BITS>'\n\t[values: 8, auto]");
        }
        else if (a == "--siting") {
            siting = value("--siting <SITING>");
            if (siting != "center" && siting != "left") video_usage_error("'" + siting + "' isn't a valid value for '--siting <SITING>'\n\t[values: center, left]");
        }
        else if (a == "--size" || a.rfind("--size=", 0) == 0) {
            size_arg = a == "--size" ? value("--size <WxH>") : a.substr(7);
            if (!parse_size(size_arg, size_w, size_h))
                video_usage_error("'" + size_arg + "' isn't a valid value for '--size <WxH>'\n\t[two whole numbers, 1..16384 each: 3840x2160]");
            has_size = true;
        }
        else if (a == "--scale" || a.rfind("--scale=", 0) == 0) {
            scale_arg = a == "--scale" ? value("--scale <S>") : a.substr(8);
            if (!parse_scale(scale_arg, scale)) video_usage_error("'" + scale_arg + "' isn't a valid value for '--scale <S>'\n\t[a positive decimal: 1.5]");
            has_scale = true;
        }
        else if (a == "--filter" || a.rfind("--filter=", 0) == 0) {
            const std::string v = a == "--filter" ? value("--filter <FILTER>") : a.substr(9);
            filter = v == "box" ? SR_FILTER_BOX : v == "triangle" ? SR_FILTER_TRIANGLE : v == "catrom" ? SR_FILTER_CATROM : v == "lanczos3" ? SR_FILTER_LANCZOS3 : -1;
            if (filter < 0) video_usage_error("'" + v + "' isn't a valid value for '--filter <FILTER>'\n\t[values: box, catrom, lanczos3, triangle]");
            has_filter = true;
        }
        else if (a == "--resize-space" || a.rfind("--resize-space=", 0) == 0) {
            const std::string v = a == "--resize-space" ? value("--resize-space <SPACE>") : a.substr(15);
            if (v != "linear" && v != "srgb") video_usage_error("'" + v + "' isn't a valid value for '--resize-space <SPACE>'\n\t[values: linear, srgb]");
            resize_flags = v == "srgb" ? SR_RESIZE_SRGB_SPACE : 0u;
            has_space = true;
        }
        else if (a == "--loss") video_usage_error("The argument '--loss' can only be used with the 'train' subcommand");
        else if (a == "--lr" || a == "--lr-schedule" || a == "--warmup" || a == "--clip" || a == "--ema" || a == "--resume") video_usage_error("The argument '" + a + "' can only be used with the 'train' subcommand");
        else if (a.size() > 1 && a[0] == '-') video_usage_error("Found argument '" + a + "' which wasn't expected, or isn't valid in this context");
        else pos.push_back(a);
    }
    if (has_p && parameters != "imagenet" && parameters != "imagenetlinear" && parameters != "anime" && parameters != "bilinear")
        video_usage_error("'" + parameters + "' isn't a valid value for '--parameters <PARAMETERS>'\n\t[values: anime, bilinear, imagenet, imagenetlinear]");
    if (has_c && has_p) video_usage_error("The argument '--custom <PARAMETER_FILE>' cannot be used with '--parameters <PARAMETERS>'");
    if (pos.size() < 2) video_usage_error("The following required arguments were not provided:\n    <INPUT|->\n    <OUTPUT|->");
    if (pos.size() > 2) video_usage_error("Found argument '" + pos[2] + "' which wasn't expected, or isn't valid in this context");
    if (precision != "f32" && precision != "split_f16") video_usage_error("'" + precision + "' isn't a valid value for '--precision <MODE>'");
    if (ensemble && parameters == "bilinear")
        video_usage_error("The argument '--ensemble <N>' cannot be used with '--parameters bilinear': bilinear interpolation has no network to average");
    const bool resize = has_size || has_scale;
    if (has_size && has_scale) video_usage_error("The argument '--size <WxH>' cannot be used with '--scale <S>'");
    if ((has_filter || has_space) && !resize) video_usage_error("The following required arguments were not provided:\n    <--size <WxH>|--scale <S>>");
    if (reuse && resize)
        video_usage_error(std::string("The argument '--reuse' cannot be used with '") + (has_size ? "--size <WxH>" : "--scale <S>") + "': the row bands do not compose with a vertical resampling");

    // ---- the stream header, before anything touches the GPU: a stream this build does not take is refused by the name of its tag
    FILE* fin = pos[0] == "-" ? stdin : fopen(pos[0].c_str(), "rb");
    if (!fin) die("Error opening input stream " + pos[0]);
    std::string line, err;
    sry4m::Header hd;
    if (sry4m::read_line(fin, line) != 1) video_usage_error("the input is not a YUV4MPEG2 stream (no header line)");
    if (!sry4m::parse_header(line.data(), line.size(), hd, err, depth_arg == "auto")) video_usage_error(err);
    const bool deep = hd.depth > 8;  // (only under --depth auto)
    if (!deep && matrix == "bt2020") video_usage_error("The argument '--matrix bt2020' can only be used with a deep stream (--depth auto, C420p10 and its kin)");
    if (!deep && !siting.empty()) video_usage_error("The argument '--siting <SITING>' can only be used with a deep stream (--depth auto, C420p10 and its kin)");
    sr_yuv_format fmt{};
    fmt.subsampling = hd.s444 ? SR_YUV_444 : SR_YUV_420;
    fmt.siting = hd.left ? SR_YUV_SITING_LEFT : SR_YUV_SITING_CENTER;
    fmt.matrix = !matrix.empty() ? (matrix == "bt709" ? SR_YUV_BT709 : SR_YUV_BT601) : (hd.w >= 1280 || hd.h > 576) ? SR_YUV_BT709 : SR_YUV_BT601;
    fmt.range = hd.full ? SR_YUV_FULL : SR_YUV_LIMITED;
    sr_yuv16_format fmt16{};  // a deep stream's: the same default matrix rule, the siting the option gives
    fmt16.subsampling = hd.s444 ? (int32_t)SR_YUV_444 : hd.s422 ? (int32_t)SR_YUV_422 : (int32_t)SR_YUV_420;
    fmt16.siting = !siting.empty() ? (siting == "left" ? SR_YUV_SITING_LEFT : SR_YUV_SITING_CENTER) : fmt.siting;
    fmt16.matrix = matrix == "bt2020" ? SR_YUV_BT2020 : fmt.matrix;
    fmt16.range = fmt.range;
    fmt16.depth = hd.depth;
    // --scale is relative to the INPUT: max(1, floor(in S + 0.5)) an axis
    if (has_scale && !(scaled_axis(hd.w, scale, size_w) && scaled_axis(hd.h, scale, size_h)))
        video_usage_error("'" + scale_arg + "' isn't a valid value for '--scale <S>'\n\t[the output would exceed 16384 pixels on an axis]");
    const int out_w = resize ? size_w : SR_FACTOR * hd.w, out_h = resize ? size_h : SR_FACTOR * hd.h;

    // ---- parameters + graph, the progress text on stderr (stdout may be the stream)
    std::vector<float> params;
    int graph = SR_GRAPH_SR_NET;
    if (has_c) {
        FILE* f = fopen(custom.c_str(), "rb");
        if (!f) die("Error opening parameter file");
        std::vector<unsigned char> data;
        unsigned char tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + n);
        fclose(f);
        params = decode_rsr(data.data(), data.size());
    } else if (!has_p || parameters == "imagenet") params = decode_rsr(imagenet_rsr_begin, imagenet_rsr_end - imagenet_rsr_begin);
    else if (parameters == "imagenetlinear") params = decode_rsr(imagenetlinear_rsr_begin, imagenetlinear_rsr_end - imagenetlinear_rsr_begin);
    else if (parameters == "anime") params = decode_rsr(anime_rsr_begin, anime_rsr_end - anime_rsr_begin);
    else graph = SR_GRAPH_BILINEAR;
    sr_ctx* ctx = nullptr;
    int rc = sr_create_graph(&ctx, graph, params.empty() ? nullptr : params.data(), params.size(), SR_FACTOR, (int)device);
    if (rc != SR_OK) die(sr_strerror(rc));
    if (precision == "split_f16" && (rc = sr_set_precision(ctx, SR_PRECISION_SPLIT_F16)) != SR_OK)
        die(std::string(sr_strerror(rc)) + " (SR_PRECISION_SPLIT_F16 cannot carry these parameters; use --precision f32)");
    sr_video* vid = nullptr;
    if (resize)
        rc = deep ? sr_video_create16_sized(ctx, &fmt16, hd.h, hd.w, out_h, out_w, filter, resize_flags, (int)slots, ensemble ? ensemble : 1u, &vid)
                  : sr_video_create_sized(ctx, &fmt, hd.h, hd.w, out_h, out_w, filter, resize_flags, (int)slots, ensemble ? ensemble : 1u, &vid);
    else
        rc = deep ? sr_video_create16(ctx, &fmt16, hd.h, hd.w, (int)slots, ensemble ? ensemble : 1u, &vid)
                  : sr_video_create(ctx, &fmt, hd.h, hd.w, (int)slots, ensemble ? ensemble : 1u, &vid);
    if (rc != SR_OK) die(sr_strerror(rc));
    if (reuse && (rc = sr_video_set_reuse(vid, SR_VIDEO_REUSE_ROWS)) != SR_OK) die(sr_strerror(rc));
    const size_t in_bytes = deep ? sr_yuv16_frame_bytes(&fmt16, hd.h, hd.w) : sr_yuv_frame_bytes(&fmt, hd.h, hd.w);
    const size_t out_bytes = deep ? sr_yuv16_frame_bytes(&fmt16, out_h, out_w) : sr_yuv_frame_bytes(&fmt, out_h, out_w);

    FILE* fout = pos[1] == "-" ? stdout : fopen(pos[1].c_str(), "wb");
    if (!fout) die("Could not write output stream " + pos[1]);
    const std::string head = resize ? sry4m::sized_header(hd, out_w, out_h) : sry4m::scaled_header(hd, SR_FACTOR);
    bool wrote = fwrite(head.data(), 1, head.size(), fout) == head.size();
    std::deque<std::string> frame_lines;  // the FRAME lines of the frames in flight, oldest first: their parameters pass through
    long frames = 0, written = 0;
    std::string failure;
    // the oldest frame in flight: its FRAME line, then its payload straight from the session's buffer
    auto write_oldest = [&]() {
        const uint8_t* out = nullptr;
        const int r = sr_video_receive(vid, &out);
        if (r != SR_OK) die(std::string("frame ") + std::to_string(written) + ": " + sr_strerror(r));
        const std::string fl = frame_lines.front() + "\n";
        frame_lines.pop_front();
        wrote = wrote && fwrite(fl.data(), 1, fl.size(), fout) == fl.size() && fwrite(out, 1, out_bytes, fout) == out_bytes;
        ++written;
    };
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    for (;;) {
        if (sr_video_pending(vid) == (int)slots) write_oldest();
        const int got = sry4m::read_line(fin, line);
        if (got == 0) break;
        if (got < 0 || !sry4m::is_frame_line(line)) { failure = "frame " + std::to_string(frames) + ": not a FRAME line"; break; }
        uint8_t* in = nullptr;
        if ((rc = sr_video_acquire(vid, &in)) != SR_OK) die(sr_strerror(rc));
        if (fread(in, 1, in_bytes, fin) != in_bytes) { failure = "frame " + std::to_string(frames) + " is truncated"; break; }
        if ((rc = sr_video_submit(vid)) != SR_OK) die(std::string("frame ") + std::to_string(frames) + ": " + sr_strerror(rc));
        frame_lines.push_back(line);
        ++frames;
    }
    while (sr_video_pending(vid) > 0) write_oldest();  // (also before a failure is reported: the frames before it are written)
    const double ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    sr_video_reuse_stats reused{};
    if (reuse) (void)sr_video_get_reuse_stats(vid, &reused);
    sr_video_destroy(vid);
    sr_destroy(ctx);
    if (fout != stdout) wrote = fclose(fout) == 0 && wrote;
    else wrote = fflush(stdout) == 0 && wrote;
    if (fin != stdin) fclose(fin);
    if (!wrote) die("Could not write output stream " + pos[1]);
    if (!failure.empty()) die(failure);
    if (timing) fprintf(stderr, "[timing] frames %ld, %.2f ms/frame\n", frames, frames ? ms / frames : 0.0);
    if (timing && reuse)
        fprintf(stderr, "[timing] reuse: %llu frames whole, %llu partial, %llu reused, %.1f %% of rows computed\n", (unsigned long long)reused.frames_full,
                (unsigned long long)reused.frames_partial, (unsigned long long)reused.frames_reused,
                reused.rows_total ? 100.0 * (double)reused.rows_computed / (double)reused.rows_total : 0.0);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    std::vector<std::string> pos;
    std::string parameters, custom, precision = "f32";
    bool has_p = false, has_c = false, downsample = false, timing = false;
    int device = 0;
    unsigned ensemble = 0;  // 0: one pass of the network
    bool alpha = false, has_bleed = false;
    int bleed = SR_ALPHA_BLEED_DEFAULT;
    int border = 0, border_pad = SR_BORDER_PAD_DEFAULT;  // --border: 0 = the plain calls (sr_upscale_rgba8_border otherwise)
    bool has_border_pad = false;
    // --size / --scale: the output is resampled to a size of the user's choosing (sr_upscale_rgba8_sized)
    bool has_size = false, has_scale = false, has_filter = false, has_space = false;
    std::string size_arg, scale_arg;
    int size_w = 0, size_h = 0, filter = SR_FILTER_LANCZOS3;
    double scale = 0;
    unsigned resize_flags = 0;
    std::vector<int> devices;
    std::string depth_arg = "8";  // --depth 8|16|auto: the deep-colour calls (sr_upscale_u16*) for 16
    if (argc >= 2 && !strcmp(argv[1], "train")) return run_train(argc, argv);  // main.rs:119-121
    if (argc >= 2 && !strcmp(argv[1], "validate")) return run_validate(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "video")) return run_video(argc, argv);
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
        else if (a == "--ensemble") {
            const std::string v = value("--ensemble <N>");
            if (!(ensemble = ensemble_mask(v))) usage_error("'" + v + "' isn't a valid value for '--ensemble <N>'\n\t[values: 2, 4, 8]");
        }
        else if (a == "--alpha") alpha = true;
        else if (a == "--bleed" || a.rfind("--bleed=", 0) == 0) {
            const std::string v = a == "--bleed" ? value("--bleed <N>") : a.substr(8);
            const auto r = std::from_chars(v.data(), v.data() + v.size(), bleed);
            if (v.empty() || r.ec != std::errc() || r.ptr != v.data() + v.size() || bleed < 0 || bleed > SR_ALPHA_BLEED_MAX)
                usage_error("'" + v + "' isn't a valid value for '--bleed <N>'\n\t[values: 0..16]");
            has_bleed = true;
        }
        else if (a == "--border" || a.rfind("--border=", 0) == 0) {
            const std::string v = a == "--border" ? value("--border <MODE>") : a.substr(9);
            border = v == "wrap" ? SR_BORDER_WRAP : v == "replicate" ? SR_BORDER_REPLICATE : v == "mirror" ? SR_BORDER_MIRROR : 0;
            if (!border) usage_error("'" + v + "' isn't a valid value for '--border <MODE>'\n\t[values: mirror, replicate, wrap]");
        }
        else if (a == "--border-pad" || a.rfind("--border-pad=", 0) == 0) {
            const std::string v = a == "--border-pad" ? value("--border-pad <N>") : a.substr(13);
            const auto r = std::from_chars(v.data(), v.data() + v.size(), border_pad);
            if (v.empty() || r.ec != std::errc() || r.ptr != v.data() + v.size() || border_pad < SR_HALO || border_pad > SR_BORDER_PAD_MAX)
                usage_error("'" + v + "' isn't a valid value for '--border-pad <N>'\n\t[values: 7..32]");
            has_border_pad = true;
        }
        else if (a == "--size" || a.rfind("--size=", 0) == 0) {
            size_arg = a == "--size" ? value("--size <WxH>") : a.substr(7);
            if (!parse_size(size_arg, size_w, size_h))
                usage_error("'" + size_arg + "' isn't a valid value for '--size <WxH>'\n\t[two whole numbers, 1..16384 each: 3840x2160]");
            has_size = true;
        }
        else if (a == "--scale" || a.rfind("--scale=", 0) == 0) {
            scale_arg = a == "--scale" ? value("--scale <S>") : a.substr(8);
            if (!parse_scale(scale_arg, scale)) usage_error("'" + scale_arg + "' isn't a valid value for '--scale <S>'\n\t[a positive decimal: 1.5]");
            has_scale = true;
        }
        else if (a == "--filter" || a.rfind("--filter=", 0) == 0) {
            const std::string v = a == "--filter" ? value("--filter <FILTER>") : a.substr(9);
            filter = v == "box" ? SR_FILTER_BOX : v == "triangle" ? SR_FILTER_TRIANGLE : v == "catrom" ? SR_FILTER_CATROM : v == "lanczos3" ? SR_FILTER_LANCZOS3 : -1;
            if (filter < 0) usage_error("'" + v + "' isn't a valid value for '--filter <FILTER>'\n\t[values: box, catrom, lanczos3, triangle]");
            has_filter = true;
        }
        else if (a == "--resize-space" || a.rfind("--resize-space=", 0) == 0) {
            const std::string v = a == "--resize-space" ? value("--resize-space <SPACE>") : a.substr(15);
            if (v != "linear" && v != "srgb") usage_error("'" + v + "' isn't a valid value for '--resize-space <SPACE>'\n\t[values: linear, srgb]");
            resize_flags = v == "srgb" ? SR_RESIZE_SRGB_SPACE : 0u;
            has_space = true;
        }
        else if (a == "--depth" || a.rfind("--depth=", 0) == 0) {
            depth_arg = a == "--depth" ? value("--depth <BITS>") : a.substr(8);
            if (depth_arg != "8" && depth_arg != "16" && depth_arg != "auto")
                usage_error("'" + depth_arg + "' isn't a valid value for '--depth <BITS>'\n\t[values: 16, 8, auto]");
        }
        else if (a == "--augment") usage_error("The argument '--augment' can only be used with the 'train' subcommand");
        else if (a == "--loss") usage_error("The argument '--loss' can only be used with the 'train' subcommand");
        else if (a == "--lr" || a == "--lr-schedule" || a == "--warmup" || a == "--clip" || a == "--ema" || a == "--resume") usage_error("The argument '" + a + "' can only be used with the 'train' subcommand");
        else if (a == "--degrade") usage_error("The argument '--degrade' can only be used with the 'train' and 'validate' subcommands");
        else if (a == "--metrics" || a == "--shave" || a.rfind("--shave=", 0) == 0)
            usage_error("The argument '" + a.substr(0, a.find('=')) + "' can only be used with the 'validate' subcommand");
        else if (a == "--reuse") usage_error("The argument '--reuse' can only be used with the 'video' subcommand");
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
    // the ensemble averages the NETWORK over flips and rotations: the parameter-free graphs commute with them, and it has no multi-GPU form
    if (ensemble && has_p && parameters == "bilinear")
        usage_error("The argument '--ensemble <N>' cannot be used with '--parameters bilinear': bilinear interpolation has no network to average");
    if (ensemble && downsample) usage_error("The argument '--ensemble <N>' cannot be used with '--downsample': there is no network to average");
    if (ensemble && devices.size() > 1)
        usage_error("The argument '--ensemble <N>' cannot be used with more than one device: the ensemble has no multi-GPU form");
    // --alpha: the bleed / upscale / merge call has no downsampling and no multi-GPU form, and only PNG carries an alpha channel
    if (has_bleed && !alpha) usage_error("The following required arguments were not provided:\n    --alpha");
    if (alpha && downsample) usage_error("The argument '--alpha' cannot be used with '--downsample'");
    if (alpha && devices.size() > 1) usage_error("The argument '--alpha' cannot be used with more than one device: the alpha path has no multi-GPU form");
    if (alpha) {
        const size_t dot = pos[1].find_last_of('.');
        std::string ext = dot == std::string::npos ? "" : pos[1].substr(dot + 1);
        for (auto& ch : ext) ch = (char)tolower((unsigned char)ch);
        if (ext != "png")
            usage_error("The argument '--alpha' cannot be used with an output file other than .png: JPEG, BMP and PPM carry no alpha channel");
    }
    // --size / --scale: one of them; the resampled call has no downsampling, no alpha-aware and no multi-GPU form
    const bool resize = has_size || has_scale;
    if (has_size && has_scale) usage_error("The argument '--size <WxH>' cannot be used with '--scale <S>'");
    if ((has_filter || has_space) && !resize) usage_error("The following required arguments were not provided:\n    <--size <WxH>|--scale <S>>");
    const std::string resize_opt = has_size ? "--size <WxH>" : "--scale <S>";
    if (resize && downsample) usage_error("The argument '" + resize_opt + "' cannot be used with '--downsample'");
    if (resize && alpha) usage_error("The argument '" + resize_opt + "' cannot be used with '--alpha': the resampling is not alpha-aware");
    if (resize && devices.size() > 1)
        usage_error("The argument '" + resize_opt + "' cannot be used with more than one device: the resampled call has no multi-GPU form");
    // --border: the padded call has no downsampling, no resampled and no multi-GPU form
    if (has_border_pad && !border) usage_error("The following required arguments were not provided:\n    --border <MODE>");
    if (border && downsample) usage_error("The argument '--border <MODE>' cannot be used with '--downsample'");
    if (border && resize) usage_error("The argument '--border <MODE>' cannot be used with '" + resize_opt + "': the resampled call has no border modes");
    if (border && devices.size() > 1)
        usage_error("The argument '--border <MODE>' cannot be used with more than one device: the padded call has no multi-GPU form");
    // --depth 16: the deep-colour calls have no transparency and no multi-GPU form, and only PNG and PPM hold 16-bit samples here
    std::string out_ext;
    {
        const size_t dot = pos[1].find_last_of('.');
        out_ext = dot == std::string::npos ? "" : pos[1].substr(dot + 1);
        for (auto& ch : out_ext) ch = (char)tolower((unsigned char)ch);
    }
    if (depth_arg == "16" && alpha) usage_error("The argument '--depth 16' cannot be used with '--alpha': there is no 16-bit bleed and merge");
    if (depth_arg == "16" && devices.size() > 1)
        usage_error("The argument '--depth 16' cannot be used with more than one device: the deep-colour call has no multi-GPU form");
    if (depth_arg == "16" && (out_ext == "jpg" || out_ext == "jpeg" || out_ext == "bmp"))
        usage_error("The argument '--depth 16' cannot be used with a ." + out_ext + " output file: 16-bit samples are written to .png and .ppm only");
    int in_pw = 0, in_ph = 0;
    // (the file's header says how large the input is: a scale that takes it beyond the largest output is refused before any device is touched)
    if (has_scale && srpng::probe_image_size(pos[0], in_pw, in_ph) && !(scaled_axis(in_pw, scale, size_w) && scaled_axis(in_ph, scale, size_h)))
        usage_error("'" + scale_arg + "' isn't a valid value for '--scale <S>'\n\t[the output would exceed 16384 pixels on an axis]");

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
        if (depth_arg == "16" && ext != "png" && ext != "ppm") die("Could not write output file (--depth 16 writes .png and .ppm)");
    }
    // The input file decodes on a second thread while this one brings up the device and the contexts (HIP start-up
    // and the weight upload take longer than a 1080p PNG); failures are then reported in the reference's order --
    // the graph first (main.rs:160-162), the image after it (main.rs:164).
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    const clk::time_point t_start = clk::now();
    srpng::Image in;
    srpng::Image16 in16;
    std::string err;
    bool decoded = false;
    double t_decode = 0;
    // --depth auto: 16 where the file holds more than 8 bits a sample and the call and the output can keep them; the file says so once
    // it is decoded (here, before the device: an 8-bit file then takes today's path untouched)
    bool deep = depth_arg == "16";
    if (depth_arg == "auto" && !alpha && devices.size() == 1 && (out_ext == "png" || out_ext == "ppm")) {
        const clk::time_point t = clk::now();
        std::string err16;
        if (srpng::decode_image_file16(pos[0], in16, err16) && in16.bits > 8) { deep = decoded = true; t_decode = ms_since(t); }
        else in16 = srpng::Image16();
    }
    std::thread decoder([&] {
        if (decoded) return;
        const clk::time_point t = clk::now();
        decoded = deep ? srpng::decode_image_file16(pos[0], in16, err) : srpng::decode_image_file(pos[0], in, err);
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
        if (!sized || deep) return;  // (the 16-bit result is an ordinary vector)
        int sw = 0, sh = 0;
        if (has_scale && !(scaled_axis(pw, scale, sw) && scaled_axis(ph, scale, sh))) return;
        const size_t bytes = has_size ? (size_t)size_w * size_h * 4 : has_scale ? (size_t)sw * sh * 4
                             : graph == SR_GRAPH_DOWNSAMPLE ? (size_t)(pw / 3) * (ph / 3) * 4 : (size_t)pw * 3 * ph * 3 * 4;
        if (sr_host_alloc(&pinned, bytes) == SR_OK) pinned_bytes = bytes; else pinned = nullptr;
    });
    std::vector<sr_ctx*> ctxs(devices.size(), nullptr);
    int rc = SR_OK;
    for (size_t k = 0; k < devices.size() && rc == SR_OK; ++k) {
        rc = sr_create_graph(&ctxs[k], graph, params.empty() ? nullptr : params.data(), params.size(), SR_FACTOR, devices[k]);
        if (rc == SR_OK && graph == SR_GRAPH_SR_NET) rc = sr_set_precision(ctxs[k], precision == "f32" ? SR_PRECISION_F32 : SR_PRECISION_SPLIT_F16);
        if (rc == SR_OK && (ensemble || alpha || resize || border || deep) && timing) rc = sr_set_profiling(ctxs[k], 1);  // (the ensemble, alpha, border and resampled calls time themselves only when asked to)
    }
    const double t_create = ms_since(t_start);
    double t_prep = 0;
    {
        const clk::time_point t = clk::now();
        if (rc == SR_OK && sized && ctxs.size() == 1 && !resize && !deep) (void)sr_reserve_rgba8(ctxs[0], 4, 1, ph, pw);  // best effort: the real call reports errors
        pinner.join();
        t_prep = ms_since(t);
    }
    decoder.join();
    if (rc != SR_OK) die(sr_strerror(rc));  // SR_E_PARAM_COUNT carries the text of main.rs:162
    sr_ctx* ctx = ctxs[0];
    if (!decoded) die("Error opening input image file. (" + err + ")");  // main.rs:164
    const double t_ready = ms_since(t_start);
    if (deep) { in.w = in16.w; in.h = in16.h; }
    if (graph == SR_GRAPH_DOWNSAMPLE && (in.w < 3 || in.h < 3)) die("input image is smaller than one 3x3 pooling block");

    if (has_scale && !(scaled_axis(in.w, scale, size_w) && scaled_axis(in.h, scale, size_h)))  // (a file whose header could not be probed)
        usage_error("'" + scale_arg + "' isn't a valid value for '--scale <S>'\n\t[the output would exceed 16384 pixels on an axis]");
    const int ow = resize ? size_w : graph == SR_GRAPH_DOWNSAMPLE ? in.w / 3 : in.w * 3;
    const int oh = resize ? size_h : graph == SR_GRAPH_DOWNSAMPLE ? in.h / 3 : in.h * 3;
    if (deep) {  // 16-bit samples in and out: grey stays grey where the container can say so (PNG colour type 0), else RGB
        const int oc = in16.channels <= 2 && out_ext == "png" ? 1 : 3;
        std::vector<uint16_t> out16((size_t)ow * oh * oc);
        const unsigned members = ensemble ? ensemble : 1u;
        const clk::time_point t_up = clk::now();
        rc = resize ? sr_upscale_u16_sized(ctx, in16.px.data(), in16.channels, 1, in.h, in.w, out16.data(), oc, oh, ow, filter, resize_flags, members)
             : border ? sr_upscale_u16_border(ctx, in16.px.data(), in16.channels, 1, in.h, in.w, out16.data(), oc, border, border_pad, members)
                      : sr_upscale_u16(ctx, in16.px.data(), in16.channels, 1, in.h, in.w, out16.data(), oc, members);
        if (rc != SR_OK) die(std::string(sr_strerror(rc)) + (rc == SR_E_HIP ? " (hipError " + std::to_string(sr_last_hip_error(ctx)) + ")" : ""));
        const double t_upscale = ms_since(t_up);
        if (timing) {
            double tot = 0, h2d = 0, d2h = 0;
            sr_last_timing(ctx, &tot, nullptr, &h2d, &d2h);
            fprintf(stderr, "\n[timing] %dx%d -> %dx%d, 16 bits, %d -> %d channels%s: kernels %.3f ms, h2d %.3f ms, d2h %.3f ms\n", in.w, in.h, ow, oh,
                    in16.channels, oc, ensemble ? (" (ensemble of " + std::to_string(__builtin_popcount(ensemble)) + ")").c_str() : "", tot, h2d, d2h);
        }
        printf(" Writing file...");
        fflush(stdout);
        const clk::time_point t_enc = clk::now();
        if (!srpng::encode_image_file16(pos[1], out16.data(), oc, ow, oh, err)) die("Could not write output file (" + err + ")");
        puts(" Done");
        if (timing)
            fprintf(stderr, "[timing] wall: decode %.1f ms || device + contexts %.1f ms -> ready at %.1f ms; upscale call %.1f ms; encode + write %.1f ms; "
                            "total %.1f ms\n", t_decode, t_create, t_ready, t_upscale, ms_since(t_enc), ms_since(t_start));
        if (pinned) sr_host_free(pinned);
        for (sr_ctx* c : ctxs) sr_destroy(c);
        return 0;
    }
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
    rc = resize ? sr_upscale_rgba8_sized(ctx, in.rgba.data(), 1, in.h, in.w, out, oh, ow, filter, resize_flags, ensemble ? ensemble : 1u)
         : border ? sr_upscale_rgba8_border(ctx, in.rgba.data(), 1, in.h, in.w, out, border, border_pad, ensemble ? ensemble : 1u, alpha ? bleed : -1)
         : alpha ? sr_upscale_rgba8_alpha(ctx, in.rgba.data(), 1, in.h, in.w, out, bleed, ensemble ? ensemble : 1u)
         : ensemble ? sr_upscale_ensemble_rgba8(ctx, in.rgba.data(), 4, 1, in.h, in.w, out, ensemble)
         : ctxs.size() > 1 ? sr_upscale_rgba8_multi(ctxs.data(), (int)ctxs.size(), in.rgba.data(), 4, in.h, in.w, out)
                           : sr_upscale_rgba8(ctx, in.rgba.data(), 4, 1, in.h, in.w, out);
    if (rc != SR_OK) die(std::string(sr_strerror(rc)) + (rc == SR_E_HIP ? " (hipError " + std::to_string(sr_last_hip_error(ctx)) + ")" : ""));
    const double t_upscale = ms_since(t_up);
    if (timing) {
        double tot = 0, h2d = 0, d2h = 0;
        sr_last_timing(ctx, &tot, nullptr, &h2d, &d2h);
        fprintf(stderr, "\n[timing] %dx%d -> %dx%d%s: kernels %.3f ms, h2d %.3f ms, d2h %.3f ms\n", in.w, in.h, ow, oh,
                ensemble ? (" (ensemble of " + std::to_string(__builtin_popcount(ensemble)) + ")").c_str() : "", tot, h2d, d2h);
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
