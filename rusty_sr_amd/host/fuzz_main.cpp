// fuzz_main.cpp -- decoder robustness harness (test infrastructure of the host CLI, SURVEY.md section 5:
// "-fsanitize=address for host C++").  Built with AddressSanitizer + UBSan by rusty_sr_amd.build.build_sanitized().
//
//   srcodec_asan FILE...        decode every file the way the CLI's `image::open` stand-in does (main.rs:164) and
//                               print one line per file: "ok WxH" or "error: <message>"
//   srcodec_asan --roundtrip W H OUT.png   encode a synthetic RGBA image, decode it again, compare
//   srcodec_asan --u16 FILE...  decode every file through the deep-colour path (decode_image_file16), touch every sample and print
//                               "ok WxH channels bits sum" or "error: <message>"
//   srcodec_asan --roundtrip16 W H CHANNELS OUT.png   encode a synthetic 16-bit image (1 or 3 channels), decode it again, compare
//   srcodec_asan --degrade-spec SPEC SEED N   parse the CLI's --degrade SPEC (degrade_spec.cpp) and print its first N draws under SEED,
//                               one "sigma noise quality seed" line each (floats as their bit patterns), or "error: <message>"
//
// A malformed file must end in a clean "error:" line -- the counterpart of the reference's
// `.expect("Error opening input image file.")`.  Any out-of-bounds access, overflow or leak makes the sanitizers
// abort the process with a non-zero status, which tests/test_decoder_robustness.py treats as failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "degrade_spec.hpp"
#include "png.hpp"

int main(int argc, char** argv) {
    if (argc >= 5 && !strcmp(argv[1], "--roundtrip")) {
        const int w = atoi(argv[2]), h = atoi(argv[3]);
        std::vector<uint8_t> px((size_t)w * h * 4);
        uint32_t z = 12345;
        for (int y = 0; y < h; ++y)  // noise, flat and ramp rows in turn: literals, long runs and every filter type
            for (int x = 0; x < w * 4; ++x) {
                z = z * 1664525u + 1013904223u;
                const int kind = (y / 3) % 4;
                px[(size_t)y * w * 4 + x] = kind == 0 ? (uint8_t)(z >> 24) : kind == 1 ? (uint8_t)(y * 7) : kind == 2 ? (uint8_t)(x / 4 + y) : (uint8_t)((x / 4) * (y & 3) + (z >> 31));
            }
        std::string err;
        if (!srpng::encode_file(argv[4], px.data(), w, h, err)) { printf("error: %s\n", err.c_str()); return 1; }
        srpng::Image img;
        if (!srpng::decode_file(argv[4], img, err)) { printf("error: %s\n", err.c_str()); return 1; }
        if (img.w != w || img.h != h || img.rgba != px) { printf("error: round trip differs\n"); return 1; }
        printf("ok %dx%d\n", w, h);
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "--roundtrip16")) {
        const int w = atoi(argv[2]), h = atoi(argv[3]), ch = atoi(argv[4]);
        if (w <= 0 || h <= 0 || w > 4096 || h > 4096) { printf("error: bad size\n"); return 1; }
        std::vector<uint16_t> px((size_t)w * h * (ch > 0 ? ch : 1));
        uint32_t z = 54321;
        for (size_t i = 0; i < px.size(); ++i) {  // noise, flat, ramp and low-byte-only rows in turn
            z = z * 1664525u + 1013904223u;
            const size_t y = i / ((size_t)w * (ch > 0 ? ch : 1));
            const int kind = (int)(y / 3) % 4;
            px[i] = kind == 0 ? (uint16_t)(z >> 16) : kind == 1 ? (uint16_t)(y * 771) : kind == 2 ? (uint16_t)(i * 37) : (uint16_t)(0x8000 + (z >> 24));
        }
        std::string err;
        if (!srpng::encode_png16_file(argv[5], px.data(), ch, w, h, err)) { printf("error: %s\n", err.c_str()); return 1; }
        srpng::Image16 img;
        if (!srpng::decode_image_file16(argv[5], img, err)) { printf("error: %s\n", err.c_str()); return 1; }
        if (img.w != w || img.h != h || img.channels != ch || img.bits != 16 || img.px != px) { printf("error: round trip differs\n"); return 1; }
        printf("ok %dx%d %d\n", w, h, ch);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "--u16")) {
        for (int i = 2; i < argc; ++i) {
            srpng::Image16 img;
            std::string err;
            if (srpng::decode_image_file16(argv[i], img, err)) {
                if (img.w <= 0 || img.h <= 0 || img.channels < 1 || img.channels > 4 || img.bits < 1 || img.bits > 16 ||
                    img.px.size() != (size_t)img.w * img.h * img.channels) { printf("error: inconsistent image\n"); continue; }
                unsigned long sum = 0;
                for (uint16_t v : img.px) sum += v;
                printf("ok %dx%d %d %d %lu\n", img.w, img.h, img.channels, img.bits, sum);
            } else {
                printf("error: %s\n", err.c_str());
            }
        }
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "--degrade-spec")) {
        srdegrade::Spec spec;
        std::string err;
        if (!srdegrade::parse(argv[2], spec, err)) { printf("error: %s\n", err.c_str()); return 1; }
        const unsigned long long seed = strtoull(argv[3], nullptr, 10);
        for (long i = 0, n = atol(argv[4]); i < n; ++i) {
            const srdegrade::Draw d = srdegrade::draw(spec, seed, (uint64_t)i);
            uint32_t bits[2];
            memcpy(&bits[0], &d.sigma, 4);
            memcpy(&bits[1], &d.noise, 4);
            printf("%08x %08x %d %llu\n", bits[0], bits[1], d.quality, (unsigned long long)d.seed);
        }
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        srpng::Image img;
        std::string err;
        if (srpng::decode_image_file(argv[i], img, err)) {
            if (img.w <= 0 || img.h <= 0 || img.rgba.size() != (size_t)img.w * img.h * 4) { printf("error: inconsistent image\n"); continue; }
            // touch every byte: a decoder that under-fills its buffer is caught by ASAN / MSAN-style checks here
            unsigned long sum = 0;
            for (uint8_t b : img.rgba) sum += b;
            printf("ok %dx%d %lu\n", img.w, img.h, sum);
        } else {
            printf("error: %s\n", err.c_str());
        }
    }
    return 0;
}
