// degrade_spec.hpp -- the CLI's --degrade SPEC and its draws (main.cpp `train` and `validate`; include/srhip.h "Degradation").
//   SPEC = key=A[:B] joined by commas, keys blur (0..4, the Gaussian's sigma in HR pixels), noise (0..64, 8-bit levels), jpeg (0..100,
//   whole numbers; 0: no JPEG); a key that is absent is off.  A[:B] is a range, A alone the range A:A.
//   Draw i (0, 1, ...) under `seed`: outputs 4i + 1 .. 4i + 4 of the SplitMix64 stream seeded with seed ^ 0xD6E8FEB86659FD93, in the order
//   blur, noise, jpeg, noise seed: value = A + u (B - A), jpeg = A + floor(u (B - A + 1)), u = (x >> 11) 2^-53; the fourth output is
//   the noise seed as is.  The stream is its own: a seed's shuffles, origins and members are what they are without --degrade.
// No HIP, no I/O: the sanitized test program (fuzz_main.cpp) links this file as it is.
#pragma once
#include <cstdint>
#include <string>

namespace srdegrade {

struct Spec {
    double blur[2] = {0, 0}, noise[2] = {0, 0};
    int jpeg[2] = {0, 0};
};
struct Draw {
    float sigma, noise;
    int quality;
    uint64_t seed;
};

// false: err names the key that is malformed, repeated, reversed or out of range
bool parse(const std::string& text, Spec& spec, std::string& err);
Draw draw(const Spec& spec, uint64_t seed, uint64_t index);

}  // namespace srdegrade
