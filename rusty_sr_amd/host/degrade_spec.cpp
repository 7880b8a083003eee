// degrade_spec.cpp -- the --degrade SPEC parser and the draw stream (degrade_spec.hpp has the rules).
#include "degrade_spec.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace srdegrade {
namespace {

// a decimal number that is the whole of s (strtod's syntax, but no hex, no inf / nan, no leading space)
bool number(const std::string& s, bool integer, double& out) {
    if (s.empty() || s.size() > 32) return false;
    for (size_t i = 0; i < s.size(); ++i) {
        const char c = s[i];
        const bool ok = (c >= '0' && c <= '9') || ((c == '-' || c == '+') && (i == 0 || s[i - 1] == 'e' || s[i - 1] == 'E')) ||
                        (!integer && (c == '.' || c == 'e' || c == 'E'));
        if (!ok) return false;
    }
    char* end = nullptr;
    out = std::strtod(s.c_str(), &end);
    return end == s.c_str() + s.size() && std::isfinite(out);
}

uint64_t output(uint64_t seed, uint64_t j) {  // output number j (1, 2, ...) of the SplitMix64 stream seeded with seed
    uint64_t z = seed + j * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

double uniform(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }

}  // namespace

bool parse(const std::string& text, Spec& spec, std::string& err) {
    spec = Spec{};
    if (text.empty()) { err = "empty spec"; return false; }
    bool seen[3] = {false, false, false};
    for (size_t pos = 0; pos <= text.size();) {
        const size_t comma = std::min(text.find(',', pos), text.size());
        const std::string part = text.substr(pos, comma - pos);
        pos = comma + 1;
        const size_t eq = part.find('=');
        const std::string key = part.substr(0, eq);
        const int which = key == "blur" ? 0 : key == "noise" ? 1 : key == "jpeg" ? 2 : -1;
        if (which < 0) { err = "unknown key '" + key + "' [keys: blur, noise, jpeg]"; return false; }
        if (eq == std::string::npos || seen[which]) { err = "malformed or repeated key '" + key + "'"; return false; }
        seen[which] = true;
        const std::string val = part.substr(eq + 1);
        const size_t colon = val.find(':');
        double a = 0, b = 0;
        if (!number(val.substr(0, colon), which == 2, a) ||
            (colon != std::string::npos ? !number(val.substr(colon + 1), which == 2, b) : (b = a, false))) {
            err = "malformed value for '" + key + "'";
            return false;
        }
        if (b < a) { err = "reversed range for '" + key + "'"; return false; }
        const double hi = which == 0 ? 4.0 : which == 1 ? 64.0 : 100.0;
        if (a < 0 || b > hi) { err = "range for '" + key + "' outside 0.." + std::to_string((int)hi); return false; }
        if (which == 0) { spec.blur[0] = a; spec.blur[1] = b; }
        else if (which == 1) { spec.noise[0] = a; spec.noise[1] = b; }
        else { spec.jpeg[0] = (int)a; spec.jpeg[1] = (int)b; }
    }
    return true;
}

Draw draw(const Spec& spec, uint64_t seed, uint64_t index) {
    const uint64_t s = seed ^ 0xD6E8FEB86659FD93ull;
    const double u0 = uniform(output(s, 4 * index + 1)), u1 = uniform(output(s, 4 * index + 2)), u2 = uniform(output(s, 4 * index + 3));
    Draw d;
    d.sigma = (float)(spec.blur[0] + u0 * (spec.blur[1] - spec.blur[0]));
    d.noise = (float)(spec.noise[0] + u1 * (spec.noise[1] - spec.noise[0]));
    d.quality = spec.jpeg[0] + (int)std::floor(u2 * (double)(spec.jpeg[1] - spec.jpeg[0] + 1));
    d.seed = output(s, 4 * index + 4);
    return d;
}

}  // namespace srdegrade
