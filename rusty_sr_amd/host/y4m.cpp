// y4m.cpp -- the YUV4MPEG2 header parser of `rusty_sr video` (y4m.hpp).
#include "y4m.hpp"

#include <cstdint>

#include <cstring>

namespace sry4m {

namespace {

// a whole number 1 .. kMaxAxis, digits only
bool parse_axis(const std::string& v, int& out) {
    if (v.empty() || v.size() > 6) return false;
    long n = 0;
    for (const char ch : v) {
        if (ch < '0' || ch > '9') return false;
        n = n * 10 + (ch - '0');
    }
    if (n < 1 || n > kMaxAxis) return false;
    out = (int)n;
    return true;
}

bool ends_with(const std::string& s, const char* tail) {
    const size_t n = strlen(tail);
    return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

// "420p10" and its kin: <420|422|444>p<9|10|12|14|16>
bool parse_deep_tag(const std::string& v, Header& out) {
    if (v.size() < 5 || v[3] != 'p') return false;
    const std::string base = v.substr(0, 3), d = v.substr(4);
    if (base != "420" && base != "422" && base != "444") return false;
    if (d != "9" && d != "10" && d != "12" && d != "14" && d != "16") return false;
    out.depth = d.size() == 1 ? d[0] - '0' : 10 + (d[1] - '0');
    out.s444 = base == "444";
    out.s422 = base == "422";
    out.left = !out.s444;
    return true;
}

}  // namespace

bool parse_header(const char* line, size_t len, Header& out, std::string& err) { return parse_header(line, len, out, err, false); }

bool parse_header(const char* line, size_t len, Header& out, std::string& err, bool deep) {
    static const char kMagic[] = "YUV4MPEG2";
    const size_t m = sizeof kMagic - 1;
    out = Header{};
    if (len > kMaxLine) { err = "the stream header is longer than " + std::to_string(kMaxLine) + " bytes"; return false; }
    if (len < m || memcmp(line, kMagic, m) != 0 || (len > m && line[m] != ' ')) { err = "not a YUV4MPEG2 stream"; return false; }
    bool has_w = false, has_h = false, has_c = false;
    size_t at = m;
    while (at < len) {
        while (at < len && line[at] == ' ') ++at;
        size_t end = at;
        while (end < len && line[end] != ' ') ++end;
        if (end == at) break;
        const std::string tag(line + at, end - at);
        at = end;
        for (const char ch : tag)
            if ((unsigned char)ch < 0x21 || (unsigned char)ch > 0x7e) { err = "a byte that is not printable in the stream header"; return false; }
        const std::string v = tag.substr(1);
        switch (tag[0]) {
        case 'W':
            if (has_w || !parse_axis(v, out.w)) { err = "'" + tag + "' isn't a valid width [1.." + std::to_string(kMaxAxis) + "]"; return false; }
            has_w = true;
            break;
        case 'H':
            if (has_h || !parse_axis(v, out.h)) { err = "'" + tag + "' isn't a valid height [1.." + std::to_string(kMaxAxis) + "]"; return false; }
            has_h = true;
            break;
        case 'I':
            if (v != "p") { err = "'" + tag + "': interlaced streams are not supported (only Ip)"; return false; }
            break;
        case 'C':
            if (has_c) { err = "more than one C tag in the stream header"; return false; }
            has_c = true;
            if (deep && parse_deep_tag(v, out)) break;
            if (ends_with(v, "p10") || ends_with(v, "p12") || ends_with(v, "p14") || ends_with(v, "p16") || v == "mono16") {
                err = "'" + tag + "': only 8-bit streams are supported";
                return false;
            }
            if (v == "420jpeg" || v == "420") out.s444 = false, out.left = false;
            else if (v == "420mpeg2") out.s444 = false, out.left = true;
            else if (v == "444") out.s444 = true, out.left = false;
            else { err = "'" + tag + "' is not supported [C420jpeg, C420, C420mpeg2, C444]"; return false; }
            break;
        case 'X':
            if (tag == "XCOLORRANGE=FULL") out.full = true;
            break;
        case 'F':
        case 'A':
            break;
        default:
            err = "'" + tag + "' is not a tag of a YUV4MPEG2 stream header";
            return false;
        }
        out.tags.push_back(tag);
    }
    if (!has_w || !has_h) { err = "the stream header has no " + std::string(has_w ? "H" : "W") + " tag"; return false; }
    return true;
}

std::string scaled_header(const Header& h, int factor) {
    std::string s = "YUV4MPEG2";
    for (const std::string& tag : h.tags) {
        s += ' ';
        if (tag[0] == 'W') s += "W" + std::to_string((long)h.w * factor);
        else if (tag[0] == 'H') s += "H" + std::to_string((long)h.h * factor);
        else s += tag;
    }
    s += '\n';
    return s;
}

namespace {

// "A<n>:<d>", both terms decimal digits alone, above 0 and small enough for 64-bit arithmetic; false: the tag passes through as it is
bool parse_aspect(const std::string& tag, uint64_t& n, uint64_t& d) {
    const size_t colon = tag.find(':');
    if (colon == std::string::npos || colon < 2 || colon + 1 >= tag.size()) return false;
    uint64_t v[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const size_t b = k ? colon + 1 : 1, e = k ? tag.size() : colon;
        if (e - b > 18) return false;
        for (size_t i = b; i < e; ++i) {
            if (tag[i] < '0' || tag[i] > '9') return false;
            v[k] = 10 * v[k] + (uint64_t)(tag[i] - '0');
        }
    }
    n = v[0];
    d = v[1];
    return n > 0 && d > 0;  // (A0:0 is "unknown"; a single zero term is no ratio)
}

uint64_t gcd64(uint64_t a, uint64_t b) {
    while (b) {
        const uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

std::string sized_header(const Header& h, int ow, int oh) {
    std::string s = "YUV4MPEG2";
    for (const std::string& tag : h.tags) {
        s += ' ';
        uint64_t n = 0, d = 0, pn = 0, pd = 0;
        if (tag[0] == 'W') s += "W" + std::to_string(ow);
        else if (tag[0] == 'H') s += "H" + std::to_string(oh);
        // the display aspect W n : H d stays: the new pixel aspect is (n W oh) : (d H ow)
        else if (tag[0] == 'A' && (uint64_t)h.w * (uint64_t)oh == (uint64_t)h.h * (uint64_t)ow) s += tag;  // a uniform resize: the tag it read
        else if (tag[0] == 'A' && h.w > 0 && h.h > 0 && ow > 0 && oh > 0 && parse_aspect(tag, n, d) &&
                 !__builtin_mul_overflow(n, (uint64_t)h.w, &pn) && !__builtin_mul_overflow(pn, (uint64_t)oh, &pn) &&
                 !__builtin_mul_overflow(d, (uint64_t)h.h, &pd) && !__builtin_mul_overflow(pd, (uint64_t)ow, &pd)) {
            const uint64_t g = gcd64(pn, pd);
            s += "A" + std::to_string(pn / g) + ":" + std::to_string(pd / g);
        }
        else s += tag;
    }
    s += '\n';
    return s;
}

int read_line(FILE* f, std::string& line) {
    line.clear();
    for (;;) {
        const int ch = fgetc(f);
        if (ch == EOF) return line.empty() ? 0 : -1;
        if (ch == '\n') return 1;
        if (line.size() >= kMaxLine) return -1;
        line.push_back((char)ch);
    }
}

bool is_frame_line(const std::string& line) {
    return line.compare(0, 5, "FRAME") == 0 && (line.size() == 5 || line[5] == ' ');
}

}  // namespace sry4m
