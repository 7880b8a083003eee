// y4m_header_deep.cpp -- the `deep` overload of the YUV4MPEG2 header parser (rusty_sr_amd/host/y4m.cpp), which `rusty_sr video --depth
// auto` reads a stream's header with: host code with its own main, built by tests/test_yuv16_cpu.py plainly and under AddressSanitizer +
// UBSan.  Each header is parsed from a heap buffer of exactly its length (no terminator), so that a read past its end is an error the
// sanitizer sees.  Prints one line a case: "ok W H 420|422|444 center|left limited|full DEPTH | <scaled header>" or "refused <message>".
//   argv: headers, parsed with deep = true; after a literal "--" with deep = false (the four-argument overload).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../rusty_sr_amd/host/y4m.hpp"

namespace {

bool parse(const std::string& text, sry4m::Header& h, std::string& err, bool deep) {
    char* buf = (char*)malloc(text.size() ? text.size() : 1);
    memcpy(buf, text.data(), text.size());
    const bool ok = deep ? sry4m::parse_header(buf, text.size(), h, err, true) : sry4m::parse_header(buf, text.size(), h, err);
    free(buf);
    return ok;
}

void show(const std::string& text, bool deep) {
    sry4m::Header h;
    std::string err;
    if (parse(text, h, err, deep)) {
        std::string out = sry4m::scaled_header(h, 3);
        out.pop_back();
        printf("ok %d %d %s %s %s %d | %s\n", h.w, h.h, h.s444 ? "444" : h.s422 ? "422" : "420", h.left ? "left" : "center",
               h.full ? "full" : "limited", h.depth, out.c_str());
    } else {
        printf("refused %s\n", err.c_str());
    }
}

}  // namespace

int main(int argc, char** argv) {
    // 1. the headers given on the command line
    bool deep = true;
    for (int k = 1; k < argc; ++k) {
        if (!strcmp(argv[k], "--")) deep = false;
        else show(argv[k], deep);
    }
    // 2. every prefix of a full deep header, and that header with every single byte replaced by a space, a NUL and 0xff
    const std::string full = "YUV4MPEG2 W17 H13 F30000:1001 Ip A1:1 C422p10 XYSCSS=422P10 XCOLORRANGE=FULL";
    int accepted = 0, refused = 0, deep_seen = 0;
    for (size_t n = 0; n <= full.size(); ++n) {
        sry4m::Header h;
        std::string err;
        const bool ok = parse(full.substr(0, n), h, err, true);
        (ok ? accepted : refused)++;
        if (ok && h.depth > 8) ++deep_seen;
        if (ok && h.depth != 8 && !(h.depth == 10 && h.s422 && h.left && !h.s444)) return 4;  // a deep header is never half read
    }
    for (size_t i = 0; i < full.size(); ++i)
        for (const char ch : {' ', '\0', '\xff'}) {
            std::string s = full;
            s[i] = ch;
            sry4m::Header h;
            std::string err;
            const bool ok = parse(s, h, err, true);
            (ok ? accepted : refused)++;
            if (ok && h.depth != 8 && h.depth != 10) return 5;
            if (!ok && err.empty()) return 6;
        }
    printf("prefixes and mutations: %d accepted, %d refused, %d deep\n", accepted, refused, deep_seen);
    return 0;
}
