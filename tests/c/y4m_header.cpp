// y4m_header.cpp -- the YUV4MPEG2 header parser of `rusty_sr video` (rusty_sr_amd/host/y4m.cpp) driven over well-formed, truncated and
// oversized headers: host code with its own main, built by tests/test_yuv_cpu.py plainly and under AddressSanitizer + UBSan.
// Each header is parsed from a heap buffer of exactly its length (no terminator), so that a read past its end is an error the
// sanitizer sees.  Prints one line a case: "ok W H 420|444 center|left limited|full | <scaled header>" or "refused <message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rusty_sr_amd/host/y4m.hpp"

namespace {

void show(const std::string& text) {
    char* buf = (char*)malloc(text.size() ? text.size() : 1);
    memcpy(buf, text.data(), text.size());
    sry4m::Header h;
    std::string err;
    if (sry4m::parse_header(buf, text.size(), h, err)) {
        std::string out = sry4m::scaled_header(h, 3);
        out.pop_back();
        printf("ok %d %d %s %s %s | %s\n", h.w, h.h, h.s444 ? "444" : "420", h.left ? "left" : "center", h.full ? "full" : "limited", out.c_str());
    } else {
        printf("refused %s\n", err.c_str());
    }
    free(buf);
}

}  // namespace

int main(int argc, char** argv) {
    // 1. the headers given on the command line
    for (int k = 1; k < argc; ++k) show(argv[k]);
    // 2. every prefix of a full header, and that header with every single byte replaced by a space, a NUL and 0xff
    const std::string full = "YUV4MPEG2 W17 H13 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL";
    int accepted = 0, refused = 0;
    for (size_t n = 0; n <= full.size(); ++n) {
        sry4m::Header h;
        std::string err;
        char* buf = (char*)malloc(n ? n : 1);
        memcpy(buf, full.data(), n);
        (sry4m::parse_header(buf, n, h, err) ? accepted : refused)++;
        free(buf);
    }
    for (size_t i = 0; i < full.size(); ++i)
        for (const char ch : {' ', '\0', '\xff'}) {
            std::string s = full;
            s[i] = ch;
            sry4m::Header h;
            std::string err;
            (sry4m::parse_header(s.data(), s.size(), h, err) ? accepted : refused)++;
        }
    // 3. oversized: a header line at the limit and one byte beyond it, a tag of 100 000 digits, and lines through read_line
    for (const size_t len : {sry4m::kMaxLine, sry4m::kMaxLine + 1, (size_t)100000}) {
        std::string s = "YUV4MPEG2 W4 H4 X";
        s.resize(len, 'x');
        sry4m::Header h;
        std::string err;
        const bool ok = sry4m::parse_header(s.data(), s.size(), h, err);
        printf("length %zu %s\n", len, ok ? "ok" : "refused");
    }
    show("YUV4MPEG2 W" + std::string(100000, '9') + " H4");
    for (const size_t len : {(size_t)0, (size_t)5, sry4m::kMaxLine, sry4m::kMaxLine + 1, (size_t)70000}) {
        for (const bool newline : {true, false}) {
            std::string s(len, 'F');
            if (newline) s += '\n';
            FILE* f = tmpfile();
            if (!f) return 3;
            fwrite(s.data(), 1, s.size(), f);
            rewind(f);
            std::string line;
            const int r = sry4m::read_line(f, line);
            printf("line %zu %s -> %d %zu\n", len, newline ? "nl" : "eof", r, line.size());
            fclose(f);
        }
    }
    printf("prefixes and mutations: %d accepted, %d refused\n", accepted, refused);
    printf("frame lines: %d %d %d %d\n", sry4m::is_frame_line("FRAME"), sry4m::is_frame_line("FRAME Ip"), sry4m::is_frame_line("FRAMES"),
           sry4m::is_frame_line("FRAM"));
    return 0;
}
