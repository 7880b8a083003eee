// y4m_header_sized.cpp -- sry4m::sized_header (rusty_sr_amd/host/y4m.cpp), the header line `rusty_sr video --size / --scale` writes,
// driven over uniform and non-uniform sizes and over A tags that are absent, unknown, plain, malformed and large: host code with its own
// main, built by tests/test_video_sized_cpu.py plainly and under AddressSanitizer + UBSan.  The arguments are triples
// "<header>" <ow> <oh>; each header is parsed from a heap buffer of exactly its length.  Prints one line a case: the sized header
// without its newline, or "refused <message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../rusty_sr_amd/host/y4m.hpp"

int main(int argc, char** argv) {
    for (int k = 1; k + 2 < argc; k += 3) {
        const std::string text = argv[k];
        const int ow = atoi(argv[k + 1]), oh = atoi(argv[k + 2]);
        char* buf = (char*)malloc(text.size() ? text.size() : 1);
        memcpy(buf, text.data(), text.size());
        sry4m::Header h;
        std::string err;
        if (sry4m::parse_header(buf, text.size(), h, err, true)) {
            std::string out = sry4m::sized_header(h, ow, oh);
            const bool newline = !out.empty() && out.back() == '\n';
            if (newline) out.pop_back();
            printf("%s%s\n", out.c_str(), newline ? "" : " (no newline)");
            // scaled_header stays what it was: the factor's size, the tags as written
            std::string plain = sry4m::scaled_header(h, 3);
            plain.pop_back();
            printf("  x3: %s\n", plain.c_str());
        } else {
            printf("refused %s\n", err.c_str());
        }
        free(buf);
    }
    return 0;
}
