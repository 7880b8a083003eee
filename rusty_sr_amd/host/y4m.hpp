// y4m.hpp -- the YUV4MPEG2 stream header, as `rusty_sr video` reads and writes it (y4m.cpp).  No GPU, no library: host code alone, so
// that tests/c/y4m_header.cpp runs it under AddressSanitizer + UBSan.
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace sry4m {

constexpr size_t kMaxLine = 1024;    // a header or FRAME line longer than this is refused (the format's own limit is 80 for FRAME lines)
constexpr int kMaxAxis = 16384;      // W and H of an input stream

struct Header {
    int w = 0, h = 0;
    bool s444 = false;   // C444; else 4:2:0 (or 4:2:2: s422)
    bool s422 = false;   // C422p<depth>: only a deep stream, only under the `deep` overload
    int depth = 8;       // bits a sample; above 8 (9, 10, 12, 14, 16) the samples are little-endian 16-bit words
    bool left = false;   // C420mpeg2: chroma horizontally co-sited with the even columns; C420jpeg / C420 / no C tag: centred
    bool full = false;   // XCOLORRANGE=FULL
    std::vector<std::string> tags;  // every tag of the line in its order, W and H included, as written
};

// "YUV4MPEG2 W.. H.. [F.. I.. A.. C.. X..]" without its newline.  false: err names what is wrong -- a refused tag by its name.
bool parse_header(const char* line, size_t len, Header& out, std::string& err);
// The same with `deep` false.  With `deep` true (`rusty_sr video --depth auto`) the deep tags C420p<d>, C422p<d> and C444p<d>, d = 9, 10,
// 12, 14 or 16, are taken as well; their chroma (4:2:0, 4:2:2) is read as co-sited (`left`): the tags carry no siting, and that is what
// such streams carry.  8-bit C422, Cmono*, C420paldv and interlacing stay refused by name either way.
bool parse_header(const char* line, size_t len, Header& out, std::string& err, bool deep);
// the header line of the upscaled stream, newline included: every tag repeated, W and H multiplied by the factor
std::string scaled_header(const Header& h, int factor);
// the header line of a stream resampled to ow x oh, newline included: every tag repeated, W and H replaced.  The A tag keeps the DISPLAY
// aspect: absent, A0:0 (unknown) or malformed it passes through; else An:d becomes (n W oh):(d H ow) reduced by their gcd, in 64-bit
// arithmetic (terms too large for it pass through); a uniform resize (W oh == H ow) writes the tag it read, as written.
std::string sized_header(const Header& h, int ow, int oh);
// One line of at most kMaxLine bytes, without its newline.  1: read; 0: end of file before any byte; -1: a line that is too long or
// ends without a newline.
int read_line(FILE* f, std::string& line);
// a FRAME line: "FRAME" alone or followed by a space and parameters
bool is_frame_line(const std::string& line);

}  // namespace sry4m
