// reuse_plan_check.cpp -- the row-reuse planner of the frame stream (sr_video_reuse_plan, rusty_sr_amd/csrc/sr_plan.cpp) without a GPU and
// without Python: built by g++ from sr_plan.cpp alone, also under ASan and UBSan (tests/test_reuse_cpu.py).
//
// stdin: one case per line, "SUB H ROW ROW ..." -- the subsampling (SR_YUV_* number), the luma rows, and the plane rows that differ,
// numbered through the Y, the Cb and the Cr plane.  stdout, per case: "N Y0 Y1 Y0 Y1 ...", the plan.  Every plan is also held to the
// invariants a band pass needs (sorted, disjoint, even edges or H, no edge inside SR_HALO of an image edge, at most SR_REUSE_MAX_BANDS,
// every row within SR_HALO of an RGB-dirty row covered, the dirty rows taken straight from the chroma tap rule); a plan that breaks one
// ends the run with status 1.  The flag array is allocated at its exact size, so that a read past it is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../rusty_sr_amd/csrc/sr_plan.h"

namespace {

// the chroma rows luma row y reads under the 4:2:0 rule of include/srhip.h: 2i reads C[i-1], C[i]; 2i + 1 reads C[i], C[i+1]; clamped
void taps(int y, int ch, int out[2]) {
    const int i = y / 2;
    out[0] = y % 2 == 0 ? std::max(0, i - 1) : i;
    out[1] = y % 2 == 0 ? i : std::min(ch - 1, i + 1);
}

bool check(const std::vector<uint32_t>& flags, int sub, int h, const sr_row_band* b, int n) {
    const int ch = sub == SR_YUV_420 ? (h + 1) / 2 : h;
    if (n < 0 || n > SR_REUSE_MAX_BANDS) return false;
    for (int i = 0; i < n; ++i) {
        if (b[i].y0 < 0 || b[i].y0 >= b[i].y1 || b[i].y1 > h) return false;
        if (i && b[i].y0 < b[i - 1].y1) return false;
        if (b[i].y0 % 2 || (b[i].y1 % 2 && b[i].y1 != h)) return false;
        if ((b[i].y0 > 0 && b[i].y0 < SR_HALO) || (b[i].y1 < h && b[i].y1 > h - SR_HALO)) return false;
    }
    for (int y = 0; y < h; ++y) {
        bool dirty = flags[(size_t)y] != 0;
        for (int p = 0; p < 2; ++p) {
            const uint32_t* c = flags.data() + h + (size_t)p * ch;
            int t[2] = {y, y};
            if (sub == SR_YUV_420) taps(y, ch, t);
            dirty = dirty || c[t[0]] || c[t[1]];
        }
        if (!dirty) continue;
        for (int r = std::max(0, y - SR_HALO); r <= std::min(h - 1, y + SR_HALO); ++r) {
            bool in = false;
            for (int i = 0; i < n; ++i) in = in || (r >= b[i].y0 && r < b[i].y1);
            if (!in) return false;
        }
    }
    return true;
}

}  // namespace

int main() {
    std::string line;
    long cases = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream words(line);
        int sub = 0, h = 0;
        if (!(words >> sub >> h) || h < 1) { fprintf(stderr, "reuse_plan_check: bad case \"%s\"\n", line.c_str()); return 2; }
        const int ch = sub == SR_YUV_420 ? (h + 1) / 2 : h;
        std::vector<uint32_t> flags((size_t)h + 2 * (size_t)ch, 0u);
        for (long r; words >> r;) {
            if (r < 0 || r >= (long)flags.size()) { fprintf(stderr, "reuse_plan_check: row %ld outside the planes\n", r); return 2; }
            flags[(size_t)r] = 1u;
        }
        std::vector<sr_row_band> bands(SR_REUSE_MAX_BANDS);
        int n = -1;
        const int rc = sr_video_reuse_plan(flags.data(), sub, h, bands.data(), SR_REUSE_MAX_BANDS, &n);
        if (rc != SR_OK) { fprintf(stderr, "reuse_plan_check: status %d for \"%s\"\n", rc, line.c_str()); return 1; }
        if (!check(flags, sub, h, bands.data(), n)) { fprintf(stderr, "reuse_plan_check: a broken plan for \"%s\"\n", line.c_str()); return 1; }
        printf("%d", n);
        for (int i = 0; i < n; ++i) printf(" %d %d", bands[i].y0, bands[i].y1);
        printf("\n");
        ++cases;
    }
    // what the call refuses
    uint32_t one[3] = {0, 0, 0};
    sr_row_band b[SR_REUSE_MAX_BANDS];
    int n = 7;
    if (sr_video_reuse_plan(nullptr, SR_YUV_444, 1, b, SR_REUSE_MAX_BANDS, &n) != SR_E_INVALID || n != 0) return 1;
    if (sr_video_reuse_plan(one, SR_YUV_444, 0, b, SR_REUSE_MAX_BANDS, &n) != SR_E_INVALID) return 1;
    if (sr_video_reuse_plan(one, 3, 1, b, SR_REUSE_MAX_BANDS, &n) != SR_E_INVALID) return 1;
    if (sr_video_reuse_plan(one, SR_YUV_444, 1, nullptr, SR_REUSE_MAX_BANDS, &n) != SR_E_INVALID) return 1;
    if (sr_video_reuse_plan(one, SR_YUV_444, 1, b, 0, &n) != SR_E_INVALID) return 1;
    if (sr_video_reuse_plan(one, SR_YUV_444, 1, b, SR_REUSE_MAX_BANDS, nullptr) != SR_E_INVALID) return 1;
    fprintf(stderr, "reuse_plan_check: %ld cases\n", cases);
    return 0;
}
