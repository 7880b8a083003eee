// yuv_rule_dump.cpp -- sr_yuv_rule.h driven from a plain C++ program (tests/test_yuv_rule_cpu.py): the header the conversion kernels and
// their host side compile is compiled here by g++ alone, and what it forms is printed for numpy to compare with tests/yuv_ref.py and
// tests/yuv16_ref.py bit for bit.
//
//   yuv_rule_dump   one line per format, every constant as a hex float, then the frame's samples at each of SHAPES:
//                     "8|16 <subsampling> <siting> <matrix> <range> <depth> ok sub left kr kb kg cr2 cb2 ir ib ig oy mid sy sc ky kc ylo yhi clo
//                     chi : n n n ..."  or  "... refused"
//                   8: through sr_yuv_rule_make, every value 0..2 of subsampling and matrix (2 is the deep format's alone), depth printed 8;
//                   16: through sr_yuv16_rule_make, depths 8..17 (8 and 17 are outside its values).
#include <cstdio>
#include <initializer_list>

#include "../../rusty_sr_amd/csrc/sr_yuv_rule.h"

static const int SHAPES[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 5}, {5, 3}, {17, 13}, {1080, 1920}, {3241, 5761}};

static void dump(int bits, int sub, int siting, int matrix, int range, int depth, bool ok, const sr_yuv_rule& k) {
    printf("%d %d %d %d %d %d ", bits, sub, siting, matrix, range, depth);
    if (!ok) {
        printf("refused\n");
        return;
    }
    printf("ok %d %d", k.sub, k.left);
    const double v[] = {k.kr, k.kb, k.kg, k.cr2, k.cb2, k.ir, k.ib, k.ig, k.oy, k.mid, k.sy, k.sc, k.ky, k.kc, k.ylo, k.yhi, k.clo, k.chi};
    for (double d : v) printf(" %a", d);
    printf(" :");
    for (const auto& s : SHAPES) printf(" %zu", sr_yuv_rule_frame_samples(k, s[0], s[1]));
    printf("\n");
}

int main() {
    sr_yuv_rule k;
    if (sr_yuv_rule_make(nullptr, &k) || sr_yuv16_rule_make(nullptr, &k)) return 1;  // a null format is refused
    for (int sub = 0; sub <= 2; ++sub)
        for (int siting = 0; siting <= 1; ++siting)
            for (int matrix = 0; matrix <= 2; ++matrix)
                for (int range = 0; range <= 1; ++range) {
                    const sr_yuv_format f8 = {sub, siting, matrix, range};
                    dump(8, sub, siting, matrix, range, 8, sr_yuv_rule_make(&f8, &k), k);
                    for (int depth = 8; depth <= 17; ++depth) {
                        const sr_yuv16_format f16 = {sub, siting, matrix, range, depth};
                        dump(16, sub, siting, matrix, range, depth, sr_yuv16_rule_make(&f16, &k), k);
                    }
                }
    // an enum outside its values, each field in turn
    for (int field = 0; field < 4; ++field)
        for (int bad : {-1, 3}) {
            int v[4] = {0, 0, 0, 0};
            v[field] = bad;
            const sr_yuv_format f8 = {v[0], v[1], v[2], v[3]};
            const sr_yuv16_format f16 = {v[0], v[1], v[2], v[3], 10};
            dump(8, v[0], v[1], v[2], v[3], 8, sr_yuv_rule_make(&f8, &k), k);
            dump(16, v[0], v[1], v[2], v[3], 10, sr_yuv16_rule_make(&f16, &k), k);
        }
    return 0;
}
