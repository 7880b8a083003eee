// sr_yuv_rule.h -- a YCbCr format as the conversion kernels take it (include/srhip.h "Video", "Deep video"): the constants of
// tests/yuv_ref.py and tests/yuv16_ref.py, the depth folded into them, each formed once on the host in f64 by a single operation (the
// kernels divide nowhere), and the frame's geometry.  One rule serves 8-bit and deep frames: an 8-bit format is the deep one at depth 8
// (s = 1, top = 255, mid = 128) with a narrower set of accepted enums.  Shared by sr_yuv.hip, sr_yuv.cpp and the host
// (tests/c/yuv_rule_dump.cpp compiles it with a plain C++ compiler and holds it to the two restatements bit for bit).  No HIP.
#pragma once

#include <stddef.h>

#include "../../include/srhip.h"

struct sr_yuv_rule {
    int sub, left;                  // SR_YUV_420 | SR_YUV_444 | SR_YUV_422; chroma horizontally co-sited with the even columns (else centred)
    double kr, kb, kg;              // the matrix; kg = 1 - kr - kb
    double cr2, cb2, ir, ib, ig;    // 2 (1 - kr), 2 (1 - kb) and their reciprocals, 1 / kg
    double oy, mid, sy, sc;         // YCbCr -> RGB: y = (Y - oy) sy, c = (C - mid) sc
    double ky, kc;                  // RGB -> YCbCr: Y' = oy + ky y, C' = mid + kc c
    double ylo, yhi, clo, chi;      // the range's limits
};

// the constants of valid values: what the two validators below have let through
inline sr_yuv_rule sr_yuv_rule_form(int subsampling, int siting, int matrix, int range, int depth) {
    sr_yuv_rule k{};
    const bool full = range == SR_YUV_FULL;
    k.sub = subsampling;
    k.left = k.sub != SR_YUV_444 && siting == SR_YUV_SITING_LEFT;
    k.kr = matrix == SR_YUV_BT2020 ? 0.2627 : matrix == SR_YUV_BT709 ? 0.2126 : 0.299;
    k.kb = matrix == SR_YUV_BT2020 ? 0.0593 : matrix == SR_YUV_BT709 ? 0.0722 : 0.114;
    k.kg = 1.0 - k.kr - k.kb;
    k.cr2 = 2.0 * (1.0 - k.kr);
    k.cb2 = 2.0 * (1.0 - k.kb);
    k.ir = 1.0 / k.cr2;
    k.ib = 1.0 / k.cb2;
    k.ig = 1.0 / k.kg;
    const double s = (double)(1 << (depth - 8)), top = (double)(1 << depth) - 1.0;  // powers of two: exact
    k.oy = full ? 0.0 : 16.0 * s;
    k.ky = full ? top : 219.0 * s;
    k.kc = full ? top : 224.0 * s;
    k.mid = full ? (double)(1 << (depth - 1)) : 128.0 * s;
    k.sy = 1.0 / k.ky;
    k.sc = 1.0 / k.kc;
    k.ylo = full ? 0.0 : 16.0 * s;
    k.yhi = full ? top : 235.0 * s;
    k.clo = full ? 0.0 : 16.0 * s;
    k.chi = full ? top : 240.0 * s;
    return k;
}

// false: a null format or an enum outside its values (4:2:2 and BT.2020 are the deep format's alone)
inline bool sr_yuv_rule_make(const sr_yuv_format* f, sr_yuv_rule* out) {
    if (!f) return false;
    if (f->subsampling != SR_YUV_420 && f->subsampling != SR_YUV_444) return false;
    if (f->siting != SR_YUV_SITING_CENTER && f->siting != SR_YUV_SITING_LEFT) return false;
    if (f->matrix != SR_YUV_BT601 && f->matrix != SR_YUV_BT709) return false;
    if (f->range != SR_YUV_LIMITED && f->range != SR_YUV_FULL) return false;
    *out = sr_yuv_rule_form(f->subsampling, f->siting, f->matrix, f->range, 8);
    return true;
}

// false: a null format, an enum outside its values, a depth outside 9..16
inline bool sr_yuv16_rule_make(const sr_yuv16_format* f, sr_yuv_rule* out) {
    if (!f) return false;
    if (f->subsampling != SR_YUV_420 && f->subsampling != SR_YUV_444 && f->subsampling != SR_YUV_422) return false;
    if (f->siting != SR_YUV_SITING_CENTER && f->siting != SR_YUV_SITING_LEFT) return false;
    if (f->matrix != SR_YUV_BT601 && f->matrix != SR_YUV_BT709 && f->matrix != SR_YUV_BT2020) return false;
    if (f->range != SR_YUV_LIMITED && f->range != SR_YUV_FULL) return false;
    if (f->depth < 9 || f->depth > 16) return false;
    *out = sr_yuv_rule_form(f->subsampling, f->siting, f->matrix, f->range, f->depth);
    return true;
}

// either chroma plane of a frame of h x w luma samples
inline void sr_yuv_rule_chroma(const sr_yuv_rule& k, size_t h, size_t w, size_t* ch, size_t* cw) {
    *ch = k.sub == SR_YUV_420 ? (h + 1) / 2 : h;
    *cw = k.sub == SR_YUV_444 ? w : (w + 1) / 2;
}

inline size_t sr_yuv_rule_frame_samples(const sr_yuv_rule& k, int h, int w) {
    size_t ch, cw;
    sr_yuv_rule_chroma(k, (size_t)h, (size_t)w, &ch, &cw);
    return (size_t)h * w + 2 * ch * cw;
}
