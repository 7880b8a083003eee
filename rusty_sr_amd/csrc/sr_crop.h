// sr_crop.h -- the device helpers that cut a crop of a training step out of a source image (sr_train.hip's header comment has the rules):
// shared by the crop kernels of sr_train.hip and the degraded step's kernel of sr_degrade.hip, which cuts its HR crops with the same code.
// Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

__device__ __forceinline__ uint32_t word_at(const uint8_t* p) {  // the aligned dword that holds *p, shifted so that *p is byte 0
    const uint32_t mis = (uint32_t)(uintptr_t)p & 3u;
    return *(const uint32_t*)(p - mis) >> (8 * mis);
}

// pixel (p, q) of T_k(window) of descriptor d (k = d.k, any member), as 0x00bbggrr; 0 outside the source image
__device__ __forceinline__ uint32_t member_pixel(const sr_train_crop_desc& d, long p, long q, int crop_h, int crop_w) {
    if (d.k & 2) p = crop_h - 1 - p;
    if (d.k & 1) q = crop_w - 1 - q;
    const long sy = (long)d.y0 + ((d.k & 4) ? q : p), sx = (long)d.x0 + ((d.k & 4) ? p : q);
    if (sy < 0 || sy >= d.h || sx < 0 || sx >= d.w) return 0u;
    const uint8_t* s = d.px + (sy * d.w + sx) * d.ch;
    if (d.ch != 3) return *(const uint32_t*)s & 0xffffffu;  // RGBA: 4-byte aligned pixels
    const uint32_t mis = (uint32_t)(uintptr_t)s & 3u;
    const uint32_t* w = (const uint32_t*)(s - mis);
    const uint32_t w0 = w[0], w1 = mis >= 2 ? w[1] : 0u;  // (with mis >= 2, w[1] holds the pixel's last byte: inside the image)
    return __builtin_amdgcn_alignbyte(w1, w0, mis) & 0xffffffu;
}

// byte ob (0 .. cb-1) of a crop of descriptor d, crop rows of rowb bytes
__device__ __forceinline__ uint32_t crop_byte(const sr_train_crop_desc& d, long ob, long rowb, int crop_h, int crop_w) {
    const long y = ob / rowb, r = ob - y * rowb, x = r / 3;
    const int c = (int)(r - x * 3);
    if (d.k != 0) return (member_pixel(d, y, x, crop_h, crop_w) >> (8 * c)) & 0xffu;
    const long sy = (long)d.y0 + y, sx = (long)d.x0 + x;
    if (sy < 0 || sy >= d.h || sx < 0 || sx >= d.w) return 0u;
    return word_at(d.px + (sy * d.w + sx) * d.ch + c) & 0xffu;
}

// The dword (four bytes of the n x crop_h x crop_w x 3 RGB batch) number blockIdx-relative `t` of those whose first byte lies in crop b;
// desc(i): the descriptor of crop i.  *k: its index in the batch.  false: no such dword.
template <class Desc>
__device__ __forceinline__ bool crop_dword(Desc&& desc, int n, int b, long t, int crop_h, int crop_w, long* k_out, uint32_t* word_out) {
    const long rowb = (long)crop_w * 3, cb = (long)crop_h * rowb;
    const long base = (long)b * cb;
    const long k = (base + 3) / 4 + t;  // the dwords whose first byte lies in crop b
    if (4 * k >= base + cb) return false;
    const long o = 4 * k - base;
    const sr_train_crop_desc d = desc(b);
    const long y = o / rowb, xb = o - y * rowb;
    const long sy = (long)d.y0 + y, x = xb / 3, sx = (long)d.x0 + x;
    const int c = (int)(xb - x * 3);
    uint32_t word;
    // (member 0) the four bytes lie in one crop row and in pixels x, x + 1 of the source row sy
    if (d.k == 0 && xb + 4 <= rowb && sy >= 0 && sy < d.h && sx >= 0 && sx + 1 < d.w) {
        const uint8_t* p = d.px + (sy * d.w + sx) * d.ch;
        if (d.ch == 3) {
            p += c;
            const uint32_t mis = (uint32_t)(uintptr_t)p & 3u;
            const uint32_t* q = (const uint32_t*)(p - mis);
            const uint32_t w0 = q[0], w1 = mis ? q[1] : 0u;  // (with mis > 0, q[1] holds byte 3 of the run: inside the image)
            word = __builtin_amdgcn_alignbyte(w1, w0, mis);
        } else {  // RGBA, 4-byte aligned rows: pixels x and x + 1 as two words, alpha dropped
            const uint32_t* q = (const uint32_t*)p;
            const uint64_t rgb = (uint64_t)(q[0] & 0xffffffu) | ((uint64_t)(q[1] & 0xffffffu) << 24);
            word = (uint32_t)(rgb >> (8 * c));
        }
    } else if (d.k != 0 && xb + 4 <= rowb) {  // any other member: the four bytes lie in pixels x, x + 1 of the batch row y
        const uint64_t rgb = (uint64_t)member_pixel(d, y, x, crop_h, crop_w) | ((uint64_t)member_pixel(d, y, x + 1, crop_h, crop_w) << 24);
        word = (uint32_t)(rgb >> (8 * c));
    } else {  // (every member) a dword that touches an image edge or crosses a crop-row end
        word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            long ob = o + j;
            int bi = b;
            if (ob >= cb) {  // the dword runs on into the next crop (cb not a multiple of 4), or into the batch's padding
                ob -= cb;
                bi = b + 1;
                if (bi >= n) break;
            }
            word |= crop_byte(desc(bi), ob, rowb, crop_h, crop_w) << (8 * j);
        }
    }
    *k_out = k;
    *word_out = word;
    return true;
}

}  // namespace
