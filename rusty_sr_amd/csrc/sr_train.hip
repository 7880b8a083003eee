// sr_train.hip -- the crop gather of a training step (include/srhip.h sr_train_step): the reference's ImageFolderSupplier cuts one random
// crop of each drawn image on the host (main.rs:207-216); here the n crops of a step are cut on the device, from images already there, into
// one contiguous n x crop_h x crop_w x 3 u8 batch that sr_backprop_rgba8_dev then reads.  Alpha is dropped; pixels outside the source image
// are 0.
//
// One thread per output dword (four bytes of the RGB batch, crossing pixel boundaries), so every store is a whole, coalesced dword.  The
// loads are aligned dwords as well: a crop row of an RGB source is a contiguous byte run (two aligned words, shifted into place with
// v_alignbyte); of an RGBA source two whole pixels.  Dwords that touch an image edge or a crop-row end take the byte-wise path (each byte
// from the aligned word that holds it: nothing outside the words of the image is read).  The descriptors arrive by value (kernel
// arguments), so a step whose images are all resident uploads nothing.  Blocks along y are items, so each block reads its descriptor with
// scalar loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

__device__ __forceinline__ uint32_t word_at(const uint8_t* p) {  // the aligned dword that holds *p, shifted so that *p is byte 0
    const uint32_t mis = (uint32_t)(uintptr_t)p & 3u;
    return *(const uint32_t*)(p - mis) >> (8 * mis);
}

// byte ob (0 .. cb-1) of a crop of descriptor d, crop rows of rowb bytes
__device__ __forceinline__ uint32_t crop_byte(const sr_train_crop_desc& d, long ob, long rowb) {
    const long y = ob / rowb, r = ob - y * rowb, x = r / 3;
    const int c = (int)(r - x * 3);
    const long sy = (long)d.y0 + y, sx = (long)d.x0 + x;
    if (sy < 0 || sy >= d.h || sx < 0 || sx >= d.w) return 0u;
    return word_at(d.px + (sy * d.w + sx) * d.ch + c) & 0xffu;
}

__global__ __launch_bounds__(256) void train_crop_kernel(sr_train_crop_args a, uint32_t* __restrict__ out) {
    const int b = blockIdx.y;
    const long rowb = (long)a.crop_w * 3, cb = (long)a.crop_h * rowb;
    const long base = (long)b * cb;
    const long k = (base + 3) / 4 + (long)blockIdx.x * 256 + threadIdx.x;  // the dwords whose first byte lies in crop b
    if (4 * k >= base + cb) return;
    const long o = 4 * k - base;
    const sr_train_crop_desc& d = a.d[b];
    const long y = o / rowb, xb = o - y * rowb;
    const long sy = (long)d.y0 + y, x = xb / 3, sx = (long)d.x0 + x;
    const int c = (int)(xb - x * 3);
    uint32_t word;
    // the four bytes lie in one crop row and in pixels x, x + 1 of the source row sy
    if (xb + 4 <= rowb && sy >= 0 && sy < d.h && sx >= 0 && sx + 1 < d.w) {
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
    } else {
        word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            long ob = o + j;
            int bi = b;
            if (ob >= cb) {  // the dword runs on into the next crop (cb not a multiple of 4), or into the batch's padding
                ob -= cb;
                bi = b + 1;
                if (bi >= a.n) break;
            }
            word |= crop_byte(a.d[bi], ob, rowb) << (8 * j);
        }
    }
    out[k] = word;
}

}  // namespace

hipError_t sr_launch_train_crop(const sr_train_crop_args& a, uint32_t* d_out, hipStream_t s) {
    if (a.n < 1 || a.n > SR_TRAIN_MAX_BATCH || a.crop_h < 1 || a.crop_w < 1) return hipErrorInvalidValue;
    const long cb = (long)a.crop_h * a.crop_w * 3;
    const long dwords = cb / 4 + 1;  // most dwords whose first byte lies in one crop
    const dim3 grid((unsigned)((dwords + 255) / 256), (unsigned)a.n);
    hipLaunchKernelGGL(train_crop_kernel, grid, dim3(256), 0, s, a, d_out);
    return hipGetLastError();
}
