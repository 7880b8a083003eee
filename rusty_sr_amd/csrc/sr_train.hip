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
//
// Augmented steps (sr_train_step_aug / sr_train_step_pairs_aug): a descriptor carries its item's member k, and blocks along y are items,
// so the branch on k is uniform within a block.  k = 0 takes the path above, unchanged.  Any other member reads whole pixels: a batch
// dword lies in two neighbouring pixels (q, q + 1) of one batch row p, pixel (p, q) of T_k(W) is pixel (p', q') or (q', p') of the window
// W (p' / q': p / q reversed within the crop if k & 2 / k & 1; swapped if k & 4), and a pixel outside the image is 0.  A pixel is one
// aligned dword (RGBA) or the one or two aligned dwords that hold its three bytes (RGB): nothing outside the words of the image is read.
// The store is the same whole dword.  Neighbouring lanes read neighbouring pixels of a source row (k < 4, backwards when k & 1) or of a
// source column (k >= 4): the column reads are not coalesced.  Measured (DESIGN.md 4j "Augmentation"): every member class takes the
// 4.2 - 4.7 us a call (member 0: 4.4 us), 0.35 % of a step against a budget of 2 %, so the members have no LDS-tile form.
//
// A step on LR / HR pairs (sr_train_step_pairs) gathers both crops in one launch, train_pair_crop_kernel: the HR crops as above, and the LR
// crops -- cut by the same code, a crop of crop_lh x crop_lw at (y0, x0) of the LR image -- converted on the way (byte / 255, the
// validation pass's table) and stored as 16-byte groups straight into the backward pass's input buffer.  Such a step has no pool launch.
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

__global__ __launch_bounds__(256) void train_crop_kernel(sr_train_crop_args a, uint32_t* __restrict__ out) {
    long k;
    uint32_t word;
    if (crop_dword([&](int i) { return a.d[i]; }, a.n, blockIdx.y, (long)blockIdx.x * 256 + threadIdx.x, a.crop_h, a.crop_w, &k, &word))
        out[k] = word;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// A paired step's gather: blocks [0, hr_blocks) of a row cut item blockIdx.y's HR crop into the u8 batch as train_crop_kernel does; the
// others cut its LR crop the same way -- one thread per four consecutive values of the n x crop_lh x crop_lw x 3 batch -- and store it
// as img_to_data makes it (tab: 256 floats byte / 255), four floats at a time, at x: the network's input.  x holds whole 16-byte
// groups (its buffer is a multiple of 256 bytes).
template <int F>
__global__ __launch_bounds__(256) void train_pair_crop_kernel(sr_train_pair_args a, uint32_t* __restrict__ out, f32x4* __restrict__ x,
                                                              const float* __restrict__ tab) {
    long k;
    uint32_t word;
    if ((int)blockIdx.x < a.hr_blocks) {
        auto hr = [&](int i) {
            const sr_train_pair_desc& p = a.d[i];
            return sr_train_crop_desc{p.hr, p.hr_ch, F * p.lh, F * p.lw, F * p.y0, F * p.x0, p.k};
        };
        if (crop_dword(hr, a.n, blockIdx.y, (long)blockIdx.x * 256 + threadIdx.x, F * a.crop_lh, F * a.crop_lw, &k, &word)) out[k] = word;
        return;
    }
    __shared__ float s_tab[256];
    s_tab[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    auto lr = [&](int i) {
        const sr_train_pair_desc& p = a.d[i];
        return sr_train_crop_desc{p.lr, p.lr_ch, p.lh, p.lw, p.y0, p.x0, p.k};
    };
    if (!crop_dword(lr, a.n, blockIdx.y, (long)(blockIdx.x - a.hr_blocks) * 256 + threadIdx.x, a.crop_lh, a.crop_lw, &k, &word)) return;
    f32x4 v;
    v.x = s_tab[word & 0xffu];
    v.y = s_tab[(word >> 8) & 0xffu];
    v.z = s_tab[(word >> 16) & 0xffu];
    v.w = s_tab[word >> 24];
    x[k] = v;
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

hipError_t sr_launch_train_pair_crop(int factor, sr_train_pair_args a, uint32_t* d_out, float* d_x, const float* d_tab, hipStream_t s) {
    if (a.n < 1 || a.n > SR_TRAIN_MAX_BATCH || a.crop_lh < 1 || a.crop_lw < 1) return hipErrorInvalidValue;
    const long lr_vals = (long)a.crop_lh * a.crop_lw * 3, hr_bytes = lr_vals * factor * factor;
    a.hr_blocks = (int)((hr_bytes / 4 + 1 + 255) / 256);  // most dwords whose first byte lies in one crop
    const dim3 grid((unsigned)(a.hr_blocks + (lr_vals / 4 + 1 + 255) / 256), (unsigned)a.n);
    switch (factor) {
        case 2: hipLaunchKernelGGL(train_pair_crop_kernel<2>, grid, dim3(256), 0, s, a, d_out, (f32x4*)d_x, d_tab); break;
        case 3: hipLaunchKernelGGL(train_pair_crop_kernel<3>, grid, dim3(256), 0, s, a, d_out, (f32x4*)d_x, d_tab); break;
        case 4: hipLaunchKernelGGL(train_pair_crop_kernel<4>, grid, dim3(256), 0, s, a, d_out, (f32x4*)d_x, d_tab); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
