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

#include "sr_crop.h"
#include "sr_internal.h"

namespace {

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
