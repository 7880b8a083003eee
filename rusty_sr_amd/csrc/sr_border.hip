// sr_border.hip -- the two pixel moves of the border modes (include/srhip.h "Borders"; host side: sr_border.cpp).  Both are pure data
// movement on whole dwords: an RGBA8 pixel is one dword, an f32 RGB pixel three, and nothing is converted -- the GPU and the numpy
// restatement (tests/border_ref.py) agree byte for byte.
//
//   border_pad_kernel<E>   the (h + 2p) x (w + 2p) image of an h x w one under a border mode: output pixel (y, x) is source pixel
//                          (sr_border_index(y - p, h), sr_border_index(x - p, w)) -- the rule of sr_border.h, per axis, for any h, w >= 1.
//   border_crop_kernel<E>  the ch x cw window at (y0, x0) of an H x W image, as a contiguous image.
//
// E = dwords per pixel (1: RGBA8, 3: f32 RGB).  Both walk the OUTPUT row by row in groups of four dwords.  Neither image's rows need be
// multiples of 16 bytes and the buffers are only 4-byte aligned, so the groups are cut where the destination ADDRESS is a multiple of 16,
// row by row (as alpha_merge_kernel does): a whole group is one 16-byte store, the ragged ends of a row single dwords.  A whole group
// whose four source dwords are consecutive -- every group of a crop, the interior of a pad -- is one 16-byte load where the source
// address allows it too, else four dword loads; only a pad's border groups evaluate the index rule per dword.  A thread of a crop
// takes one group column of 4 consecutive rows, a thread of a pad one group; a workgroup 256 group columns.
//
// Every output dword belongs to exactly one thread, the grids are functions of the shape alone, there are no atomics: the same bits on
// every run.  The batch is folded into blockIdx.x.  All global offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_border.h"
#include "sr_internal.h"

namespace {

constexpr int kCropRows = 4;   // output rows per thread of a crop: four independent 16-byte loads in flight
constexpr int kPadRows = 1;    // ... of a pad: its launches are small (a padded LR image), and four times the threads hide the latency
                               // that four rows in turn would pay (1080p RGBA8: 8.5 -> 5.7 us)
constexpr int kGroups = 256;   // groups of four dwords across a workgroup

// four consecutive dwords at src (any 4-byte aligned address)
__device__ __forceinline__ uint4 load_run(const uint32_t* __restrict__ src) {
    if (((uintptr_t)src & 15u) == 0) return *(const uint4*)src;
    return make_uint4(src[0], src[1], src[2], src[3]);
}

template <int E>
__global__ __launch_bounds__(kGroups) void border_pad_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int h, int w, int p,
                                                             int mode, unsigned blocks_x, unsigned blocks_y) {
    const unsigned per_image = blocks_x * blocks_y;
    const unsigned img = blockIdx.x / per_image, b_in = blockIdx.x - img * per_image;
    const unsigned by = b_in / blocks_x, bx = b_in - by * blocks_x;
    const int OH = h + 2 * p;
    const long RW = ((long)w + 2 * p) * E, lo = (long)p * E, hi = ((long)p + w) * E;  // the output row in dwords; its straight-copy part
    const size_t word0 = (size_t)((uintptr_t)out >> 2);
    const long g = (long)bx * kGroups + threadIdx.x;
    // dword dd of the output row <- the source row's dword under the index rule
    auto mapped = [&](const uint32_t* __restrict__ src_row, long dd) {
        const int x = (int)(dd / E), c = (int)(dd - (long)x * E);
        return src_row[(size_t)sr_border_index(x - p, w, mode) * E + c];
    };
#pragma unroll
    for (int r = 0; r < kPadRows; ++r) {
        const int y = (int)by * kPadRows + r;
        if (y >= OH) break;
        const size_t row_word = ((size_t)img * OH + y) * (size_t)RW;
        const int shift = (int)((word0 + row_word) & 3u);  // dwords of this row in front of its first 16-byte boundary ... (4 - shift) & 3
        const long d = 4 * g - shift;
        if (d >= RW || d + 4 <= 0) continue;
        const uint32_t* __restrict__ src_row = in + ((size_t)img * h + sr_border_index(y - p, h, mode)) * (size_t)w * E;
        uint32_t* __restrict__ dst = out + row_word;
        if (d >= 0 && d + 4 <= RW) {
            uint4 v;
            if (d >= lo && d + 4 <= hi) v = load_run(src_row + (d - lo));
            else v = make_uint4(mapped(src_row, d), mapped(src_row, d + 1), mapped(src_row, d + 2), mapped(src_row, d + 3));
            *(uint4*)(dst + d) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (d + e >= 0 && d + e < RW) dst[d + e] = mapped(src_row, d + e);
        }
    }
}

template <int E>
__global__ __launch_bounds__(kGroups) void border_crop_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int H, int W, int y0,
                                                              int x0, int ch, int cw, unsigned blocks_x, unsigned blocks_y) {
    const unsigned per_image = blocks_x * blocks_y;
    const unsigned img = blockIdx.x / per_image, b_in = blockIdx.x - img * per_image;
    const unsigned by = b_in / blocks_x, bx = b_in - by * blocks_x;
    const long RW = (long)cw * E;
    const size_t word0 = (size_t)((uintptr_t)out >> 2);
    const long g = (long)bx * kGroups + threadIdx.x;
#pragma unroll
    for (int r = 0; r < kCropRows; ++r) {
        const int y = (int)by * kCropRows + r;
        if (y >= ch) break;
        const size_t row_word = ((size_t)img * ch + y) * (size_t)RW;
        const int shift = (int)((word0 + row_word) & 3u);
        const long d = 4 * g - shift;
        if (d >= RW || d + 4 <= 0) continue;
        const uint32_t* __restrict__ src = in + (((size_t)img * H + (size_t)(y0 + y)) * (size_t)W + (size_t)x0) * E;
        uint32_t* __restrict__ dst = out + row_word;
        if (d >= 0 && d + 4 <= RW) {
            *(uint4*)(dst + d) = load_run(src + d);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (d + e >= 0 && d + e < RW) dst[d + e] = src[d + e];
        }
    }
}

// workgroups for n images of `rows` rows of `row_dwords` dwords (one group more than the row's dwords need: a row that starts off a
// 16-byte boundary holds its dwords up to three places to the right)
size_t row_blocks(int n, size_t rows, size_t per_thread, size_t row_dwords, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    const size_t bx = (row_dwords + 3 + 4 * kGroups - 1) / (4 * kGroups), by = (rows + per_thread - 1) / per_thread;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    if (blocks_y_out) *blocks_y_out = (unsigned)by;
    return bx * by * (size_t)n;
}

}  // namespace

size_t sr_border_pad_blocks(bool f32, int n, int h, int w, int pad, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    if (n < 1 || h < 1 || w < 1 || pad < 0 || pad > SR_BORDER_PAD_MAX) return 0;
    return row_blocks(n, (size_t)h + 2 * pad, kPadRows, ((size_t)w + 2 * pad) * (f32 ? 3 : 1), blocks_x_out, blocks_y_out);
}

size_t sr_border_crop_blocks(bool f32, int n, int ch, int cw, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    if (n < 1 || ch < 1 || cw < 1) return 0;
    return row_blocks(n, (size_t)ch, kCropRows, (size_t)cw * (f32 ? 3 : 1), blocks_x_out, blocks_y_out);
}

hipError_t sr_launch_border_pad(const void* d_in, bool f32, int n, int h, int w, int mode, int pad, void* d_out, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_border_pad_blocks(f32, n, h, w, pad, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || mode < SR_BORDER_WRAP || mode > SR_BORDER_MIRROR) return hipErrorInvalidValue;
    if (h > INT32_MAX / 2 - 2 * SR_BORDER_PAD_MAX || w > INT32_MAX / 2 - 2 * SR_BORDER_PAD_MAX) return hipErrorInvalidValue;  // (sr_border.h: 2 size)
    const uint32_t* in = (const uint32_t*)d_in;
    uint32_t* out = (uint32_t*)d_out;
    if (f32) hipLaunchKernelGGL(border_pad_kernel<3>, dim3((unsigned)blocks), dim3(kGroups), 0, s, in, out, h, w, pad, mode, bx, by);
    else hipLaunchKernelGGL(border_pad_kernel<1>, dim3((unsigned)blocks), dim3(kGroups), 0, s, in, out, h, w, pad, mode, bx, by);
    return hipGetLastError();
}

hipError_t sr_launch_border_crop(const void* d_in, bool f32, int n, int H, int W, int y0, int x0, int ch, int cw, void* d_out, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_border_crop_blocks(f32, n, ch, cw, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    if (y0 < 0 || x0 < 0 || ch > H - y0 || cw > W - x0) return hipErrorInvalidValue;  // the window lies inside its image
    const uint32_t* in = (const uint32_t*)d_in;
    uint32_t* out = (uint32_t*)d_out;
    if (f32) hipLaunchKernelGGL(border_crop_kernel<3>, dim3((unsigned)blocks), dim3(kGroups), 0, s, in, out, H, W, y0, x0, ch, cw, bx, by);
    else hipLaunchKernelGGL(border_crop_kernel<1>, dim3((unsigned)blocks), dim3(kGroups), 0, s, in, out, H, W, y0, x0, ch, cw, bx, by);
    return hipGetLastError();
}
