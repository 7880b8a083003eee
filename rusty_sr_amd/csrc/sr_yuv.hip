// sr_yuv.hip -- the two colour conversions of the video path (include/srhip.h "Video", "Deep video"; host side: sr_yuv.cpp): planar
// YCbCr frames, laid out like a Y4M frame payload, to the network's f32 RGB input, and the network's unquantised f32 output back to such
// a frame, quantised once.  A sample S is a byte (8-bit frames) or a little-endian uint16 (9..16 bits); both are the same two kernels.
// tests/yuv_ref.py and tests/yuv16_ref.py are the rule in numpy; all arithmetic here is f64 in the written order, the file is built
// without contraction (build.py FLAGS), the constants -- the depth is in them -- are formed on the host (sr_yuv_rule.h), and there is no
// division: the kernels equal the restatements bit for bit.
//
//   yuv_to_rgb_kernel<S, SUB, LEFT>   a thread makes 2 rows x 4 columns of RGB from its 2 x 4 luma samples and its chroma neighbourhood
//                                     (4:2:0: rows i - 1 .. i + 1, 4:2:2: its two rows; columns 2g - 1 .. 2g + 2, clamped to the plane);
//                                     the bilinear taps are compile-time indices into it: an exact integer sum over 16 (4:2:2: over 4).
//                                     The samples are read straight from memory, one by one: the planes start at any sample.  A
//                                     thread's four pixels of a row are 48 consecutive bytes: dword stores from bytes, three 16-byte
//                                     stores where the address allows from deep samples (kWideStore: measured).
//   rgb_to_yuv_kernel<S, SUB, LEFT>   the one that matters (1080p x 3: 224 MB read, 28 .. 112 MB written).  A thread reads 2 rows x 4
//                                     columns of f32 RGB, three 16-byte loads a row where the address allows (else dwords), so that the
//                                     2 x 2 chroma block is thread-local; under the left siting column 2j - 1 of the thread's first block
//                                     is its neighbour's last column, passed through LDS (the first thread of a workgroup that is not the
//                                     first of its row reads that one pixel column again: 1 in 1024).  The samples do not go to memory
//                                     from the thread that made them: the workgroup lays each of its runs -- two luma rows, one or two
//                                     rows of either chroma plane -- into LDS at the destination's offset within its 16-byte group and
//                                     after one barrier stores whole aligned groups; only a run's ragged head and tail are stored
//                                     sample by sample.
//
// Both grids: 256 threads = 1024 columns x 2 rows a workgroup, the batch and both axes folded into blockIdx.x, a function of the shape
// alone (sr_yuv_blocks).  Every output sample / group belongs to exactly one thread, no atomics: the same bits on every run.  All global
// offsets are 64-bit.  Resources: profiles/yuv_one_path_kernel_resources.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"
#include "sr_yuv_tile.h"

namespace {

// to RGB, a thread's row as three 16-byte stores: faster from deep samples, slower from bytes, the one choice S makes
template <class S>
constexpr bool kWideStore = sizeof(S) == 2;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- YCbCr -> RGB ---------------------------------------------------------------------------------------------------------------------
template <class S, int SUB, bool LEFT>
__global__ __launch_bounds__(kThreads) void yuv_to_rgb_kernel(const S* __restrict__ in, float* __restrict__ out, int H, int W, size_t frame,
                                                              sr_yuv_rule k, unsigned blocks_x, unsigned blocks_y) {
    constexpr int kRows = SUB == S420 ? 3 : 2;  // the chroma rows a thread reads: 4:2:0 i - 1, i, i + 1; 4:2:2 and 4:4:4 its two rows
    const BlockAt at = block_at(blocks_x, blocks_y);
    const int g = (int)at.bx * kThreads + (int)threadIdx.x, x0 = g * kCols, y0 = (int)at.by * 2;
    if (x0 >= W) return;
    const int CH = SUB == S420 ? (H + 1) / 2 : H, CW = SUB == S444 ? W : (W + 1) / 2;
    const bool two = y0 + 1 < H;
    const S* __restrict__ yp = in + (size_t)at.img * frame;
    const S* __restrict__ cbp = yp + (size_t)H * W;
    const S* __restrict__ crp = cbp + (size_t)CH * CW;
    // the rows the thread reads, each indexed by its plane's column (the row below the image is the last row, read and not stored)
    const S* yrow[2];
    const S* cbrow[kRows];
    const S* crrow[kRows];
#pragma unroll
    for (int r = 0; r < 2; ++r) yrow[r] = yp + (size_t)(two ? y0 + r : y0) * W;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int row = SUB == S420 ? clampi((int)at.by - 1 + r, CH - 1) : (two ? y0 + r : y0);
        cbrow[r] = cbp + (size_t)row * CW;
        crrow[r] = crp + (size_t)row * CW;
    }
    // the chroma at the thread's 2 x 4 pixels as exact integers: 16 x (4:2:0), 4 x (4:2:2); 4:4:4 reads its own below
    int cb_n[2][kCols], cr_n[2][kCols];
    if (SUB != S444) {
        int nb[kRows][4], nr[kRows][4];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = clampi(2 * g - 1 + c, CW - 1);
                nb[r][c] = cbrow[r][col];
                nr[r][c] = crrow[r][col];
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            // 4:2:0 row 2i: (i - 1, i) x (1, 3); row 2i + 1: (i, i + 1) x (3, 1).  4:2:2: the row itself
            const int ra = r, rb = SUB == S420 ? r + 1 : r, wa = r ? 3 : 1, wb = r ? 1 : 3;
#pragma unroll
            for (int c = 0; c < kCols; ++c) {
                const int j = 1 + (c >> 1), odd = c & 1;  // the neighbourhood's column of chroma sample x div 2
                const int ca = LEFT ? j : (odd ? j : j - 1), cc = odd ? j + 1 : j;
                const int va = LEFT ? (odd ? 2 : 4) : (odd ? 3 : 1), vb = LEFT ? (odd ? 2 : 0) : (odd ? 1 : 3);
                if (SUB == S420) {
                    cb_n[r][c] = wa * (va * nb[ra][ca] + vb * nb[ra][cc]) + wb * (va * nb[rb][ca] + vb * nb[rb][cc]);
                    cr_n[r][c] = wa * (va * nr[ra][ca] + vb * nr[ra][cc]) + wb * (va * nr[rb][ca] + vb * nr[rb][cc]);
                } else {
                    cb_n[r][c] = va * nb[ra][ca] + vb * nb[ra][cc];
                    cr_n[r][c] = va * nr[ra][ca] + vb * nr[ra][cc];
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (y >= H) break;
        float v[kCols * 3];
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const int x = x0 + c < W ? x0 + c : W - 1;  // (a column beyond the row is computed from the last one and not stored)
            double cb, cr;
            if (SUB == S444) {
                cb = (double)cbrow[r][x];
                cr = (double)crrow[r][x];
            } else {
                const double scale = SUB == S420 ? 0.0625 : 0.25;
                cb = (double)cb_n[r][c] * scale;
                cr = (double)cr_n[r][c] * scale;
            }
            const double yy = ((double)yrow[r][x] - k.oy) * k.sy;
            cb = (cb - k.mid) * k.sc;
            cr = (cr - k.mid) * k.sc;
            const double rr = yy + k.cr2 * cr;
            const double bb = yy + k.cb2 * cb;
            const double gg = ((yy - k.kr * rr) - k.kb * bb) * k.ig;
            v[3 * c] = (float)unit(rr);
            v[3 * c + 1] = (float)unit(gg);
            v[3 * c + 2] = (float)unit(bb);
        }
        float* __restrict__ dst = out + (((size_t)at.img * H + y) * (size_t)W + (size_t)x0) * 3;
        if (kWideStore<S> && x0 + kCols <= W && ((uintptr_t)dst & 15u) == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) ((float4*)dst)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (int c = 0; c < kCols; ++c)
                if (x0 + c < W) {  // a pixel is one 12-byte store, the thread's four are 48 consecutive bytes
                    dst[3 * c] = v[3 * c];
                    dst[3 * c + 1] = v[3 * c + 1];
                    dst[3 * c + 2] = v[3 * c + 2];
                }
        }
    }
}

// ---- RGB -> YCbCr ---------------------------------------------------------------------------------------------------------------------
template <class S, int SUB, bool LEFT>
__global__ __launch_bounds__(kThreads) void rgb_to_yuv_kernel(const float* __restrict__ in, S* __restrict__ out, int H, int W, size_t frame,
                                                              sr_yuv_rule k, unsigned blocks_x, unsigned blocks_y) {
    constexpr bool kEdge = LEFT && SUB != S444;
    __shared__ uint4 lds[kRuns<SUB>][kRunGroups<S>];
    __shared__ double edge[kEdge ? kThreads : 1][4];  // the thread's last column: Cb', Cr' of row 0, of row 1
    const BlockAt at = block_at(blocks_x, blocks_y);
    const int tid = (int)threadIdx.x;
    const int bx0 = (int)at.bx * kSpan, x0 = bx0 + tid * kCols, y0 = (int)at.by * 2;
    const bool two = y0 + 1 < H;
    const int span = W - bx0 < kSpan ? W - bx0 : kSpan;  // the workgroup's columns
    Run<S> run[kRuns<SUB>];
    tile_runs<S, SUB>(run, out, frame, at.img, at.by, H, W, bx0, span, two);
    Ycc p[2][kCols];
    const bool live = x0 < W;
    if (live) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two) {  // the row below the image is the last row
#pragma unroll
                for (int c = 0; c < kCols; ++c) p[1][c] = p[0][c];
                break;
            }
            const float* __restrict__ src = in + (((size_t)at.img * H + (size_t)(y0 + r)) * (size_t)W + (size_t)x0) * 3;
            float v[kCols * 3];
            if (x0 + kCols <= W) {
                if (((uintptr_t)src & 15u) == 0) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const float4 t = ((const float4*)src)[q];
                        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < kCols * 3; ++e) v[e] = src[e];
                }
            } else {  // the ragged end of a row: a column beyond it is the last one
#pragma unroll
                for (int c = 0; c < kCols; ++c) {
                    const int cc = x0 + c < W ? c : W - 1 - x0;
                    v[3 * c] = src[3 * cc]; v[3 * c + 1] = src[3 * cc + 1]; v[3 * c + 2] = src[3 * cc + 2];
                }
            }
#pragma unroll
            for (int c = 0; c < kCols; ++c) p[r][c] = to_ycc(v[3 * c], v[3 * c + 1], v[3 * c + 2], k);
        }
    }
    tile_store<S, SUB, LEFT>(p, live, two, x0, W, k, run, lds, edge, [&](int r) {  // the neighbouring workgroup's last column
        const int y = r == 1 && !two ? y0 : y0 + r;
        const float* __restrict__ s = in + (((size_t)at.img * H + (size_t)y) * (size_t)W + (size_t)(x0 - 1)) * 3;
        return to_ycc(s[0], s[1], s[2], k);
    });
}

}  // namespace

size_t sr_yuv_blocks(int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    if (n < 1 || h < 1 || w < 1) return 0;
    const size_t bx = ((size_t)w + kSpan - 1) / kSpan, by = ((size_t)h + 1) / 2;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    if (blocks_y_out) *blocks_y_out = (unsigned)by;
    return bx * by * (size_t)n;
}

template <class S>
hipError_t sr_launch_yuv_to_rgb(const S* d_yuv, const sr_yuv_rule& k, int n, int h, int w, float* d_rgb, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_yuv_blocks(n, h, w, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || !sr_dword_aligned(d_rgb) || ((uintptr_t)d_yuv & (alignof(S) - 1))) return hipErrorInvalidValue;
    const size_t frame = sr_yuv_rule_frame_samples(k, h, w);
    return by_format<S>(k, [&](auto sub, auto left) {
        hipLaunchKernelGGL((yuv_to_rgb_kernel<S, decltype(sub)::value, decltype(left)::value>), dim3((unsigned)blocks), dim3(kThreads), 0, s, d_yuv,
                           d_rgb, h, w, frame, k, bx, by);
    });
}

template <class S>
hipError_t sr_launch_rgb_to_yuv(const float* d_rgb, const sr_yuv_rule& k, int n, int h, int w, S* d_yuv, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_yuv_blocks(n, h, w, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || !sr_dword_aligned(d_rgb) || ((uintptr_t)d_yuv & (alignof(S) - 1))) return hipErrorInvalidValue;
    const size_t frame = sr_yuv_rule_frame_samples(k, h, w);
    return by_format<S>(k, [&](auto sub, auto left) {
        hipLaunchKernelGGL((rgb_to_yuv_kernel<S, decltype(sub)::value, decltype(left)::value>), dim3((unsigned)blocks), dim3(kThreads), 0, s, d_rgb,
                           d_yuv, h, w, frame, k, bx, by);
    });
}

template hipError_t sr_launch_yuv_to_rgb<uint8_t>(const uint8_t*, const sr_yuv_rule&, int, int, int, float*, hipStream_t);
template hipError_t sr_launch_yuv_to_rgb<uint16_t>(const uint16_t*, const sr_yuv_rule&, int, int, int, float*, hipStream_t);
template hipError_t sr_launch_rgb_to_yuv<uint8_t>(const float*, const sr_yuv_rule&, int, int, int, uint8_t*, hipStream_t);
template hipError_t sr_launch_rgb_to_yuv<uint16_t>(const float*, const sr_yuv_rule&, int, int, int, uint16_t*, hipStream_t);
