// sr_yuv.hip -- the two colour conversions of the video path (include/srhip.h "Video"; host side: sr_yuv.cpp): planar 8-bit YCbCr
// frames, laid out like a Y4M frame payload, to the network's f32 RGB input, and the network's unquantised f32 output back to such a
// frame, quantised once.  tests/yuv_ref.py is the rule in numpy; all arithmetic here is f64 in the written order, the file is built
// without contraction (build.py FLAGS), the constants are formed on the host (sr_yuv.cpp), and there is no division: the kernels equal
// the restatement bit for bit.
//
//   yuv_to_rgb_kernel<S420, LEFT>   a thread makes 2 rows x 4 columns of RGB.  4:2:0: its 3 x 4 neighbourhood of either chroma plane (rows
//                                   i - 1 .. i + 1, columns 2g - 1 .. 2g + 2, addresses clamped to the plane) is read byte by byte -- the
//                                   planes start at any byte -- and the bilinear taps are compile-time indices into it: an integer sum of
//                                   wy wx C over 16.  A pixel is one 12-byte store; a thread's four pixels of a row are 48 consecutive bytes.
//   rgb_to_yuv_kernel<S420, LEFT>   the one that matters (1080p x 3: 224 MB read, 28 MB written).  A thread reads 2 rows x 4 columns of
//                                   f32 RGB, three 16-byte loads a row where the address allows (else dwords), so that the 2 x 2 chroma
//                                   block is thread-local; under the left siting column 2j - 1 of the thread's first block is its
//                                   neighbour's last column, passed through LDS (the first thread of a workgroup that is not the first of
//                                   its row reads that one pixel column again: 1 in 1024).  The bytes do not go to memory from the thread
//                                   that made them: the workgroup lays each of its runs -- two luma rows of up to 1024 bytes, one or two
//                                   rows of either chroma plane -- into LDS at the destination's offset within its dword, and after one
//                                   barrier stores whole aligned dwords; only the run's ragged head and tail are byte stores.
//
// Both grids: 256 threads = 1024 columns x 2 rows a workgroup, the batch and both axes folded into blockIdx.x, a function of the shape
// alone (sr_yuv_blocks).  Every output byte / dword belongs to exactly one thread, no atomics: the same bits on every run.  All global
// offsets are 64-bit.  Resources: profiles/video_kernel_resources.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 4;                       // columns per thread: 12 floats, three 16-byte groups
constexpr int kSpan = kThreads * kCols;        // columns per workgroup
constexpr int kRunWords = kSpan / 4 + 1;       // a run of kSpan bytes that starts up to 3 bytes into its first dword

struct BlockAt {
    unsigned img, by, bx;
};

__device__ __forceinline__ BlockAt block_at(unsigned blocks_x, unsigned blocks_y) {
    const unsigned per_image = blocks_x * blocks_y;
    BlockAt b;
    b.img = blockIdx.x / per_image;
    const unsigned in = blockIdx.x - b.img * per_image;
    b.by = in / blocks_x;
    b.bx = in - b.by * blocks_x;
    return b;
}

__device__ __forceinline__ double unit(double v) {  // clamp to [0, 1]; NaN -> 0
    v = v > 0.0 ? v : 0.0;
    return v < 1.0 ? v : 1.0;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- YCbCr -> RGB ---------------------------------------------------------------------------------------------------------------------
template <bool S420, bool LEFT>
__global__ __launch_bounds__(kThreads) void yuv_to_rgb_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int H, int W, size_t frame,
                                                              sr_yuv_rule k, unsigned blocks_x, unsigned blocks_y) {
    const BlockAt at = block_at(blocks_x, blocks_y);
    const int g = (int)at.bx * kThreads + (int)threadIdx.x, x0 = g * kCols, y0 = (int)at.by * 2;
    if (x0 >= W) return;
    const int CH = S420 ? (H + 1) / 2 : H, CW = S420 ? (W + 1) / 2 : W;
    const uint8_t* __restrict__ yp = in + (size_t)at.img * frame;
    const uint8_t* __restrict__ cbp = yp + (size_t)H * W;
    const uint8_t* __restrict__ crp = cbp + (size_t)CH * CW;
    // 4:2:0: 16 x the chroma at the thread's 2 x 4 pixels, exact integers
    int cb16[2][kCols], cr16[2][kCols];
    if (S420) {
        int nb[3][4], nr[3][4];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const size_t row = (size_t)clampi((int)at.by - 1 + r, CH - 1) * CW;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const size_t o = row + (size_t)clampi(2 * g - 1 + c, CW - 1);
                nb[r][c] = cbp[o];
                nr[r][c] = crp[o];
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int ra = r, rb = r + 1, wa = r ? 3 : 1, wb = r ? 1 : 3;  // row 2i: (i - 1, i) x (1, 3); row 2i + 1: (i, i + 1) x (3, 1)
#pragma unroll
            for (int c = 0; c < kCols; ++c) {
                const int j = 1 + (c >> 1), odd = c & 1;  // the neighbourhood's column of chroma sample x div 2
                const int ca = LEFT ? j : (odd ? j : j - 1), cc = LEFT ? (odd ? j + 1 : j) : (odd ? j + 1 : j);
                const int va = LEFT ? (odd ? 2 : 4) : (odd ? 3 : 1), vb = LEFT ? (odd ? 2 : 0) : (odd ? 1 : 3);
                cb16[r][c] = wa * (va * nb[ra][ca] + vb * nb[ra][cc]) + wb * (va * nb[rb][ca] + vb * nb[rb][cc]);
                cr16[r][c] = wa * (va * nr[ra][ca] + vb * nr[ra][cc]) + wb * (va * nr[rb][ca] + vb * nr[rb][cc]);
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
            const size_t o = (size_t)y * W + x;
            double cb, cr;
            if (S420) {
                cb = (double)cb16[r][c] * 0.0625;
                cr = (double)cr16[r][c] * 0.0625;
            } else {
                cb = (double)cbp[o];
                cr = (double)crp[o];
            }
            const double yy = ((double)yp[o] - k.oy) * k.sy;
            cb = (cb - 128.0) * k.sc;
            cr = (cr - 128.0) * k.sc;
            const double rr = yy + k.cr2 * cr;
            const double bb = yy + k.cb2 * cb;
            const double gg = ((yy - k.kr * rr) - k.kb * bb) * k.ig;
            v[3 * c] = (float)unit(rr);
            v[3 * c + 1] = (float)unit(gg);
            v[3 * c + 2] = (float)unit(bb);
        }
        float* __restrict__ dst = out + (((size_t)at.img * H + y) * (size_t)W + (size_t)x0) * 3;
#pragma unroll
        for (int c = 0; c < kCols; ++c)
            if (x0 + c < W) {  // a pixel is one 12-byte store, the thread's four are 48 consecutive bytes
                dst[3 * c] = v[3 * c];
                dst[3 * c + 1] = v[3 * c + 1];
                dst[3 * c + 2] = v[3 * c + 2];
            }
    }
}

// ---- RGB -> YCbCr ---------------------------------------------------------------------------------------------------------------------
struct Ycc {
    double y, cb, cr;  // Y', Cb', Cr' before rounding
};

__device__ __forceinline__ Ycc to_ycc(float rf, float gf, float bf, const sr_yuv_rule& k) {
    const double r = unit((double)rf), g = unit((double)gf), b = unit((double)bf);
    const double y = (k.kr * r + k.kg * g) + k.kb * b;
    const double cb = (b - y) * k.ib, cr = (r - y) * k.ir;
    Ycc o;
    o.y = k.oy + k.ky * y;
    o.cb = 128.0 + k.kc * cb;
    o.cr = 128.0 + k.kc * cr;
    return o;
}

__device__ __forceinline__ uint8_t to_byte(double v, double lo, double hi) {
    v = floor(v + 0.5);
    v = v > lo ? v : lo;
    v = v < hi ? v : hi;
    return (uint8_t)(int)v;
}

// One run of a workgroup: `len` bytes for global address dst, laid into LDS `shift` = dst & 3 bytes into its first dword
struct Run {
    uint8_t* dst;
    int len, shift;
};

__device__ __forceinline__ Run make_run(uint8_t* dst, int len) {
    Run r;
    r.dst = dst;
    r.len = len;
    r.shift = (int)((uintptr_t)dst & 3u);
    return r;
}

// whole aligned dwords from LDS to memory; the ragged head and tail byte by byte
__device__ __forceinline__ void store_run(const Run& r, const uint32_t* __restrict__ words) {
    if (r.len <= 0) return;
    const int end = r.shift + r.len;
    uint8_t* __restrict__ base = r.dst - r.shift;  // 4-byte aligned
    for (int d = (int)threadIdx.x; 4 * d < end; d += kThreads) {
        const int lo = 4 * d, hi = lo + 4;
        if (lo >= r.shift && hi <= end) {
            *(uint32_t*)(base + lo) = words[d];
        } else {
            const uint8_t* __restrict__ bytes = (const uint8_t*)words;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (lo + e >= r.shift && lo + e < end) base[lo + e] = bytes[lo + e];
        }
    }
}

template <bool S420, bool LEFT>
__global__ __launch_bounds__(kThreads) void rgb_to_yuv_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int H, int W, size_t frame,
                                                              sr_yuv_rule k, unsigned blocks_x, unsigned blocks_y) {
    // runs 0, 1: the two luma rows; 4:2:0: 2, 3 = Cb, Cr; 4:4:4: 2, 3 = Cb rows, 4, 5 = Cr rows
    __shared__ uint32_t words[6][kRunWords + 1];
    __shared__ double edge[LEFT && S420 ? kThreads : 1][4];  // the thread's last column: Cb', Cr' of row 0, of row 1
    const BlockAt at = block_at(blocks_x, blocks_y);
    const int tid = (int)threadIdx.x;
    const int bx0 = (int)at.bx * kSpan, x0 = bx0 + tid * kCols, y0 = (int)at.by * 2;
    const int CH = S420 ? (H + 1) / 2 : H, CW = S420 ? (W + 1) / 2 : W;
    const bool two = y0 + 1 < H;
    const int span = W - bx0 < kSpan ? W - bx0 : kSpan;  // the workgroup's columns
    uint8_t* __restrict__ yp = out + (size_t)at.img * frame;
    uint8_t* __restrict__ cbp = yp + (size_t)H * W;
    uint8_t* __restrict__ crp = cbp + (size_t)CH * CW;
    Run run[6];
    run[0] = make_run(yp + (size_t)y0 * W + bx0, span);
    run[1] = make_run(yp + (size_t)(y0 + 1) * W + bx0, two ? span : 0);
    if (S420) {
        const int cspan = (span + 1) / 2;  // (bx0 is even)
        const size_t co = (size_t)at.by * CW + (size_t)(bx0 / 2);
        run[2] = make_run(cbp + co, cspan);
        run[3] = make_run(crp + co, cspan);
        run[4] = make_run(nullptr, 0);
        run[5] = make_run(nullptr, 0);
    } else {
        const size_t co = (size_t)y0 * W + bx0;
        run[2] = make_run(cbp + co, span);
        run[3] = make_run(cbp + co + W, two ? span : 0);
        run[4] = make_run(crp + co, span);
        run[5] = make_run(crp + co + W, two ? span : 0);
    }
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
        // luma (and 4:4:4 chroma): one byte a pixel into the runs
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two) break;
#pragma unroll
            for (int c = 0; c < kCols; ++c) {
                if (x0 + c >= W) break;
                const int at_col = tid * kCols + c;
                ((uint8_t*)words[r])[run[r].shift + at_col] = to_byte(p[r][c].y, k.ylo, k.yhi);
                if (!S420) {
                    ((uint8_t*)words[2 + r])[run[2 + r].shift + at_col] = to_byte(p[r][c].cb, k.clo, k.chi);
                    ((uint8_t*)words[4 + r])[run[4 + r].shift + at_col] = to_byte(p[r][c].cr, k.clo, k.chi);
                }
            }
        }
        if (S420 && LEFT) {
            edge[tid][0] = p[0][kCols - 1].cb; edge[tid][1] = p[0][kCols - 1].cr;
            edge[tid][2] = p[1][kCols - 1].cb; edge[tid][3] = p[1][kCols - 1].cr;
        }
    }
    if (S420 && LEFT) __syncthreads();
    if (S420 && live) {
        double lcb[2], lcr[2];  // column 2j - 1 of the thread's first block, rows 0 and 1
        if (LEFT) {
            if (tid > 0) {
                lcb[0] = edge[tid - 1][0]; lcr[0] = edge[tid - 1][1]; lcb[1] = edge[tid - 1][2]; lcr[1] = edge[tid - 1][3];
            } else if (x0 == 0) {  // left of the image is its first column
                lcb[0] = p[0][0].cb; lcr[0] = p[0][0].cr; lcb[1] = p[1][0].cb; lcr[1] = p[1][0].cr;
            } else {  // the neighbouring workgroup's last column
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int y = r == 1 && !two ? y0 : y0 + r;
                    const float* __restrict__ s = in + (((size_t)at.img * H + (size_t)y) * (size_t)W + (size_t)(x0 - 1)) * 3;
                    const Ycc q = to_ycc(s[0], s[1], s[2], k);
                    lcb[r] = q.cb; lcr[r] = q.cr;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kCols / 2; ++j) {
            if (x0 + 2 * j >= W) break;
            const int a = 2 * j, b = 2 * j + 1;  // (a column beyond the row already holds the last one)
            double cb, cr;
            if (LEFT) {
                const double m0b = j ? p[0][a - 1].cb : lcb[0], m1b = j ? p[1][a - 1].cb : lcb[1];
                const double m0r = j ? p[0][a - 1].cr : lcr[0], m1r = j ? p[1][a - 1].cr : lcr[1];
                const double r0b = ((m0b + 2.0 * p[0][a].cb) + p[0][b].cb) * 0.25, r1b = ((m1b + 2.0 * p[1][a].cb) + p[1][b].cb) * 0.25;
                const double r0r = ((m0r + 2.0 * p[0][a].cr) + p[0][b].cr) * 0.25, r1r = ((m1r + 2.0 * p[1][a].cr) + p[1][b].cr) * 0.25;
                cb = (r0b + r1b) * 0.5;
                cr = (r0r + r1r) * 0.5;
            } else {
                cb = ((p[0][a].cb + p[0][b].cb) + (p[1][a].cb + p[1][b].cb)) * 0.25;
                cr = ((p[0][a].cr + p[0][b].cr) + (p[1][a].cr + p[1][b].cr)) * 0.25;
            }
            const int at_col = tid * (kCols / 2) + j;
            ((uint8_t*)words[2])[run[2].shift + at_col] = to_byte(cb, k.clo, k.chi);
            ((uint8_t*)words[3])[run[3].shift + at_col] = to_byte(cr, k.clo, k.chi);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < (S420 ? 4 : 6); ++r) store_run(run[r], words[r]);
}

template <class Launch>
hipError_t by_format(const sr_yuv_rule& k, Launch&& launch) {
    if (!k.sub420) launch(std::false_type{}, std::false_type{});
    else if (k.left) launch(std::true_type{}, std::true_type{});
    else launch(std::true_type{}, std::false_type{});
    return hipGetLastError();
}

}  // namespace

static size_t sr_yuv_blocks(int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    if (n < 1 || h < 1 || w < 1) return 0;
    const size_t bx = ((size_t)w + kSpan - 1) / kSpan, by = ((size_t)h + 1) / 2;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    if (blocks_y_out) *blocks_y_out = (unsigned)by;
    return bx * by * (size_t)n;
}

size_t sr_yuv_to_rgb_blocks(int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    return sr_yuv_blocks(n, h, w, blocks_x_out, blocks_y_out);
}

size_t sr_rgb_to_yuv_blocks(int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    return sr_yuv_blocks(n, h, w, blocks_x_out, blocks_y_out);
}

hipError_t sr_launch_yuv_to_rgb(const uint8_t* d_yuv, const sr_yuv_rule& k, int n, int h, int w, float* d_rgb, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_yuv_to_rgb_blocks(n, h, w, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || !sr_dword_aligned(d_rgb)) return hipErrorInvalidValue;
    const size_t frame = sr_yuv_rule_frame_bytes(k, h, w);
    return by_format(k, [&](auto s420, auto left) {
        hipLaunchKernelGGL((yuv_to_rgb_kernel<decltype(s420)::value, decltype(left)::value>), dim3((unsigned)blocks), dim3(kThreads), 0, s, d_yuv,
                           d_rgb, h, w, frame, k, bx, by);
    });
}

hipError_t sr_launch_rgb_to_yuv(const float* d_rgb, const sr_yuv_rule& k, int n, int h, int w, uint8_t* d_yuv, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_rgb_to_yuv_blocks(n, h, w, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || !sr_dword_aligned(d_rgb)) return hipErrorInvalidValue;
    const size_t frame = sr_yuv_rule_frame_bytes(k, h, w);
    return by_format(k, [&](auto s420, auto left) {
        hipLaunchKernelGGL((rgb_to_yuv_kernel<decltype(s420)::value, decltype(left)::value>), dim3((unsigned)blocks), dim3(kThreads), 0, s, d_rgb,
                           d_yuv, h, w, frame, k, bx, by);
    });
}
