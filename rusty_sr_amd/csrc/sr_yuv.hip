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

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 4;                 // columns per thread: 12 floats, three 16-byte groups
constexpr int kSpan = kThreads * kCols;  // columns per workgroup

enum { S420 = SR_YUV_420, S444 = SR_YUV_444, S422 = SR_YUV_422 };  // sr_yuv_rule::sub

template <class S>
constexpr int kGroup = 16 / sizeof(S);  // samples in a 16-byte group
template <class S>
constexpr int kRunGroups = kSpan / kGroup<S> + 1;  // a run of up to kSpan samples that starts up to kGroup - 1 samples into its first group
// to RGB, a thread's row as three 16-byte stores: faster from deep samples, slower from bytes, the one choice S makes
template <class S>
constexpr bool kWideStore = sizeof(S) == 2;

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

// One run of a workgroup: `len` samples for global address p, laid into LDS `shift` = its offset in samples within its 16-byte group
template <class S>
struct Run {
    S* p;
    int len, shift;
};

template <class S>
__device__ __forceinline__ Run<S> make_run(S* p, int len) {
    Run<S> r;
    r.p = p;
    r.len = len;
    r.shift = (int)(((uintptr_t)p & 15u) / sizeof(S));
    return r;
}

// LDS -> memory: whole aligned groups inside the run as 16-byte stores, the ragged head and tail sample by sample
template <class S>
__device__ __forceinline__ void store_run(const Run<S>& r, const uint4* __restrict__ groups) {
    if (r.len <= 0) return;
    const int end = r.shift + r.len;
    S* __restrict__ base = r.p - r.shift;  // 16-byte aligned
    for (int d = (int)threadIdx.x; kGroup<S> * d < end; d += kThreads) {
        const int lo = kGroup<S> * d, hi = lo + kGroup<S>;
        if (lo >= r.shift && hi <= end) {
            *(uint4*)(base + lo) = groups[d];
        } else {
            const S* __restrict__ s = (const S*)groups;
#pragma unroll
            for (int e = 0; e < kGroup<S>; ++e)
                if (lo + e >= r.shift && lo + e < end) base[lo + e] = s[lo + e];
        }
    }
}

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
struct Ycc {
    double y, cb, cr;  // Y', Cb', Cr' before rounding
};

__device__ __forceinline__ Ycc to_ycc(float rf, float gf, float bf, const sr_yuv_rule& k) {
    const double r = unit((double)rf), g = unit((double)gf), b = unit((double)bf);
    const double y = (k.kr * r + k.kg * g) + k.kb * b;
    const double cb = (b - y) * k.ib, cr = (r - y) * k.ir;
    Ycc o;
    o.y = k.oy + k.ky * y;
    o.cb = k.mid + k.kc * cb;
    o.cr = k.mid + k.kc * cr;
    return o;
}

template <class S>
__device__ __forceinline__ S to_code(double v, double lo, double hi) {
    v = floor(v + 0.5);
    v = v > lo ? v : lo;
    v = v < hi ? v : hi;
    return (S)(int)v;
}

template <class S, int SUB, bool LEFT>
__global__ __launch_bounds__(kThreads) void rgb_to_yuv_kernel(const float* __restrict__ in, S* __restrict__ out, int H, int W, size_t frame,
                                                              sr_yuv_rule k, unsigned blocks_x, unsigned blocks_y) {
    // runs 0, 1: the two luma rows; 4:2:0: 2, 3 = Cb, Cr; 4:2:2 and 4:4:4: 2, 3 = Cb's rows, 4, 5 = Cr's rows
    constexpr int kRuns = SUB == S420 ? 4 : 6;
    constexpr bool kEdge = LEFT && SUB != S444;
    __shared__ uint4 lds[kRuns][kRunGroups<S>];
    __shared__ double edge[kEdge ? kThreads : 1][4];  // the thread's last column: Cb', Cr' of row 0, of row 1
    const BlockAt at = block_at(blocks_x, blocks_y);
    const int tid = (int)threadIdx.x;
    const int bx0 = (int)at.bx * kSpan, x0 = bx0 + tid * kCols, y0 = (int)at.by * 2;
    const int CH = SUB == S420 ? (H + 1) / 2 : H, CW = SUB == S444 ? W : (W + 1) / 2;
    const bool two = y0 + 1 < H;
    const int span = W - bx0 < kSpan ? W - bx0 : kSpan;  // the workgroup's columns
    S* __restrict__ yp = out + (size_t)at.img * frame;
    S* __restrict__ cbp = yp + (size_t)H * W;
    S* __restrict__ crp = cbp + (size_t)CH * CW;
    Run<S> run[kRuns];
    run[0] = make_run(yp + (size_t)y0 * W + bx0, span);
    run[1] = make_run(yp + (size_t)(y0 + 1) * W + bx0, two ? span : 0);
    if (SUB == S420) {
        const int cspan = (span + 1) / 2;  // (bx0 is even)
        const size_t co = (size_t)at.by * CW + (size_t)(bx0 / 2);
        run[2] = make_run(cbp + co, cspan);
        run[3] = make_run(crp + co, cspan);
    } else {
        const int cspan = SUB == S422 ? (span + 1) / 2 : span;
        const size_t co = (size_t)y0 * CW + (size_t)(SUB == S422 ? bx0 / 2 : bx0);
        run[2] = make_run(cbp + co, cspan);
        run[3] = make_run(cbp + co + CW, two ? cspan : 0);
        run[kRuns - 2] = make_run(crp + co, cspan);
        run[kRuns - 1] = make_run(crp + co + CW, two ? cspan : 0);
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
        // luma (and 4:4:4 chroma): one sample a pixel into the runs
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two) break;
#pragma unroll
            for (int c = 0; c < kCols; ++c) {
                if (x0 + c >= W) break;
                const int at_col = tid * kCols + c;
                ((S*)lds[r])[run[r].shift + at_col] = to_code<S>(p[r][c].y, k.ylo, k.yhi);
                if (SUB == S444) {
                    ((S*)lds[2 + r])[run[2 + r].shift + at_col] = to_code<S>(p[r][c].cb, k.clo, k.chi);
                    ((S*)lds[kRuns - 2 + r])[run[kRuns - 2 + r].shift + at_col] = to_code<S>(p[r][c].cr, k.clo, k.chi);
                }
            }
        }
        if (kEdge) {
            edge[tid][0] = p[0][kCols - 1].cb; edge[tid][1] = p[0][kCols - 1].cr;
            edge[tid][2] = p[1][kCols - 1].cb; edge[tid][3] = p[1][kCols - 1].cr;
        }
    }
    if (kEdge) __syncthreads();
    if (SUB != S444 && live) {
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
            double cb[2], cr[2];                 // the horizontally subsampled rows
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (LEFT) {
                    const double mb = j ? p[r][a - 1].cb : lcb[r], mr = j ? p[r][a - 1].cr : lcr[r];
                    cb[r] = ((mb + 2.0 * p[r][a].cb) + p[r][b].cb) * 0.25;
                    cr[r] = ((mr + 2.0 * p[r][a].cr) + p[r][b].cr) * 0.25;
                } else if (SUB == S422) {
                    cb[r] = (p[r][a].cb + p[r][b].cb) * 0.5;
                    cr[r] = (p[r][a].cr + p[r][b].cr) * 0.5;
                } else {
                    cb[r] = p[r][a].cb + p[r][b].cb;
                    cr[r] = p[r][a].cr + p[r][b].cr;
                }
            }
            const int at_col = tid * (kCols / 2) + j;
            if (SUB == S420) {
                const double vb = LEFT ? (cb[0] + cb[1]) * 0.5 : (cb[0] + cb[1]) * 0.25;
                const double vr = LEFT ? (cr[0] + cr[1]) * 0.5 : (cr[0] + cr[1]) * 0.25;
                ((S*)lds[2])[run[2].shift + at_col] = to_code<S>(vb, k.clo, k.chi);
                ((S*)lds[3])[run[3].shift + at_col] = to_code<S>(vr, k.clo, k.chi);
            } else {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (r == 1 && !two) break;
                    ((S*)lds[2 + r])[run[2 + r].shift + at_col] = to_code<S>(cb[r], k.clo, k.chi);
                    ((S*)lds[kRuns - 2 + r])[run[kRuns - 2 + r].shift + at_col] = to_code<S>(cr[r], k.clo, k.chi);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRuns; ++r) store_run(run[r], lds[r]);
}

// the forms that exist: 4:4:4, and 4:2:0 and (deep frames alone) 4:2:2 under either siting
template <class S, class Launch>
hipError_t by_format(const sr_yuv_rule& k, Launch&& launch) {
    using std::integral_constant;
    if (k.sub == S444) launch(integral_constant<int, S444>{}, std::false_type{});
    else if (k.sub == S420 && k.left) launch(integral_constant<int, S420>{}, std::true_type{});
    else if (k.sub == S420) launch(integral_constant<int, S420>{}, std::false_type{});
    else if constexpr (sizeof(S) == 1) return hipErrorInvalidValue;
    else if (k.left) launch(integral_constant<int, S422>{}, std::true_type{});
    else launch(integral_constant<int, S422>{}, std::false_type{});
    return hipGetLastError();
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
