// sr_yuv16.hip -- the two colour conversions of the deep video path (include/srhip.h "Deep video"; host side: sr_yuv16.cpp): planar
// YCbCr frames of 9..16-bit samples in little-endian uint16, laid out like a Y4M frame payload, to the network's f32 RGB input, and the
// network's unquantised f32 output back to such a frame, quantised once.  tests/yuv16_ref.py is the rule in numpy; all arithmetic here
// is f64 in the written order, the file is built without contraction (build.py FLAGS), the constants -- the depth is in them -- are
// formed on the host (sr_yuv16.cpp), and there is no division: the kernels equal the restatement bit for bit.  The 8-bit pair
// (sr_yuv.hip) is untouched; what differs here is that samples sit at even addresses, so memory is moved in 16-byte groups both ways.
//
//   yuv16_to_rgb_kernel<SUB, LEFT>  the workgroup's runs -- two luma rows of up to 1024 samples and its chroma neighbourhood (4:2:0: rows
//                                   i - 1 .. i + 1, 4:2:2 / 4:4:4: its two rows; columns one beyond either end, clamped to the plane) --
//                                   enter LDS at the source's offset within its 16-byte group: whole aligned groups as 16-byte loads,
//                                   only a run's ragged head and tail as 2-byte loads.  After one barrier a thread makes 2 rows x 4
//                                   columns of RGB; its 3 x 4 (4:2:2: 2 x 4) chroma samples come from LDS at clamped columns and the taps
//                                   are compile-time indices into them: an exact integer sum over 16 (4:2:2: over 4).  A thread's four
//                                   pixels of a row leave as three 16-byte stores where the address allows, else as dwords.
//   rgb_to_yuv16_kernel<SUB, LEFT>  the one that matters (1080p x 3: 224 MB read, 56 / 75 / 112 MB written).  Reads as the 8-bit kernel:
//                                   2 rows x 4 columns of f32 RGB a thread, three 16-byte loads a row where the address allows, the
//                                   co-sited neighbour column through LDS.  The workgroup lays each of its runs into LDS at the
//                                   destination's offset within its 16-byte group (0..7 samples) and after one barrier stores whole
//                                   aligned 16-byte groups; only a run's ragged head and tail are 2-byte stores.
//
// Both grids: 256 threads = 1024 columns x 2 rows a workgroup, the batch and both axes folded into blockIdx.x, a function of the shape
// alone (sr_yuv16_blocks).  Every output sample / group belongs to exactly one thread, no atomics: the same bits on every run.  All
// global offsets are 64-bit.  Resources: profiles/video_deep_kernel_resources.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 4;                        // columns per thread: 12 floats, three 16-byte groups
constexpr int kSpan = kThreads * kCols;         // columns per workgroup
constexpr int kGroup = 8;                       // samples in a 16-byte group
constexpr int kRunGroups = kSpan / kGroup + 1;  // a run of up to kSpan samples that starts up to 7 samples into its first group
constexpr int kHood = kSpan / 2 + 2;            // chroma columns a workgroup's neighbourhood can span (4:2:0, 4:2:2)

enum { S420 = 0, S444 = 1, S422 = 2 };  // sr_yuv16_rule::sub, the SR_YUV_* numbers

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

// One run of a workgroup: `len` samples at global address p, held in LDS `shift` = its offset in samples within its 16-byte group
struct Run {
    uint16_t* p;
    int len, shift;
};

__device__ __forceinline__ Run make_run(const uint16_t* p, int len) {
    Run r;
    r.p = const_cast<uint16_t*>(p);
    r.len = len;
    r.shift = (int)(((uintptr_t)p & 15u) >> 1);
    return r;
}

// memory -> LDS: whole aligned groups inside the run as 16-byte loads, the ragged head and tail sample by sample
__device__ __forceinline__ void load_run(const Run& r, uint4* __restrict__ groups) {
    if (r.len <= 0) return;
    const int end = r.shift + r.len;
    const uint16_t* __restrict__ base = r.p - r.shift;  // 16-byte aligned
    for (int d = (int)threadIdx.x; kGroup * d < end; d += kThreads) {
        const int lo = kGroup * d, hi = lo + kGroup;
        if (lo >= r.shift && hi <= end) {
            groups[d] = *(const uint4*)(base + lo);
        } else {
            uint16_t* __restrict__ s = (uint16_t*)groups;
#pragma unroll
            for (int e = 0; e < kGroup; ++e)
                if (lo + e >= r.shift && lo + e < end) s[lo + e] = base[lo + e];
        }
    }
}

// LDS -> memory, the same way
__device__ __forceinline__ void store_run(const Run& r, const uint4* __restrict__ groups) {
    if (r.len <= 0) return;
    const int end = r.shift + r.len;
    uint16_t* __restrict__ base = r.p - r.shift;  // 16-byte aligned
    for (int d = (int)threadIdx.x; kGroup * d < end; d += kThreads) {
        const int lo = kGroup * d, hi = lo + kGroup;
        if (lo >= r.shift && hi <= end) {
            *(uint4*)(base + lo) = groups[d];
        } else {
            const uint16_t* __restrict__ s = (const uint16_t*)groups;
#pragma unroll
            for (int e = 0; e < kGroup; ++e)
                if (lo + e >= r.shift && lo + e < end) base[lo + e] = s[lo + e];
        }
    }
}

// ---- YCbCr -> RGB ---------------------------------------------------------------------------------------------------------------------
template <int SUB, bool LEFT>
__global__ __launch_bounds__(kThreads) void yuv16_to_rgb_kernel(const uint16_t* __restrict__ in, float* __restrict__ out, int H, int W, size_t frame,
                                                                sr_yuv16_rule k, unsigned blocks_x, unsigned blocks_y) {
    // runs 0, 1: the two luma rows; then Cb's rows, then Cr's: 4:2:0 three each (i - 1, i, i + 1), 4:2:2 and 4:4:4 two each
    constexpr int kRows = SUB == S420 ? 3 : 2;
    __shared__ uint4 lds[2 + 2 * kRows][kRunGroups];
    const BlockAt at = block_at(blocks_x, blocks_y);
    const int tid = (int)threadIdx.x;
    const int g = (int)at.bx * kThreads + tid, bx0 = (int)at.bx * kSpan, x0 = bx0 + tid * kCols, y0 = (int)at.by * 2;
    const int CH = SUB == S420 ? (H + 1) / 2 : H, CW = SUB == S444 ? W : (W + 1) / 2;
    const bool two = y0 + 1 < H;
    const int span = W - bx0 < kSpan ? W - bx0 : kSpan;  // the workgroup's columns
    const uint16_t* __restrict__ yp = in + (size_t)at.img * frame;
    const uint16_t* __restrict__ cbp = yp + (size_t)H * W;
    const uint16_t* __restrict__ crp = cbp + (size_t)CH * CW;
    // the chroma columns the workgroup holds: [cs, ce)
    const int cs = SUB == S444 ? bx0 : (bx0 / 2 > 0 ? bx0 / 2 - 1 : 0);
    const int ce = SUB == S444 ? bx0 + span : (bx0 / 2 + kHood - 1 < CW ? bx0 / 2 + kHood - 1 : CW);
    Run run[2 + 2 * kRows];
    run[0] = make_run(yp + (size_t)y0 * W + bx0, span);
    run[1] = make_run(yp + (size_t)(y0 + 1) * W + bx0, two ? span : 0);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int row = SUB == S420 ? clampi((int)at.by - 1 + r, CH - 1) : y0 + r;
        const size_t o = (size_t)row * CW + (size_t)cs;
        const int len = SUB == S420 || r == 0 || two ? ce - cs : 0;
        run[2 + r] = make_run(cbp + o, len);
        run[2 + kRows + r] = make_run(crp + o, len);
    }
#pragma unroll
    for (int r = 0; r < 2 + 2 * kRows; ++r) load_run(run[r], lds[r]);
    __syncthreads();
    if (x0 >= W) return;
    // the chroma at the thread's 2 x 4 pixels as exact integers: 16 x (4:2:0), 4 x (4:2:2), 1 x (4:4:4)
    int cb_n[2][kCols], cr_n[2][kCols];
    if (SUB != S444) {
        int nb[kRows][4], nr[kRows][4];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const uint16_t* __restrict__ sb = (const uint16_t*)lds[2 + r] + run[2 + r].shift - cs;
            const uint16_t* __restrict__ sr = (const uint16_t*)lds[2 + kRows + r] + run[2 + kRows + r].shift - cs;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = clampi(2 * g - 1 + c, CW - 1);
                nb[r][c] = sb[col];
                nr[r][c] = sr[col];
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
        const uint16_t* __restrict__ sy = (const uint16_t*)lds[r] + run[r].shift - bx0;
        float v[kCols * 3];
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const int x = x0 + c < W ? x0 + c : W - 1;  // (a column beyond the row is computed from the last one and not stored)
            double cb, cr;
            if (SUB == S444) {
                cb = (double)((const uint16_t*)lds[2 + r] + run[2 + r].shift - bx0)[x];
                cr = (double)((const uint16_t*)lds[4 + r] + run[4 + r].shift - bx0)[x];
            } else {
                const double scale = SUB == S420 ? 0.0625 : 0.25;
                cb = (double)cb_n[r][c] * scale;
                cr = (double)cr_n[r][c] * scale;
            }
            const double yy = ((double)sy[x] - k.oy) * k.sy;
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
        if (x0 + kCols <= W && ((uintptr_t)dst & 15u) == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) ((float4*)dst)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (int c = 0; c < kCols; ++c)
                if (x0 + c < W) {
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

__device__ __forceinline__ Ycc to_ycc(float rf, float gf, float bf, const sr_yuv16_rule& k) {
    const double r = unit((double)rf), g = unit((double)gf), b = unit((double)bf);
    const double y = (k.kr * r + k.kg * g) + k.kb * b;
    const double cb = (b - y) * k.ib, cr = (r - y) * k.ir;
    Ycc o;
    o.y = k.oy + k.ky * y;
    o.cb = k.mid + k.kc * cb;
    o.cr = k.mid + k.kc * cr;
    return o;
}

__device__ __forceinline__ uint16_t to_code(double v, double lo, double hi) {
    v = floor(v + 0.5);
    v = v > lo ? v : lo;
    v = v < hi ? v : hi;
    return (uint16_t)(int)v;
}

template <int SUB, bool LEFT>
__global__ __launch_bounds__(kThreads) void rgb_to_yuv16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int H, int W, size_t frame,
                                                                sr_yuv16_rule k, unsigned blocks_x, unsigned blocks_y) {
    // runs 0, 1: the two luma rows; 4:2:0: 2, 3 = Cb, Cr; 4:2:2 and 4:4:4: 2, 3 = Cb's rows, 4, 5 = Cr's rows
    constexpr int kRuns = SUB == S420 ? 4 : 6;
    constexpr bool kEdge = LEFT && SUB != S444;
    __shared__ uint4 lds[kRuns][kRunGroups];
    __shared__ double edge[kEdge ? kThreads : 1][4];  // the thread's last column: Cb', Cr' of row 0, of row 1
    const BlockAt at = block_at(blocks_x, blocks_y);
    const int tid = (int)threadIdx.x;
    const int bx0 = (int)at.bx * kSpan, x0 = bx0 + tid * kCols, y0 = (int)at.by * 2;
    const int CH = SUB == S420 ? (H + 1) / 2 : H, CW = SUB == S444 ? W : (W + 1) / 2;
    const bool two = y0 + 1 < H;
    const int span = W - bx0 < kSpan ? W - bx0 : kSpan;  // the workgroup's columns
    uint16_t* __restrict__ yp = out + (size_t)at.img * frame;
    uint16_t* __restrict__ cbp = yp + (size_t)H * W;
    uint16_t* __restrict__ crp = cbp + (size_t)CH * CW;
    Run run[kRuns];
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
                ((uint16_t*)lds[r])[run[r].shift + at_col] = to_code(p[r][c].y, k.ylo, k.yhi);
                if (SUB == S444) {
                    ((uint16_t*)lds[2 + r])[run[2 + r].shift + at_col] = to_code(p[r][c].cb, k.clo, k.chi);
                    ((uint16_t*)lds[kRuns - 2 + r])[run[kRuns - 2 + r].shift + at_col] = to_code(p[r][c].cr, k.clo, k.chi);
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
                ((uint16_t*)lds[2])[run[2].shift + at_col] = to_code(vb, k.clo, k.chi);
                ((uint16_t*)lds[3])[run[3].shift + at_col] = to_code(vr, k.clo, k.chi);
            } else {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (r == 1 && !two) break;
                    ((uint16_t*)lds[2 + r])[run[2 + r].shift + at_col] = to_code(cb[r], k.clo, k.chi);
                    ((uint16_t*)lds[kRuns - 2 + r])[run[kRuns - 2 + r].shift + at_col] = to_code(cr[r], k.clo, k.chi);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRuns; ++r) store_run(run[r], lds[r]);
}

template <class Launch>
hipError_t by_format(const sr_yuv16_rule& k, Launch&& launch) {
    using std::integral_constant;
    if (k.sub == S444) launch(integral_constant<int, S444>{}, std::false_type{});
    else if (k.sub == S420 && k.left) launch(integral_constant<int, S420>{}, std::true_type{});
    else if (k.sub == S420) launch(integral_constant<int, S420>{}, std::false_type{});
    else if (k.left) launch(integral_constant<int, S422>{}, std::true_type{});
    else launch(integral_constant<int, S422>{}, std::false_type{});
    return hipGetLastError();
}

size_t yuv16_blocks(int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    if (n < 1 || h < 1 || w < 1) return 0;
    const size_t bx = ((size_t)w + kSpan - 1) / kSpan, by = ((size_t)h + 1) / 2;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    if (blocks_y_out) *blocks_y_out = (unsigned)by;
    return bx * by * (size_t)n;
}

}  // namespace

size_t sr_yuv16_to_rgb_blocks(int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    return yuv16_blocks(n, h, w, blocks_x_out, blocks_y_out);
}

size_t sr_rgb_to_yuv16_blocks(int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    return yuv16_blocks(n, h, w, blocks_x_out, blocks_y_out);
}

hipError_t sr_launch_yuv16_to_rgb(const uint16_t* d_yuv, const sr_yuv16_rule& k, int n, int h, int w, float* d_rgb, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_yuv16_to_rgb_blocks(n, h, w, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || !sr_dword_aligned(d_rgb) || ((uintptr_t)d_yuv & 1u)) return hipErrorInvalidValue;
    const size_t frame = sr_yuv16_rule_frame_samples(k, h, w);
    return by_format(k, [&](auto sub, auto left) {
        hipLaunchKernelGGL((yuv16_to_rgb_kernel<decltype(sub)::value, decltype(left)::value>), dim3((unsigned)blocks), dim3(kThreads), 0, s, d_yuv,
                           d_rgb, h, w, frame, k, bx, by);
    });
}

hipError_t sr_launch_rgb_to_yuv16(const float* d_rgb, const sr_yuv16_rule& k, int n, int h, int w, uint16_t* d_yuv, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_rgb_to_yuv16_blocks(n, h, w, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || !sr_dword_aligned(d_rgb) || ((uintptr_t)d_yuv & 1u)) return hipErrorInvalidValue;
    const size_t frame = sr_yuv16_rule_frame_samples(k, h, w);
    return by_format(k, [&](auto sub, auto left) {
        hipLaunchKernelGGL((rgb_to_yuv16_kernel<decltype(sub)::value, decltype(left)::value>), dim3((unsigned)blocks), dim3(kThreads), 0, s, d_rgb,
                           d_yuv, h, w, frame, k, bx, by);
    });
}
