// sr_yuv_tile.h -- the device helpers of a workgroup that makes a tile of a planar YCbCr frame from f32 RGB pixels (sr_yuv.hip's header
// comment has the rules): shared by rgb_to_yuv_kernel of sr_yuv.hip, which reads its pixels, and resize_v_yuv_kernel of
// sr_resize_yuv.hip, which sums them from the resampler's intermediate.  A tile is 2 rows x 1024 columns: 256 threads, 4 columns each.
// Device code only; the including file is built without contraction.
#pragma once
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
// runs 0, 1: the two luma rows; 4:2:0: 2, 3 = Cb, Cr; 4:2:2 and 4:4:4: 2, 3 = Cb's rows, 4, 5 = Cr's rows
template <int SUB>
constexpr int kRuns = SUB == S420 ? 4 : 6;

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

// the runs of the tile at row pair `pair`, columns bx0 .. bx0 + span - 1, of frame `img` of n frames of H x W luma samples at out
template <class S, int SUB>
__device__ __forceinline__ void tile_runs(Run<S>* run, S* __restrict__ out, size_t frame, unsigned img, unsigned pair, int H, int W, int bx0,
                                          int span, bool two) {
    const int y0 = (int)pair * 2;
    const int CH = SUB == S420 ? (H + 1) / 2 : H, CW = SUB == S444 ? W : (W + 1) / 2;
    S* __restrict__ yp = out + (size_t)img * frame;
    S* __restrict__ cbp = yp + (size_t)H * W;
    S* __restrict__ crp = cbp + (size_t)CH * CW;
    run[0] = make_run(yp + (size_t)y0 * W + bx0, span);
    run[1] = make_run(yp + (size_t)(y0 + 1) * W + bx0, two ? span : 0);
    if (SUB == S420) {
        const int cspan = (span + 1) / 2;  // (bx0 is even)
        const size_t co = (size_t)pair * CW + (size_t)(bx0 / 2);
        run[2] = make_run(cbp + co, cspan);
        run[3] = make_run(crp + co, cspan);
    } else {
        const int cspan = SUB == S422 ? (span + 1) / 2 : span;
        const size_t co = (size_t)y0 * CW + (size_t)(SUB == S422 ? bx0 / 2 : bx0);
        run[2] = make_run(cbp + co, cspan);
        run[3] = make_run(cbp + co + CW, two ? cspan : 0);
        run[kRuns<SUB> - 2] = make_run(crp + co, cspan);
        run[kRuns<SUB> - 1] = make_run(crp + co + CW, two ? cspan : 0);
    }
}

// The tile from a thread's pixels to memory: p = its 2 rows x 4 columns (a column beyond the row holds the last one, the row below the
// image the last row), live = its first column is inside the row.  Luma (and 4:4:4 chroma) go into the runs a sample a pixel, the
// subsampled chroma a sample a block; under the left siting column 2j - 1 of the thread's first block is its neighbour's last column,
// passed through `edge` -- the first thread of a workgroup that is not the first of its row asks left_col(r) for the Cb', Cr' of that
// column in row r.  Then one barrier and the runs' stores.  Every thread of the workgroup calls this.
template <class S, int SUB, bool LEFT, class LeftCol>
__device__ __forceinline__ void tile_store(const Ycc (&p)[2][kCols], bool live, bool two, int x0, int W, const sr_yuv_rule& k,
                                           const Run<S>* run, uint4 (*lds)[kRunGroups<S>], double (*edge)[4], LeftCol&& left_col) {
    constexpr bool kEdge = LEFT && SUB != S444;
    const int tid = (int)threadIdx.x;
    if (live) {
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
                    ((S*)lds[kRuns<SUB> - 2 + r])[run[kRuns<SUB> - 2 + r].shift + at_col] = to_code<S>(p[r][c].cr, k.clo, k.chi);
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
                    const Ycc q = left_col(r);
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
                    ((S*)lds[kRuns<SUB> - 2 + r])[run[kRuns<SUB> - 2 + r].shift + at_col] = to_code<S>(cr[r], k.clo, k.chi);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRuns<SUB>; ++r) store_run(run[r], lds[r]);
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
