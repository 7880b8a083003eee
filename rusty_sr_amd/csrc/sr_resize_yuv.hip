// sr_resize_yuv.hip -- the vertical pass of a resampling that ends in a planar YCbCr frame (include/srhip.h "Video at any size"; host
// side: sr_yuv.cpp), for gfx950: resize_v_kernel of sr_resize.hip and rgb_to_yuv_kernel of sr_yuv.hip as one launch, without
// the oh x ow x 3 f32 image the one writes and the other reads straight back.
//
//   resize_v_yuv_kernel<S, SUB, LEFT, LINEAR, PAIRS>
//       a workgroup takes PAIRS tiles of rgb_to_yuv_kernel one below the other: 1024 columns x 2 PAIRS output rows, a thread 4 columns of
//       each.  The rows of the intermediate under those output rows are walked once, in ascending order, four rows in flight; a thread's
//       four columns of a row are 48 consecutive bytes: three 16-byte loads where the address allows (ow % 4 != 0 misaligns every second
//       row or three rows in four), dwords elsewhere.  A row is added into every output row whose taps hold it -- first tap, count and
//       weight are uniform: a scalar compare and a scalar load -- one multiplication and one addition a tap, in ascending tap index, then
//       LinearToSrgb unless the resampling is in sRGB space: the expressions of resize_v_kernel, so the f32 value is the one that kernel
//       would have stored.  From there on it is rgb_to_yuv_kernel (sr_yuv_tile.h): to_ycc, the chroma subsampling, to_code, the runs in
//       LDS, whole aligned 16-byte groups to memory.  Under the left siting column 2j - 1 of a workgroup's first thread is the
//       neighbouring workgroup's: that thread sums that one column too, 1 column in 1024, as the other kernel reads it again.
//
// Grid: the batch, the groups of PAIRS row pairs and the 1024-column blocks folded into blockIdx.x, a function of the shape alone
// (sr_resize_yuv_blocks).  Every output sample / group belongs to exactly one thread, no atomics: the same bits on every run, and the
// bits of the chain of the two kernels.  All global offsets are 64-bit.  Resources: profiles/video_sized_kernel_resources.txt.
// Which format classes run this kernel and which the chain is the host's rule, by measurement (sr_yuv.cpp fused_pays).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"
#include "sr_transfer.h"
#include "sr_yuv_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPairsDefault = 2;  // row pairs of a workgroup: 4 output rows share a walk, as in resize_v_kernel (measured: DESIGN.md 4w)

// a thread's four columns of a row of the intermediate (p: its first column's pixel); beyond the row's end a column is the last one
__device__ __forceinline__ void load_cols(const float* __restrict__ p, int x0, int ow, float (&v)[kCols * 3]) {
    if (x0 + kCols <= ow) {
        if (((uintptr_t)p & 15u) == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float4 t = ((const float4*)p)[q];
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kCols * 3; ++e) v[e] = p[e];
        }
    } else {
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const int cc = x0 + c < ow ? c : ow - 1 - x0;
            v[3 * c] = p[3 * cc]; v[3 * c + 1] = p[3 * cc + 1]; v[3 * c + 2] = p[3 * cc + 2];
        }
    }
}

template <bool LINEAR>
__device__ __forceinline__ Ycc sum_to_ycc(const float* acc, const sr_yuv_rule& k) {  // what resize_v_kernel stores, then to_ycc
    float o3[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o3[ch] = LINEAR ? linear_to_srgb_fast(acc[ch]) : acc[ch];
    return to_ycc(o3[0], o3[1], o3[2], k);
}

template <class S, int SUB, bool LEFT, bool LINEAR, int PAIRS>
__global__ __launch_bounds__(kThreads) void resize_v_yuv_kernel(const float* __restrict__ mid, S* __restrict__ out, int h, int oh, int ow,
                                                                size_t frame, sr_yuv_rule k, const int* __restrict__ lo,
                                                                const int* __restrict__ cnt, const float* __restrict__ wt, unsigned blocks_x,
                                                                unsigned blocks_y) {
    constexpr int kRowsW = 2 * PAIRS;  // output rows of a workgroup
    constexpr bool kEdge = LEFT && SUB != S444;
    __shared__ uint4 lds[kRuns<SUB>][kRunGroups<S>];
    __shared__ double edge[kEdge ? kThreads : 1][4];  // the thread's last column: Cb', Cr' of row 0, of row 1
    const BlockAt at = block_at(blocks_x, blocks_y);   // (image, group of PAIRS row pairs, column block), uniform
    const int tid = (int)threadIdx.x;
    const int bx0 = (int)at.bx * kSpan, x0 = bx0 + tid * kCols, oy0 = (int)at.by * kRowsW;
    const int span = ow - bx0 < kSpan ? ow - bx0 : kSpan;  // the workgroup's columns
    const bool live = x0 < ow;
    const bool has_left = kEdge && tid == 0 && x0 > 0;  // the one thread that sums the neighbouring workgroup's last column too
    int first[kRowsW], end[kRowsW];  // taps [first, end) of each output row of the group (a row past the image's last: none)
    int j0 = h, j1 = 0;
#pragma unroll
    for (int m = 0; m < kRowsW; ++m) {
        const bool row_live = oy0 + m < oh;
        const int oy = min(oy0 + m, oh - 1);
        first[m] = row_live ? lo[oy] : 0;
        end[m] = row_live ? min(first[m] + cnt[oy], h) : 0;
        if (row_live) { j0 = min(j0, first[m]); j1 = max(j1, end[m]); }
    }
    float acc[kRowsW][kCols * 3], accl[kRowsW][3];
#pragma unroll
    for (int m = 0; m < kRowsW; ++m) {
#pragma unroll
        for (int e = 0; e < kCols * 3; ++e) acc[m][e] = 0.0f;
        accl[m][0] = accl[m][1] = accl[m][2] = 0.0f;
    }
    const size_t pitch = (size_t)ow * 3;
    // walk(col, each(u, p), added(m, u, wk)): the walk over rows j0 .. j1 - 1 of the intermediate, four in flight -- each(u, p) loads what
    // the caller wants of row j + u at p = col + row * pitch, added(m, u, wk) adds it into output row m under weight wk
    auto walk = [&](const float* __restrict__ col, auto&& each, auto&& added) __attribute__((always_inline)) {
        for (int j = j0; j < j1; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) each(u, col + (size_t)min(j + u, j1 - 1) * pitch);  // (rows past the walk's end redo its last: loaded, never used)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int jj = j + u;
#pragma unroll
                for (int m = 0; m < kRowsW; ++m)
                    if (jj >= first[m] && jj < end[m]) added(m, u, wt[(size_t)(jj - first[m]) * oh + (oy0 + m)]);
            }
        }
    };
    if (has_left) {
        float vl[4][3];
        walk(mid + ((size_t)at.img * h * (size_t)ow + (size_t)(x0 - 1)) * 3,
             [&](int u, const float* __restrict__ p) { vl[u][0] = p[0]; vl[u][1] = p[1]; vl[u][2] = p[2]; },
             [&](int m, int u, float wk) {
#pragma unroll
                 for (int ch = 0; ch < 3; ++ch) accl[m][ch] += wk * vl[u][ch];
             });
    }
    if (live) {
        float v[4][kCols * 3];
        walk(mid + ((size_t)at.img * h * (size_t)ow + (size_t)x0) * 3, [&](int u, const float* __restrict__ p) { load_cols(p, x0, ow, v[u]); },
             [&](int m, int u, float wk) {
#pragma unroll
                 for (int e = 0; e < kCols * 3; ++e) acc[m][e] += wk * v[u][e];
             });
    }
#pragma unroll
    for (int pp = 0; pp < PAIRS; ++pp) {
        const int y0 = oy0 + 2 * pp;
        if (y0 >= oh) break;  // (uniform)
        const bool two = y0 + 1 < oh;
        if (pp > 0) __syncthreads();  // the tile above has left the LDS
        Run<S> run[kRuns<SUB>];
        tile_runs<S, SUB>(run, out, frame, at.img, at.by * PAIRS + pp, oh, ow, bx0, span, two);
        Ycc p[2][kCols];
        if (live) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (r == 1 && !two) {  // the row below the image is the last row
#pragma unroll
                    for (int c = 0; c < kCols; ++c) p[1][c] = p[0][c];
                    break;
                }
#pragma unroll
                for (int c = 0; c < kCols; ++c) p[r][c] = sum_to_ycc<LINEAR>(&acc[2 * pp + r][3 * c], k);
            }
        }
        if (kEdge && !two) {  // the row below the image is the last row, for the neighbouring workgroup's column too
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) accl[2 * pp + 1][ch] = accl[2 * pp][ch];
        }
        // the neighbouring workgroup's last column (inlined: r is a constant there, and the sums stay in registers)
        tile_store<S, SUB, LEFT>(p, live, two, x0, ow, k, run, lds, edge,
                                 [&](int r) __attribute__((always_inline)) { return sum_to_ycc<LINEAR>(accl[2 * pp + r], k); });
    }
}

int pairs_of(int pairs) { return pairs == 1 || pairs == 2 ? pairs : kPairsDefault; }

}  // namespace

size_t sr_resize_yuv_blocks(int n, int oh, int ow, int pairs, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    if (n < 1 || oh < 1 || ow < 1) return 0;
    const size_t rows = 2 * (size_t)pairs_of(pairs);
    const size_t bx = ((size_t)ow + kSpan - 1) / kSpan, by = ((size_t)oh + rows - 1) / rows;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    if (blocks_y_out) *blocks_y_out = (unsigned)by;
    return bx * by * (size_t)n;
}

template <class S>
hipError_t sr_launch_resize_v_yuv(const float* d_mid, int n, int ow, const sr_resize_axis& y, const sr_yuv_rule& k, S* d_yuv, bool linear,
                                  int pairs, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_resize_yuv_blocks(n, y.n_out, ow, pairs, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || !sr_dword_aligned(d_mid) || ((uintptr_t)d_yuv & (alignof(S) - 1))) return hipErrorInvalidValue;
    if (y.n_in < 1 || !y.lo || !y.cnt || !y.w) return hipErrorInvalidValue;
    const size_t frame = sr_yuv_rule_frame_samples(k, y.n_out, ow);
    const dim3 grid((unsigned)blocks), block(kThreads);
    return by_format<S>(k, [&](auto sub, auto left) {
        constexpr int SUB = decltype(sub)::value;
        constexpr bool LEFT = decltype(left)::value;
        auto go = [&](auto lin, auto prs) {
            hipLaunchKernelGGL((resize_v_yuv_kernel<S, SUB, LEFT, decltype(lin)::value, decltype(prs)::value>), grid, block, 0, s, d_mid, d_yuv,
                               y.n_in, y.n_out, ow, frame, k, y.lo, y.cnt, y.w, bx, by);
        };
        using std::integral_constant;
        if (pairs_of(pairs) == 1) {
            if (linear) go(std::true_type{}, integral_constant<int, 1>{});
            else go(std::false_type{}, integral_constant<int, 1>{});
        } else {
            if (linear) go(std::true_type{}, integral_constant<int, 2>{});
            else go(std::false_type{}, integral_constant<int, 2>{});
        }
    });
}

template hipError_t sr_launch_resize_v_yuv<uint8_t>(const float*, int, int, const sr_resize_axis&, const sr_yuv_rule&, uint8_t*, bool, int, hipStream_t);
template hipError_t sr_launch_resize_v_yuv<uint16_t>(const float*, int, int, const sr_resize_axis&, const sr_yuv_rule&, uint16_t*, bool, int, hipStream_t);
