// sr_resize.hip -- the three launches of a resampling to any size (include/srhip.h "Resampling to any size"; host side: sr_resize.cpp;
// the rule restated in numpy: tests/resize_ref.py), for gfx950.
//
//   resize_taps_kernel      one thread per output index of either axis: first tap, tap count and the normalised weights of that index, the
//                           filter evaluated and the weights normalised in f64, stored as f32.  The weights of an axis are tap-major
//                           (w[k][o]) and padded with zeros to the axis' tap bound, so that the lanes of the horizontal pass, which own
//                           consecutive o, read consecutive floats, and the vertical pass, whose o is the same for a whole workgroup,
//                           reads them through the scalar cache.  Nothing comes from the host: the call stays asynchronous, and a capturing stream records
//                           the launches alone (once the workspace stands: sr_resize.cpp reserves it, and refuses to on such a stream).
//   resize_h_staged_kernel  columns: a workgroup takes 256 consecutive output columns of R consecutive input rows (the batch is n h rows:
//                           rows do not see each other).  The input pixels under those columns -- one contiguous run of each row, first
//                           tap of the first column to last tap of the last -- are read ONCE, as consecutive dwords by consecutive
//                           threads, linearised ONCE and staged in LDS as three planes of floats per row; then a lane owns one column of
//                           each row and takes its taps from LDS (lane stride = the scale in floats: no conflict at 3, two-way at 2).
//                           RGBA8 pixels go through a 256-entry table the workgroup builds in LDS with lut_kernel's expression
//                           (sr_aux.hip), f32 pixels through srgb_to_linear_fast.  R = 4 where four rows' runs fit the LDS budget, else 1.
//   resize_h_direct_kernel  the same work item without the staging, every tap read from global memory and linearised where it is used: the
//                           form for scales so large that one row's run does not fit (beyond ~13 x for lanczos3), for a box filter that
//                           shrinks (its windows abut: no sample is read twice), and the form the staged one was measured against
//                           (DESIGN.md 4n).
//   resize_v_kernel         rows: a workgroup takes 256 consecutive columns of kRowsV consecutive output rows, a lane one column of each.
//                           The rows of the intermediate under those output rows are walked once, in ascending order, four loads in
//                           flight; each is added into every output row whose taps hold it -- first tap, count and weight are uniform,
//                           so that is a scalar compare and a scalar load -- which keeps every sum in ascending tap order.  Consecutive
//                           lanes read consecutive pixels of a row, and every store is one contiguous run: a dword a pixel for RGBA8
//                           (LinearToSrgb, data_to_img, alpha 255), three floats for f32.
//
// Both passes accumulate in f32 over the taps in ascending index (a multiplication and an addition per tap: the file set is built with
// -ffp-contract=off).  Every output element belongs to one thread, the grids are functions of the shape alone, there are no atomics: the
// same bits on every run.  Rows and the batch are folded into blockIdx.x; all global offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "sr_internal.h"
#include "sr_transfer.h"

#pragma clang fp contract(off)

namespace {

constexpr int kCols = 256;           // output columns of a workgroup, both passes
constexpr int kRowsH = 4;            // input rows of a workgroup of the horizontal pass (staged: where they fit, else 1)
constexpr int kRowsV = 4;            // output rows of a workgroup of the vertical pass
constexpr int kStageBytes = 40960;   // LDS a workgroup of the staged horizontal pass may take: three to four workgroups a CU

__device__ __forceinline__ double sinc_pi(double x) {
    if (x == 0.0) return 1.0;
    const double t = 3.14159265358979323846 * x;
    return sin(t) / t;
}

__device__ double filter_value(int filter, double x) {
    const double a = fabs(x);
    switch (filter) {
        case SR_FILTER_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
        case SR_FILTER_TRIANGLE: return a < 1.0 ? 1.0 - a : 0.0;
        case SR_FILTER_CATROM:  // Keys, a = -0.5
            if (a < 1.0) return (1.5 * a - 2.5) * a * a + 1.0;
            if (a < 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
            return 0.0;
        default: return a < 3.0 ? sinc_pi(x) * sinc_pi(x / 3.0) : 0.0;
    }
}

__global__ __launch_bounds__(256) void resize_taps_kernel(sr_resize_axis ax, sr_resize_axis ay, int filter) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const bool is_x = idx < ax.n_out;
    const long o = is_x ? idx : idx - ax.n_out;
    const int n_in = is_x ? ax.n_in : ay.n_in, n_out = is_x ? ax.n_out : ay.n_out, taps = is_x ? ax.taps : ay.taps;
    if (o >= n_out) return;
    const double scale = is_x ? ax.scale : ay.scale, fs = is_x ? ax.fs : ay.fs, reach = is_x ? ax.reach : ay.reach;
    int* const d_lo = is_x ? ax.lo : ay.lo;
    int* const d_cnt = is_x ? ax.cnt : ay.cnt;
    float* const d_w = is_x ? ax.w : ay.w;
    const double c = ((double)o + 0.5) * scale;
    const int lo = (int)fmax(trunc(c - reach + 0.5), 0.0);
    const int hi = (int)fmin(trunc(c + reach + 0.5), (double)n_in);
    const int cnt = min(max(hi - lo, 0), taps);  // (taps is an upper bound of hi - lo: the table is never overrun)
    double sum = 0.0;
    for (int k = 0; k < cnt; ++k) sum += filter_value(filter, ((double)(lo + k) + 0.5 - c) / fs);
    d_lo[o] = lo;
    d_cnt[o] = cnt;
    for (int k = 0; k < taps; ++k)
        d_w[(size_t)k * n_out + o] = k < cnt ? (float)(filter_value(filter, ((double)(lo + k) + 0.5 - c) / fs) / sum) : 0.0f;
}

// img_to_data (main.rs:170), then SrgbToLinear, of the 256 bytes: lut_kernel's expression (sr_aux.hip); the caller synchronises
__device__ __forceinline__ void build_lut(float* s_lut, bool linear) {
    const float v = __fdiv_rn((float)threadIdx.x, 255.0f);
    s_lut[threadIdx.x] = linear ? srgb_to_linear_powf(v) : v;
}

template <bool IN_U8, int R>
__global__ __launch_bounds__(256) void resize_h_staged_kernel(const void* __restrict__ in, float* __restrict__ mid, size_t rows, int w, int ow,
                                                              const int* __restrict__ lo, const int* __restrict__ cnt,
                                                              const float* __restrict__ wt, unsigned blocks_x, int cap, int linear) {
    extern __shared__ float s_px[];  // [R][3][cap]: the rows' runs, linear
    __shared__ float s_lut[IN_U8 ? 256 : 1];
    const int tid = (int)threadIdx.x;
    if constexpr (IN_U8) build_lut(s_lut, linear != 0);
    const unsigned by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const int ox0 = (int)bx * kCols, ox = ox0 + tid, ox_last = min(ox0 + kCols - 1, ow - 1);
    const size_t r0 = (size_t)by * R;
    // first tap of the first column to last tap of the last: first taps and ends both grow with the column.  (cap bounds the run by the
    // rule's arithmetic, sr_resize_h_form; the min keeps the staging inside the LDS whatever the tables hold)
    const int first = lo[ox0];
    const int span = min(lo[ox_last] + cnt[ox_last] - first, cap);
    if constexpr (IN_U8) __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t row = min(r0 + r, rows - 1);  // rows past the last redo it (staged, never stored)
        float* plane = s_px + (size_t)r * 3 * cap;
        if constexpr (IN_U8) {
            const uint32_t* src = (const uint32_t*)in + row * (size_t)w + first;
            for (int i = tid; i < span; i += 256) {
                const uint32_t px = src[i];
                plane[i] = s_lut[px & 0xffu];
                plane[cap + i] = s_lut[(px >> 8) & 0xffu];
                plane[2 * cap + i] = s_lut[(px >> 16) & 0xffu];
            }
        } else {
            const float* src = (const float*)in + (row * (size_t)w + first) * 3;
            for (int i = tid; i < 3 * span; i += 256) {
                const float v = src[i];
                const int px = i / 3, ch = i - 3 * px;
                plane[ch * cap + px] = linear ? srgb_to_linear_fast(v) : v;
            }
        }
    }
    __syncthreads();
    if (ox >= ow) return;
    const int mine = max(lo[ox] - first, 0);
    const int taps = min(cnt[ox], span - mine);
    float acc[R][3];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.0f;
    for (int k = 0; k < taps; ++k) {
        const float wk = wt[(size_t)k * ow + ox];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[r][ch] += wk * s_px[((size_t)r * 3 + ch) * cap + mine + k];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r0 + r >= rows) break;
        float* q = mid + ((r0 + r) * (size_t)ow + ox) * 3;
        q[0] = acc[r][0]; q[1] = acc[r][1]; q[2] = acc[r][2];
    }
}

template <bool IN_U8>
__global__ __launch_bounds__(256) void resize_h_direct_kernel(const void* __restrict__ in, float* __restrict__ mid, size_t rows, int w, int ow,
                                                              const int* __restrict__ lo, const int* __restrict__ cnt,
                                                              const float* __restrict__ wt, unsigned blocks_x, int linear) {
    __shared__ float s_lut[IN_U8 ? 256 : 1];
    if constexpr (IN_U8) {
        build_lut(s_lut, linear != 0);
        __syncthreads();
    }
    const unsigned by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const int ox = (int)bx * kCols + (int)threadIdx.x;
    if (ox >= ow) return;
    const size_t r0 = (size_t)by * kRowsH;
    const int first = lo[ox], taps = cnt[ox];
    size_t row[kRowsH];  // rows past the last redo it (loaded, never stored)
#pragma unroll
    for (int r = 0; r < kRowsH; ++r) row[r] = min(r0 + r, rows - 1) * (size_t)w + first;
    float acc[kRowsH][3];
#pragma unroll
    for (int r = 0; r < kRowsH; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.0f;
    for (int k = 0; k < taps; ++k) {
        const float wk = wt[(size_t)k * ow + ox];
#pragma unroll
        for (int r = 0; r < kRowsH; ++r) {
            float v[3];
            if constexpr (IN_U8) {
                const uint32_t px = ((const uint32_t*)in)[row[r] + k];
                v[0] = s_lut[px & 0xffu]; v[1] = s_lut[(px >> 8) & 0xffu]; v[2] = s_lut[(px >> 16) & 0xffu];
            } else {
                const float* p = (const float*)in + (row[r] + k) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch] = linear ? srgb_to_linear_fast(p[ch]) : p[ch];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[r][ch] += wk * v[ch];
        }
    }
#pragma unroll
    for (int r = 0; r < kRowsH; ++r) {
        if (r0 + r >= rows) break;
        float* q = mid + ((r0 + r) * (size_t)ow + ox) * 3;
        q[0] = acc[r][0]; q[1] = acc[r][1]; q[2] = acc[r][2];
    }
}

template <bool OUT_U8, bool LINEAR>
__global__ __launch_bounds__(256) void resize_v_kernel(const float* __restrict__ mid, void* __restrict__ out, int h, int oh, int ow,
                                                       const int* __restrict__ lo, const int* __restrict__ cnt,
                                                       const float* __restrict__ wt, unsigned blocks_x, unsigned groups) {
    // (image, group of kRowsV output rows), uniform; a group never spans two images
    const unsigned g = blockIdx.x / blocks_x, bx = blockIdx.x - g * blocks_x;
    const unsigned img = g / groups;
    const int oy0 = (int)(g - img * groups) * kRowsV;
    const int ox = (int)bx * kCols + (int)threadIdx.x;
    if (ox >= ow) return;
    int first[kRowsV], end[kRowsV];  // taps [first, end) of each output row of the group (a row past the image's last: none)
    int j0 = h, j1 = 0;
#pragma unroll
    for (int m = 0; m < kRowsV; ++m) {
        const bool live = oy0 + m < oh;
        const int oy = min(oy0 + m, oh - 1);
        first[m] = live ? lo[oy] : 0;
        end[m] = live ? min(first[m] + cnt[oy], h) : 0;
        if (live) { j0 = min(j0, first[m]); j1 = max(j1, end[m]); }
    }
    float acc[kRowsV][3];
#pragma unroll
    for (int m = 0; m < kRowsV; ++m) acc[m][0] = acc[m][1] = acc[m][2] = 0.0f;
    const float* col = mid + ((size_t)img * h * (size_t)ow + ox) * 3;
    const size_t pitch = (size_t)ow * 3;
    for (int j = j0; j < j1; j += 4) {
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // (rows past the walk's end redo its last: loaded, never used)
            const float* p = col + (size_t)min(j + u, j1 - 1) * pitch;
            v[u][0] = p[0]; v[u][1] = p[1]; v[u][2] = p[2];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j + u;
#pragma unroll
            for (int m = 0; m < kRowsV; ++m) {
                if (jj >= first[m] && jj < end[m]) {
                    const float wk = wt[(size_t)(jj - first[m]) * oh + (oy0 + m)];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[m][ch] += wk * v[u][ch];
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < kRowsV; ++m) {
        if (oy0 + m >= oh) break;
        float o3[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o3[ch] = LINEAR ? linear_to_srgb_fast(acc[m][ch]) : acc[m][ch];
        const size_t at = ((size_t)img * oh + (oy0 + m)) * (size_t)ow + ox;
        if constexpr (OUT_U8) {
            ((uint32_t*)out)[at] = quant_u8(o3[0]) | (quant_u8(o3[1]) << 8) | (quant_u8(o3[2]) << 16) | 0xff000000u;
        } else {
            float* q = (float*)out + at * 3;
            q[0] = o3[0]; q[1] = o3[1]; q[2] = o3[2];
        }
    }
}

}  // namespace

// The form of the horizontal pass for an axis: rows a workgroup takes, and for the staged form (*cap > 0) the pixels of a row's run the LDS
// holds.  A workgroup's 256 columns o0 .. o0 + 255 read the input from lo(o0) to hi(o0 + 255): at most 255 scale + 2 reach + 1 pixels by
// the rule (hi <= c + reach + 0.5, lo > c - reach - 0.5), one more for the rounding of c, never more than the row has.
int sr_resize_h_form(const sr_resize_axis& x, int* cap_out) {
    const double run = std::min(std::floor(255.0 * x.scale + 2.0 * x.reach) + 2.0, (double)x.n_in);
    int rows = kRowsH, cap = 0;
    // An input sample serves 2 reach / scale output columns: 6 for lanczos3, 1 for a box that shrinks -- windows that abut, nothing read
    // twice, nothing for the staging to save (measured: DESIGN.md 4n).
    if (2.0 * x.reach <= x.scale) cap = 0;
    else if (run * 3 * sizeof(float) * kRowsH <= kStageBytes) cap = (int)run;
    else if (run * 3 * sizeof(float) <= kStageBytes) { cap = (int)run; rows = 1; }
    if (cap_out) *cap_out = cap;
    return rows;
}

size_t sr_resize_h_blocks(size_t rows, const sr_resize_axis& x, unsigned* blocks_x_out) {
    if (rows < 1 || x.n_out < 1) return 0;
    const size_t bx = ((size_t)x.n_out + kCols - 1) / kCols, per = (size_t)sr_resize_h_form(x, nullptr);
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    return bx * ((rows + per - 1) / per);
}

size_t sr_resize_v_blocks(int n, int oh, int ow, unsigned* blocks_x_out, unsigned* groups_out) {
    if (n < 1 || oh < 1 || ow < 1) return 0;
    const size_t bx = ((size_t)ow + kCols - 1) / kCols, groups = ((size_t)oh + kRowsV - 1) / kRowsV;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    if (groups_out) *groups_out = (unsigned)groups;
    return bx * groups * (size_t)n;
}

hipError_t sr_launch_resize_taps(const sr_resize_axis& x, const sr_resize_axis& y, int filter, hipStream_t s) {
    if (x.n_out < 1 || y.n_out < 1 || !x.lo || !x.cnt || !x.w || !y.lo || !y.cnt || !y.w) return hipErrorInvalidValue;
    const size_t blocks = ((size_t)x.n_out + (size_t)y.n_out + 255) / 256;
    hipLaunchKernelGGL(resize_taps_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, filter);
    return hipGetLastError();
}

hipError_t sr_launch_resize_h(const void* d_in, bool in_u8, bool linear, size_t rows, const sr_resize_axis& x, float* d_mid, hipStream_t s) {
    unsigned bx = 0;
    int cap = 0;
    const size_t blocks = sr_resize_h_blocks(rows, x, &bx);
    const int per = sr_resize_h_form(x, &cap);
    if (blocks == 0 || blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    const int lin = linear ? 1 : 0;
    if (cap > 0) {
        const size_t lds = (size_t)per * 3 * cap * sizeof(float);
        if (in_u8 && per == kRowsH)
            hipLaunchKernelGGL((resize_h_staged_kernel<true, kRowsH>), grid, block, lds, s, d_in, d_mid, rows, x.n_in, x.n_out, x.lo, x.cnt, x.w, bx, cap, lin);
        else if (in_u8)
            hipLaunchKernelGGL((resize_h_staged_kernel<true, 1>), grid, block, lds, s, d_in, d_mid, rows, x.n_in, x.n_out, x.lo, x.cnt, x.w, bx, cap, lin);
        else if (per == kRowsH)
            hipLaunchKernelGGL((resize_h_staged_kernel<false, kRowsH>), grid, block, lds, s, d_in, d_mid, rows, x.n_in, x.n_out, x.lo, x.cnt, x.w, bx, cap, lin);
        else
            hipLaunchKernelGGL((resize_h_staged_kernel<false, 1>), grid, block, lds, s, d_in, d_mid, rows, x.n_in, x.n_out, x.lo, x.cnt, x.w, bx, cap, lin);
    } else if (in_u8) {
        hipLaunchKernelGGL((resize_h_direct_kernel<true>), grid, block, 0, s, d_in, d_mid, rows, x.n_in, x.n_out, x.lo, x.cnt, x.w, bx, lin);
    } else {
        hipLaunchKernelGGL((resize_h_direct_kernel<false>), grid, block, 0, s, d_in, d_mid, rows, x.n_in, x.n_out, x.lo, x.cnt, x.w, bx, lin);
    }
    return hipGetLastError();
}

hipError_t sr_launch_resize_v(const float* d_mid, int n, int ow, const sr_resize_axis& y, void* d_out, bool out_u8, bool linear, hipStream_t s) {
    unsigned bx = 0, groups = 0;
    const size_t blocks = sr_resize_v_blocks(n, y.n_out, ow, &bx, &groups);
    if (blocks == 0 || blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    if (out_u8 && linear) hipLaunchKernelGGL((resize_v_kernel<true, true>), grid, block, 0, s, d_mid, d_out, y.n_in, y.n_out, ow, y.lo, y.cnt, y.w, bx, groups);
    else if (out_u8) hipLaunchKernelGGL((resize_v_kernel<true, false>), grid, block, 0, s, d_mid, d_out, y.n_in, y.n_out, ow, y.lo, y.cnt, y.w, bx, groups);
    else if (linear) hipLaunchKernelGGL((resize_v_kernel<false, true>), grid, block, 0, s, d_mid, d_out, y.n_in, y.n_out, ow, y.lo, y.cnt, y.w, bx, groups);
    else hipLaunchKernelGGL((resize_v_kernel<false, false>), grid, block, 0, s, d_mid, d_out, y.n_in, y.n_out, ow, y.lo, y.cnt, y.w, bx, groups);
    return hipGetLastError();
}
