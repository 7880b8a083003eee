// sr_alpha.hip -- the two pixel passes of the transparency path (include/srhip.h "Transparency"; host side: sr_alpha.cpp).  Both are pure
// integer arithmetic: the GPU and the numpy restatement (tests/alpha_ref.py) agree bit for bit.
//
//   alpha_bleed_kernel     the colours of the visible pixels (alpha > 0) spread under the transparent ones, R Jacobi steps of an 8-neighbour
//                          mean.  One workgroup per kBleedTile x kBleedTile output tile: the tile and an apron of R pixels are staged in LDS
//                          as dwords, colour in bytes 0..2 and a STAMP in byte 3: 0 for a visible pixel, t for one filled by step t, 0xFF
//                          for one still unknown, 0xFE outside the image (never filled, never feeds a mean).  "Known before step t" is
//                          stamp < t, so one buffer serves every step in place: a cell that is filled during step t carries stamp t and
//                          is, like the unknown cell it was, invisible to the other cells of that step whichever way the race goes --
//                          each step still reads the step before only.  Cells that are known are never touched again.  A barrier per step.
//                          After t steps the cells within t of the staged region's edge would be stale (their neighbours beyond the edge
//                          were never seen), so step t computes only the cells at least t inside it: what it reads was exact at step
//                          t - 1, and after R steps exactly the tile is left, exact.  A wavefront walks a band of rows downwards, a lane
//                          per column, and keeps the masked sums of the two rows above in registers: three LDS reads per cell.  A tile
//                          whose staged region holds no transparent pixel, or no visible one, is copied straight through.  64 x 64
//                          dwords = 16 KB of LDS.
//   alpha_merge_kernel<f>  byte 3 of every dword of the f h x f w RGBA8 output <- the LR alpha interpolated bilinearly in exact integers
//                          (half-pixel centres, edge-clamped, rounded half up).  A workgroup takes 4 f output rows x 64 groups of four
//                          pixels; the six LR rows it needs go through LDS as alpha values, edge clamp applied while staging.  The output is
//                          only 4-byte aligned and its rows need not be multiples of 16 bytes, so the groups of four are cut where the
//                          ADDRESS is a multiple of 16, row by row: whole groups are one 16-byte load and store, the ragged ends of a row
//                          single dwords.
//
// Every output dword belongs to exactly one thread, the grids are functions of the shape alone, there are no atomics: the same bits on every
// run.  The batch is folded into blockIdx.x.  All global offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

constexpr int kBleedTile = SR_ALPHA_BLEED_TILE;
constexpr int kBleedSide = kBleedTile + 2 * SR_ALPHA_BLEED_MAX;  // 64: the staged region at the largest radius, and the LDS pitch
constexpr uint32_t kUnknown = 0xffu << 24, kOutside = 0xfeu << 24, kColour = 0x00ffffffu;

// (2 sum + n) div (2 n) for n = 1..8 and sum <= 8 x 255 as one multiplication by recip = ceil(2^19 / n): the numerator is at most 4088, and
// recip / 2^20 overshoots 1 / (2 n) by less than 2^-20, so the product overshoots the quotient by less than 2^-8 < 1 / (2 n) -- it cannot
// reach the next integer -- and stays below 2^32.  (tests/test_alpha_cpu.py checks every numerator.)
__device__ __forceinline__ uint32_t mean_round(uint32_t sum, uint32_t n, uint32_t recip) {
    return ((2u * sum + n) * recip) >> 20;
}

// The cells left of, at and right of p, those known before this step (stamp < limit >> 24) only: red and blue summed in the two halves of
// rb (8 x 255 fits 16 bits), green in g, their number in n.
struct RowSums {
    uint32_t rb, g, n;
};
__device__ __forceinline__ RowSums row_sums(const uint32_t* p, uint32_t limit, uint32_t& centre) {
    RowSums s{0u, 0u, 0u};
    const uint32_t q[3] = {p[-1], p[0], p[1]};
    centre = q[1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool known = q[k] < limit;
        const uint32_t m = known ? q[k] : 0u;
        s.rb += m & 0x00ff00ffu;
        s.g += (m >> 8) & 0xffu;
        s.n += known ? 1u : 0u;
    }
    return s;
}

__global__ __launch_bounds__(256) void alpha_bleed_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int H, int W, int R,
                                                          unsigned tiles_x, unsigned tiles_y) {
    __shared__ uint32_t cell[kBleedSide * kBleedSide];
    const unsigned per_image = tiles_x * tiles_y;
    const unsigned img = blockIdx.x / per_image, t_in = blockIdx.x - img * per_image;
    const unsigned ty = t_in / tiles_x, tx = t_in - ty * tiles_x;
    const int y0 = (int)ty * kBleedTile, x0 = (int)tx * kBleedTile;
    const size_t base = (size_t)img * H * W;
    const int side = kBleedTile + 2 * R;
    const int lx = threadIdx.x & (kBleedSide - 1), ly = threadIdx.x >> 6;  // a wavefront per staged row
    // ---- stage the region: rows y0 - R .., columns x0 - R ..
    int any_unknown = 0, any_known = 0;
    if (lx < side) {
        const int gx = x0 - R + lx;
        for (int ry = ly; ry < side; ry += 4) {
            const int gy = y0 - R + ry;
            uint32_t v = kOutside;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const uint32_t px = in[base + (size_t)gy * W + gx];
                const bool known = (px >> 24) != 0;
                v = (px & kColour) | (known ? 0u : kUnknown);
                any_known |= known;
                any_unknown |= !known;
            }
            cell[ry * kBleedSide + lx] = v;
        }
    }
    const int some_unknown = __syncthreads_or(any_unknown), some_known = __syncthreads_or(any_known);  // (also: the region is staged)
    const bool work = some_unknown && some_known;
    // ---- R Jacobi steps in place; step t leaves the cells [t, side - t) of either axis exact
    if (work) {
        for (int t = 1; t <= R; ++t) {
            const uint32_t limit = (uint32_t)t << 24;
            const int per = (side - 2 * t + 3) >> 2;                   // rows of this step per wavefront
            const int r0 = t + ly * per, r1 = min(r0 + per, side - t);
            if (lx >= t && lx < side - t && r0 < r1) {
                uint32_t* p = cell + r0 * kBleedSide + lx;
                uint32_t centre, next_centre;
                RowSums above = row_sums(p - kBleedSide, limit, centre), here = row_sums(p, limit, centre);
                for (int ry = r0; ry < r1; ++ry, p += kBleedSide) {
                    const RowSums below = row_sums(p + kBleedSide, limit, next_centre);
                    if (centre >= kUnknown) {  // (its own colour is masked out of `here`: the nine cells are its eight neighbours)
                        const uint32_t n = above.n + here.n + below.n;
                        if (n) {
                            const uint32_t rb = above.rb + here.rb + below.rb, g = above.g + here.g + below.g;
                            const uint32_t recip = n == 1 ? 524288u : n == 2 ? 262144u : n == 3 ? 174763u : n == 4 ? 131072u  // ceil(2^19 / n)
                                                   : n == 5 ? 104858u : n == 6 ? 87382u : n == 7 ? 74899u : 65536u;
                            *p = mean_round(rb & 0xffffu, n, recip) | (mean_round(g, n, recip) << 8) | (mean_round(rb >> 16, n, recip) << 16) | limit;
                        }
                    }
                    above = here; here = below; centre = next_centre;
                }
            }
            __syncthreads();
        }
    }
    // ---- the tile: a pixel that was visible keeps its dword, a transparent one takes the bled colour under its alpha of 0 (a cell that
    // was never filled still holds the pixel's own colour)
    const int cx = threadIdx.x & (kBleedTile - 1);
    const int gx = x0 + cx;
    if (gx < W) {
        for (int cy = threadIdx.x / kBleedTile; cy < kBleedTile; cy += 256 / kBleedTile) {
            const int gy = y0 + cy;
            if (gy >= H) break;
            const size_t at = base + (size_t)gy * W + gx;
            uint32_t px = in[at];
            if (work && (px >> 24) == 0) px = cell[(cy + R) * kBleedSide + cx + R] & kColour;
            out[at] = px;
        }
    }
}

// ---- alpha x f

constexpr int kMergeQuads = 64;    // groups of four output pixels across a workgroup's tile
constexpr int kMergeLrRows = 4;    // LR rows under it: 4 f output rows
constexpr int kMergePitch = 136;   // staged LR columns: (4 x 64 + 3) / 2 + 3 at the most

// One axis of the interpolation: output index o -> the first of its two taps (the second is the next one) and that tap's weight out of 2 f.
template <int F>
__device__ __forceinline__ void axis_taps(int o, int& tap, int& w0) {
    const int i = o / F, m = 2 * (o - i * F) + 1 - F;
    if (m >= 0) { tap = i; w0 = 2 * F - m; }
    else { tap = i - 1; w0 = -m; }
}

template <int F>
__global__ __launch_bounds__(256) void alpha_merge_kernel(const uint32_t* __restrict__ lr, uint32_t* __restrict__ out, int h, int w,
                                                          unsigned blocks_x, unsigned blocks_y) {
    __shared__ uint32_t a[(kMergeLrRows + 2) * kMergePitch];
    const unsigned per_image = blocks_x * blocks_y;
    const unsigned img = blockIdx.x / per_image, b_in = blockIdx.x - img * per_image;
    const unsigned by = b_in / blocks_x, bx = b_in - by * blocks_x;
    const int OW = F * w, OH = F * h;
    const int ly0 = (int)by * kMergeLrRows - 1;                                         // LR row of staged row 0 (before the clamp)
    const int X0 = (int)bx * kMergeQuads * 4 - 3;                                       // the leftmost output pixel a group of this tile may hold
    const int lx0 = (X0 > 0 ? X0 : 0) / F - 1;                                          // LR column of staged column 0
    const int X1 = min(OW, (int)(bx + 1) * kMergeQuads * 4);                            // one past the rightmost
    const int cols = (X1 - 1) / F + 1 - lx0 + 1;                                        // staged columns: up to the right tap of the last pixel
    const uint32_t* lr_img = lr + (size_t)img * h * w;
    for (int k = threadIdx.x; k < (kMergeLrRows + 2) * kMergePitch; k += 256) {
        const int r = k / kMergePitch, c = k - r * kMergePitch;
        if (c >= cols) continue;
        const int sy = min(max(ly0 + r, 0), h - 1), sx = min(max(lx0 + c, 0), w - 1);
        a[k] = lr_img[(size_t)sy * w + sx] >> 24;
    }
    __syncthreads();
    const int q = threadIdx.x & (kMergeQuads - 1), rg = threadIdx.x >> 6;
    const size_t word0 = (size_t)((uintptr_t)out >> 2);
    uint32_t* out_img = out + (size_t)img * OH * OW;
#pragma unroll
    for (int i = 0; i < F; ++i) {
        const int oy = (int)by * kMergeLrRows * F + rg * F + i;
        if (oy >= OH) break;
        int ty, wy0;
        axis_taps<F>(oy, ty, wy0);
        const uint32_t* row0 = a + (ty - ly0) * kMergePitch - lx0;
        const uint32_t* row1 = row0 + kMergePitch;
        const size_t row_word = ((size_t)img * OH + oy) * OW;
        const int shift = (int)((word0 + row_word) & 3u);  // pixels of this row in front of its first 16-byte boundary ... (4 - shift) & 3
        const int x = ((int)bx * kMergeQuads + q) * 4 - shift;
        if (x >= OW || x + 4 <= 0) continue;
        uint32_t* p = out_img + (size_t)oy * OW;
        uint32_t alpha[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xe = min(max(x + e, 0), OW - 1);
            int tx, wx0;
            axis_taps<F>(xe, tx, wx0);
            const uint32_t top = row0[tx] * wx0 + row0[tx + 1] * (2 * F - wx0);
            const uint32_t bot = row1[tx] * wx0 + row1[tx + 1] * (2 * F - wx0);
            alpha[e] = (top * wy0 + bot * (2 * F - wy0) + 2 * F * F) / (4 * F * F);
        }
        if (x >= 0 && x + 4 <= OW) {
            uint4 v = *(const uint4*)(p + x);
            v.x = (v.x & 0x00ffffffu) | (alpha[0] << 24);
            v.y = (v.y & 0x00ffffffu) | (alpha[1] << 24);
            v.z = (v.z & 0x00ffffffu) | (alpha[2] << 24);
            v.w = (v.w & 0x00ffffffu) | (alpha[3] << 24);
            *(uint4*)(p + x) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e >= 0 && x + e < OW) p[x + e] = (p[x + e] & 0x00ffffffu) | (alpha[e] << 24);
        }
    }
}

}  // namespace

size_t sr_alpha_bleed_blocks(int n, int h, int w, unsigned* tiles_x_out, unsigned* tiles_y_out) {
    if (n < 1 || h < 1 || w < 1) return 0;
    const size_t tx = ((size_t)w + kBleedTile - 1) / kBleedTile, ty = ((size_t)h + kBleedTile - 1) / kBleedTile;
    if (tiles_x_out) *tiles_x_out = (unsigned)tx;
    if (tiles_y_out) *tiles_y_out = (unsigned)ty;
    return tx * ty * (size_t)n;
}

size_t sr_alpha_merge_blocks(int factor, int n, int h, int w, unsigned* blocks_x_out, unsigned* blocks_y_out) {
    if (n < 1 || h < 1 || w < 1 || factor < 2 || factor > 4) return 0;
    // (one group more than the row's pixels need: a row that starts off a 16-byte boundary holds its pixels up to three places to the right)
    const size_t bx = ((size_t)factor * w + 3 + 4 * kMergeQuads - 1) / (4 * kMergeQuads), by = ((size_t)h + kMergeLrRows - 1) / kMergeLrRows;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    if (blocks_y_out) *blocks_y_out = (unsigned)by;
    return bx * by * (size_t)n;
}

hipError_t sr_launch_alpha_bleed(const uint8_t* d_in, uint8_t* d_out, int n, int h, int w, int radius, hipStream_t s) {
    unsigned tx = 0, ty = 0;
    const size_t blocks = sr_alpha_bleed_blocks(n, h, w, &tx, &ty);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || radius < 0 || radius > SR_ALPHA_BLEED_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alpha_bleed_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint32_t*)d_in, (uint32_t*)d_out, h, w, radius, tx, ty);
    return hipGetLastError();
}

hipError_t sr_launch_alpha_merge(int factor, const uint8_t* d_lr, uint8_t* d_out, int n, int h, int w, hipStream_t s) {
    unsigned bx = 0, by = 0;
    const size_t blocks = sr_alpha_merge_blocks(factor, n, h, w, &bx, &by);
    if (blocks == 0 || blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    const uint32_t* lr = (const uint32_t*)d_lr;
    uint32_t* out = (uint32_t*)d_out;
    if (factor == 2) hipLaunchKernelGGL(alpha_merge_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, lr, out, h, w, bx, by);
    else if (factor == 3) hipLaunchKernelGGL(alpha_merge_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, s, lr, out, h, w, bx, by);
    else hipLaunchKernelGGL(alpha_merge_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, lr, out, h, w, bx, by);
    return hipGetLastError();
}
