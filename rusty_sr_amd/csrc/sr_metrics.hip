// sr_metrics.hip -- the benchmark protocol's scores of an image A against its ground truth B (include/srhip.h, "Metrics"), on gfx950:
//
//   Y        = (65481 R + 128553 G + 24966 B + 127500) div 255000 + 16      the 8-bit BT.601 luma, in integers
//   y_sq_err = sum (Y_A - Y_B)^2 over the region left by shaving s pixels off every border, an exact integer
//   ssim_sum = sum over the region's "valid" 11 x 11 window positions of the SSIM map of Y_A, Y_B (Gaussian window, sigma 1.5), in f64
//
// A is u8 (3 or 4 channels) or the network's f32 output, quantised on load by data_to_img's rule clamp(floor(255 v + 0.5), 0, 255): the
// scores are those of the pixels the CLI would save, and no u8 copy of the output is written.  B is u8.
//
// Tile plan.  The shaved region is cut into tiles of kMetricsTile x kMetricsTile pixels, one workgroup of 256 each.  A tile owns its pixels
// (their squared luma error is counted by it, once) and the window positions whose top-left pixel is one of them, so it reads its pixels
// plus an apron of 10 to the right and below -- (T + 10)^2 pixels of both operands, once from HBM, 1.72 x the image at T = 32:
//   1. load: four consecutive pixels per work item -- u8 as the aligned dwords that hold them (BytePiece), f32 as three 16-byte loads of
//      an aligned group of four pixels of the contiguous output -- to luma, kept in LDS as bytes (2 x 42 x 48 B);
//   2. luma SSE of the tile's own pixels, in integers;
//   3. row filter: the 11-tap Gaussian of Y_A, Y_B, Y_A^2, Y_B^2, Y_A Y_B along the row, f64, to LDS (5 x 42 x 32 doubles, 53 760 B);
//   4. column filter of those five, the SSIM map, the thread's f64 sum -- 4 window positions per thread, in a fixed order.
// Steps 3 and 4 are skipped by a tile that owns no valid window position (the region's last 10 rows and columns; every tile of a region
// with a side below 11).  57.8 KB of LDS: two workgroups per CU.  About 127 f64 FMAs per pixel.
// One f64 and one u64 partial per workgroup; the grid depends on the shape alone, and metrics_sum_kernel adds the partials in a fixed
// order in one workgroup: the same bits on every run, context and device.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sr_bytes.h"
#include "sr_internal.h"
#include "sr_reduce.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kT = SR_METRICS_TILE;  // tile side
constexpr int kA = kT + 10;          // ... with its apron
constexpr int kYP = 48;              // row pitch of a luma tile in LDS, bytes (whole dwords)

struct MetricsGeo {
    int s;             // pixels shaved off every border
    int RH, RW;        // the shaved region
    int tiles_x;
    long pitch_a, pitch_b;  // pixels per row of A and of B
    long npx_a;        // f32 A only: the pixels of the (contiguous) image
    double g[11];      // the window's weights
};

__device__ __forceinline__ uint32_t luma(uint32_t r, uint32_t g, uint32_t b) {
    return (65481u * r + 128553u * g + 24966u * b + 127500u) / 255000u + 16u;
}

// data_to_img (reference main.rs:175): clamp(floor(255 v + 0.5), 0, 255) in f32 -- a product, then a sum (contraction is off)
__device__ __forceinline__ uint32_t quantise(float v) {
    const float q = floorf(v * 255.0f + 0.5f);
    return (uint32_t)fminf(fmaxf(q, 0.0f), 255.0f);
}

// rows x cols pixels (at most kA x kA) of a u8 image from (y0, x0) -> their luma at s_y[r * kYP + c]; the rest of the tile is 0
template <int CH>
struct OperandU8 {
    static __device__ __forceinline__ void load(const void* img, long pitch, long, int y0, int x0, int rows, int cols, uint8_t* s_y) {
        constexpr int G = (kA + 3) / 4;  // groups of 4 pixels per tile row
        for (int i = threadIdx.x; i < kA * G; i += 256) {
            const int r = i / G, c = 4 * (i - r * G);
            uint32_t y4 = 0;
            if (r < rows && c < cols) {
                const uint8_t* p = (const uint8_t*)img + ((size_t)(y0 + r) * pitch + (size_t)(x0 + c)) * CH;
                if (c + 4 <= cols) {
                    BytePiece<4 * CH> piece;
                    piece.load(p);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        y4 |= luma(piece.byte(CH * j), piece.byte(CH * j + 1), piece.byte(CH * j + 2)) << (8 * j);
                } else {  // the row's last, partial group: byte by byte, each from the aligned dword that holds it
                    for (int j = 0; c + j < cols; ++j) {
                        uint32_t v[3];
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const uint8_t* q = p + CH * j + k;
                            const uint32_t mis = (uint32_t)(uintptr_t)q & 3u;
                            v[k] = (*(const uint32_t*)(q - mis) >> (8 * mis)) & 0xffu;
                        }
                        y4 |= luma(v[0], v[1], v[2]) << (8 * j);
                    }
                }
            }
            *(uint32_t*)(s_y + r * kYP + c) = y4;
        }
    }
};

// ... of the f32 output: contiguous (pitch = its width), 16-byte aligned, npx pixels in all.  A work item is an aligned group of four
// pixels of the whole image (it may begin before the tile row or end behind it: those pixels are dropped); the image's last, partial
// group goes value by value.  Pixels of the tile outside rows x cols keep whatever the LDS held: no valid window reads them.
struct OperandF32 {
    static __device__ __forceinline__ void load(const void* img, long pitch, long npx, int y0, int x0, int rows, int cols, uint8_t* s_y) {
        constexpr int G = kA / 4 + 2;  // aligned groups that kA consecutive pixels can touch
        const float* out = (const float*)img;
        for (int i = threadIdx.x; i < kA * G; i += 256) {
            const int r = i / G, k = i - r * G;
            if (r >= rows) continue;
            const long p0 = (long)(y0 + r) * pitch + x0;  // the tile row's first pixel
            const long g0 = (p0 & ~3L) + 4 * k;
            if (g0 >= p0 + cols) continue;
            float v[12];
            if (g0 + 4 <= npx) {
                const f32x4* o4 = (const f32x4*)(out + 3 * g0);
                const f32x4 a = o4[0], b = o4[1], c = o4[2];
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) v[j] = g0 + j / 3 < npx ? out[3 * g0 + j] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long c = g0 + j - p0;
                if (c >= 0 && c < cols) s_y[r * kYP + (int)c] = (uint8_t)luma(quantise(v[3 * j]), quantise(v[3 * j + 1]), quantise(v[3 * j + 2]));
            }
        }
    }
};

__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t* s_part) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// a, b: the images' first pixels; the tile of block t begins at region pixel (kT (t / tiles_x), kT (t % tiles_x)), image pixel + (s, s)
template <class OpA, class OpB>
__global__ __launch_bounds__(256) void metrics_tile_kernel(const void* __restrict__ a, const void* __restrict__ b, MetricsGeo geo,
                                                           double* __restrict__ part_ssim, unsigned long long* __restrict__ part_sse) {
    __shared__ __attribute__((aligned(16))) uint8_t s_ya[kA * kYP];
    __shared__ __attribute__((aligned(16))) uint8_t s_yb[kA * kYP];
    __shared__ double s_h[5][kA][kT];
    __shared__ double s_part[4];
    __shared__ uint32_t s_upart[4];
    const int ty = (int)(blockIdx.x / (unsigned)geo.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)geo.tiles_x);
    const int ry = ty * kT, rx = tx * kT;  // the tile's origin in the region
    const int rows = min(kA, geo.RH - ry), cols = min(kA, geo.RW - rx);        // pixels of the region the tile holds
    const int own_rows = min(kT, rows), own_cols = min(kT, cols);              // ... and owns
    const int win_rows = min(kT, geo.RH - 10 - ry), win_cols = min(kT, geo.RW - 10 - rx);  // its valid window positions (<= 0: none)
    OpA::load(a, geo.pitch_a, geo.npx_a, geo.s + ry, geo.s + rx, rows, cols, s_ya);
    OpB::load(b, geo.pitch_b, 0, geo.s + ry, geo.s + rx, rows, cols, s_yb);
    __syncthreads();

    uint32_t sse = 0;  // (at most 4 x 219^2 per thread, 1024 x 219^2 per workgroup)
    for (int i = threadIdx.x; i < kT * kT; i += 256) {
        const int r = i / kT, c = i - r * kT;
        if (r < own_rows && c < own_cols) {
            const int d = (int)s_ya[r * kYP + c] - (int)s_yb[r * kYP + c];
            sse += (uint32_t)(d * d);
        }
    }

    double acc = 0.0;
    if (win_rows > 0 && win_cols > 0) {  // (the same for the whole workgroup)
        for (int i = threadIdx.x; i < kA * kT; i += 256) {
            const int r = i / kT, c = i - r * kT;
            if (r < win_rows + 10 && c < win_cols) {
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const double ya = (double)s_ya[r * kYP + c + k], yb = (double)s_yb[r * kYP + c + k], w = geo.g[k];
                    m[0] = __builtin_fma(w, ya, m[0]);
                    m[1] = __builtin_fma(w, yb, m[1]);
                    m[2] = __builtin_fma(w, ya * ya, m[2]);  // (products of bytes: exact)
                    m[3] = __builtin_fma(w, yb * yb, m[3]);
                    m[4] = __builtin_fma(w, ya * yb, m[4]);
                }
#pragma unroll
                for (int q = 0; q < 5; ++q) s_h[q][r][c] = m[q];
            }
        }
        __syncthreads();
        constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
        for (int i = threadIdx.x; i < kT * kT; i += 256) {
            const int r = i / kT, c = i - r * kT;
            if (r < win_rows && c < win_cols) {
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const double w = geo.g[k];
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = __builtin_fma(w, s_h[q][r + k][c], m[q]);
                }
                // identical operands: m[0] == m[1] and m[2] == m[3] == m[4] bit for bit, so numerator and denominator are the same
                // double (2 x == x + x) and the map is exactly 1
                const double mab = m[0] * m[1], maa = m[0] * m[0], mbb = m[1] * m[1];
                const double va = m[2] - maa, vb = m[3] - mbb, vab = m[4] - mab;
                acc += ((2.0 * mab + C1) * (2.0 * vab + C2)) / ((maa + mbb + C1) * (va + vb + C2));
            }
        }
    }
    acc = block_sum(acc, s_part);
    sse = block_sum_u32(sse, s_upart);
    if (threadIdx.x == 0) {
        part_ssim[blockIdx.x] = acc;
        part_sse[blockIdx.x] = sse;
    }
}

// one workgroup: partials t, t + 256, ... per thread, then the workgroup's sums; the 16-byte result -- the u64 luma SSE, then the f64
// SSIM sum -- is stored as four dwords (the caller's pointer is only 4-byte aligned).  n = 0 (an empty region): zeros.
__global__ __launch_bounds__(256) void metrics_sum_kernel(const double* __restrict__ part_ssim, const unsigned long long* __restrict__ part_sse,
                                                          int n, uint32_t* __restrict__ result) {
    __shared__ double s_part[4];
    __shared__ unsigned long long s_sse[256];
    double acc = 0.0;
    unsigned long long sse = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        acc += part_ssim[i];
        sse += part_sse[i];
    }
    acc = block_sum(acc, s_part);
    s_sse[threadIdx.x] = sse;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int i = 0; i < 256; ++i) total += s_sse[i];
        const uint64_t bits = (uint64_t)__double_as_longlong(acc);
        result[0] = (uint32_t)total;
        result[1] = (uint32_t)(total >> 32);
        result[2] = (uint32_t)bits;
        result[3] = (uint32_t)(bits >> 32);
    }
}

template <class OpA>
void launch_tiles(int b_ch, unsigned blocks, const void* a, const void* b, const MetricsGeo& geo, double* ps, unsigned long long* pe, hipStream_t s) {
    if (b_ch == 3) hipLaunchKernelGGL((metrics_tile_kernel<OpA, OperandU8<3>>), dim3(blocks), dim3(256), 0, s, a, b, geo, ps, pe);
    else hipLaunchKernelGGL((metrics_tile_kernel<OpA, OperandU8<4>>), dim3(blocks), dim3(256), 0, s, a, b, geo, ps, pe);
}

}  // namespace

long sr_metrics_blocks(int H, int W, int shave) {
    const long RH = (long)H - 2L * shave, RW = (long)W - 2L * shave;
    if (RH <= 0 || RW <= 0) return 0;
    return ((RH + kT - 1) / kT) * ((RW + kT - 1) / kT);
}

hipError_t sr_launch_metrics(const void* d_a, bool a_u8, int a_ch, long pitch_a, const uint8_t* d_b, int b_ch, long pitch_b, int H, int W,
                             int shave, const double* weights, void* d_partial, void* d_result16, hipStream_t s) {
    if (H <= 0 || W <= 0 || shave < 0 || !sr_hr_channels_ok(a_u8, a_ch) || !sr_hr_channels_ok(true, b_ch) || pitch_a < W || pitch_b < W)
        return hipErrorInvalidValue;
    if (!a_u8 && (pitch_a != W || ((uintptr_t)d_a & 15u))) return hipErrorInvalidValue;
    const long blocks = sr_metrics_blocks(H, W, shave);
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    double* ps = (double*)d_partial;
    unsigned long long* pe = (unsigned long long*)(ps + blocks);
    if (blocks > 0) {
        MetricsGeo geo;
        geo.s = shave;
        geo.RH = H - 2 * shave;
        geo.RW = W - 2 * shave;
        geo.tiles_x = (geo.RW + kT - 1) / kT;
        geo.pitch_a = pitch_a;
        geo.pitch_b = pitch_b;
        geo.npx_a = (long)H * W;
        for (int k = 0; k < 11; ++k) geo.g[k] = weights[k];
        if (!a_u8) launch_tiles<OperandF32>(b_ch, (unsigned)blocks, d_a, d_b, geo, ps, pe, s);
        else if (a_ch == 3) launch_tiles<OperandU8<3>>(b_ch, (unsigned)blocks, d_a, d_b, geo, ps, pe, s);
        else launch_tiles<OperandU8<4>>(b_ch, (unsigned)blocks, d_a, d_b, geo, ps, pe, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(metrics_sum_kernel, dim3(1), dim3(256), 0, s, ps, pe, (int)blocks, (uint32_t*)d_result16);
    return hipGetLastError();
}
