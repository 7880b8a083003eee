// sr_valid.hip -- the forward half of the reference's training graph, for its validation pass (reference main.rs:220-247,
// network.rs:88-102), on gfx950:
//
//   input  = LinearToSrgb(mean_{f x f}(SrgbToLinear(hr)))       valid_pool_kernel    (the network's LR input, f32, not quantised)
//         or img_to_data(lr) of a supplied LR image (pairs)       lr_input_kernel      (u8; an f32 LR image is copied)
//   output = sr_net(f)(input)                                     the stage kernels (sr_kernels.hip), f32 output
//   err    = sum (output - hr)^2                                  valid_loss_kernel + loss_sum_kernel
//         or sum (SrgbToLinear(output) - SrgbToLinear(hr))^2     (-l / --linearLoss)
//
// over the top-left f*floor(h/f) x f*floor(w/f) crop of the HR image (UNPINNED: the remainder rule of the downsample graph).
//
// Pool: one thread per LR pixel, nothing staged.  Each of its f rows is read as the aligned dwords that hold the row's f*CH bytes (u8,
// shifted into place with v_alignbyte, as downsample_net's kernel in sr_aux.hip does) or as 3f floats; SrgbToLinear of a byte is the
// context's 256-entry table (LDS), of a float the hardware log2 / exp2 form; LinearToSrgb likewise on v_log_f32 / v_exp_f32.  Error of
// the LR image against an f64 restatement: below 2e-6 absolute for inputs in [-0.5, 1.5] (tests/test_gpu_validation.py; 2.1e-7 measured
// on dark, bright and out-of-range pixels, tests/test_gpu_pixel_ranges.py), beyond that range below 2e-6 relative to the value (f32
// itself keeps no absolute bar there); the same class as the aux graphs' f32 entry points (1.8e-7 measured there,
// tests/measure_aux_error.py), plus the f32 sum of f*f samples.
//
// Loss: memory-bound (a 4K HR image: 100 MB of f32 output + 33 MB of RGBA8), so the kernel is sized against the measured 6.29 TB/s copy
// rate: a thread takes 4 output pixels at a time -- three 16-byte loads of the output, the 4 HR pixels as the aligned dwords that hold
// them -- and every difference is formed in f32 and squared and summed in f64.  One f64 partial per workgroup; the grid depends on
// the shape alone (never on the CU count), and loss_sum_kernel adds the partials in a fixed order in one workgroup: the result is
// the same bits on every run, context and device.  No atomics.
// In linear-loss mode SrgbToLinear must be a function the tests can restate bit for bit: it is the correctly rounded f32 of the
// formula (an f32 estimate on the hardware pow, two Newton steps for the fifth root in f64 -- x^2.4 = x^2 * (x^2)^(1/5) -- then one
// rounding), and the HR bytes' table holds the same rounding of the same formula, computed on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "sr_bytes.h"
#include "sr_internal.h"
#include "sr_reduce.h"
#include "sr_transfer.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct __attribute__((packed, aligned(4))) F3 { float v[3]; };

// HR (n = 1, h x w x CH u8, or h x w x 3 f32) -> LR (h/f x w/f x 3 f32).  tab: 256 floats SrgbToLinear(byte / 255) (u8 only).
template <int F, bool HR_U8, int CH>
__global__ __launch_bounds__(256) void valid_pool_kernel(const void* __restrict__ hr, float* __restrict__ lr, const float* __restrict__ tab,
                                                         int W, int OH, int OW) {
    __shared__ float s_lin[HR_U8 ? 256 : 1];
    if constexpr (HR_U8) {
        s_lin[threadIdx.x] = tab[threadIdx.x];
        __syncthreads();
    }
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)OH * OW) return;
    const int oy = (int)(idx / OW), ox = (int)(idx - (long)oy * OW);
    float acc[3] = {0.f, 0.f, 0.f};
    if constexpr (HR_U8) {
        BytePiece<F * CH> piece[F];
#pragma unroll
        for (int dy = 0; dy < F; ++dy)
            piece[dy].load((const uint8_t*)hr + ((size_t)(F * oy + dy) * W + (size_t)F * ox) * CH);
#pragma unroll
        for (int dy = 0; dy < F; ++dy)  // rows, then columns: the reference's order
#pragma unroll
            for (int dx = 0; dx < F; ++dx)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += s_lin[piece[dy].byte(CH * dx + c)];
    } else {
        float v[F][3 * F];
#pragma unroll
        for (int dy = 0; dy < F; ++dy) {
            const float* src = (const float*)hr + ((size_t)(F * oy + dy) * W + (size_t)F * ox) * 3;
#pragma unroll
            for (int k = 0; k < 3 * F; ++k) v[dy][k] = src[k];
        }
#pragma unroll
        for (int dy = 0; dy < F; ++dy)
#pragma unroll
            for (int dx = 0; dx < F; ++dx)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += srgb_to_linear_fast(v[dy][3 * dx + c]);
    }
    F3 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) o.v[c] = linear_to_srgb_fast(acc[c] / (float)(F * F));
    ((F3*)lr)[idx] = o;
}

// A supplied LR batch (pairs): npx pixels of CH bytes, contiguous from any byte address -> npx x 3 f32, img_to_data (tab: byte / 255).
// One thread per four consecutive output floats, which cross pixel boundaries: of an RGB source they are four consecutive bytes (the two
// aligned dwords that hold them, shifted into place with v_alignbyte), of an RGBA source RGB bytes c .. c + 3 of two pixels (three aligned
// dwords at most); every store is a whole 16-byte group, consecutive across the wave.  The last, partial group goes float by float,
// each byte from the aligned dword that holds it: nothing outside the words of the image is read, nothing outside x written.
template <int CH>
__global__ __launch_bounds__(256) void lr_input_kernel(const uint8_t* __restrict__ lr, float* __restrict__ x, const float* __restrict__ tab, long nval) {
    __shared__ float s_tab[256];
    s_tab[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    const long v0 = 4 * ((long)blockIdx.x * 256 + threadIdx.x);  // the first of this thread's values (value v: pixel v / 3, channel v % 3)
    if (v0 >= nval) return;
    if (v0 + 4 <= nval) {
        uint32_t word;
        if constexpr (CH == 3) {
            const uint8_t* p = lr + v0;
            const uint32_t mis = (uint32_t)(uintptr_t)p & 3u;
            const uint32_t* q = (const uint32_t*)(p - mis);
            const uint32_t w0 = q[0], w1 = mis ? q[1] : 0u;  // (with mis > 0, q[1] holds byte 3 of the run: inside the image)
            word = __builtin_amdgcn_alignbyte(w1, w0, mis);
        } else {
            const long px = v0 / 3;
            const int c = (int)(v0 - 3 * px);
            const uint8_t* p = lr + 4 * px;  // pixels px, px + 1 (the second exists: value v0 + 3 is in it)
            const uint32_t mis = (uint32_t)(uintptr_t)p & 3u;
            const uint32_t* q = (const uint32_t*)(p - mis);
            const uint32_t w0 = q[0], w1 = q[1], w2 = mis ? q[2] : 0u;  // (with mis > 0, q[2] holds pixel px + 1's last byte)
            const uint32_t p0 = __builtin_amdgcn_alignbyte(w1, w0, mis), p1 = __builtin_amdgcn_alignbyte(w2, w1, mis);
            const uint64_t rgb = (uint64_t)(p0 & 0xffffffu) | ((uint64_t)(p1 & 0xffffffu) << 24);
            word = (uint32_t)(rgb >> (8 * c));
        }
        f32x4 v;
        v.x = s_tab[word & 0xffu];
        v.y = s_tab[(word >> 8) & 0xffu];
        v.z = s_tab[(word >> 16) & 0xffu];
        v.w = s_tab[word >> 24];
        *(f32x4*)(x + v0) = v;
    } else {
        for (long v = v0; v < nval; ++v) {
            const long px = v / 3;
            const uint8_t* p = lr + CH * px + (v - 3 * px);
            const uint32_t mis = (uint32_t)(uintptr_t)p & 3u;
            x[v] = s_tab[(*(const uint32_t*)(p - mis) >> (8 * mis)) & 0xffu];
        }
    }
}

constexpr int kLossMaxGrid = 2048;   // workgroups of valid_loss_kernel at most (the number of f64 partials)

// out: the network's f32 output, HC x WC x 3, contiguous and 16-byte aligned (a context buffer); hr: the HR image, row pitch W pixels;
// tab: [0, 256) byte / 255 (img_to_data), [256, 512) srgb_to_linear_cr of those.  A work item is 4 consecutive output pixels.
template <bool HR_U8, int CH, bool LINEAR>
__global__ __launch_bounds__(256) void valid_loss_kernel(const float* __restrict__ out, const void* __restrict__ hr, const float* __restrict__ tab,
                                                         int W, int HC, int WC, double* __restrict__ partial) {
    __shared__ float s_tab[HR_U8 ? 256 : 1];
    __shared__ double s_part[4];
    if constexpr (HR_U8) {
        s_tab[threadIdx.x] = tab[(LINEAR ? 256 : 0) + threadIdx.x];
        __syncthreads();
    }
    const long npx = (long)HC * WC, items = (npx + 3) / 4;
    auto hr_value = [&](uint32_t byte_or_bits) -> float {
        if constexpr (HR_U8) return s_tab[byte_or_bits];
        else return LINEAR ? srgb_to_linear_cr(__uint_as_float(byte_or_bits)) : __uint_as_float(byte_or_bits);
    };
    auto out_value = [&](float v) -> float { return LINEAR ? srgb_to_linear_cr(v) : v; };
    double acc = 0.0;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const long p0 = 4 * it;
        const int y = (int)(p0 / WC), x = (int)(p0 - (long)y * WC);
        if (p0 + 4 <= npx && x + 4 <= WC) {  // four pixels of one row: contiguous in both images
            const f32x4* o4 = (const f32x4*)(out + 3 * p0);
            const f32x4 a = o4[0], b = o4[1], c = o4[2];
            const float o[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
            uint32_t h[12];
            if constexpr (HR_U8) {
                BytePiece<4 * CH> piece;
                piece.load((const uint8_t*)hr + ((size_t)y * W + x) * CH);
#pragma unroll
                for (int k = 0; k < 12; ++k) h[k] = piece.byte(CH * (k / 3) + k % 3);
            } else {
                const uint32_t* src = (const uint32_t*)hr + ((size_t)y * W + x) * 3;
#pragma unroll
                for (int k = 0; k < 12; ++k) h[k] = src[k];
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const double d = (double)(out_value(o[k]) - hr_value(h[k]));
                acc += d * d;
            }
        } else {  // a row seam (WC % 4 != 0) or the last, partial item: pixel by pixel
            for (int i = 0; i < 4 && p0 + i < npx; ++i) {
                const long p = p0 + i;
                const int py = (int)(p / WC), px = (int)(p - (long)py * WC);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    uint32_t hv;
                    if constexpr (HR_U8) hv = ((const uint8_t*)hr)[((size_t)py * W + px) * CH + k];
                    else hv = ((const uint32_t*)hr)[((size_t)py * W + px) * 3 + k];
                    const double d = (double)(out_value(out[3 * p + k]) - hr_value(hv));
                    acc += d * d;
                }
            }
        }
    }
    acc = block_sum(acc, s_part);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// one workgroup: partials t, t + 256, ... per thread, then the workgroup's sum; stored as two dwords (the caller's pointer is only
// 4-byte aligned).  Also the sum of the backward pass's loss partials (sr_grad.hip).
__global__ __launch_bounds__(256) void loss_sum_kernel(const double* __restrict__ partial, int n, uint32_t* __restrict__ result) {
    __shared__ double s_part[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    acc = block_sum(acc, s_part);
    if (threadIdx.x == 0) {
        const uint64_t bits = (uint64_t)__double_as_longlong(acc);
        result[0] = (uint32_t)bits;
        result[1] = (uint32_t)(bits >> 32);
    }
}

template <int F>
void launch_pool(const void* hr, bool hr_u8, int ch, float* lr, const float* tab, int W, int OH, int OW, hipStream_t s) {
    const dim3 grid((unsigned)(((long)OH * OW + 255) / 256));
    sr_dispatch_hr(hr_u8, ch, false, [&](auto u8, auto channels, auto) {  // (the pool is the same in both loss modes)
        hipLaunchKernelGGL((valid_pool_kernel<F, decltype(u8)::value, decltype(channels)::value>), grid, dim3(256), 0, s, hr, lr, tab, W, OH, OW);
    });
}

}  // namespace

int sr_valid_loss_grid(int HC, int WC) {
    const long items = ((long)HC * WC + 3) / 4;
    return (int)std::min<long>(kLossMaxGrid, std::max<long>(1, (items + 255) / 256));
}

hipError_t sr_launch_valid_pool(int factor, const void* d_hr, bool hr_u8, int ch, int W, int OH, int OW, float* d_lr, const float* d_tab,
                                hipStream_t s) {
    if (OH <= 0 || OW <= 0 || !sr_hr_channels_ok(hr_u8, ch)) return hipErrorInvalidValue;
    switch (factor) {
        case 2: launch_pool<2>(d_hr, hr_u8, ch, d_lr, d_tab, W, OH, OW, s); break;
        case 3: launch_pool<3>(d_hr, hr_u8, ch, d_lr, d_tab, W, OH, OW, s); break;
        case 4: launch_pool<4>(d_hr, hr_u8, ch, d_lr, d_tab, W, OH, OW, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t sr_launch_lr_input(const uint8_t* d_lr, int ch, long npx, float* d_x, const float* d_tab, hipStream_t s) {
    if (npx <= 0 || (ch != 3 && ch != 4) || ((uintptr_t)d_x & 15u)) return hipErrorInvalidValue;
    const long nval = 3 * npx;
    const dim3 grid((unsigned)(((nval + 3) / 4 + 255) / 256));
    if (ch == 3) hipLaunchKernelGGL(lr_input_kernel<3>, grid, dim3(256), 0, s, d_lr, d_x, d_tab, nval);
    else hipLaunchKernelGGL(lr_input_kernel<4>, grid, dim3(256), 0, s, d_lr, d_x, d_tab, nval);
    return hipGetLastError();
}

hipError_t sr_queue_lr_input(const sr_lr_input& lr, long npx, float* d_x, const float* d_tab, hipStream_t s) {
    if (lr.in_place) return hipSuccess;
    if (lr.u8) return sr_launch_lr_input((const uint8_t*)lr.d_lr, lr.ch, npx, d_x, d_tab, s);
    return hipMemcpyAsync(d_x, lr.d_lr, (size_t)npx * 3 * sizeof(float), hipMemcpyDeviceToDevice, s);
}

hipError_t sr_launch_valid_loss(const float* d_out, const void* d_hr, bool hr_u8, int ch, bool linear, int W, int HC, int WC, const float* d_tab,
                                double* d_partial, void* d_result, hipStream_t s) {
    if (HC <= 0 || WC <= 0 || !sr_hr_channels_ok(hr_u8, ch)) return hipErrorInvalidValue;
    const int grid = sr_valid_loss_grid(HC, WC);
    sr_dispatch_hr(hr_u8, ch, linear, [&](auto u8, auto channels, auto lin) {
        hipLaunchKernelGGL((valid_loss_kernel<decltype(u8)::value, decltype(channels)::value, decltype(lin)::value>), dim3(grid), dim3(256), 0,
                           s, d_out, d_hr, d_tab, W, HC, WC, d_partial);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return sr_launch_loss_sum(d_partial, grid, d_result, s);
}

hipError_t sr_launch_loss_sum(const double* d_partial, int n, void* d_result, hipStream_t s) {
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, s, d_partial, n, (uint32_t*)d_result);
    return hipGetLastError();
}
