// sr_deep.hip -- the two conversions of the deep-colour path (include/srhip.h "Deep colour"; host side: sr_deep.cpp): 16-bit samples to
// the network's f32 RGB input, and the network's unquantised f32 output back to 16-bit samples, quantised once.  tests/deep_ref.py is
// the rule in numpy; the arithmetic here is f32 in the written order, every product, sum and quotient rounded once: the file is built
// without contraction (build.py FLAGS) and the divisions are IEEE divisions, so the kernels equal the restatement bit for bit.
//
// Both are streaming kernels over the flat pixel index of the whole batch (the rule acts on one pixel at a time, so the images' shape
// does not enter).  A lane takes one GROUP of 8 pixels:
//   u16_to_f32_kernel<IC>   8 pixels are IC 16-byte loads (8 IC samples) and six 16-byte stores (24 floats);
//   f32_to_u16_kernel<OC>   8 pixels are six 16-byte loads, all issued before the first use, and OC = 3: three, OC = 4: four, OC = 1: one
//                           16-byte store.  The one that carries the bytes: at 5760 x 3240 it reads 224 MB and writes 112-149 MB.
// IN16 / OUT16: that side's pointer is 16-byte aligned, so every group of it is (a group is 16 IC, 96, 48, 64 or 16 bytes): the wide form.
// Otherwise that side is read or written sample by sample -- dwords for f32 (4-byte aligned), shorts for u16 (2-byte aligned).  The host
// picks either side's form from the pointer (sr_launch_*); the composed calls' workspace buffers always take the wide one.
// The tail -- a pixel count that is not a multiple of 8 -- is the last lane's: up to 7 pixels, sample by sample.
//
// No LDS, no scratch; the group's values live in registers through compile-time indices.  Grid: 256 lanes = 2048 pixels a workgroup, a
// function of the pixel count alone (sr_deep_blocks); nothing loops.  Every output sample belongs to exactly one lane, no atomics: the
// same bits on every run.  All offsets are 64-bit.  Resources: profiles/deep_kernel_resources.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 8;  // pixels a lane takes

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float to_unit(uint32_t v) { return (float)v / 65535.0f; }

// floor(65535 v + 0.5) clamped to 0 .. 65535; NaN -> 0 (fmaxf gives its other argument)
__device__ __forceinline__ uint32_t quantise(float v) {
    return (uint32_t)fminf(fmaxf(floorf(65535.0f * v + 0.5f), 0.0f), 65535.0f);
}

__device__ __forceinline__ float grey_of(float r, float g, float b) { return ((r + g) + b) / 3.0f; }

// ---- 16-bit samples -> f32 RGB ---------------------------------------------------------------------------------------------------------
template <int IC, bool IN16, bool OUT16>
__global__ __launch_bounds__(kThreads) void u16_to_f32_kernel(const uint16_t* __restrict__ in, float* __restrict__ out, size_t npx) {
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, p0 = g * kGroup;
    if (p0 >= npx) return;
    const uint16_t* __restrict__ src = in + p0 * IC;
    float* __restrict__ dst = out + p0 * 3;
    if (p0 + kGroup > npx) {  // the tail: sample by sample
        const int left = (int)(npx - p0);
        for (int i = 0; i < left; ++i) {
            const float r = to_unit(src[i * IC]);
            const float gr = IC >= 3 ? to_unit(src[i * IC + 1]) : r, b = IC >= 3 ? to_unit(src[i * IC + 2]) : r;
            dst[i * 3] = r;
            dst[i * 3 + 1] = gr;
            dst[i * 3 + 2] = b;
        }
        return;
    }
    uint32_t word[IC * 4];  // the group's 8 IC samples, two a dword
    if (IN16) {
#pragma unroll
        for (int q = 0; q < IC; ++q) {
            const u32x4 t = ((const u32x4*)src)[q];
            word[4 * q] = t.x; word[4 * q + 1] = t.y; word[4 * q + 2] = t.z; word[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < IC * 4; ++q) word[q] = (uint32_t)src[2 * q] | ((uint32_t)src[2 * q + 1] << 16);
    }
    const auto sample = [&](int j) { return (j & 1) ? word[j >> 1] >> 16 : word[j >> 1] & 0xffffu; };
    float v[kGroup * 3];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        const float r = to_unit(sample(i * IC));
        v[3 * i] = r;
        v[3 * i + 1] = IC >= 3 ? to_unit(sample(i * IC + 1)) : r;
        v[3 * i + 2] = IC >= 3 ? to_unit(sample(i * IC + 2)) : r;
    }
    if (OUT16) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            f32x4 t;
            t.x = v[4 * q]; t.y = v[4 * q + 1]; t.z = v[4 * q + 2]; t.w = v[4 * q + 3];
            ((f32x4*)dst)[q] = t;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kGroup * 3; ++q) dst[q] = v[q];
    }
}

// ---- f32 RGB -> 16-bit samples ---------------------------------------------------------------------------------------------------------
template <int OC, bool IN16, bool OUT16>
__global__ __launch_bounds__(kThreads) void f32_to_u16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, size_t npx) {
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, p0 = g * kGroup;
    if (p0 >= npx) return;
    const float* __restrict__ src = in + p0 * 3;
    uint16_t* __restrict__ dst = out + p0 * OC;
    if (p0 + kGroup > npx) {  // the tail: sample by sample
        const int left = (int)(npx - p0);
        for (int i = 0; i < left; ++i) {
            const float r = src[3 * i], gr = src[3 * i + 1], b = src[3 * i + 2];
            if (OC == 1) {
                dst[i] = (uint16_t)quantise(grey_of(r, gr, b));
            } else {
                dst[i * OC] = (uint16_t)quantise(r);
                dst[i * OC + 1] = (uint16_t)quantise(gr);
                dst[i * OC + 2] = (uint16_t)quantise(b);
                if (OC == 4) dst[i * OC + 3] = 0xffffu;
            }
        }
        return;
    }
    float v[kGroup * 3];
    if (IN16) {  // six independent 16-byte loads in flight before the first use
        f32x4 t[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) t[q] = ((const f32x4*)src)[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            v[4 * q] = t[q].x; v[4 * q + 1] = t[q].y; v[4 * q + 2] = t[q].z; v[4 * q + 3] = t[q].w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kGroup * 3; ++q) v[q] = src[q];
    }
    uint32_t s[kGroup * OC];  // the group's samples
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
        if (OC == 1) {
            s[i] = quantise(grey_of(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
        } else {
            s[i * OC] = quantise(v[3 * i]);
            s[i * OC + 1] = quantise(v[3 * i + 1]);
            s[i * OC + 2] = quantise(v[3 * i + 2]);
            if (OC == 4) s[i * OC + 3] = 0xffffu;
        }
    }
    if (OUT16) {
#pragma unroll
        for (int q = 0; q < OC * kGroup / 8; ++q) {
            u32x4 t;
            t.x = s[8 * q] | (s[8 * q + 1] << 16);
            t.y = s[8 * q + 2] | (s[8 * q + 3] << 16);
            t.z = s[8 * q + 4] | (s[8 * q + 5] << 16);
            t.w = s[8 * q + 6] | (s[8 * q + 7] << 16);
            ((u32x4*)dst)[q] = t;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kGroup * OC; ++q) dst[q] = (uint16_t)s[q];
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int IC>
hipError_t launch_to_f32(const uint16_t* d_in, size_t npx, float* d_out, unsigned blocks, hipStream_t s) {
    const bool i16 = aligned16(d_in), o16 = aligned16(d_out);
    if (i16 && o16) u16_to_f32_kernel<IC, true, true><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    else if (i16) u16_to_f32_kernel<IC, true, false><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    else if (o16) u16_to_f32_kernel<IC, false, true><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    else u16_to_f32_kernel<IC, false, false><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    return hipGetLastError();
}

template <int OC>
hipError_t launch_to_u16(const float* d_in, size_t npx, uint16_t* d_out, unsigned blocks, hipStream_t s) {
    const bool i16 = aligned16(d_in), o16 = aligned16(d_out);
    if (i16 && o16) f32_to_u16_kernel<OC, true, true><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    else if (i16) f32_to_u16_kernel<OC, true, false><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    else if (o16) f32_to_u16_kernel<OC, false, true><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    else f32_to_u16_kernel<OC, false, false><<<blocks, kThreads, 0, s>>>(d_in, d_out, npx);
    return hipGetLastError();
}

}  // namespace

size_t sr_deep_blocks(size_t npx) {
    const size_t groups = npx / kGroup + (npx % kGroup ? 1 : 0);
    return groups / kThreads + (groups % kThreads ? 1 : 0);
}

const char* sr_deep_form(const void* d_in, const void* d_out) {
    const bool i16 = aligned16(d_in), o16 = aligned16(d_out);
    return i16 && o16 ? "wide" : i16 ? "wide_in" : o16 ? "wide_out" : "narrow";
}

hipError_t sr_launch_u16_to_f32(const uint16_t* d_in, int in_channels, size_t npx, float* d_out, hipStream_t s) {
    const size_t blocks = sr_deep_blocks(npx);
    if (blocks == 0 || blocks > (size_t)INT32_MAX || in_channels < 1 || in_channels > 4) return hipErrorInvalidValue;
    switch (in_channels) {
        case 1: return launch_to_f32<1>(d_in, npx, d_out, (unsigned)blocks, s);
        case 2: return launch_to_f32<2>(d_in, npx, d_out, (unsigned)blocks, s);
        case 3: return launch_to_f32<3>(d_in, npx, d_out, (unsigned)blocks, s);
        default: return launch_to_f32<4>(d_in, npx, d_out, (unsigned)blocks, s);
    }
}

hipError_t sr_launch_f32_to_u16(const float* d_in, size_t npx, uint16_t* d_out, int out_channels, hipStream_t s) {
    const size_t blocks = sr_deep_blocks(npx);
    if (blocks == 0 || blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    switch (out_channels) {
        case 1: return launch_to_u16<1>(d_in, npx, d_out, (unsigned)blocks, s);
        case 3: return launch_to_u16<3>(d_in, npx, d_out, (unsigned)blocks, s);
        case 4: return launch_to_u16<4>(d_in, npx, d_out, (unsigned)blocks, s);
        default: return hipErrorInvalidValue;
    }
}
