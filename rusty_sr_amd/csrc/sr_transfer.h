// sr_transfer.h -- the sRGB transfer functions of the training graph's device code (sr_valid.hip, sr_grad.hip), with the constants of
// sr_aux.hip (alumina SrgbToLinear / LinearToSrgb: IEC 61966-2-1).  Device code only; included by .hip sources.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

__device__ __forceinline__ float fast_pow(float x, float p) { return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x)); }
__device__ __forceinline__ float srgb_to_linear_fast(float s) { return s <= 0.04045f ? s / 12.92f : fast_pow((s + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float linear_to_srgb_fast(float l) { return l <= 0.0031308f ? 12.92f * l : 1.055f * fast_pow(l, 1.0f / 2.4f) - 0.055f; }
// ... SrgbToLinear on the library's powf: the expression sr_aux.hip's lut_kernel tabulates for the 256 bytes (sr_resize.hip builds the same
// table in LDS), and data_to_img (main.rs:175) of one value
__device__ __forceinline__ float srgb_to_linear_powf(float s) { return s <= 0.04045f ? s / 12.92f : powf((s + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ uint32_t quant_u8(float v) { return (uint32_t)fminf(fmaxf(floorf(255.0f * v + 0.5f), 0.0f), 255.0f); }

// SrgbToLinear(s), correctly rounded to f32 but for inputs within ~1e-16 relative of a rounding boundary: the f64 formula
// ((s + 0.055) / 1.055)^2.4, with the power as a^2 * y, y = (a^2)^(1/5) refined by two Newton steps from the hardware estimate
// (relative error ~3e-7 -> ~1e-13 -> below f64 rounding).  The same formula holds outside [0, 1] (s > 1; s <= 0.04045: s / 12.92).
__device__ __forceinline__ float srgb_to_linear_cr(float s) {
    if (s <= 0.04045f) return (float)((double)s * (1.0 / 12.92));
    const double a = ((double)s + 0.055) * (1.0 / 1.055);
    const double t = a * a;
    double y = (double)fast_pow((float)a, 0.4f);
#pragma unroll
    for (int it = 0; it < 2; ++it) {  // y <- y + y (t / y^5 - 1) / 5
        const double y2 = y * y, y5 = y2 * y2 * y;
        double r = __builtin_amdgcn_rcp(y5);
        r = fma(r, fma(-y5, r, 1.0), r);
        r = fma(r, fma(-y5, r, 1.0), r);
        const double e = fma(t, r, -1.0);
        y = fma(y * 0.2, e, y);
    }
    return (float)(t * y);
}
