// sr_optim.hip -- what a long training run adds to the optimiser (include/srhip.h "Optimiser"): the gradient's norm in f64 with a fixed
// order of additions, the clipping scale and the skip flag made from it on the device, and Adam on the scaled gradient with an optional
// average of the parameters.  No atomics, no host round trip.  Built with -ffp-contract=off like the rest of the library: every product
// and sum below is its own rounding.
#include <hip/hip_runtime.h>

#include "sr_internal.h"
#include "sr_reduce.h"

namespace {

// Partial b = the block_sum of (double)g[256 b + t]^2 over the workgroup's 256 lanes t (lanes past n add 0.0).  One dword a lane: the
// order of additions is a function of n alone, whatever the pointer's alignment.
__global__ __launch_bounds__(256) void optim_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part) {
    __shared__ double s_part[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if (i < n) {
        const double d = (double)g[i];
        acc = d * d;
    }
    acc = block_sum(acc, s_part);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// One workgroup: lane t adds partials t, t + 256, t + 512, ... in that order, then block_sum.  From S: the norm, the scale, the flag.
// mirror (optional): a second copy of the result, for a ring the host reads.
__global__ __launch_bounds__(256) void optim_norm_kernel(const double* __restrict__ part, unsigned nparts, float clip, sr_grad_norm* __restrict__ out,
                                                         sr_grad_norm* __restrict__ mirror) {
    __shared__ double s_part[4];
    double acc = 0.0;
    for (unsigned k = threadIdx.x; k < nparts; k += 256) acc += part[k];
    const double S = block_sum(acc, s_part);
    if (threadIdx.x != 0) return;
    const double norm = __builtin_sqrt(S);
    sr_grad_norm r;
    r.sumsq = S;
    r.scale = (clip > 0.0f && norm > (double)clip) ? (float)((double)clip / norm) : 1.0f;
    r.skip = __builtin_isfinite(S) ? 0 : 1;  // every square is >= 0: S is NaN or +inf exactly when some element is not finite
    *out = r;
    if (mirror) *mirror = r;
}

// grad_adam_kernel's arithmetic (sr_grad.hip), in its written order, on gc = scale g; then the average on the parameter just written
__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, float scale, float lr, float b1, float b2, float eps, float bc1,
                                         float bc2) {
    const float gi = scale * g;
    const float mi = b1 * m + (1.0f - b1) * gi;
    const float vi = b2 * v + (1.0f - b2) * (gi * gi);
    m = mi;
    v = vi;
    const float mh = mi / bc1, vh = vi / bc2;
    p = p - lr * mh / (__builtin_sqrtf(vh) + eps);
}

// WIDE: 4 elements a lane through 16-byte accesses (every pointer 16-byte aligned; the last lane takes the n % 4 tail as dwords);
// otherwise one dword a lane.  The arithmetic is per element either way.
template <bool WIDE, bool EMA>
__global__ __launch_bounds__(256) void optim_adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                         float* __restrict__ e, size_t n, float lr, float b1, float b2, float eps, float bc1, float bc2,
                                                         float d, float omd, const sr_grad_norm* __restrict__ norm,
                                                         unsigned long long* __restrict__ skipped) {
    float scale = 1.0f;
    if (norm) {
        if (norm->skip) {  // (uniform over the launch) nothing is written but the count
            if (skipped && blockIdx.x == 0 && threadIdx.x == 0) *skipped = *skipped + 1;
            return;
        }
        scale = norm->scale;
    }
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (WIDE) {
        const size_t i = 4 * t;
        if (i + 4 <= n) {
            float4 pp = *(const float4*)(p + i), mm = *(const float4*)(m + i), vv = *(const float4*)(v + i);
            const float4 gg = *(const float4*)(g + i);
            adam_one(pp.x, mm.x, vv.x, gg.x, scale, lr, b1, b2, eps, bc1, bc2);
            adam_one(pp.y, mm.y, vv.y, gg.y, scale, lr, b1, b2, eps, bc1, bc2);
            adam_one(pp.z, mm.z, vv.z, gg.z, scale, lr, b1, b2, eps, bc1, bc2);
            adam_one(pp.w, mm.w, vv.w, gg.w, scale, lr, b1, b2, eps, bc1, bc2);
            *(float4*)(m + i) = mm;
            *(float4*)(v + i) = vv;
            *(float4*)(p + i) = pp;
            if constexpr (EMA) {
                float4 ee = *(const float4*)(e + i);
                ee.x = d * ee.x + omd * pp.x;
                ee.y = d * ee.y + omd * pp.y;
                ee.z = d * ee.z + omd * pp.z;
                ee.w = d * ee.w + omd * pp.w;
                *(float4*)(e + i) = ee;
            }
            return;
        }
        for (size_t k = i; k < n; ++k) {
            float pk = p[k], mk = m[k], vk = v[k];
            adam_one(pk, mk, vk, g[k], scale, lr, b1, b2, eps, bc1, bc2);
            m[k] = mk;
            v[k] = vk;
            p[k] = pk;
            if constexpr (EMA) e[k] = d * e[k] + omd * pk;
        }
    } else {
        if (t >= n) return;
        float pk = p[t], mk = m[t], vk = v[t];
        adam_one(pk, mk, vk, g[t], scale, lr, b1, b2, eps, bc1, bc2);
        m[t] = mk;
        v[t] = vk;
        p[t] = pk;
        if constexpr (EMA) e[t] = d * e[t] + omd * pk;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

size_t sr_optim_parts(size_t n) { return (n + 255) / 256; }

hipError_t sr_launch_grad_norm(const float* d_grad, size_t n, float clip, double* d_part, sr_grad_norm* d_out, sr_grad_norm* d_mirror, hipStream_t s) {
    const size_t parts = sr_optim_parts(n);
    if (parts == 0 || parts > (size_t)INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)parts), dim3(256), 0, s, d_grad, n, d_part);
    hipLaunchKernelGGL(optim_norm_kernel, dim3(1), dim3(256), 0, s, (const double*)d_part, (unsigned)parts, clip, d_out, d_mirror);
    return hipGetLastError();
}

hipError_t sr_launch_adam_clipped(float* d_p, float* d_m, float* d_v, const float* d_g, float* d_e, size_t n, float lr, float b1, float b2, float eps,
                                  float bc1, float bc2, float d, float omd, const sr_grad_norm* d_norm, unsigned long long* d_skipped,
                                  hipStream_t s) {
    const bool wide = aligned16(d_p) && aligned16(d_m) && aligned16(d_v) && aligned16(d_g) && aligned16(d_e);  // (a null d_e passes)
    const size_t lanes = wide ? (n + 3) / 4 : n, blocks = (lanes + 255) / 256;
    if (blocks == 0 || blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_p, d_m, d_v, d_g, d_e, n, lr, b1, b2, eps, bc1, bc2, d, omd, d_norm,
                           d_skipped);
    };
    if (wide) {
        if (d_e) go(optim_adam_kernel<true, true>);
        else go(optim_adam_kernel<true, false>);
    } else {
        if (d_e) go(optim_adam_kernel<false, true>);
        else go(optim_adam_kernel<false, false>);
    }
    return hipGetLastError();
}
