// sr_reduce.h -- the f64 sum of a workgroup of 256, in a fixed order of additions: what makes the loss sums of the training graph's device
// code (sr_valid.hip, sr_grad.hip) the same bits on every run.  Device code only; included by .hip sources.
#pragma once
#include <hip/hip_runtime.h>

// sum over the 64 lanes of a wave by butterfly shuffles: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// workgroup of 256: every wave's sum, then the four in order; s_part: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* s_part) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) s_part[wave] = v;
    __syncthreads();
    return ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}
