// sr_bytes.h -- u8 images at any byte address, read as the aligned dwords that hold them (sr_valid.hip, sr_metrics.hip).  Device code only;
// included by .hip sources.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the aligned dwords that hold `len` bytes starting at p (all of them hold a byte of the piece: nothing outside the words of the
// image is read), then the piece's bytes 0 .. 4 NW - 1 in place
template <int LEN>
struct BytePiece {
    static constexpr int NW = (LEN + 3) / 4;
    uint32_t w[NW + 1];
    uint32_t mis;
    __device__ __forceinline__ void load(const uint8_t* p) {
        mis = (uint32_t)(uintptr_t)p & 3u;
        const uint32_t* src = (const uint32_t*)(p - mis);
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = src[k];
        w[NW] = (mis + LEN > 4 * NW) ? src[NW] : 0u;
    }
    __device__ __forceinline__ uint32_t byte(int b) const {  // b a compile-time constant after unrolling
        const uint32_t al = __builtin_amdgcn_alignbyte(w[(b >> 2) + 1], w[b >> 2], mis);
        return (al >> (8 * (b & 3))) & 0xffu;
    }
};
