// sr_reuse.hip -- the row compare of the frame stream's row reuse (include/srhip.h "Video"): flags[r] = 1 where row r of two
// byte buffers differs, else 0.  One launch covers up to three segments -- the three planes of a frame, each with its own row length --
// whose rows are numbered one after another.
//
// One wave owns a row (and, past the grid, the rows a whole grid further on).  Where both row pointers share their alignment modulo 16
// a lane loads 16 bytes of each per step over the aligned body of the row, and the bytes before and after it -- fewer than 16 each --
// one a lane; where they share it modulo 4 only, the same with 4-byte loads; else byte by byte.  The lanes' verdicts meet in a ballot
// and lane 0 stores the flag with a plain vector store: every flag is written exactly once, by one wave, whatever the data -- no
// atomics, nothing between waves, nothing to clear beforehand, the same bits on every run.  Nothing outside [row, row + row_bytes) is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

__device__ inline bool words_differ(uint4 x, uint4 y) { return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0; }
__device__ inline bool words_differ(uint32_t x, uint32_t y) { return x != y; }

// this lane's verdict on the nb bytes at pa and pb, which share their alignment modulo sizeof(T)
template <class T>
__device__ inline bool row_differs(const uint8_t* pa, const uint8_t* pb, size_t nb, unsigned lane) {
    constexpr size_t kT = sizeof(T);
    const size_t to_aligned = (size_t)(0 - (uintptr_t)pa) & (kT - 1), head = to_aligned < nb ? to_aligned : nb;  // < kT <= 16 bytes
    const size_t body = (nb - head) / kT, tail_at = head + body * kT;                                                // nb - tail_at < kT
    bool diff = false;
    if (lane < head) diff = pa[lane] != pb[lane];
    const T* qa = (const T*)(pa + head);
    const T* qb = (const T*)(pb + head);
    for (size_t i = lane; i < body; i += 64) diff |= words_differ(qa[i], qb[i]);
    if (tail_at + lane < nb) diff |= pa[tail_at + lane] != pb[tail_at + lane];
    return diff;
}

__global__ __launch_bounds__(kThreads) void rows_differ_kernel(sr_rows_differ_args a) {
    const unsigned lane = threadIdx.x & 63u;
    const size_t waves = (size_t)gridDim.x * kWaves;
    for (size_t r = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < a.rows_total; r += waves) {
        size_t row = r;
        int s = 0;
        while (s + 1 < a.n_seg && row >= a.seg[s].rows) row -= a.seg[s++].rows;
        const size_t nb = a.seg[s].row_bytes, at = a.seg[s].offset + row * nb;
        const uint8_t* pa = a.a + at;
        const uint8_t* pb = a.b + at;
        const unsigned apart = (unsigned)(((uintptr_t)pa ^ (uintptr_t)pb) & 15u);  // wave-uniform: one path per row
        bool diff;
        if (apart == 0) diff = row_differs<uint4>(pa, pb, nb, lane);
        else if ((apart & 3u) == 0) diff = row_differs<uint32_t>(pa, pb, nb, lane);
        else {
            diff = false;
            for (size_t i = lane; i < nb; i += 64) diff |= pa[i] != pb[i];
        }
        const unsigned long long any = __ballot(diff);
        if (lane == 0) a.flags[r] = any != 0 ? 1u : 0u;
    }
}

}  // namespace

size_t sr_rows_differ_blocks(size_t rows_total) {
    // a wave a row; beyond 64 workgroups a compute unit the waves take further rows a grid apart
    return std::min((rows_total + kWaves - 1) / kWaves, (size_t)64 * 256);
}

hipError_t sr_launch_rows_differ(const sr_rows_differ_args& a, hipStream_t s) {
    const size_t blocks = sr_rows_differ_blocks(a.rows_total);
    if (blocks == 0 || a.n_seg < 1 || a.n_seg > 3 || !a.a || !a.b || !a.flags || !sr_dword_aligned(a.flags)) return hipErrorInvalidValue;
    size_t rows = 0;
    for (int i = 0; i < a.n_seg; ++i) {
        if (a.seg[i].rows == 0 || a.seg[i].row_bytes == 0) return hipErrorInvalidValue;
        rows += a.seg[i].rows;
    }
    if (rows != a.rows_total) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rows_differ_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}
