// sr_ensemble.hip -- the pixel moves of the self-ensemble (include/srhip.h sr_upscale_ensemble_*): member k runs the network on T_k(x), one
// of the 8 flips and rotations of the image, and its output is carried back by T_k^-1 and added to an accumulator.  Both directions are
// the same gather,
//     dst[p][q] = src[r][c],   (r0, c0) = swap ? (q, p) : (p, q),   r = flip_r ? SH - 1 - r0 : r0,   c = flip_c ? SW - 1 - c0 : c0
// (sr_ensemble.cpp derives swap / flip_r / flip_c from k for either direction), over pixels of 3 or 4 bytes (the u8 image on its way in,
// converted to f32 where it lands) or 12 bytes (the f32 image on its way in, the f32 output map on its way back).  One thread moves one pixel.
//
//   ens_rows_kernel   swap = 0: a row of dst is a row of src, possibly reversed -- a wavefront reads one contiguous run and writes one
//                     contiguous run, straight through registers.
//   ens_tile_kernel   swap = 1: a 32 x 32 pixel tile goes through LDS, read along src rows and written along dst rows, so that both sides
//                     are contiguous runs.  The tile is kept as planes of dwords with rows of 33: the transposed read (lane l takes
//                     t[w][l][j]) then walks the 32 banks of ds_read_b32 with stride 33, conflict-free, and so does the row-wise write.
//
// What is done with the pixel at dst is the sink's business: stored as it is (the input transforms), or -- the way back -- added to the
// accumulator, and by the last member scaled by 1 / count and stored as f32 or quantised RGBA8.  Every dst pixel belongs to exactly one
// thread and the grid is a function of the shape alone: no atomics, the same bits on every run.  All offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_internal.h"

namespace {

constexpr int kTile = 32;

struct EnsGeo {
    int DH, DW;          // dst pixels
    int SH, SW;          // src pixels
    int flip_r, flip_c;  // in src coordinates
    int lw;              // rows kernel: a block is 2^lw pixels wide and 256 >> lw rows high
    unsigned blocks_x;   // blocks (rows kernel) / tiles (tile kernel) across dst
};

// ---- sources: pixel `px` of the image as NW dwords
struct SrcF32 {
    static constexpr int NW = 3;
    const float* p;
    __device__ __forceinline__ void load(size_t px, uint32_t (&v)[3]) const {
        const float* q = p + px * 3;
        v[0] = __float_as_uint(q[0]); v[1] = __float_as_uint(q[1]); v[2] = __float_as_uint(q[2]);
    }
};

template <int CH>  // u8 pixels of CH bytes at any byte address; alpha is dropped here
struct SrcU8 {
    static constexpr int NW = 1;
    const uint8_t* p;
    __device__ __forceinline__ void load(size_t px, uint32_t (&v)[1]) const {
        const uint8_t* q = p + px * CH;
        v[0] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
};

// ---- sinks
struct SinkF32 {  // the transformed f32 image
    float* p;
    __device__ __forceinline__ void store(size_t px, const uint32_t (&v)[3]) const {
        float* q = p + px * 3;
        q[0] = __uint_as_float(v[0]); q[1] = __uint_as_float(v[1]); q[2] = __uint_as_float(v[2]);
    }
};

// the transformed u8 image as the f32 image the plain call makes of it, img_to_data: byte / 255, an f32 division (the stage kernels'
// own table, sr_kernels.hip) -- a member's pass writes f32, and the stage kernels pair f32 output with f32 input
struct SinkUnit {
    float* p;
    __device__ __forceinline__ void store(size_t px, const uint32_t (&v)[1]) const {
        float* q = p + px * 3;
        q[0] = __fdiv_rn((float)(v[0] & 0xffu), 255.0f);
        q[1] = __fdiv_rn((float)((v[0] >> 8) & 0xffu), 255.0f);
        q[2] = __fdiv_rn((float)((v[0] >> 16) & 0xffu), 255.0f);
    }
};

// acc = acc + v in plain f32 (the first member adds to 0.0f); the last member stores (acc + v) * scale instead: as f32 at `out` (which may
// be acc itself: a thread reads and writes its own pixel only) or as RGBA8 by the stage kernels' rule, clamp(floor(255 v + 0.5)), alpha 255
template <bool OUT_U8>
struct SinkAcc {
    float* acc;
    void* out;
    float scale;
    int first, last;
    __device__ __forceinline__ void store(size_t px, const uint32_t (&v)[3]) const {
        float a[3] = {0.0f, 0.0f, 0.0f};
        if (!first) { const float* q = acc + px * 3; a[0] = q[0]; a[1] = q[1]; a[2] = q[2]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = a[k] + __uint_as_float(v[k]);
        if (!last) {
            float* q = acc + px * 3;
            q[0] = a[0]; q[1] = a[1]; q[2] = a[2];
            return;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = a[k] * scale;
        if constexpr (OUT_U8) {
            uint32_t w = 0xff000000u;
#pragma unroll
            for (int k = 0; k < 3; ++k) w = __builtin_amdgcn_cvt_pk_u8_f32(floorf(a[k] * 255.0f + 0.5f), (uint32_t)k, w);  // saturates; NaN -> 0
            ((uint32_t*)out)[px] = w;
        } else {
            float* q = (float*)out + px * 3;
            q[0] = a[0]; q[1] = a[1]; q[2] = a[2];
        }
    }
};

template <class Src, class Sink>
__global__ __launch_bounds__(256) void ens_rows_kernel(Src src, Sink sink, EnsGeo g) {
    const unsigned by = blockIdx.x / g.blocks_x, bx = blockIdx.x - by * g.blocks_x;
    const long p = (long)by * (256 >> g.lw) + (threadIdx.x >> g.lw);
    const long q = ((long)bx << g.lw) + (threadIdx.x & ((1u << g.lw) - 1u));
    if (p >= g.DH || q >= g.DW) return;
    const long r = g.flip_r ? g.SH - 1 - p : p, c = g.flip_c ? g.SW - 1 - q : q;
    uint32_t v[Src::NW];
    src.load((size_t)r * g.SW + c, v);
    sink.store((size_t)p * g.DW + q, v);
}

template <class Src, class Sink>
__global__ __launch_bounds__(256) void ens_tile_kernel(Src src, Sink sink, EnsGeo g) {
    __shared__ uint32_t t[Src::NW][kTile][kTile + 1];
    const unsigned ty = blockIdx.x / g.blocks_x, tx = blockIdx.x - ty * g.blocks_x;
    const long p0 = (long)ty * kTile, q0 = (long)tx * kTile;  // the dst tile; its src tile is rows q0.., columns p0.. before the flips
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < kTile; j += 8) {
        const long r0 = q0 + ly + j, c0 = p0 + lx;
        if (r0 < g.DW && c0 < g.DH) {
            const long r = g.flip_r ? g.SH - 1 - r0 : r0, c = g.flip_c ? g.SW - 1 - c0 : c0;
            uint32_t v[Src::NW];
            src.load((size_t)r * g.SW + c, v);
#pragma unroll
            for (int w = 0; w < Src::NW; ++w) t[w][ly + j][lx] = v[w];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTile; j += 8) {
        const long p = p0 + ly + j, q = q0 + lx;
        if (p < g.DH && q < g.DW) {
            uint32_t v[Src::NW];
#pragma unroll
            for (int w = 0; w < Src::NW; ++w) v[w] = t[w][lx][ly + j];
            sink.store((size_t)p * g.DW + q, v);
        }
    }
}

template <class Src, class Sink>
hipError_t launch(const Src& src, const Sink& sink, const sr_ens_map& m, hipStream_t s) {
    EnsGeo g{};
    g.DH = m.DH; g.DW = m.DW;
    g.SH = m.swap ? m.DW : m.DH; g.SW = m.swap ? m.DH : m.DW;
    g.flip_r = m.flip_r; g.flip_c = m.flip_c;
    const size_t blocks = sr_ens_blocks(m.DH, m.DW, m.swap != 0, &g.lw, &g.blocks_x);
    if (blocks == 0 || blocks > (size_t)INT32_MAX) return hipErrorInvalidValue;  // (sr_ensemble.cpp has refused such a shape already)
    if (m.swap) hipLaunchKernelGGL((ens_tile_kernel<Src, Sink>), dim3((unsigned)blocks), dim3(256), 0, s, src, sink, g);
    else hipLaunchKernelGGL((ens_rows_kernel<Src, Sink>), dim3((unsigned)blocks), dim3(256), 0, s, src, sink, g);
    return hipGetLastError();
}

}  // namespace

size_t sr_ens_blocks(int DH, int DW, bool swap, int* lw_out, unsigned* blocks_x_out) {
    if (DH < 1 || DW < 1) return 0;
    int lw = 0;
    size_t bx, by;
    if (swap) {
        bx = ((size_t)DW + kTile - 1) / kTile; by = ((size_t)DH + kTile - 1) / kTile;
    } else {
        while (lw < 8 && (1 << lw) < DW) ++lw;  // narrow images: a block takes several rows
        bx = ((size_t)DW + (1u << lw) - 1) >> lw; by = ((size_t)DH + (256 >> lw) - 1) / (256 >> lw);
    }
    if (lw_out) *lw_out = lw;
    if (blocks_x_out) *blocks_x_out = (unsigned)bx;
    return bx * by;
}

hipError_t sr_launch_ens_input(const void* d_src, bool u8, int ch, void* d_dst, const sr_ens_map& m, hipStream_t s) {
    if (!u8) return launch(SrcF32{(const float*)d_src}, SinkF32{(float*)d_dst}, m, s);
    if (ch == 3) return launch(SrcU8<3>{(const uint8_t*)d_src}, SinkUnit{(float*)d_dst}, m, s);
    return launch(SrcU8<4>{(const uint8_t*)d_src}, SinkUnit{(float*)d_dst}, m, s);
}

hipError_t sr_launch_ens_accumulate(const float* d_member, float* d_acc, void* d_out, bool out_u8, bool first, bool last, float scale,
                                    const sr_ens_map& m, hipStream_t s) {
    if (out_u8) return launch(SrcF32{d_member}, SinkAcc<true>{d_acc, d_out, scale, first, last}, m, s);
    return launch(SrcF32{d_member}, SinkAcc<false>{d_acc, d_out, scale, first, last}, m, s);
}
