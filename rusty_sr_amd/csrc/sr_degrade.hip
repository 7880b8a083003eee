// sr_degrade.hip -- the degradation operator (include/srhip.h "Degradation"): the LR image a training recipe synthesises from an HR crop --
// Gaussian blur in linear light, the f x f pool, sensor noise, 8-bit quantisation and a 4:4:4 JPEG round trip -- made on the device, with
// its own parameters per item.  The reference has no counterpart (network.rs:87-92 pools, nothing else); tests/degrade_ref.py restates
// the rule in numpy.
//
// One workgroup of 256 threads per 8 x 8 block of LR pixels -- a JPEG block, anchored at the LR frame's origin -- of one item:
//   1. the source pixels the block's blur can reach, (8f + 2R)^2 of them (R = ceil(3 sigma) <= 12: 56^2 at most), are read byte by byte
//      (any pointer offset, nothing outside the image) into LDS, one dword a pixel, through the window's member mapping;
//   2. the row pass: every row of that tile, the 8f columns of the block, linearised by a 256-entry f64 table and filtered, into LDS (f64);
//   3. the column pass and the pool: one thread per LR value (64 pixels x 3 channels) -- f x f columns sums, their mean;
//   4. encode, noise (SplitMix64 by random access, Box-Muller), quantise: the block's 192 bytes;
//   5. the JPEG round trip of the block in LDS: colour transform, 8 x 8 DCT as two 8-term passes, quantise and dequantise, the inverse
//      passes, colour back; pixels beyond the frame's ragged edge replicate the last row / column and are not stored;
//   6. the store: bytes, or byte / 255 floats straight into the backward pass's input (a degraded training step).
// All arithmetic is f64 and the file is built without contraction (build.py FLAGS), every sum in the order the header gives, so that the
// bytes can be held to the numpy restatement exactly: the rounding rule's bias (2^-30) keeps every structural tie away from its boundary,
// and the remaining values are not within an ulp's reach of one (tests/test_degrade_cpu.py checks that on the reference alone).
// The workload is a few hundred thousand values a step: f64's rate does not matter (DESIGN.md 4o has the measurements).
//
// train_degrade_kernel is a degraded step's whole gather: blocks [0, hr_blocks) of a grid row cut item blockIdx.y's HR crop into the u8
// batch with the crop kernels' code (sr_crop.h), the others are the item's 8 x 8 blocks.  Such a step has no extra launch.
// LDS: 63 KB a workgroup (two workgroups a CU); resources: profiles/degrade_kernel_resources.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_crop.h"
#include "sr_internal.h"

namespace {

constexpr int kMaxR = 12;  // ceil(3 SR_DEGRADE_MAX_SIGMA)
constexpr int kMaxF = 4;
constexpr int kTile = 8 * kMaxF + 2 * kMaxR;  // 56: side of the source tile at most

// ITU-T T.81 Annex K, tables K.1 (luma) and K.2 (chroma), row-major: row = vertical frequency
__constant__ uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

__device__ __forceinline__ uint64_t splitmix(uint64_t z) {  // SplitMix64's output function of the state z
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// R(v) = sign(v) floor(|v| + 0.5 + 2^-30), clamped to [0, 255]
__device__ __forceinline__ double round_byte(double v) {
    const double r = copysign(floor(fabs(v) + (0.5 + 0x1.0p-30)), v);
    return fmin(fmax(r, 0.0), 255.0);
}

// Batch-frame pixel (p, q) of item d -- any p, q: the blur reads beyond the frame -- as 0x00bbggrr: member_pixel's mapping (sr_crop.h)
// without its bounds, read byte by byte; 0 outside the source image.
__device__ __forceinline__ uint32_t frame_pixel(const sr_train_crop_desc& d, long p, long q, int frame_h, int frame_w) {
    if (d.k & 2) p = frame_h - 1 - p;
    if (d.k & 1) q = frame_w - 1 - q;
    const long sy = (long)d.y0 + ((d.k & 4) ? q : p), sx = (long)d.x0 + ((d.k & 4) ? p : q);
    if (sy < 0 || sy >= d.h || sx < 0 || sx >= d.w) return 0u;
    const uint8_t* s = d.px + (sy * d.w + sx) * d.ch;
    return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
}

// LDS of a workgroup.  The DCT passes' two buffers lie in the source tile, which is dead once the row pass has run.
struct Shared {
    double row[kTile][8 * kMaxF][3];  // the row pass: tile rows x block columns x channels
    double src[kTile * kTile / 2];    // the source tile, one dword a pixel; later the two buffers of the DCT passes, 192 doubles each
    double lin[256];                  // SrgbToLinear(byte / 255)
    double dct[64];                   // the DCT matrix C[u][x]
    double w[2 * kMaxR + 1];          // the blur's weights
    double px[192];                   // the block's bytes [y][x][c], as doubles
};
static_assert(sizeof(Shared) <= 64 * 1024, "one workgroup's LDS");
static_assert(kTile * kTile / 2 >= 2 * 192, "the DCT buffers fit the source tile");

// The block (by, bx) of item d's LR frame (lh x lw LR pixels, factor f) with parameters g.  tab: 256 + 64 doubles (the linearisation, the
// DCT matrix).  Every thread of the workgroup calls this.  store(y, x, c, byte) is called once for every value of the block inside the frame.
template <class Store>
__device__ __forceinline__ void degrade_block(Shared& sh, const sr_train_crop_desc& d, const sr_degrade& g, int f, int lh, int lw, int by, int bx,
                                              const double* __restrict__ tab, Store&& store) {
    const int tid = threadIdx.x;
    const double sigma = (double)g.sigma;
    const int R = sigma > 0.0 ? min((int)ceil(3.0 * sigma), kMaxR) : 0;  // (the host has refused sigma > 4: the bound only guards the LDS)
    const int side = 8 * f + 2 * R, cols = 8 * f;
    uint32_t* src = (uint32_t*)sh.src;
    sh.lin[tid] = tab[tid];
    if (tid < 64) sh.dct[tid] = tab[256 + tid];
    if (tid <= 2 * R) {
        const double t = (double)(tid - R);
        sh.w[tid] = R ? exp(-(t * t) / (2.0 * sigma * sigma)) : 1.0;
    }
    const long p0 = (long)by * cols - R, q0 = (long)bx * cols - R;  // the tile's origin in the batch frame
    for (int i = tid; i < side * side; i += 256) {
        const int r = i / side, c = i - r * side;
        src[i] = frame_pixel(d, p0 + r, q0 + c, lh * f, lw * f);
    }
    __syncthreads();
    if (R && tid == 0) {  // normalise: the sum in tap order
        double sum = 0.0;
        for (int t = 0; t <= 2 * R; ++t) sum += sh.w[t];
        for (int t = 0; t <= 2 * R; ++t) sh.w[t] /= sum;
    }
    __syncthreads();
    // rows: tile row r, block column c (tile column c + R), along q
    for (int i = tid; i < side * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        const uint32_t* s = src + r * side + c;
        if (R) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int t = 0; t <= 2 * R; ++t) {
                const uint32_t px = s[t];
                const double w = sh.w[t];
                a0 += w * sh.lin[px & 0xffu];
                a1 += w * sh.lin[(px >> 8) & 0xffu];
                a2 += w * sh.lin[px >> 16];
            }
            sh.row[r][c][0] = a0; sh.row[r][c][1] = a1; sh.row[r][c][2] = a2;
        } else {
            const uint32_t px = s[0];
            sh.row[r][c][0] = sh.lin[px & 0xffu]; sh.row[r][c][1] = sh.lin[(px >> 8) & 0xffu]; sh.row[r][c][2] = sh.lin[px >> 16];
        }
    }
    __syncthreads();
    // columns, pool, encode, noise, quantise: thread = (LR pixel, channel) of the block
    const int ly = tid / 24, lx = (tid / 3) % 8, ch = tid % 3;  // tid < 192
    const long y = (long)by * 8 + ly, x = (long)bx * 8 + lx;    // in the LR frame
    if (tid < 192) {
        double sum = 0.0;
        for (int i = 0; i < f; ++i)
            for (int j = 0; j < f; ++j) {
                const int r = ly * f + i, c = lx * f + j;  // the HR pixel: tile row r + R, block column c
                double v;
                if (R) {
                    v = 0.0;
                    for (int t = 0; t <= 2 * R; ++t) v += sh.w[t] * sh.row[r + t][c][ch];
                } else {
                    v = sh.row[r][c][ch];
                }
                sum += v;
            }
        const double mean = sum / (double)(f * f);
        double v = 255.0 * (mean <= 0.0031308 ? 12.92 * mean : 1.055 * pow(mean, 1.0 / 2.4) - 0.055);
        if (g.noise > 0.0f && y < lh && x < lw) {
            const uint64_t i = (uint64_t)(y * lw + x) * 3u + (uint64_t)ch;
            const uint64_t x1 = splitmix(g.seed + (2 * i + 1) * 0x9e3779b97f4a7c15ull), x2 = splitmix(g.seed + (2 * i + 2) * 0x9e3779b97f4a7c15ull);
            const double u1 = (double)(x1 >> 11) * 0x1.0p-53, u2 = (double)(x2 >> 11) * 0x1.0p-53;
            v += (double)g.noise * sqrt(-2.0 * log(1.0 - u1)) * cos(2.0 * 3.14159265358979323846 * u2);
        }
        sh.px[tid] = round_byte(v);
    }
    __syncthreads();
    if (g.quality > 0) {
        double* a = sh.src;  // [3][64]
        double* b = sh.src + 192;
        const int pl = tid / 64, e = tid % 64, u = e / 8, k = e % 8;  // tid < 192: plane, element (u, k) of an 8 x 8
        // ragged edges replicate the frame's last row / column
        const int ry = (int)min((long)u, lh - 1 - (long)by * 8), rx = (int)min((long)k, lw - 1 - (long)bx * 8);
        if (tid < 192) {
            const double* p = sh.px + (ry * 8 + rx) * 3;
            const double r_ = p[0], g_ = p[1], b_ = p[2];
            const double v = pl == 0   ? 0.299 * r_ + 0.587 * g_ + 0.114 * b_
                             : pl == 1 ? 128.0 - 0.168735892 * r_ - 0.331264108 * g_ + 0.5 * b_
                                       : 128.0 + 0.5 * r_ - 0.418687589 * g_ - 0.081312411 * b_;
            a[tid] = round_byte(v) - 128.0;
        }
        __syncthreads();
        if (tid < 192) {  // b[u][x] = sum_y C[u][y] a[y][x]
            double s = 0.0;
            for (int yy = 0; yy < 8; ++yy) s += sh.dct[u * 8 + yy] * a[pl * 64 + yy * 8 + k];
            b[tid] = s;
        }
        __syncthreads();
        if (tid < 192) {  // coef[u][v] = sum_x b[u][x] C[v][x]; quantised and dequantised
            double s = 0.0;
            for (int xx = 0; xx < 8; ++xx) s += b[pl * 64 + u * 8 + xx] * sh.dct[k * 8 + xx];
            const int q = g.quality, scale = q < 50 ? 5000 / q : 200 - 2 * q;
            const double t = (double)min(max(((int)kBaseQ[pl ? 1 : 0][e] * scale + 50) / 100, 1), 255);
            const double c = s / t;
            a[tid] = copysign(floor(fabs(c) + (0.5 + 0x1.0p-30)), c) * t;
        }
        __syncthreads();
        if (tid < 192) {  // b[y][v] = sum_u C[u][y] a[u][v]
            double s = 0.0;
            for (int uu = 0; uu < 8; ++uu) s += sh.dct[uu * 8 + u] * a[pl * 64 + uu * 8 + k];
            b[tid] = s;
        }
        __syncthreads();
        if (tid < 192) {  // out[y][x] = sum_v b[y][v] C[v][x]
            double s = 0.0;
            for (int vv = 0; vv < 8; ++vv) s += b[pl * 64 + u * 8 + vv] * sh.dct[vv * 8 + k];
            a[tid] = round_byte(s + 128.0);
        }
        __syncthreads();
        if (tid < 192) {
            const int pix = tid / 3;  // = ly * 8 + lx
            const double Y = a[pix], cb = a[64 + pix] - 128.0, cr = a[128 + pix] - 128.0;
            const double v = ch == 0 ? Y + 1.402 * cr : ch == 1 ? Y - 0.344136286 * cb - 0.714136286 * cr : Y + 1.772 * cb;
            sh.px[tid] = round_byte(v);
        }
        // (each thread reads back its own value below)
    }
    if (tid < 192 && y < lh && x < lw) store(y, x, ch, (uint32_t)sh.px[tid]);
}

__global__ __launch_bounds__(256) void degrade_kernel(sr_degrade_one a, const double* __restrict__ tab, uint8_t* __restrict__ out) {
    __shared__ Shared sh;
    const int lh = a.frame_h / a.f, lw = a.frame_w / a.f, bw = (lw + 7) / 8;
    degrade_block(sh, a.d, a.g, a.f, lh, lw, blockIdx.x / bw, blockIdx.x % bw, tab,
                  [&](long y, long x, int c, uint32_t byte) { out[(y * lw + x) * 3 + c] = (uint8_t)byte; });
}

__global__ __launch_bounds__(256) void train_degrade_kernel(sr_train_degrade_args a, uint32_t* __restrict__ batch, float* __restrict__ xin,
                                                            const float* __restrict__ ftab, const double* __restrict__ tab) {
    const int b = blockIdx.y;
    if ((int)blockIdx.x < a.hr_blocks) {
        long k;
        uint32_t word;
        if (crop_dword([&](int i) { return a.d[i]; }, a.n, b, (long)blockIdx.x * 256 + threadIdx.x, a.crop_h, a.crop_w, &k, &word)) batch[k] = word;
        return;
    }
    __shared__ Shared sh;
    const int lh = a.crop_h / a.f, lw = a.crop_w / a.f, bw = (lw + 7) / 8, blk = (int)blockIdx.x - a.hr_blocks;
    float* dst = xin + (long)b * lh * lw * 3;
    degrade_block(sh, a.d[b], a.g[b], a.f, lh, lw, blk / bw, blk % bw, tab,
                  [&](long y, long x, int c, uint32_t byte) { dst[(y * lw + x) * 3 + c] = ftab[byte]; });
}

}  // namespace

hipError_t sr_launch_degrade(const sr_degrade_one& a, const double* d_tab, uint8_t* d_out, hipStream_t s) {
    if (a.f < 2 || a.f > kMaxF || a.frame_h < a.f || a.frame_w < a.f || a.frame_h % a.f || a.frame_w % a.f) return hipErrorInvalidValue;
    const long bh = (a.frame_h / a.f + 7) / 8, bw = (a.frame_w / a.f + 7) / 8;
    if (bh * bw > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(degrade_kernel, dim3((unsigned)(bh * bw)), dim3(256), 0, s, a, d_tab, d_out);
    return hipGetLastError();
}

hipError_t sr_launch_train_degrade(sr_train_degrade_args a, uint32_t* d_batch, float* d_x, const float* d_ftab, const double* d_tab,
                                   hipStream_t s) {
    if (a.n < 1 || a.n > SR_TRAIN_MAX_BATCH || a.f < 2 || a.f > kMaxF || a.crop_h < a.f || a.crop_w < a.f || a.crop_h % a.f || a.crop_w % a.f)
        return hipErrorInvalidValue;
    const long hr_bytes = (long)a.crop_h * a.crop_w * 3;
    const long hr_blocks = (hr_bytes / 4 + 1 + 255) / 256;  // most dwords whose first byte lies in one crop
    const long blocks = (long)((a.crop_h / a.f + 7) / 8) * ((a.crop_w / a.f + 7) / 8);
    if (hr_blocks + blocks > INT32_MAX) return hipErrorInvalidValue;
    a.hr_blocks = (int)hr_blocks;
    hipLaunchKernelGGL(train_degrade_kernel, dim3((unsigned)(hr_blocks + blocks), (unsigned)a.n), dim3(256), 0, s, a, d_batch, d_x, d_ftab, d_tab);
    return hipGetLastError();
}
