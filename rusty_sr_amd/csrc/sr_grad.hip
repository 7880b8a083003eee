// sr_grad.hip -- backpropagation of the reference's training graph sr_net(f, Some((l2, linear_loss))) (network.rs:78-103,
// `g.backprop` inside Adam::optimise_from, main.rs:181-257) on gfx950, and one Adam step.  Host side: sr_grad.cpp.
//
// One call, for a batch of n HR images pooled to n LR images of H x W (NP = n H W LR pixels), on one stream:
//
//   pool       input = LinearToSrgb(mean_fxf(SrgbToLinear(hr)))       sr_launch_valid_pool (sr_valid.hip), 1 launch (n if h % f != 0)
//   forward    z, a of f, l1, l2, l3; e (3f^2 expand channels)        grad_conv_kernel<FWD/LIN>, 5 launches (one per stage)
//   loss       out = LinearInterp(input) + d2s(e); e' = out - hr      grad_loss_kernel: d_e = 2 s e' (x SrgbToLinear'(out)) and one f64
//              (or of SrgbToLinear of both)                           partial of sum e'^2 per workgroup; sr_launch_loss_sum adds them in order
//                                                                     (sr_set_loss: s sign(e') or s e' / sqrt(e'^2 + eps^2) in place of 2 s e')
//   bias of e  sum of d_e over pixels                                 grad_colsum_kernel, per-chunk partials
//   data grads d_a3 = conv10^T d_e; d_a2 = conv9^T d_e + conv8^T d_z3; grad_conv_kernel<BWD>, 4 launches, each summing all its
//              d_a1 = conv7^T d_e + conv6^T d_z3 + conv5^T d_z2;       sources; epilogue: d_z = d_a (beta + z / sqrt(z^2 + 1)) and per-
//              d_f = conv3^T d_z3 + conv2^T d_z2 + conv1^T d_z1        workgroup partials of sum d_a z (beta) and sum d_z (bias)
//   weights    dW[o][kh][kw][i] = sum_p d_z[p][o] a[p + tap][i]         grad_wgrad_kernel<5>, <3>: one launch per tap size, all convs
//                                                                       of that size; per-chunk partials (K = pixels split in chunks)
//   assembly   grad = (partials summed in chunk order) + 2 l2 p        grad_assemble_kernel, .rsr segment order
//
// 16 launches, the pool included (n + 15 when h is not a multiple of f).  Every matrix product is v_mfma_f32_32x32x2_f32: exact f32 products,
// f32 accumulation (cdna_hip_programming.md s3).  No float atomics anywhere: every sum is a per-workgroup partial written to its own slot
// and added in a fixed order by a later launch, and every grid is a function of the shape alone -- the gradient and err_sum are the same
// bits on every run, context and device.  The context's precision setting is not consulted: backprop is always exact f32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sr_internal.h"
#include "sr_params.h"
#include "sr_reduce.h"
#include "sr_transfer.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxSrc = 3;
constexpr int kFwd = 0, kLin = 1, kBwd = 2;  // grad_conv_kernel epilogues

// One source of a convolution: `in` NHWC with channel pitch `pitch`; the reduction runs over `cin` channels (a multiple of 8 in the
// vector form; channels >= cin_real get weight 0 and must hold finite values).  Weight of (output column j, tap t, input channel c) is
// w[base + j sj + t st + c sc]: forward [O][KH][KW][I] is (sj, st, sc, base) = (KK I, I, 1, 0); the transposed convolution of the data
// gradient reads the same array with taps flipped and O / I swapped: (1, -I, KK I, (KK - 1) I).
struct GradSrc {
    const float* in;
    const float* w;
    int pitch, cin, cin_real, ks;
    int sj, st, sc, base;
};

struct GradConvArgs {
    GradSrc src[kMaxSrc];
    int nsrc;
    int n, H, W;
    int cout, out_pitch;
    const float* bias;   // kFwd, kLin
    const float* beta;   // kFwd, kBwd
    float* out0;         // kFwd: z; kLin: e; kBwd: d_z
    float* out1;         // kFwd: a
    const float* z;      // kBwd: the saved pre-activation
    float* part_beta;    // kBwd: [blockIdx.x][32] sum of d_a z
    float* part_bias;    // kBwd: [blockIdx.x][32] sum of d_z
};

// alumina BeLU, in the inference kernels' operation order (sr_kernels.hip belu): beta z + sqrt(z z + 1) - 1
__device__ __forceinline__ float belu(float z, float beta) {
    return __fadd_rn(__fadd_rn(__fmul_rn(beta, z), __builtin_amdgcn_sqrtf(__fadd_rn(__fmul_rn(z, z), 1.0f))), -1.0f);
}

// Implicit-GEMM convolution, "Same" zero padding, stride 1: M = 32 pixels per wave (4 waves: 128 consecutive pixels of the flattened
// n x H x W index), N = 32 output channels (blockIdx.y selects the block of 32), K = taps x channels of every source.  Lane l holds
// A[pixel l & 31][k = l >> 5] and B[k][channel l & 31]; in the vector form a lane loads 4 consecutive channels with one 16-byte load
// and the 4 products are 4 MFMAs (the two lane halves take channels c0 .. c0+3 and c0+4 .. c0+7: a permutation of K that A and B share).
// SCALAR: one source of cin_real channels (conv0, 3 channels), K = KK cin_real flattened, one element per lane.
template <int MODE, bool SCALAR>
__global__ __launch_bounds__(256) void grad_conv_kernel(GradConvArgs a) {
    __shared__ float s_red[2][4][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const long HW = (long)a.H * a.W, NP = (long)a.n * HW;
    const long p_base = (long)blockIdx.x * 128 + wave * 32;
    const long p = p_base + i;
    const bool pv = p < NP;
    int img = 0, y = 0, x = 0;
    if (pv) {
        img = (int)(p / HW);
        const long r = p - (long)img * HW;
        y = (int)(r / a.W);
        x = (int)(r - (long)y * a.W);
    }
    const int jj = blockIdx.y * 32 + i;
    const bool jok = jj < a.cout;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if constexpr (SCALAR) {
        const GradSrc S = a.src[0];
        const int pad = S.ks >> 1, K = S.ks * S.ks * S.cin_real;
        for (int k0 = 0; k0 < K; k0 += 2) {
            const int k = k0 + h;
            float av = 0.f, bv = 0.f;
            if (k < K) {
                const int tap = k / S.cin_real, c = k - tap * S.cin_real;
                const int kh = tap / S.ks, kw = tap - kh * S.ks;
                const int yy = y + kh - pad, xx = x + kw - pad;
                if (pv && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W)
                    av = S.in[((size_t)img * HW + (size_t)yy * a.W + xx) * S.pitch + c];
                if (jok) bv = S.w[S.base + (long)jj * S.sj + (long)tap * S.st + (long)c * S.sc];
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    } else {
        for (int s = 0; s < a.nsrc; ++s) {
            const GradSrc S = a.src[s];
            const int pad = S.ks >> 1;
            for (int kh = 0; kh < S.ks; ++kh) {
                const int yy = y + kh - pad;
                const bool rowok = pv && yy >= 0 && yy < a.H;
                for (int kw = 0; kw < S.ks; ++kw) {
                    const int xx = x + kw - pad;
                    const bool ok = rowok && xx >= 0 && xx < a.W;
                    const float* ip = S.in + ((size_t)img * HW + (size_t)(ok ? yy : 0) * a.W + (ok ? xx : 0)) * S.pitch;
                    const float* wp = S.w + S.base + (long)jj * S.sj + (long)(kh * S.ks + kw) * S.st;
                    for (int c0 = 0; c0 < S.cin; c0 += 8) {
                        const int c = c0 + 4 * h;
                        f32x4 av = {0.f, 0.f, 0.f, 0.f};
                        if (ok) av = *(const f32x4*)(ip + c);
                        float bv[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) bv[t] = (jok && c + t < S.cin_real) ? wp[(long)(c + t) * S.sc] : 0.f;
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc, 0, 0, 0);
                    }
                }
            }
        }
    }
    // acc[r] = pixel p_base + (r & 3) + 8 (r >> 2) + 4 h, channel jj
    float pbeta = 0.f, pbias = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long q = p_base + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (q < NP && jok) {
            const float v = acc[r];
            if constexpr (MODE == kFwd) {
                const float z = v + a.bias[jj];
                a.out0[q * a.out_pitch + jj] = z;
                a.out1[q * a.out_pitch + jj] = belu(z, a.beta[jj]);
            } else if constexpr (MODE == kLin) {
                a.out0[q * a.out_pitch + jj] = v + a.bias[jj];
            } else {
                const float z = a.z[q * 32 + jj];
                const float dz = v * (a.beta[jj] + z / __builtin_amdgcn_sqrtf(z * z + 1.0f));
                a.out0[q * 32 + jj] = dz;
                pbeta += v * z;
                pbias += dz;
            }
        }
    }
    if constexpr (MODE == kBwd) {  // lanes l and l + 32 hold the same channel; then the four waves in order
        pbeta += __shfl_xor(pbeta, 32, 64);
        pbias += __shfl_xor(pbias, 32, 64);
        if (h == 0) {
            s_red[0][wave][i] = pbeta;
            s_red[1][wave][i] = pbias;
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const int t = threadIdx.x;
            a.part_beta[(size_t)blockIdx.x * 32 + t] = ((s_red[0][0][t] + s_red[0][1][t]) + s_red[0][2][t]) + s_red[0][3][t];
            a.part_bias[(size_t)blockIdx.x * 32 + t] = ((s_red[1][0][t] + s_red[1][1][t]) + s_red[1][2][t]) + s_red[1][3][t];
        }
    }
}

// One convolution's weight gradient: x (the conv's input, cin channels, pitch x_pitch), dy (the gradient of its output, cout channels,
// pitch dy_pitch); part: [chunk][O][KH][KW][I].
struct WgradJob {
    const float* x;
    const float* dy;
    float* part;
    int cin, x_pitch, cout, dy_pitch;
};
constexpr int kMaxJobs = 6;
struct WgradArgs {
    WgradJob job[kMaxJobs];
    int n, H, W;
    long chunk;  // pixels per chunk (blockIdx.x)
};

// dW[o][kh][kw][i] = sum_p dy[p][o] x[p + (kh - pad, kw - pad)][i]: one wave per (chunk, kh, job, block of 32 outputs); M = input
// channel (A = x, one 128-byte row of 32 channels per lane half), N = output channel (B = dy), K = the chunk's pixels, two per MFMA.
// The wave holds the KS taps of its row kh in KS accumulators, so one load of dy feeds KS MFMAs.
template <int KS>
__global__ __launch_bounds__(64) void grad_wgrad_kernel(WgradArgs a) {
    const WgradJob J = a.job[blockIdx.z >> 1];
    const int nt = blockIdx.z & 1;
    if (nt * 32 >= J.cout) return;  // (wave-uniform)
    constexpr int pad = KS / 2;
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5, kh = blockIdx.y;
    const int o = nt * 32 + i;
    const long HW = (long)a.H * a.W, NP = (long)a.n * HW;
    const long p0 = (long)blockIdx.x * a.chunk, p1 = std::min(NP, p0 + a.chunk);
    f32x16 acc[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const bool iok = i < J.cin, ook = o < J.cout;
    for (long q = p0; q < p1; q += 2) {
        const long p = q + h;
        const bool pv = p < p1;
        int img = 0, y = 0, x = 0;
        if (pv) {
            img = (int)(p / HW);
            const long r = p - (long)img * HW;
            y = (int)(r / a.W);
            x = (int)(r - (long)y * a.W);
        }
        const float bv = (pv && ook) ? J.dy[(size_t)p * J.dy_pitch + o] : 0.f;
        const int yy = y + kh - pad;
        const bool rowok = pv && iok && yy >= 0 && yy < a.H;
        const float* xrow = J.x + ((size_t)img * HW + (size_t)(rowok ? yy : 0) * a.W) * J.x_pitch + i;
        float av[KS];
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
            const int xx = x + kw - pad;
            av[kw] = (rowok && xx >= 0 && xx < a.W) ? xrow[(size_t)xx * J.x_pitch] : 0.f;
        }
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) acc[kw] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kw], bv, acc[kw], 0, 0, 0);
    }
    // acc[kw][r]: input channel (r & 3) + 8 (r >> 2) + 4 h, output channel o
    if (!ook) return;
    const size_t seglen = (size_t)J.cout * KS * KS * J.cin;
    float* dst = J.part + (size_t)blockIdx.x * seglen + (size_t)o * KS * KS * J.cin;
#pragma unroll
    for (int kw = 0; kw < KS; ++kw)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (ci < J.cin) dst[(size_t)(kh * KS + kw) * J.cin + ci] = acc[kw][r];
        }
}

// per-channel sums of d[NP][pitch] (C <= 64 channels) over chunks of `chunk` pixels: part[blockIdx.x][C]
__global__ __launch_bounds__(256) void grad_colsum_kernel(const float* __restrict__ d, int pitch, int C, long NP, long chunk,
                                                          float* __restrict__ part) {
    __shared__ float s[4][64];
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const long p0 = (long)blockIdx.x * chunk, p1 = std::min(NP, p0 + chunk);
    float acc = 0.f;
    if (c < C)
        for (long p = p0 + r0; p < p1; p += 4) acc += d[(size_t)p * pitch + c];
    s[r0][c] = acc;
    __syncthreads();
    if (threadIdx.x < C) part[(size_t)blockIdx.x * C + threadIdx.x] = ((s[0][threadIdx.x] + s[1][threadIdx.x]) + s[2][threadIdx.x]) + s[3][threadIdx.x];
}

// SrgbToLinear'(s): 1 / 12.92 on the linear segment, else 2.4 / 1.055 a^1.4 with a = (s + 0.055) / 1.055 (f64, rounded once)
__device__ __forceinline__ float srgb_to_linear_deriv(float s) {
    if (s <= 0.04045f) return (float)(1.0 / 12.92);
    const double a = ((double)s + 0.055) * (1.0 / 1.055);
    return (float)((2.4 / 1.055) * a * (double)fast_pow((float)a, 0.4f));
}

// One thread per LR pixel P: the f x f x 3 outputs it owns (out[f Y + dy][f X + dx][c] = LinearInterp(x) + e[P][(dy f + dx) 3 + c],
// network.rs:27,39; LinearInterp with half-pixel centres and clamped edges, the C oracle's linterp_f_acc), their error against the HR
// crop, d_e = 2 s err (x SrgbToLinear'(out) in linear mode), zeros in the pad channels [E, ep).  One f64 partial of sum err^2 per workgroup.
// hr: n images of hr_h x hr_w x CH (u8) or x 3 (f32); tab: 512 floats, byte / 255 then SrgbToLinear of those (sr_valid.cpp).
// LOSS (include/srhip.h sr_set_loss): what of err the seed multiplies -- SR_LOSS_MSE err itself (seed = 2 s), SR_LOSS_L1 its sign, 0 at
// err == 0 (seed = s), SR_LOSS_CHARBONNIER err / sqrt(err^2 + eps2) (seed = s; IEEE square root and division, the same bits everywhere).
// The partial is of sum err^2 under every kind; eps2 is read by the Charbonnier instances alone.
template <int F, bool HR_U8, int CH, bool LINEAR, int LOSS>
__global__ __launch_bounds__(256) void grad_loss_kernel(const float* __restrict__ x, const float* __restrict__ e, const void* __restrict__ hr,
                                                        const float* __restrict__ tab, int n, int H, int W, int hr_h, int hr_w, float seed,
                                                        float* __restrict__ d_e, int ep, double* __restrict__ partial, float eps2) {
    constexpr int E = 3 * F * F;
    __shared__ double s_part[4];
    const long HW = (long)H * W, NP = (long)n * HW;
    const long P = (long)blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if (P < NP) {
        const int img = (int)(P / HW);
        const long r = P - (long)img * HW;
        const int Y = (int)(r / W), X = (int)(r - (long)Y * W);
        const float* xi = x + (size_t)img * HW * 3;
        const float* ep_in = e + (size_t)P * E;
        float* g = d_e + (size_t)P * ep;
#pragma unroll
        for (int dy = 0; dy < F; ++dy) {
            const int ny = 2 * dy + 1 - F;
            const int ya = std::min(std::max(Y + (ny < 0 ? -1 : 0), 0), H - 1), yb = std::min(std::max(Y + (ny < 0 ? 0 : 1), 0), H - 1);
            const float ty = (float)(ny < 0 ? ny + 2 * F : ny) / (float)(2 * F);
            const size_t hrow = ((size_t)img * hr_h + (size_t)(F * Y + dy)) * hr_w + (size_t)F * X;
#pragma unroll
            for (int dx = 0; dx < F; ++dx) {
                const int nx = 2 * dx + 1 - F;
                const int xa = std::min(std::max(X + (nx < 0 ? -1 : 0), 0), W - 1), xb = std::min(std::max(X + (nx < 0 ? 0 : 1), 0), W - 1);
                const float tx = (float)(nx < 0 ? nx + 2 * F : nx) / (float)(2 * F);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float va = (1.0f - tx) * xi[((size_t)ya * W + xa) * 3 + c] + tx * xi[((size_t)ya * W + xb) * 3 + c];
                    const float vb = (1.0f - tx) * xi[((size_t)yb * W + xa) * 3 + c] + tx * xi[((size_t)yb * W + xb) * 3 + c];
                    const int ch = (dy * F + dx) * 3 + c;
                    const float out = ((1.0f - ty) * va + ty * vb) + ep_in[ch];
                    float hv;
                    if constexpr (HR_U8) hv = tab[(LINEAR ? 256 : 0) + ((const uint8_t*)hr)[(hrow + dx) * CH + c]];
                    else {
                        hv = ((const float*)hr)[(hrow + dx) * 3 + c];
                        if (LINEAR) hv = srgb_to_linear_cr(hv);
                    }
                    const float d = (LINEAR ? srgb_to_linear_cr(out) : out) - hv;
                    acc += (double)d * (double)d;
                    float gv;
                    if constexpr (LOSS == SR_LOSS_MSE) gv = seed * d;
                    else if constexpr (LOSS == SR_LOSS_L1) gv = d > 0.f ? seed : d < 0.f ? -seed : 0.f * d;  // (a NaN stays one)
                    else {
                        const float r = __builtin_sqrtf(d * d + eps2);  // r == 0: err and eps^2 both below f32's range; the L1 limit
                        gv = r > 0.f ? seed * (d / r) : 0.f * d;
                    }
                    if (LINEAR) gv = gv * srgb_to_linear_deriv(out);
                    g[ch] = gv;
                }
            }
        }
        for (int ch = E; ch < ep; ++ch) g[ch] = 0.f;
    }
    acc = block_sum(acc, s_part);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// The gradient in .rsr order: each segment is the sum of its nparts partials (in order) plus 2 l2 p.
struct SegDesc {
    const float* part;
    int off, len, nparts;
};
struct AssembleArgs {
    SegDesc seg[SR_SEGS];
    int total;
};

__global__ __launch_bounds__(256) void grad_assemble_kernel(AssembleArgs a, const float* __restrict__ params, float two_l2, float* __restrict__ grad) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.total) return;
    int s = 0;
    while (s + 1 < SR_SEGS && g >= a.seg[s + 1].off) ++s;
    const SegDesc d = a.seg[s];
    const int k = g - d.off;
    float acc = 0.f;
    for (int t = 0; t < d.nparts; ++t) acc += d.part[(size_t)t * d.len + k];
    grad[g] = acc + two_l2 * params[g];
}

// Adam (UNPINNED, alumina's source is not at hand: the textbook form with bias correction, all in f32)
__global__ __launch_bounds__(256) void grad_adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                        long n, float lr, float b1, float b2, float eps, float bc1, float bc2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * (gi * gi);
    m[i] = mi;
    v[i] = vi;
    const float mh = mi / bc1, vh = vi / bc2;
    p[i] = p[i] - lr * mh / (__builtin_sqrtf(vh) + eps);
}

// ---- the plan: where everything lives, as a function of (factor, n, H, W) alone
struct Layout {
    int E, EP;
    long NP;
    int conv_grid;        // workgroups of grad_conv_kernel (128 pixels each) = partial rows of beta / bias
    int loss_grid;        // workgroups (= f64 partials) of grad_loss_kernel
    int wchunks; long wchunk;  // weight-gradient chunks
    int cchunks; long cchunk;  // expand-bias column-sum chunks
    size_t o_zf, o_z[4], o_a[4], o_e, o_de, o_dz[4], o_wpart[10], o_pbeta[4], o_pbias[4], o_pebias, o_err;  // float offsets
    size_t floats;
};

Layout layout(int f, int n, int H, int W) {
    Layout L;
    L.E = 3 * f * f;
    L.EP = (L.E + 15) / 16 * 16;
    L.NP = (long)n * H * W;
    L.conv_grid = (int)((L.NP + 127) / 128);
    L.loss_grid = (int)((L.NP + 255) / 256);
    L.wchunks = (int)std::min<long>(128, std::max<long>(1, (L.NP + 511) / 512));
    L.wchunk = (L.NP + L.wchunks - 1) / L.wchunks;
    L.cchunks = (int)std::min<long>(256, std::max<long>(1, (L.NP + 1023) / 1024));
    L.cchunk = (L.NP + L.cchunks - 1) / L.cchunks;
    const sr_param_layout S(f);
    size_t o = 0;
    auto take = [&](size_t floats) { const size_t at = o; o += (floats + 63) / 64 * 64; return at; };
    L.o_zf = 0;
    for (int k = 0; k < 4; ++k) L.o_z[k] = take((size_t)L.NP * 32);
    for (int k = 0; k < 4; ++k) L.o_a[k] = take((size_t)L.NP * 32);
    L.o_e = take((size_t)L.NP * L.E);
    L.o_de = take((size_t)L.NP * L.EP);
    for (int k = 0; k < 4; ++k) L.o_dz[k] = take((size_t)L.NP * 32);
    for (int sg = 0, k = 0; sg < SR_SEGS; ++sg)  // the convolutions, in segment order
        if (S.is_conv(sg)) L.o_wpart[k++] = take((size_t)L.wchunks * S.len[sg]);
    for (int k = 0; k < 4; ++k) L.o_pbeta[k] = take((size_t)L.conv_grid * 32);
    for (int k = 0; k < 4; ++k) L.o_pbias[k] = take((size_t)L.conv_grid * 32);
    L.o_pebias = take((size_t)L.cchunks * L.E);
    L.o_err = take((size_t)2 * (L.loss_grid + 1));  // doubles: partials, then the host-pointer call's result slot
    L.floats = o;
    return L;
}

template <int MODE, bool SCALAR>
hipError_t launch_conv(const GradConvArgs& a, int grid, hipStream_t s) {
    const int ny = (a.cout + 31) / 32;
    hipLaunchKernelGGL((grad_conv_kernel<MODE, SCALAR>), dim3((unsigned)grid, (unsigned)ny), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int F, int LOSS>
hipError_t launch_loss(const sr_grad_plan& P, const Layout& L, float* ws, hipStream_t s) {
    const float seed = LOSS == SR_LOSS_MSE ? 2.0f * P.loss_scale : P.loss_scale;  // rho'(err) = 2 err, or a factor of magnitude <= 1
    sr_dispatch_hr(P.hr_u8, P.hr_ch, P.linear, [&](auto u8, auto ch, auto lin) {
        hipLaunchKernelGGL((grad_loss_kernel<F, decltype(u8)::value, decltype(ch)::value, decltype(lin)::value, LOSS>),
                           dim3((unsigned)L.loss_grid), dim3(256), 0, s, P.x, (const float*)(ws + L.o_e), P.hr, P.tab, P.n, P.H, P.W, P.hr_h,
                           P.hr_w, seed, ws + L.o_de, L.EP, (double*)(ws + L.o_err), P.loss_eps * P.loss_eps);
    });
    return hipGetLastError();
}

template <int F>
hipError_t launch_loss(const sr_grad_plan& P, const Layout& L, float* ws, hipStream_t s) {
    switch (P.loss_kind) {
        case SR_LOSS_MSE: return launch_loss<F, SR_LOSS_MSE>(P, L, ws, s);
        case SR_LOSS_L1: return launch_loss<F, SR_LOSS_L1>(P, L, ws, s);
        case SR_LOSS_CHARBONNIER: return launch_loss<F, SR_LOSS_CHARBONNIER>(P, L, ws, s);
        default: return hipErrorInvalidValue;
    }
}

#define SR_TRY(expr)                          \
    do {                                      \
        const hipError_t e__ = (expr);        \
        if (e__ != hipSuccess) return e__;    \
    } while (0)

}  // namespace

size_t sr_grad_workspace_bytes(int factor, int n, int H, int W) {
    return layout(factor, n, H, W).floats * sizeof(float);
}

sr_grad_split sr_grad_split_of(int factor, int n, int H, int W) {
    const Layout L = layout(factor, n, H, W);
    return sr_grad_split{L.conv_grid, L.loss_grid, L.wchunks, L.wchunk, L.cchunks, L.cchunk};
}

double* sr_grad_result_slot(const sr_grad_plan& P) {
    const Layout L = layout(P.factor, P.n, P.H, P.W);
    return (double*)(P.ws + L.o_err) + L.loss_grid;
}

hipError_t sr_launch_grad(const sr_grad_plan& P, hipStream_t s) {
    const int f = P.factor;
    if (f < 2 || f > 4 || P.n <= 0 || P.H <= 0 || P.W <= 0) return hipErrorInvalidValue;
    const Layout L = layout(f, P.n, P.H, P.W);
    const sr_param_layout S(f);
    float* ws = P.ws;
    const float* prm = P.params;
    auto seg = [&](int k) { return prm + S.off[k]; };
    // convolution `sg` applied to `in` (channel pitch `pitch`), and the data gradient through it: source = the gradient of its output
    // (the reduction loops over all `pitch` channels, cout of them real)
    auto fwd = [&](const float* in, int pitch, int sg) {
        const int ks = S.ks(sg), cin = S.cin(sg);
        return GradSrc{in, seg(sg), pitch, cin, cin, ks, ks * ks * cin, cin, 1, 0};
    };
    auto bwd_of = [&](const float* dy, int pitch, int sg) {
        const int ks = S.ks(sg), cin = S.cin(sg);
        return GradSrc{dy, seg(sg), pitch, pitch, S.cout(sg), ks, 1, -cin, ks * ks * cin, (ks * ks - 1) * cin};
    };
    float* wpart[SR_SEGS] = {};  // a convolution's weight-gradient partials
    for (int sg = 0, k = 0; sg < SR_SEGS; ++sg)
        if (S.is_conv(sg)) wpart[sg] = ws + L.o_wpart[k++];
    float* z[4];
    float* act[4];
    float* dz[4];
    for (int k = 0; k < 4; ++k) {
        z[k] = ws + L.o_z[k];
        act[k] = ws + L.o_a[k];
        dz[k] = ws + L.o_dz[k];
    }
    float* e = ws + L.o_e;
    float* de = ws + L.o_de;
    const int E = L.E, EP = L.EP;
    const int bias_seg[4] = {SR_SEG_F_BIAS, SR_SEG_L1_BIAS, SR_SEG_L2_BIAS, SR_SEG_L3_BIAS};
    const int beta_seg[4] = {SR_SEG_F_ACTIV, SR_SEG_L1_ACTIV, SR_SEG_L2_ACTIV, SR_SEG_L3_ACTIV};
    const float* bias[4] = {seg(bias_seg[0]), seg(bias_seg[1]), seg(bias_seg[2]), seg(bias_seg[3])};
    const float* beta[4] = {seg(beta_seg[0]), seg(beta_seg[1]), seg(beta_seg[2]), seg(beta_seg[3])};

    // ---- forward with saved state
    GradConvArgs a{};
    a.n = P.n; a.H = P.H; a.W = P.W;
    a.cout = 32; a.out_pitch = 32;
    a.nsrc = 1;
    a.src[0] = fwd(P.x, 3, SR_SEG_CONV0);
    a.bias = bias[0]; a.beta = beta[0]; a.out0 = z[0]; a.out1 = act[0];
    SR_TRY((launch_conv<kFwd, true>(a, L.conv_grid, s)));
    a.src[0] = fwd(act[0], 32, SR_SEG_CONV1);
    a.bias = bias[1]; a.beta = beta[1]; a.out0 = z[1]; a.out1 = act[1];
    SR_TRY((launch_conv<kFwd, false>(a, L.conv_grid, s)));
    a.nsrc = 2;
    a.src[1] = fwd(act[1], 32, SR_SEG_CONV5);
    a.src[0] = fwd(act[0], 32, SR_SEG_CONV2);
    a.bias = bias[2]; a.beta = beta[2]; a.out0 = z[2]; a.out1 = act[2];
    SR_TRY((launch_conv<kFwd, false>(a, L.conv_grid, s)));
    a.nsrc = 3;
    a.src[0] = fwd(act[0], 32, SR_SEG_CONV3);
    a.src[1] = fwd(act[1], 32, SR_SEG_CONV6);
    a.src[2] = fwd(act[2], 32, SR_SEG_CONV8);
    a.bias = bias[3]; a.beta = beta[3]; a.out0 = z[3]; a.out1 = act[3];
    SR_TRY((launch_conv<kFwd, false>(a, L.conv_grid, s)));
    a.src[0] = fwd(act[1], 32, SR_SEG_CONV7);
    a.src[1] = fwd(act[2], 32, SR_SEG_CONV9);
    a.src[2] = fwd(act[3], 32, SR_SEG_CONV10);
    a.cout = E; a.out_pitch = E;
    a.bias = seg(SR_SEG_EXP_BIAS); a.beta = nullptr; a.out0 = e; a.out1 = nullptr;
    SR_TRY((launch_conv<kLin, false>(a, L.conv_grid, s)));

    // ---- loss and seed
    switch (f) {
        case 2: SR_TRY(launch_loss<2>(P, L, ws, s)); break;
        case 3: SR_TRY(launch_loss<3>(P, L, ws, s)); break;
        default: SR_TRY(launch_loss<4>(P, L, ws, s)); break;
    }
    double* err_part = (double*)(ws + L.o_err);
    SR_TRY(sr_launch_loss_sum(err_part, L.loss_grid, P.err_out ? P.err_out : (void*)(err_part + L.loss_grid), s));
    hipLaunchKernelGGL(grad_colsum_kernel, dim3((unsigned)L.cchunks), dim3(256), 0, s, (const float*)de, EP, E, L.NP, L.cchunk,
                       ws + L.o_pebias);
    SR_TRY(hipGetLastError());

    // ---- data gradients, last layer first
    GradConvArgs b{};
    b.n = P.n; b.H = P.H; b.W = P.W;
    b.cout = 32; b.out_pitch = 32;
    auto bwd = [&](int layer) {
        b.beta = beta[layer]; b.z = z[layer]; b.out0 = dz[layer];
        b.part_beta = ws + L.o_pbeta[layer]; b.part_bias = ws + L.o_pbias[layer];
        return launch_conv<kBwd, false>(b, L.conv_grid, s);
    };
    b.nsrc = 1;
    b.src[0] = bwd_of(de, EP, SR_SEG_CONV10);
    SR_TRY(bwd(3));
    b.nsrc = 2;
    b.src[0] = bwd_of(de, EP, SR_SEG_CONV9);
    b.src[1] = bwd_of(dz[3], 32, SR_SEG_CONV8);
    SR_TRY(bwd(2));
    b.nsrc = 3;
    b.src[0] = bwd_of(de, EP, SR_SEG_CONV7);
    b.src[1] = bwd_of(dz[3], 32, SR_SEG_CONV6);
    b.src[2] = bwd_of(dz[2], 32, SR_SEG_CONV5);
    SR_TRY(bwd(1));
    b.src[0] = bwd_of(dz[3], 32, SR_SEG_CONV3);
    b.src[1] = bwd_of(dz[2], 32, SR_SEG_CONV2);
    b.src[2] = bwd_of(dz[1], 32, SR_SEG_CONV1);
    SR_TRY(bwd(0));

    // ---- weight gradients: the 5x5 convs in one launch, the 3x3 ones in another
    WgradArgs w5{}, w3{};
    w5.n = w3.n = P.n; w5.H = w3.H = P.H; w5.W = w3.W = P.W;
    w5.chunk = w3.chunk = L.wchunk;
    auto wjob = [&](const float* x, int x_pitch, const float* dy, int dy_pitch, int sg) {
        return WgradJob{x, dy, wpart[sg], S.cin(sg), x_pitch, S.cout(sg), dy_pitch};
    };
    w5.job[0] = wjob(P.x, 3, dz[0], 32, SR_SEG_CONV0);
    w5.job[1] = wjob(act[0], 32, dz[1], 32, SR_SEG_CONV1);
    w5.job[2] = wjob(act[0], 32, dz[2], 32, SR_SEG_CONV2);
    w5.job[3] = wjob(act[0], 32, dz[3], 32, SR_SEG_CONV3);
    w3.job[0] = wjob(act[1], 32, dz[2], 32, SR_SEG_CONV5);
    w3.job[1] = wjob(act[1], 32, dz[3], 32, SR_SEG_CONV6);
    w3.job[2] = wjob(act[1], 32, de, EP, SR_SEG_CONV7);
    w3.job[3] = wjob(act[2], 32, dz[3], 32, SR_SEG_CONV8);
    w3.job[4] = wjob(act[2], 32, de, EP, SR_SEG_CONV9);
    w3.job[5] = wjob(act[3], 32, de, EP, SR_SEG_CONV10);
    hipLaunchKernelGGL((grad_wgrad_kernel<5>), dim3((unsigned)L.wchunks, 5, 4 * 2), dim3(64), 0, s, w5);
    SR_TRY(hipGetLastError());
    hipLaunchKernelGGL((grad_wgrad_kernel<3>), dim3((unsigned)L.wchunks, 3, 6 * 2), dim3(64), 0, s, w3);
    SR_TRY(hipGetLastError());

    // ---- assembly
    AssembleArgs as{};
    as.total = (int)S.total;
    for (int sg = 0; sg < SR_SEGS; ++sg) {
        as.seg[sg].off = (int)S.off[sg];
        as.seg[sg].len = (int)S.len[sg];
        if (S.is_conv(sg)) {
            as.seg[sg].part = wpart[sg];
            as.seg[sg].nparts = L.wchunks;
        }
    }
    for (int k = 0; k < 4; ++k) {
        as.seg[bias_seg[k]].part = ws + L.o_pbias[k];
        as.seg[bias_seg[k]].nparts = L.conv_grid;
        as.seg[beta_seg[k]].part = ws + L.o_pbeta[k];
        as.seg[beta_seg[k]].nparts = L.conv_grid;
    }
    as.seg[SR_SEG_EXP_BIAS].part = ws + L.o_pebias;
    as.seg[SR_SEG_EXP_BIAS].nparts = L.cchunks;
    hipLaunchKernelGGL(grad_assemble_kernel, dim3((unsigned)((as.total + 255) / 256)), dim3(256), 0, s, as, prm, 2.0f * P.l2, P.grad);
    return hipGetLastError();
}

hipError_t sr_launch_grad_adam(float* d_params, float* d_m, float* d_v, const float* d_grad, size_t n, float lr, float beta1, float beta2,
                               float eps, float bc1, float bc2, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(grad_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_params, d_m, d_v, d_grad, (long)n, lr, beta1,
                       beta2, eps, bc1, bc2);
    return hipGetLastError();
}
