// sr_api.cpp -- the C ABI of libsrhip.so (include/srhip.h): context, weight
// re-packing, workspace, stage scheduling.  No CPU compute fallback exists:
// without a HIP device sr_create fails with SR_E_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/srhip.h"
#include "../../include/srhip_experimental.h"
#include "sr_kernels.h"
#include "sr_internal.h"
#include "sr_params.h"

namespace {

constexpr int kChunk = 1024;  // floats per tap chunk (32 cin x 32 cout)
constexpr int kAutoBlockWidth = 16;  // default tile order of the stage kernels (StageArgs::bw): 16-tile (512 px) column blocks;
                                     // measured 1080p / 4K, both modes (scripts/bw_exp.py): 0-3 % faster than row-major, 8..32 alike

// w = hi + lo/2048 with hi, lo halves (see split_half in sr_kernels.hip)
void split_half_host(float v, _Float16& hi, _Float16& lo) {
    hi = std::fabs(v) < 6.103515625e-05f ? (_Float16)0.0f : (_Float16)v;
    lo = (_Float16)((v - (float)hi) * 2048.0f);
}
// The expand node's 3 f^2 channels ((dy*f+dx)*3+c, network.rs:39) are laid out in whole RGB
// triples, 10 per 32-lane N-tile and 5 per 16-lane DPP row (lanes 15 and 31 idle), so that the u8 packing of the
// last kernel gathers G and B from the two lanes above R with row_shl DPP moves and never crosses a row:
// lane j of tile nt carries channel 3*(10 nt + 5 (j/16) + (j%16)/3) + (j%16)%3.  Returns that channel, or -1.
int expand_channel(int f, int nt, int j) {
    const int jj = j % 16, tr = nt * 10 + 5 * (j / 16) + jj / 3;
    return (jj < 15 && tr < f * f) ? tr * 3 + jj % 3 : -1;
}
int expand_tiles(int f) { return (f * f + 9) / 10; }
// The split-half mode's last stage computes the transposed tile (weights as the MFMA's A operand, sr_kernels.hip half_steps_h): lane
// (pixel, h) then holds output slots 8 a + 4 h + b (a, b = 0..3) in register 4 a + b.  Slot j of that form carries the channel that sits in
// column 16 h + 4 a + b of the layout above, so a lane's sixteen registers are the five whole triples of "row" h (stage_epilogue_final_t).
int expand_channel_t(int f, int nt, int j) { return expand_channel(f, nt, 16 * ((j >> 2) & 1) + 4 * (j >> 3) + (j & 3)); }

// Weight chunks of the stage kernels (both forms): one 4 KB chunk per STEP = two taps of one 16-channel half
// (and, for a node with more than 32 output channels, per N-tile).  Steps run half 0 (channels 0-15) over the
// tap pairs (0,1), (2,3), ... then half 1; a lone last tap leaves its slot zero.
//   f32  : [q = 2 tapslot + rr][h 2][lane 32][4]    channel = 16 half + 8 rr + 4 h + e
//   split: [hi | lo] x [tapslot 2][h 2][lane 32][8]  channel = 16 half + 8 h + e
// `lane_channel(nt, j)` maps MFMA column j of N-tile nt to the output channel of w ([O][ks][ks][32]) or -1.
// Only the halves [half_lo, half_hi) are written (stage 2's conv5 in the Winograd form: the halves that stay direct).
template <typename F>
void pack_steps(std::vector<float>& dst, const float* w, int ks, int ntn, bool split, F lane_channel, int half_lo = 0, int half_hi = 2) {
    const int nt = ks * ks, np = (nt + 1) / 2;
    for (int half = half_lo; half < half_hi; ++half)
        for (int p = 0; p < np; ++p)
            for (int tile = 0; tile < ntn; ++tile) {
                const size_t base = dst.size();
                dst.resize(base + kChunk, 0.0f);
                _Float16* hp = (_Float16*)(dst.data() + base);
                for (int ts = 0; ts < 2; ++ts) {
                    const int t = 2 * p + ts;
                    if (t >= nt) continue;
                    // the split loop walks the taps column by column (row re-use, half_steps_h), the f32 loop row by row
                    const int tap = split ? (t % ks) * ks + t / ks : t;
                    for (int j = 0; j < 32; ++j) {
                        const int o = lane_channel(tile, j);
                        if (o < 0) continue;
                        const float* src = w + ((size_t)o * nt + tap) * 32 + 16 * half;
                        for (int c = 0; c < 16; ++c) {
                            if (!split) {
                                const int rr = c / 8, h = (c / 4) % 2, e = c % 4;
                                dst[base + (size_t)(2 * ts + rr) * 256 + (h * 32 + j) * 4 + e] = src[c];
                            } else {
                                _Float16 hi, lo;
                                split_half_host(src[c], hi, lo);
                                const int h = c / 8, e = c % 8;
                                hp[ts * 512 + (h * 32 + j) * 8 + e] = hi;
                                hp[1024 + ts * 512 + (h * 32 + j) * 8 + e] = lo;
                            }
                        }
                    }
                }
            }
}

// The 5x5 weights of stages 1 and 2 (conv1, conv2) for the exact mode's Winograd form (sr_kernels.hip half_steps_wino): per 16-channel half, operand groups
// g = (kernel row ky, position k, 8-channel group rr) = 14 ky + 2 k + rr, four to a 4 KB chunk (the last chunk of a half two):
//   [q = g % 4][h 2][lane 32][4]    channel = 16 half + 8 rr + 4 h + e
// Position k < 4 is position k of chunk A (taps 0, 1, 2 of the row), k = 4..6 position k - 3 of chunk B (a zero tap, then taps 3, 4);
// V = (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2), computed in double and rounded once.
// A 3x3 weight (ks = 3: conv5, stage 2's second source) has chunk A alone: g = 8 ky + 2 k + rr, 24 groups = 6 chunks per half; only the
// halves [half_lo, half_hi) are written.
void pack_steps_wino(std::vector<float>& dst, const float* w, int ks = 5, int half_lo = 0, int half_hi = 2) {
    const int npos = ks == 5 ? 7 : 4, kGroups = ks * npos * 2, kSteps = (kGroups + 3) / 4;
    for (int half = half_lo; half < half_hi; ++half) {
        const size_t base = dst.size();
        dst.resize(base + (size_t)kSteps * kChunk, 0.0f);
        for (int g = 0; g < kGroups; ++g) {
            const int rr = g & 1, k = (g >> 1) % npos, ky = (g >> 1) / npos;
            float* chunk = dst.data() + base + (size_t)(g / 4) * kChunk + (g % 4) * 256;
            for (int j = 0; j < 32; ++j)
                for (int h = 0; h < 2; ++h)
                    for (int e = 0; e < 4; ++e) {
                        const int c = 16 * half + 8 * rr + 4 * h + e;
                        auto tap = [&](int kx) { return (double)w[((size_t)j * ks * ks + ky * ks + kx) * 32 + c]; };
                        const double g0 = k < 4 ? tap(0) : 0.0, g1 = k < 4 ? tap(1) : tap(3), g2 = k < 4 ? tap(2) : tap(4);
                        const int pos = k < 4 ? k : k - 3;
                        const double v = pos == 0 ? g0 : pos == 1 ? (g0 + g1 + g2) * 0.5 : pos == 2 ? (g0 - g1 + g2) * 0.5 : g2;
                        chunk[(h * 32 + j) * 4 + e] = (float)v;
                    }
        }
    }
}

// Split-half weight chunks of stages 1-3 for the 16x16x32 step loop (sr_kernels.hip half_steps_h16): one 4 KB chunk per STEP,
//   [hi | lo][output-channel half 2][lane 64][8 halves],  lane = 16 g + n:  output channel 16 ch + n,  K block g: taps[g >> 1],
//   input channels 16 half + 8 (g & 1) + e  -- a step's K = 32 is two taps x the half's 16 channels.
// Taps run column by column (t = kx * ks + ky, as in the 32x32x16 split loop).  Steps of one source: the first half's tap pairs
// (0,1) (2,3) ..., then ONE step shared by the two halves' odd last tap (K 0-15: first half, K 16-31: second half), then the second
// half's pairs: ks^2 steps per source, none half empty.
void pack_steps_h16(std::vector<float>& dst, const float* w, int ks) {
    const int nt = ks * ks, np = (nt - 1) / 2;
    auto chunk = [&](int tap_a, int half_a, int tap_b, int half_b) {
        const size_t base = dst.size();
        dst.resize(base + kChunk, 0.0f);
        _Float16* hp = (_Float16*)(dst.data() + base);
        for (int ch = 0; ch < 2; ++ch)
            for (int lane = 0; lane < 64; ++lane) {
                const int g = lane >> 4, o = 16 * ch + (lane & 15);
                const int t = (g >> 1) ? tap_b : tap_a, half = (g >> 1) ? half_b : half_a;
                const int tap = (t % ks) * ks + t / ks;  // column-major walk -> [ky][kx] index of w ([O][ks][ks][32])
                for (int e = 0; e < 8; ++e) {
                    _Float16 hi, lo;
                    split_half_host(w[((size_t)o * nt + tap) * 32 + 16 * half + 8 * (g & 1) + e], hi, lo);
                    hp[(ch * 64 + lane) * 8 + e] = hi;
                    hp[1024 + (ch * 64 + lane) * 8 + e] = lo;
                }
            }
    };
    for (int p = 0; p < np; ++p) chunk(2 * p, 0, 2 * p + 1, 0);
    chunk(nt - 1, 0, nt - 1, 1);
    for (int p = 0; p < np; ++p) chunk(2 * p, 1, 2 * p + 1, 1);
}

// conv0 [32][5][5][3]: K packed per kernel row -- slot k = 3 kx + c (15 used of 16) -- as
// [ky 5][jj 4][h 2][o 32][e 2] with k = 2 (2 jj + e) + h  (conv0_kernel: B[k][o] for MFMA j = 2 jj + e).
void pack_conv0(std::vector<float>& dst, const float* w) {
    dst.assign(5 * 8 * 64, 0.0f);
    for (int ky = 0; ky < 5; ++ky)
        for (int jj = 0; jj < 4; ++jj)
            for (int h = 0; h < 2; ++h)
                for (int o = 0; o < 32; ++o)
                    for (int e = 0; e < 2; ++e) {
                        const int k = 2 * (2 * jj + e) + h;
                        if (k < 15) dst[(((ky * 4 + jj) * 2 + h) * 32 + o) * 2 + e] = w[(((size_t)o * 5 + ky) * 5 + k / 3) * 3 + k % 3];
                    }
}

// conv0 for the split-half mode's own stage-0 kernel (conv0_split_kernel): K slot s = 4 tap + channel, tap = 5 ky + kx (100 slots, the
// fourth channel and slots 100-111 zero), seven K-blocks of 16: [b 7][hi | lo][h 2][o 32][e 8] halves with s = 16 b + 8 h + e.
void pack_conv0_split(std::vector<float>& dst, const float* w) {
    dst.assign(7 * 2 * 2 * 32 * 8 / 2, 0.0f);
    _Float16* hp = (_Float16*)dst.data();
    for (int b = 0; b < 7; ++b)
        for (int h = 0; h < 2; ++h)
            for (int o = 0; o < 32; ++o)
                for (int e = 0; e < 8; ++e) {
                    const int s = 16 * b + 8 * h + e, tap = s / 4, c = s % 4;
                    if (tap >= 25 || c >= 3) continue;
                    _Float16 hi, lo;
                    split_half_host(w[((size_t)o * 25 + tap) * 3 + c], hi, lo);
                    hp[(((b * 2 + 0) * 2 + h) * 32 + o) * 8 + e] = hi;
                    hp[(((b * 2 + 1) * 2 + h) * 32 + o) * 8 + e] = lo;
                }
}

// LinearInterp x f (network.rs:27) as a 3x3 convolution of the edge-replicated 3-channel
// input onto the expand channels: 9 taps x N-tiles x [h 2][lane 32][q 2], cin = 2h+q.
// Along one axis output phase p of pixel i sits at s - i = (2p+1-f)/(2f) (half-pixel centres,
// SURVEY.md 8(a) G1): negative -> inputs (i-1, i) with weights (1-t, t), t = (2p+1+f)/(2f);
// otherwise -> inputs (i, i+1) with weights (1-t, t), t = (2p+1-f)/(2f).  Same f32 constants
// as the oracle; the 2-D weight is their f32 product.
void lin_taps(int f, float w1[4][3]) {
    for (int p = 0; p < f; ++p) {
        const int nn = 2 * p + 1 - f;
        const float t = (float)(nn < 0 ? nn + 2 * f : nn) / (float)(2 * f);
        if (nn < 0) { w1[p][0] = 1.0f - t; w1[p][1] = t; }
        else { w1[p][1] = 1.0f - t; w1[p][2] = t; }
    }
}
void pack_lin(std::vector<float>& dst, int f) {
    float w1[4][3] = {};
    lin_taps(f, w1);
    const int ntn = expand_tiles(f);
    const size_t base = dst.size();
    dst.resize(base + (size_t)9 * ntn * 128, 0.0f);
    for (int u = 0; u < 3; ++u)
        for (int v = 0; v < 3; ++v)
            for (int nt = 0; nt < ntn; ++nt)
                for (int j = 0; j < 32; ++j) {
                    const int ch = expand_channel(f, nt, j);
                    if (ch < 0) continue;
                    const int c = ch % 3, tr = ch / 3, dy = tr / f, dx = tr % f;
                    dst[base + ((u * 3 + v) * ntn + nt) * 128 + ((c >> 1) * 32 + j) * 2 + (c & 1)] = w1[dy][u] * w1[dx][v];
                }
}

// The same residual for the split-half mode's last stage (sr_kernels.hip lin_mfma_h): the staged pixels are divided by (2 f)^2, which
// makes every weight a small integer -- exact in a half, no lo part.  K slot = 4 tap + colour (36 of 48 used), three K-blocks of 16:
// [b 3][N-tile][h 2][lane 32][e 8] halves, slot 16 b + 8 h + e.
void pack_lin_split(std::vector<float>& dst, int f) {
    float w1[4][3] = {};
    lin_taps(f, w1);
    const int ntn = expand_tiles(f);
    const float scale = 4.0f * f * f;
    const size_t base = dst.size();
    dst.resize(base + (size_t)3 * ntn * 256, 0.0f);
    _Float16* hp = (_Float16*)(dst.data() + base);
    for (int b = 0; b < 3; ++b)
        for (int nt = 0; nt < ntn; ++nt)
            for (int h = 0; h < 2; ++h)
                for (int j = 0; j < 32; ++j)
                    for (int e = 0; e < 8; ++e) {
                        const int s = 16 * b + 8 * h + e, tap = s / 4, c = s % 4, ch = expand_channel_t(f, nt, j);
                        if (tap >= 9 || c >= 3 || ch < 0 || ch % 3 != c) continue;
                        const int tr = ch / 3, dy = tr / f, dx = tr % f;
                        hp[(((size_t)(b * ntn + nt) * 2 + h) * 32 + j) * 8 + e] = (_Float16)std::nearbyint(w1[dy][tap / 3] * w1[dx][tap % 3] * scale);
                    }
}

// Every parameter of sr_net(factor) in the layouts the kernels read, one vector (sr_create uploads it, sr_set_params copies it over the
// upload); the segment offsets go to c (they depend on the factor alone).  *split_ok: every conv weight can be carried as a pair of halves.
std::vector<float> pack_params(sr_ctx* c, const float* params, int factor, bool* split_ok) {
    std::vector<float> host, w;
    auto push = [&](const std::vector<float>& v) {
        const size_t off = host.size();
        host.insert(host.end(), v.begin(), v.end());
        while (host.size() % 64) host.push_back(0.0f);  // keep 256-B alignment
        return off;
    };
    auto vec32 = [&](size_t off, int n) {
        std::vector<float> v(32, 0.0f);
        for (int i = 0; i < n; ++i) v[i] = params[off + i];
        return v;
    };
    const sr_param_layout L(factor);
    pack_conv0(w, params + L.off[SR_SEG_CONV0]);
    c->off_w0 = push(w);
    pack_conv0_split(w, params + L.off[SR_SEG_CONV0]);
    c->off_w0h = push(w);
    for (int split = 0; split < 2; ++split) {  // exact-f32 chunks, then the same stages in split-half form
        auto ident = [](int, int j) { return j; };
        auto expand = [&](int nt, int j) { return split ? expand_channel_t(factor, nt, j) : expand_channel(factor, nt, j); };
        const bool h16 = split != 0;  // stages 1-3 of the split-half mode on 16x16x32 MFMAs: their own step order
        auto conv = [&](const float* wp, int ks) { if (h16) pack_steps_h16(w, wp, ks); else pack_steps(w, wp, ks, 1, split != 0, ident); };
        auto exp3 = [&](const float* wp) { pack_steps(w, wp, 3, expand_tiles(factor), split != 0, expand); };
        size_t* off = split ? c->off_wh : c->off_w;
        w.clear(); conv(params + L.off[SR_SEG_CONV1], 5);
        off[1] = push(w);
        w.clear(); conv(params + L.off[SR_SEG_CONV2], 5); conv(params + L.off[SR_SEG_CONV5], 3);
        off[2] = push(w);
        w.clear(); conv(params + L.off[SR_SEG_CONV3], 5); conv(params + L.off[SR_SEG_CONV6], 3); conv(params + L.off[SR_SEG_CONV8], 3);
        off[3] = push(w);
        w.clear();
        exp3(params + L.off[SR_SEG_CONV7]); exp3(params + L.off[SR_SEG_CONV9]); exp3(params + L.off[SR_SEG_CONV10]);
        if (split) pack_lin_split(w, factor);  // the split-half mode: on the f16 pipe too, with exact integer weights (lin_mfma_h)
        else pack_lin(w, factor);
        off[4] = push(w);
    }
    w.clear(); pack_steps_wino(w, params + L.off[SR_SEG_CONV1]);
    c->off_wino1 = push(w);
    for (int h5 = 0; h5 <= 2; ++h5) {  // 46 + h5 chunks per tile: a Winograd half of conv5 is 6 chunks, a direct half 5
        w.clear(); pack_steps_wino(w, params + L.off[SR_SEG_CONV2]);
        pack_steps_wino(w, params + L.off[SR_SEG_CONV5], 3, 0, h5);
        pack_steps(w, params + L.off[SR_SEG_CONV5], 3, 1, false, [](int, int j) { return j; }, h5, 2);
        c->off_wino2[h5] = push(w);
    }
    const size_t boff[4] = {L.off[SR_SEG_F_BIAS], L.off[SR_SEG_L1_BIAS], L.off[SR_SEG_L2_BIAS], L.off[SR_SEG_L3_BIAS]};
    const size_t aoff[4] = {L.off[SR_SEG_F_ACTIV], L.off[SR_SEG_L1_ACTIV], L.off[SR_SEG_L2_ACTIV], L.off[SR_SEG_L3_ACTIV]};
    for (int s = 0; s < 4; ++s) c->off_bias[s] = push(vec32(boff[s], 32));
    for (int s = 0; s < 4; ++s) c->off_beta[s] = push(vec32(aoff[s], 32));
    {   // expand_bias in the triple layout, 32 floats per N-tile
        std::vector<float> eb((size_t)expand_tiles(factor) * 32, 0.0f);
        for (int nt = 0; nt < expand_tiles(factor); ++nt)
            for (int j = 0; j < 32; ++j) {
                const int ch = expand_channel(factor, nt, j);
                if (ch >= 0) eb[nt * 32 + j] = params[L.off[SR_SEG_EXP_BIAS] + ch];
            }
        c->off_bias[4] = push(eb);
    }
    // the split-half mode carries every conv weight as a pair of halves: all of them finite and below the largest half, or the mode is refused
    bool ok = true;
    for (size_t k = L.off[SR_SEG_CONV1]; k < L.total && ok; ++k) ok = std::fabs(params[k]) < 65504.0f;   // (false for NaN too)
    for (size_t k = L.off[SR_SEG_CONV0]; k < L.off[SR_SEG_CONV0] + L.len[SR_SEG_CONV0] && ok; ++k) ok = std::fabs(params[k]) < 65504.0f;
    *split_ok = ok;
    return host;
}

// FNV-1a over the parameter bits: contexts that share a sharded call must hold the same parameters
unsigned long long params_fnv(const float* params, size_t n) {
    unsigned long long hsh = 1469598103934665603ull;
    const unsigned char* pb = (const unsigned char*)params;
    for (size_t i = 0; i < n * sizeof(float); ++i) { hsh ^= pb[i]; hsh *= 1099511628211ull; }
    return hsh;
}

}  // namespace

extern "C" {

const char* sr_strerror(int s) {
    switch (s) {
        case SR_OK: return "ok";
        case SR_E_INVALID: return "invalid argument";
        case SR_E_PARAM_COUNT:
            return "Parameters selected do not have the size required by the neural net. Ensure that the "
                   "same sample factor is used for upscaling and training";  // reference main.rs:162
        case SR_E_FACTOR: return "unsupported upscaling factor (sr_net: 2, 3 or 4; the reference ships 3, main.rs:31)";
        case SR_E_NO_DEVICE: return "no HIP (gfx950) device available; libsrhip has no CPU fallback";
        case SR_E_HIP: return "HIP runtime error";
        case SR_E_NOMEM: return "out of device memory";
        case SR_E_BYTEVEC: return "ByteVec conversion failed";  // reference main.rs:138
        case SR_E_HALO: return "band halo must be 0 (true image edge) or >= SR_HALO, and a sharded band at least SR_HALO rows";
        case SR_E_COMM: return "RCCL communicator missing or failed (librccl not loadable, sr_comm_init_* not called, or an RCCL error)";
        case SR_E_DOMAIN: return "outside the domain of SR_PRECISION_SPLIT_F16: a weight, an input or an activation is not finite or reaches 65504 in magnitude (use SR_PRECISION_F32)";
        default: return "unknown error";
    }
}

int sr_rsr_decode(const uint8_t* blob, size_t len, float* out, size_t cap, size_t* n_out) {
    if (!blob || len < 4) return SR_E_BYTEVEC;
    uint32_t n;
    memcpy(&n, blob, 4);
    if (len != 4 + (size_t)8 * n) return SR_E_BYTEVEC;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t sz;
        memcpy(&sz, blob + 4 + (size_t)4 * i, 4);
        if (sz != 4) return SR_E_BYTEVEC;
    }
    if (n_out) *n_out = n;
    if (out) {
        if (cap < n) return SR_E_INVALID;
        memcpy(out, blob + 4 + (size_t)4 * n, (size_t)4 * n);
    }
    return SR_OK;
}

int sr_rsr_encode(const float* params, size_t n, uint8_t* out, size_t cap, size_t* len_out) {
    if (n > 0xffffffffu) return SR_E_INVALID;
    const size_t len = 4 + 8 * n;
    if (len_out) *len_out = len;
    if (!out) return SR_OK;
    if (!params || cap < len) return SR_E_INVALID;
    const uint32_t n32 = (uint32_t)n, four = 4;
    memcpy(out, &n32, 4);
    for (size_t i = 0; i < n; ++i) memcpy(out + 4 + 4 * i, &four, 4);
    memcpy(out + 4 + 4 * n, params, 4 * n);
    return SR_OK;
}

int sr_create(sr_ctx** out, const float* params, size_t n_params, int factor, int device) {
    return sr_create_graph(out, SR_GRAPH_SR_NET, params, n_params, factor, device);
}

int sr_create_graph(sr_ctx** out, int graph, const float* params, size_t n_params, int factor, int device) {
    if (!out) return SR_E_INVALID;
    *out = nullptr;
    if (graph != SR_GRAPH_SR_NET && graph != SR_GRAPH_BILINEAR && graph != SR_GRAPH_DOWNSAMPLE) return SR_E_INVALID;
    // the reference is hard-wired to 3 (main.rs:31); sr_net itself takes the factor as an argument
    // (network.rs:16), so user-trained 2x / 4x parameter files are accepted too
    if (graph == SR_GRAPH_SR_NET ? (factor < 2 || factor > 4) : factor != SR_FACTOR) return SR_E_FACTOR;
    // main.rs:162 assert_eq!(params.len(), graph.num_params()): 130459 for sr_net(3), 0 for the other two
    if (n_params != (graph == SR_GRAPH_SR_NET ? sr_param_layout(factor).total : 0)) return SR_E_PARAM_COUNT;
    if (graph == SR_GRAPH_SR_NET && !params) return SR_E_INVALID;
    int ndev = 0;
    if (sr_no_device(false, &ndev)) return SR_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return SR_E_INVALID;
    sr_ctx* c = new (std::nothrow) sr_ctx();
    if (!c) return SR_E_NOMEM;
    sr_device_guard restore_device;
    c->device = device;
    c->graph = graph;
    c->factor = factor;
    // experiment switches: the environment gives the defaults, read here once; sr_set_experiment changes them
    static const char* const kSwitch[13][2] = {{"wino", "SRHIP_WINO"}, {"th", "SRHIP_TH"}, {"pipe", "SRHIP_PIPE"}, {"bw", "SRHIP_BW"}, {"tail", "SRHIP_TAIL"},
                                               {"bands", "SRHIP_BANDS"}, {"geo", "SRHIP_GEO"}, {"rows", "SRHIP_ROWS"}, {"fork", "SRHIP_FORK"},
                                               {"forkshare", "SRHIP_FORKSHARE"}, {"forkmin", "SRHIP_FORKMIN"}, {"forktune", "SRHIP_FORKTUNE"}, {"halo", "SRHIP_HALO"}};
    for (const auto& sw : kSwitch)
        if (const char* e = getenv(sw[1])) (void)sr_set_experiment(c, sw[0], e);
    c->params_hash = params_fnv(params, n_params);
    // SRHIP_TRACE=1: where sr_create spends its time (a one-shot process pays it once per image)
    const bool trace = getenv("SRHIP_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[srhip] sr_create: %-28s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    int rc = [&]() -> int {
        HIPCHK(c, hipSetDevice(device));
        mark("hipSetDevice");
        hipDeviceProp_t prop;
        HIPCHK(c, hipGetDeviceProperties(&prop, device));
        mark("hipGetDeviceProperties");
        snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
        c->cus = prop.multiProcessorCount;
        c->clock_mhz = prop.clockRate / 1000;
        // no stream yet: each costs 8-40 ms of start-up (a hardware queue), the device-pointer entry points run on the
        // caller's streams, a host call of one chunk needs one stream and only a pipelined one all three (sr_ensure_streams)
        for (auto& e : c->ev) HIPCHK(c, hipEventCreate(&e));
        mark("events");

        if (graph != SR_GRAPH_SR_NET) {  // parameter-free graphs: only the quantiser table of their u8 entry points
            const hipError_t te = sr_aux_build_tables(&c->d_qtab);
            // hipErrorUnknown: the builder's own plausibility checks of the device's powf failed -- no table, the u8 entry points of this
            // context answer SR_E_HIP (sr_launch_aux), its f32 entry points need none; anything else is a real HIP error
            if (te != hipSuccess && te != hipErrorUnknown) HIPCHK(c, te);
            if (te == hipErrorUnknown) { (void)hipGetLastError(); c->last_hip = (int)te; }
            mark("quantiser table");
            return SR_OK;
        }
        bool split_ok = true;
        const std::vector<float> host = pack_params(c, params, factor, &split_ok);
        c->split_ok = split_ok;
        mark("weight packing (host)");
        HIPCHK(c, hipHostMalloc((void**)&c->h_domain, 64, hipHostMallocMapped));
        *c->h_domain = 0;
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->d_domain, c->h_domain, 0));
        for (auto& w : c->ws) HIPCHK(c, hipMalloc((void**)&w.d_queue, 5 * 8 * sizeof(int)));

        HIPCHK(c, hipMalloc((void**)&c->d_params, host.size() * sizeof(float)));
        mark("hipMalloc x3");
        HIPCHK(c, hipMemcpy(c->d_params, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
        mark("parameter upload");
        return SR_OK;
    }();
    if (rc != SR_OK) {
        sr_destroy(c);
        return rc;
    }
    *out = c;
    return SR_OK;
}

void sr_destroy(sr_ctx* c) {
    if (!c) return;
    sr_device_guard restore_device;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    sr_train_detach_all(c);
    sr_video_detach_all(c);
    sr_yuv_release(c);
    sr_deep_release(c);
    sr_optim_release(c);
    sr_comm_release(c);
    sr_valid_release(c);
    sr_grad_release(c);
    sr_ensemble_release(c);
    sr_metrics_release(c);
    sr_alpha_release(c);
    sr_resize_release(c);
    sr_degrade_release(c);
    sr_border_release(c);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    for (auto& w : c->ws) {
        for (auto& p : w.d_feat) if (p) (void)hipFree(p);
        if (w.d_queue) (void)hipFree(w.d_queue);
    }
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->d_params) (void)hipFree(c->d_params);
    if (c->d_qtab) (void)hipFree(c->d_qtab);
    if (c->h_domain) (void)hipHostFree(c->h_domain);
    for (auto& b : c->d_in) sr_free_buf(b);
    for (auto& b : c->d_out) sr_free_buf(b);
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_fork) if (e) (void)hipEventDestroy(e);
    sr_fork_tune_clear(c);
    for (auto& e : c->pool) if (e) (void)hipEventDestroy(e);
    if (c->copy_in) { (void)hipStreamSynchronize(c->copy_in); (void)hipStreamDestroy(c->copy_in); }
    if (c->copy_out) { (void)hipStreamSynchronize(c->copy_out); (void)hipStreamDestroy(c->copy_out); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int sr_last_hip_error(sr_ctx* c) { return c ? c->last_hip : 0; }

int sr_num_params_factor(int factor) { return factor >= 2 && factor <= 4 ? (int)sr_param_layout(factor).total : -1; }

int sr_num_params(int graph) { return graph == SR_GRAPH_SR_NET ? SR_NUM_PARAMS : (graph == SR_GRAPH_BILINEAR || graph == SR_GRAPH_DOWNSAMPLE ? 0 : -1); }

int sr_set_precision(sr_ctx* c, int mode) {
    if (!c || (mode != SR_PRECISION_F32 && mode != SR_PRECISION_SPLIT_F16)) return SR_E_INVALID;
    if (mode == SR_PRECISION_SPLIT_F16 && !c->split_ok) return SR_E_DOMAIN;  // a weight that no pair of halves can carry: refused, not clamped
    if (mode != c->precision) {
        // the two modes lay their feature maps out differently (sr_kernels.h: row-planar against pixel-major): what was interior for one is border
        // for the other, so the workspaces' borders are cleared again before the next pass (ensure_features)
        for (auto& w : c->ws) w.geo_n = 0;
        c->last_h = c->last_w = 0;
    }
    c->precision = mode;
    return SR_OK;
}

int sr_set_params(sr_ctx* c, const float* params, size_t n_params) {
    if (!c) return sr_no_device() ? SR_E_NO_DEVICE : SR_E_INVALID;
    sr_plan_clear(c);
    if (c->graph != SR_GRAPH_SR_NET || !params) return SR_E_INVALID;
    if (n_params != sr_param_layout(c->factor).total) return SR_E_PARAM_COUNT;
    bool split_ok = true;
    const std::vector<float> host = pack_params(c, params, c->factor, &split_ok);
    if (c->precision == SR_PRECISION_SPLIT_F16 && !split_ok) return SR_E_DOMAIN;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    for (hipStream_t s : {c->stream, c->stream2, c->copy_in, c->copy_out})
        if (s) HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipMemcpy(c->d_params, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    c->split_ok = split_ok;
    c->params_hash = params_fnv(params, n_params);
    return SR_OK;
}

int sr_set_experiment(sr_ctx* c, const char* key, const char* value) {
    if (!c || !key) return SR_E_INVALID;
    const char* v = value ? value : "";
    if (!strcmp(key, "th")) {          // tile height: "" automatic, one digit (4 | 8) for all stages, or five digits
        for (int k = 0; k < 5; ++k) {
            const char ch = strlen(v) == 5 ? v[k] : v[0];
            c->env_th[k] = ch == '4' ? 4 : (ch == '8' ? 8 : 0);
        }
    } else if (!strcmp(key, "pipe")) { // "" automatic; "none": first form of the stage kernels everywhere; "all": pipe form also for small launches
        c->env_pipe = !strcmp(v, "none") ? 0 : !strcmp(v, "all") ? 2 : 1;
    } else if (!strcmp(key, "bands")) {  // host pipeline: row bands of one large image ("" / "0": automatic)
        c->env_bands = *v ? atoi(v) : 0;
    } else if (!strcmp(key, "rows")) {  // host pipeline: the bands' heights themselves, "r0,r1,..." top to bottom (used when they add up to the
        c->env_rows.clear();            // rows of the call); computed in order on one stream, with a leading '=' on alternating streams
        c->env_rows_two = *v == '=';
        if (*v == '=') ++v;
        while (*v) {
            c->env_rows.push_back(atoi(v));
            while (*v && *v != ',') ++v;
            if (*v) ++v;
        }
    } else if (!strcmp(key, "geo")) {  // "0": equal bands also where the host pipeline would shrink them geometrically
        c->env_geo = strcmp(v, "0") != 0;
    } else if (!strcmp(key, "tail")) {  // how many 4-row tiles end a launch of 8-row tiles, in units of the resident workgroups ("" : automatic, "0": none)
        c->env_tail = *v ? (float)atof(v) : -1.0f;
    } else if (!strcmp(key, "fork")) {  // device entry points, one image as two bands on two streams: "" automatic, "0" never, "1" always, N > 1: always, N rows first
        c->env_fork = *v ? atoi(v) : -1;
    } else if (!strcmp(key, "forkshare")) {  // ... the first band's share of the rows ("" : 0.5)
        c->fork_share = *v ? std::min(0.9, std::max(0.1, atof(v))) : 0.5;
    } else if (!strcmp(key, "forkmin")) {  // ... automatic rule: fork from this many rounds of tiles on
        c->fork_min_rounds = *v ? atof(v) : 3.5;
    } else if (!strcmp(key, "forktune")) {  // ... automatic rule, mid-size shapes: "" / "1": measure both plans on the caller's calls and keep the faster (ForkTune); "0": the rule alone; either forgets what was measured
        c->fork_autotune = strcmp(v, "0") != 0;
        sr_device_guard restore_device;
        (void)hipSetDevice(c->device);
        sr_fork_tune_clear(c);
    } else if (!strcmp(key, "halo")) {  // sharded calls: "" / "input": 7 input rows per neighbour, the overlap recomputed; "layers": feature rows after every stage
        c->layer_halos = !strcmp(v, "layers");
    } else if (!strcmp(key, "wino")) {  // exact mode: "": stages 1 and 2 as Winograd F(2,3) rows, half of conv5 included; "2": conv5 direct (the form before);
                                        // "3": both halves of conv5 (measurement only); "1": stage 1 only, "0": all direct (same bar, other last bits)
        c->wino = !strcmp(v, "0") ? 0 : !strcmp(v, "1") ? 1 : 2;
        c->wino5 = !strcmp(v, "3") ? 2 : !strcmp(v, "2") ? 0 : kWinoConv5Halves;
    } else if (!strcmp(key, "bw")) {   // tile-order column-block width in tiles; "" / negative: automatic, 0: plain row-major
        c->env_bw = *v ? atoi(v) : -1;
    } else if (!strcmp(key, "vyuv")) {  // the vertical pass to a YCbCr frame: "" the measured rule, "1" | "2": the fused kernel, that many row pairs a workgroup, "chain": resize_v + rgb_to_yuv (same bits every way)
        if (*v && strcmp(v, "1") && strcmp(v, "2") && strcmp(v, "chain")) return SR_E_INVALID;
        c->env_vyuv_pairs = !strcmp(v, "1") ? 1 : !strcmp(v, "2") ? 2 : !strcmp(v, "chain") ? -1 : 0;
    } else if (!strcmp(key, "auxgrid")) {  // bilinear_net / downsample_net: "" automatic, "N" (N >= 1): never more than N workgroups per launch
        long cap = 0;
        for (const char* p = v; *p; ++p) {
            if (*p < '0' || *p > '9' || cap > INT32_MAX / 10) return SR_E_INVALID;
            cap = 10 * cap + (*p - '0');
        }
        if (*v && (cap < 1 || cap > INT32_MAX)) return SR_E_INVALID;
        c->env_auxgrid = (int)cap;
    } else if (!strcmp(key, "cus")) {  // the tile and fork planners and conv0's grid (all that reads sr_plan_cus): "" the device's compute units, "N" (1 .. that many): as if it had N;
                                       // forgets what the fork tuner measured, like "forktune" (sr_device_info still reports the device's own)
        long n = 0;
        for (const char* p = v; *p; ++p) {
            if (*p < '0' || *p > '9' || n > INT32_MAX / 10) return SR_E_INVALID;
            n = 10 * n + (*p - '0');
        }
        if (*v && (n < 1 || n > c->cus)) return SR_E_INVALID;
        c->plan_cus = (int)n;
        sr_device_guard restore_device;
        (void)hipSetDevice(c->device);
        sr_fork_tune_clear(c);
    } else {
        return SR_E_INVALID;
    }
    return SR_OK;
}

int sr_get_experiment(sr_ctx* c, const char* key, char* buf, size_t cap) {
    if (!c || !key || !buf || cap == 0) return SR_E_INVALID;
    std::string out;
    if (!strcmp(key, "forktune")) {  // one line per shape the tuner has met: "HxW prec io state undivided_ms forked_ms"
        char line[160];
        for (const auto& t : c->fork_tune) {
            snprintf(line, sizeof line, "%dx%d+%d+%d %s %s %s %.4f %.4f\n", t.H, t.W, t.top, t.bot, t.precision == SR_PRECISION_F32 ? "f32" : "split_f16",
                     t.img_u8 ? "u8" : "f32", t.decided < 0 ? "measuring" : (t.decided ? "forked" : "undivided"),
                     t.best[0] < 1e29f ? t.best[0] : 0.f, t.best[1] < 1e29f ? t.best[1] : 0.f);
            out += line;
        }
    } else if (!strcmp(key, "plan")) {  // what the last public call ran: "host ...", "fork ...", "launch ..." lines; " xN": N identical ones in a row
        for (const auto& r : c->plan_rec) out += r.first + (r.second > 1 ? " x" + std::to_string(r.second) : std::string()) + "\n";
    } else {
        return SR_E_INVALID;
    }
    if (out.size() + 1 > cap) return SR_E_INVALID;
    memcpy(buf, out.c_str(), out.size() + 1);
    return SR_OK;
}

int sr_set_pipeline(sr_ctx* c, int enabled) {
    if (!c) return SR_E_INVALID;
    c->pipeline = enabled != 0;
    return SR_OK;
}

int sr_host_alloc(void** out, size_t bytes) {
    if (!out || bytes == 0) return SR_E_INVALID;
    *out = nullptr;
    if (sr_no_device(false)) return SR_E_NO_DEVICE;
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return e == hipErrorOutOfMemory ? SR_E_NOMEM : SR_E_HIP; }
    return SR_OK;
}

void sr_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int sr_set_profiling(sr_ctx* c, int enabled) {
    if (!c) return SR_E_INVALID;
    c->profiling = enabled != 0;
    return SR_OK;
}

int sr_device_info(sr_ctx* c, char* name, size_t cap, int* cus, int* clock_mhz) {
    if (!c) return SR_E_INVALID;
    if (name && cap) snprintf(name, cap, "%s", c->name);
    if (cus) *cus = c->cus;
    if (clock_mhz) *clock_mhz = c->clock_mhz;
    return SR_OK;
}

}  // extern "C"

namespace {

// (Re)allocate the four zero-bordered feature maps for n images of H x W and make
// sure every border pixel is zero.  Kernels only store inside [0,H) x [0,W), so the
// borders stay clean until the geometry changes.
int ensure_features(sr_ctx* c, sr_ctx::Workspace& w, int n, int H, int W, int tiles_x, hipStream_t s) {
    const int pitch = tiles_x * 32 + 2 * kFeatPad;
    const long rows = (long)H + kFeatPad + kFeatPadBottom;
    const long img_stride = rows * pitch;
    const size_t npx = (size_t)n * img_stride + (size_t)kFeatPad * pitch + 64;  // slack for the row above image 0
    if (sr_capture_refuses(c, npx > w.feat_cap_px)) return SR_E_INVALID;
    if (c->capturing) w.captured = true;
    if (npx > w.feat_cap_px) {
        for (auto& p : w.d_feat) {
            if (p) HIPCHK(c, hipFree(p));
            p = nullptr;
        }
        w.feat_cap_px = 0; w.geo_n = 0;
        for (auto& p : w.d_feat) HIPCHK(c, hipMalloc((void**)&p, npx * 32 * sizeof(float)));
        w.feat_cap_px = npx;
        // fresh memory: everything once (interiors too: tile rows past a band's last row are computed and discarded,
        // and what they read should at least be numbers)
        for (auto& p : w.d_feat) HIPCHK(c, hipMemsetAsync(p, 0, npx * 32 * sizeof(float), s));
        w.geo_n = n; w.geo_h = H; w.geo_w = W;
    }
    if (w.captured || w.geo_n != n || w.geo_h != H || w.geo_w != W) {
        // another geometry in the same allocation: what was interior may now be border.  Only the border is cleared
        // (1080p: 6 MB per map instead of 270 MB), so a context that meets a new image size per call pays microseconds.
        // Once a pass on these maps has been captured, the clear is queued with EVERY pass, captured or not: a graph replays whenever
        // its owner likes, between calls of other geometries, so the geometry tracked here no longer says what the maps hold.
        ClearArgs ca{};
        for (int k = 0; k < 4; ++k) ca.map[k] = w.d_feat[k];
        ca.n = n; ca.H = H; ca.W = W; ca.pitch = pitch; ca.img_stride = img_stride; ca.total_px = (long)npx;
        ca.planar = c->precision == SR_PRECISION_SPLIT_F16;
        HIPCHK(c, sr_launch_clear_borders(ca, s));
        w.geo_n = n; w.geo_h = H; w.geo_w = W;
    }
    w.pitch = pitch; w.img_stride = img_stride;
    return SR_OK;
}

}  // namespace

// ensure_features would not have to allocate: the maps hold n images of H x W
static bool features_fit(const sr_ctx::Workspace& w, int n, int H, int W) {
    const int pitch = (W + 31) / 32 * 32 + 2 * kFeatPad;
    const long rows = (long)H + kFeatPad + kFeatPadBottom;
    return (size_t)n * rows * pitch + (size_t)kFeatPad * pitch + 64 <= w.feat_cap_px;
}

// The plan of a device call on a capturing stream (include/srhip.h "Stream capture"): the rule's -- the fork tuner neither decides nor
// samples there -- with the second band given up where its stream, events or maps do not exist yet.  SR_E_INVALID: the call would have to
// allocate.  *fork: run as two bands, the first of *rows_a rows.
static int capture_plan(sr_ctx* c, bool img_u8, int img_ch, int n, int H, int W, int halo_top, int halo_bot, bool* fork, int* rows_a) {
    *fork = false;
    if (c->graph != SR_GRAPH_SR_NET) return SR_OK;
    if (sr_plan_fork(*c, c->env_fork, img_u8, img_ch, n, H, W, halo_top, halo_bot, rows_a)) {  // (a tunable shape has no "fork" set: the rule)
        sr_fork_band fb[2];
        sr_fork_bands(H, halo_top, halo_bot, *rows_a, fb);
        *fork = c->stream2 && c->ev_fork[0] && c->ev_fork[1] && features_fit(c->ws[0], 1, fb[0].H, W) && features_fit(c->ws[1], 1, fb[1].H, W);
        if (*fork) return SR_OK;
    }
    return features_fit(c->ws[0], n, H, W) ? SR_OK : SR_E_INVALID;
}

int sr_net_capture_ready(sr_ctx* c, bool u8, int ch, int n, int h, int w, unsigned members) {
    if (!c->capturing) return SR_OK;
    bool fork = false;
    int rows_a = 0;
    if (members == 1u) return capture_plan(c, u8, ch, n, h, w, 0, 0, &fork, &rows_a);
    // an ensemble runs its members one image at a time on f32 copies: members 0-3 as the image lies, 4-7 transposed
    if (members & 0x0fu) SRCHK(capture_plan(c, false, 3, 1, h, w, 0, 0, &fork, &rows_a));
    if (members & 0xf0u) SRCHK(capture_plan(c, false, 3, 1, w, h, 0, 0, &fork, &rows_a));
    return SR_OK;
}

// Workspace 0's feature maps for one image of H x W, allocated now (a later pass over fewer rows finds them large enough: the frame
// stream's row bands, sr_yuv.cpp).  The context's device is current.
int sr_reserve_features(sr_ctx* c, int H, int W, hipStream_t s) { return ensure_features(c, c->ws[0], 1, H, W, (W + 31) / 32, s); }

// The context's own streams, created when first needed: `stream` for everything the library runs by itself, and for a
// pipelined host call a second compute stream and the download stream.
int sr_ensure_streams(sr_ctx* c, bool pipelined) {
    if (sr_capture_refuses(c, !c->stream || (pipelined && (!c->stream2 || !c->copy_out)))) return SR_E_INVALID;
    if (!c->stream) HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (pipelined) {
        if (!c->stream2) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        if (!c->copy_out) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking));
    }
    return SR_OK;
}

int sr_ensure_buf(sr_ctx* c, sr_buf& b, size_t bytes) {
    if (bytes <= b.cap) return SR_OK;
    if (sr_capture_refuses(c, true)) return SR_E_INVALID;
    if (b.p) HIPCHK(c, hipFree(b.p));
    b = sr_buf{};
    HIPCHK(c, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return SR_OK;
}

int sr_ensure_bufs(sr_ctx* c, std::initializer_list<sr_buf_want> group) {
    for (const sr_buf_want& w : group)  // (on a capturing stream nothing grows, and nothing of the group is given back either)
        if (sr_capture_refuses(c, w.bytes > w.buf->cap)) return SR_E_INVALID;
    for (const sr_buf_want& w : group) {
        const int rc = sr_ensure_buf(c, *w.buf, w.bytes);
        if (rc == SR_OK) continue;
        for (const sr_buf_want& g : group) sr_free_buf(*g.buf);
        return rc;
    }
    return SR_OK;
}

// The synchronous host-pointer call on the context's own stream (sr_internal.h).  The phases are callables so that whatever fails in one
// of them -- a HIPCHK around a copy as much as the queued work -- returns HERE: between the first queued operation and the drain there is
// no return, so the stream is drained also on failure: nothing of the call may still run once it has returned, neither a copy from or to
// the caller's memory nor a kernel.
int sr_host_call(sr_ctx* c, bool network, sr_host_times times, std::initializer_list<sr_buf_want> staging, const sr_host_phase& upload,
                 const sr_host_phase& work, const sr_host_phase& download) {
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    c->capturing = false;  // (the context's own stream)
    SRCHK(sr_ensure_streams(c, false));
    if (network) sr_domain_set_aside(c);
    SRCHK(sr_ensure_bufs(c, staging));
    const bool prof = c->profiling && times != SR_TIMES_NONE, parts = prof && times == SR_TIMES_PARTS;
    while (prof && c->pool.size() < 4) {
        hipEvent_t e = nullptr;
        HIPCHK(c, hipEventCreate(&e));
        c->pool.push_back(e);
    }
    hipStream_t s = c->stream;
    const auto queue = [&]() -> int {
        if (prof) HIPCHK(c, hipEventRecord(c->pool[0], s));
        int r = upload(s);
        if (r != SR_OK) return r;
        if (parts) HIPCHK(c, hipEventRecord(c->pool[1], s));
        r = work(s);
        if (r != SR_OK) return r;
        if (parts) HIPCHK(c, hipEventRecord(c->pool[2], s));
        r = download(s);
        if (r != SR_OK) return r;
        if (prof) HIPCHK(c, hipEventRecord(c->pool[3], s));
        return SR_OK;
    };
    const auto run = [&]() -> int {
        const int r = queue();
        const hipError_t drained = hipStreamSynchronize(s);
        if (r != SR_OK) return r;
        HIPCHK(c, drained);
        return SR_OK;
    };
    int rc = run();
    if (rc == SR_OK && network && sr_domain_tripped(c)) {
        // Some value of the call left the split-half mode's domain (the stream has drained: the flag is final).  A synchronous call never
        // hands out clamped pixels: the whole job is computed again in exact f32 -- graph.forward takes any f32 (main.rs:171).
        sr_plan_clear(c);
        (void)sr_set_precision(c, SR_PRECISION_F32);
        rc = run();
        (void)sr_set_precision(c, SR_PRECISION_SPLIT_F16);
    }
    if (rc != SR_OK || !prof) return rc;
    float ms = 0;  // sr_last_timing; the stage times are the conv stack's own (its last pass's)
    if (parts) {
        HIPCHK(c, hipEventElapsedTime(&ms, c->pool[0], c->pool[1])); c->h2d_ms = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, c->pool[1], c->pool[2])); c->total_ms = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, c->pool[2], c->pool[3])); c->d2h_ms = ms;
    } else {
        HIPCHK(c, hipEventElapsedTime(&ms, c->pool[0], c->pool[3])); c->total_ms = ms;
    }
    return SR_OK;
}

int sr_host_image_call(sr_ctx* c, bool network, const void* in, size_t in_bytes, void* out, size_t out_bytes, const sr_image_work& work) {
    return sr_host_call(
        c, network, SR_TIMES_PARTS, {{&c->d_in[0], in_bytes}, {&c->d_out[0], out_bytes}},
        [&](hipStream_t s) { return sr_hip_status(c, hipMemcpyAsync(c->d_in[0].p, in, in_bytes, hipMemcpyHostToDevice, s)); },
        [&](hipStream_t s) { return work(c->d_in[0].p, c->d_out[0].p, s); },
        [&](hipStream_t s) { return sr_hip_status(c, hipMemcpyAsync(out, c->d_out[0].p, out_bytes, hipMemcpyDeviceToHost, s)); });
}

int sr_reserve_bufs(sr_ctx* c, std::initializer_list<sr_buf_want> group) {
    bool fits = true;
    for (const sr_buf_want& w : group) fits = fits && w.bytes <= w.buf->cap;
    if (fits) return SR_OK;
    if (sr_capture_refuses(c, true)) return SR_E_INVALID;
    if (!c->total_mem) HIPCHK(c, hipDeviceTotalMem(&c->total_mem, c->device));
    size_t all = 0;
    if (!sr_sum_wants(group, &all) || all > c->total_mem) return SR_E_NOMEM;
    return sr_ensure_bufs(c, group);
}

int sr_net_check(const sr_ctx* c, const void* in, const void* out, int n, int h, int w, unsigned members) {
    if (!in || !out) return SR_E_INVALID;
    return sr_net_check_shape(c, n, h, w, members);
}

int sr_net_check_shape(const sr_ctx* c, int n, int h, int w, unsigned members) {
    if (!c) return SR_E_INVALID;
    if (c->graph != SR_GRAPH_SR_NET && c->graph != SR_GRAPH_BILINEAR) return SR_E_INVALID;
    if (n < 1 || h < 1 || w < 1 || h > INT32_MAX / c->factor || w > INT32_MAX / c->factor) return SR_E_INVALID;
    if (members == 0 || members > 255u) return SR_E_INVALID;
    if (members != 1u && c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    return SR_OK;
}

int sr_net_queue(sr_ctx* c, const void* d_in, bool u8, int ch, int n, int h, int w, void* d_out, bool out_u8, unsigned members, hipStream_t s) {
    if (members == 1u) return sr_run_stack_auto(c, d_in, u8, ch, n, h, w, 0, 0, d_out, out_u8, s);
    const sr_net_strides at = sr_net_image_strides(c->factor, u8, ch, out_u8, h, w);
    for (int i = 0; i < n; ++i)
        SRCHK(sr_ensemble_queue(c, (const char*)d_in + i * at.in_img, u8, ch, h, w, (char*)d_out + i * at.out_img, out_u8, members, s));
    return SR_OK;
}

namespace {

// One pass of the conv stack over rows [top, bot) of n images of H x W on one stream with one workspace: planned first
// (tile classes, grids), then launched stage by stage -- so that two jobs (the two bands of a forked call) can be issued
// interleaved, stage for stage, each on its own stream.
struct StackJob {
    sr_ctx* c = nullptr;
    sr_ctx::Workspace* ws = nullptr;
    const void* d_img = nullptr;
    void* d_out = nullptr;
    bool img_u8 = false, out_u8 = false;
    int img_ch = 3, n = 1, H = 0, W = 0, top = 0, bot = 0, tiles_x = 0;
    bool forked = false;  // one of the two bands of sr_run_stack_auto: no 4-row tail (sr_tile_plan)
    bool layers = false;  // every stage computes rows [top, bot) only: the rows beyond come from the neighbours' maps (sr_band_pass)
    // rows [0, late_top) and [H - late_bot, H) of the image arrive with gate->ready (sr_internal.h sr_halo_gate); mark: record gate->mark around the wait
    const sr_halo_gate* gate = nullptr;
    int late_top = 0, late_bot = 0;
    bool mark = false;
    hipStream_t s = nullptr;
    sr_launch_plan L[5];
    float* feat[4] = {nullptr, nullptr, nullptr, nullptr};
    int prepare();
    int launch(int st) const;
};

int StackJob::prepare() {
    tiles_x = (W + 31) / 32;
    SRCHK(ensure_features(c, *ws, n, H, W, tiles_x, s));
    // pointers to pixel (0,0) of image 0 inside the zero-bordered maps
    // (row-planar maps of the split-half mode: pixel (0,0) of channel group 0 -- kFeatPad rows down, kFeatPad 16-byte cells in)
    const bool planar = c->precision == SR_PRECISION_SPLIT_F16;
    for (int k = 0; k < 4; ++k) feat[k] = ws->d_feat[k] + (planar ? (size_t)kFeatPad * ws->pitch * 32 + kFeatPad * 4 : ((size_t)kFeatPad * ws->pitch + kFeatPad) * 32);
    // ---- plan every launch first: conv0 (the call's first launch) sets the tile-queue heads of the four stage kernels
    sr_tile_plan(*c, n, H, W, top, bot, forked, layers, L);
    return SR_OK;
}

// A job over rows [top, bot) of n images of H x W, on stream s with workspace `slot`; gate: all of it behind that gate, the wait marked
StackJob stack_job(sr_ctx* c, int slot, const void* d_img, bool img_u8, int img_ch, int n, int H, int W, int top, int bot, void* d_out, bool out_u8,
                   hipStream_t s, const sr_halo_gate* gate = nullptr) {
    StackJob job;
    job.c = c; job.ws = &c->ws[slot]; job.d_img = d_img; job.d_out = d_out; job.img_u8 = img_u8; job.out_u8 = out_u8;
    job.img_ch = img_ch; job.n = n; job.H = H; job.W = W; job.top = top; job.bot = bot; job.s = s;
    if (gate) { job.gate = gate; job.late_top = gate->top; job.late_bot = gate->bot; job.mark = true; }
    return job;
}

int StackJob::launch(int st) const {
    const int cus = sr_plan_cus(*c);
    const float* P = c->d_params;
    const int bw = c->env_bw >= 0 ? c->env_bw : kAutoBlockWidth;
    const sr_launch_plan& l = L[st];
    const int y0 = l.y0, y1 = l.y1;
    {
        char line[160];
        snprintf(line, sizeof line, "launch st=%d form=%s ty8=%d ty4=%d grid=%d prec=%s f=%d img=%s out=%s ch=%d", st, l.pipe ? "pipe" : "first", l.ty8,
                 l.ty4, l.grid, c->precision == SR_PRECISION_SPLIT_F16 ? "split_f16" : "f32", c->factor, img_u8 ? "u8" : "f32", out_u8 ? "u8" : "f32",
                 img_u8 ? img_ch : 3);
        sr_plan_note(c, line);
    }
    if (st == 0) {
        auto rows = [&](int ya, int yb) -> int {  // f rows [ya, yb)
            if (ya >= yb) return SR_OK;
            const int tiles_y = (yb - ya + l.th - 1) / l.th;
            Conv0Args a{};
            a.img = d_img; a.wpack = P + c->off_w0; a.wpack_split = P + c->off_w0h; a.bias = P + c->off_bias[0]; a.beta = P + c->off_beta[0];
            a.dst = feat[0]; a.H = H; a.W = W; a.img_ch = img_ch;
            a.pitch = ws->pitch; a.img_stride = ws->img_stride;
            a.y_begin = ya; a.y_end = yb; a.tiles_x = tiles_x; a.tiles_y = tiles_y;
            a.div_tpi = make_tile_div((uint32_t)(tiles_x * tiles_y)); a.div_tx = make_tile_div((uint32_t)tiles_x);
            a.n_tiles = n * tiles_x * tiles_y;
            a.queue_reset = ws->d_queue;  // (every stage-0 launch of the call sets the same heads: the stage kernels follow them all)
            a.domain = c->d_domain;
            for (int k = 1; k < 5; ++k) a.queue_grid[k] = L[k].grid;
            // (grid: 8 workgroups per CU walking the tiles with a fixed stride; measured with 8 / 12 / 16 / 32 per CU, one per tile, and
            // a grid that divides the tile count evenly: conv0's time does not depend on it)
            HIPCHK(c, sr_launch_conv0(a, l.th, c->precision, std::min(a.n_tiles, 8 * cus), img_u8, s));
            return SR_OK;
        };
        if (!gate || !gate->ready) return rows(y0, y1);
        // Interior first (sr_halo_gate): f row y reads image rows y - 2 .. y + 2; those that touch none of the rows still on their way
        // are launched now, the rest -- at most 2 + the stage's margin rows either side -- behind the wait.
        const int lo = late_top > 0 ? std::max(y0, late_top + 2) : y0, hi = late_bot > 0 ? std::min(y1, H - late_bot - 2) : y1;
        SRCHK(lo < hi ? rows(lo, hi) : SR_OK);
        if (mark && gate->mark[0]) HIPCHK(c, hipEventRecord(gate->mark[0], s));
        HIPCHK(c, hipStreamWaitEvent(s, gate->ready, 0));
        if (mark && gate->mark[1]) HIPCHK(c, hipEventRecord(gate->mark[1], s));
        if (lo >= hi) return rows(y0, y1);
        SRCHK(rows(y0, lo));
        return rows(hi, y1);
    }
    StageArgs a{};
    float* f = feat[0]; float* l1 = feat[1]; float* l2 = feat[2]; float* l3 = feat[3];
    a.pitch = ws->pitch; a.img_stride = ws->img_stride;
    switch (st) {
        case 1: a.src[0] = f; a.dst = l1; break;
        case 2: a.src[0] = f; a.src[1] = l1; a.dst = l2; break;
        case 3: a.src[0] = f; a.src[1] = l1; a.src[2] = l2; a.dst = l3; break;
        case 4: a.src[0] = l1; a.src[1] = l2; a.src[2] = l3; a.img = d_img; a.out = d_out; break;
    }
    const bool wino = c->precision == SR_PRECISION_F32 && (st == 1 || st == 2) && st <= c->wino;
    const int wino5 = wino && st == 2 ? c->wino5 : 0;
    a.wpack = P + (c->precision ? c->off_wh[st] : !wino ? c->off_w[st] : st == 1 ? c->off_wino1 : c->off_wino2[wino5]); a.bias = P + c->off_bias[st];
    a.beta = st < 4 ? P + c->off_beta[st] : nullptr;
    a.H = H; a.W = W; a.img_ch = img_ch;
    a.y_begin = y0; a.y_end = y1; a.tiles_x = tiles_x;
    a.n_img = n; a.queue = ws->d_queue + st * 8; a.domain = c->d_domain;
    a.grid[0] = make_tile_grid(8, y0, l.ty8, tiles_x, n, bw);
    a.grid[1] = make_tile_grid(4, y0 + 8 * l.ty8, l.ty4, tiles_x, n, bw);
    if (l.pipe) HIPCHK(c, sr_launch_stage_pipe(st, c->factor, a, c->precision, l.grid, img_u8, out_u8, wino, wino5, s));
    else HIPCHK(c, sr_launch_stage(st, c->factor, a, l.th, c->precision, l.grid, img_u8, out_u8, wino, wino5, s));
    return SR_OK;
}

}  // namespace

// The whole conv stack on device buffers.  Rows [halo_top, H - halo_bot) of each
// of the n images are produced; each earlier stage computes just the extra rows
// the later ones read (f +-5, l1 +-3, l2 +-2, l3 +-1 around the band).
int sr_run_stack(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int n, int H, int W, int halo_top,
                 int halo_bot, void* d_out, bool out_u8, hipStream_t s, int slot, const sr_halo_gate* gate) {
    if (!c || !d_img || !d_out || slot < 0 || slot > 1) return SR_E_INVALID;
    sr_device_guard restore_device;
    if (c->graph != SR_GRAPH_SR_NET && (halo_top || halo_bot || gate)) return SR_E_INVALID;  // (a parameter-free graph takes no band)
    SRCHK(sr_check_band_args(img_u8, img_ch, n, H, W, halo_top, halo_bot));
    if (c->graph != SR_GRAPH_SR_NET) {  // bilinear_net / downsample_net: one elementwise kernel
        if (c->graph == SR_GRAPH_DOWNSAMPLE && (H < 3 || W < 3)) return SR_E_INVALID;
        if (img_u8 != out_u8) return SR_E_INVALID;
        HIPCHK(c, hipSetDevice(c->device));
        AuxArgs a{d_img, d_out, n, H, W, img_ch, c->d_qtab};
        AuxLaunch ran{0, 0};
        HIPCHK(c, sr_launch_aux(c->graph, a, img_u8, out_u8, s, c->env_auxgrid, &ran));
        if (ran.grid > 0) {
            char line[128];
            snprintf(line, sizeof line, "aux graph=%s img=%s ch=%d grid=%d units=%ld", c->graph == SR_GRAPH_BILINEAR ? "bilinear" : "downsample",
                     img_u8 ? "u8" : "f32", img_u8 ? img_ch : 3, ran.grid, ran.units);
            sr_plan_note(c, line);
        }
        c->last_h = H; c->last_w = W;
        return SR_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // s == nullptr is HIP's legacy default stream (what torch's default stream is);
    // the context's own non-blocking stream is used only by the host-pointer entry points.
    StackJob job = stack_job(c, slot, d_img, img_u8, img_ch, n, H, W, halo_top, H - halo_bot, d_out, out_u8, s, gate);
    SRCHK(job.prepare());
    const bool prof = c->profiling && !c->capturing;  // (the stage events are waited for below: not on a capturing stream)
    static const bool trace_stages_env = [] { const char* e = getenv("SRHIP_TRACE"); return e && atoi(e) >= 2; }();
    const bool trace_stages = trace_stages_env && !c->capturing;
    if (prof) HIPCHK(c, hipEventRecord(c->ev[0], s));
    for (int st = 0; st < 5; ++st) {
        SRCHK(job.launch(st));
        if (prof) HIPCHK(c, hipEventRecord(c->ev[st + 1], s));
        if (trace_stages) {  // SRHIP_TRACE=2: which launch a hang or a fault belongs to
            const sr_launch_plan& l = job.L[st];
            fprintf(stderr, "[srhip] stage %d launched: rows [%d,%d) th8 x%d th4 x%d grid %d %s ... ", st, l.y0, l.y1, l.ty8, l.ty4, l.grid, l.pipe ? "pipe" : "first");
            const hipError_t e = hipStreamSynchronize(s);
            fprintf(stderr, "%s\n", e == hipSuccess ? "done" : hipGetErrorString(e));
        }
    }
    c->last_h = H; c->last_w = W;
    if (prof) {
        c->band_pending = false;
        HIPCHK(c, hipEventSynchronize(c->ev[5]));
        float ms = 0;
        for (int st = 0; st < 5; ++st) {
            HIPCHK(c, hipEventElapsedTime(&ms, c->ev[st], c->ev[st + 1]));
            c->stage_ms[st] = ms;
        }
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[5]));
        c->total_ms = ms;
    }
    return SR_OK;
}

struct sr_band_pass {
    StackJob job;
};

int sr_band_pass_begin(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int H, int W, int halo_top, int halo_bot, void* d_out, bool out_u8,
                       hipStream_t s, bool layers, const sr_halo_gate* gate, sr_band_pass** out) {
    if (!c || !d_img || !d_out || !out || c->graph != SR_GRAPH_SR_NET || H <= 0 || W <= 0) return SR_E_INVALID;
    *out = nullptr;
    SRCHK(sr_check_band_args(img_u8, img_ch, 1, H, W, halo_top, halo_bot));
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    sr_band_pass* p = new (std::nothrow) sr_band_pass();
    if (!p) return SR_E_NOMEM;
    StackJob& job = p->job;
    job = stack_job(c, 0, d_img, img_u8, img_ch, 1, H, W, halo_top, H - halo_bot, d_out, out_u8, s, gate);
    job.layers = layers;
    const int rc = job.prepare();
    if (rc != SR_OK) { delete p; return rc; }
    c->band_pending = false;
    c->last_h = c->last_w = 0;  // (with `layers` the maps hold this band's own rows and its neighbours' edge rows: not an image sr_read_feature could return)
    *out = p;
    return SR_OK;
}

int sr_band_pass_stage(sr_band_pass* p, int st) {
    if (!p || st < 0 || st > 4) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(p->job.c, hipSetDevice(p->job.c->device));
    return p->job.launch(st);
}

float* sr_band_pass_row(const sr_band_pass* p, int map, int y) {
    // pixel (y, -kFeatPad) of the map: in both layouts row y of the padded buffer begins (kFeatPad + y) x pitch pixels of 32 floats in
    return p->job.ws->d_feat[map] + (size_t)(kFeatPad + y) * p->job.ws->pitch * 32;
}

size_t sr_band_pass_row_floats(const sr_band_pass* p) { return (size_t)p->job.ws->pitch * 32; }

void sr_band_pass_end(sr_band_pass* p) { delete p; }

// One image as TWO row bands on two streams.  Each band carries the SR_HALO rows of the other it needs and is
// bit-identical to the undivided pass like every band; the second runs on the context's own second stream and workspace, forked
// from the caller's stream by an event and joined back by another, the launches of the two issued alternately -- the call stays
// asynchronous and ordered on the caller's stream.  What it buys, measured: the dispatcher runs the two bands' stage launches side
// by side (a workgroup of either per CU), so their ramps -- every workgroup's first gather from a cold L2, the partly filled last
// round of tiles -- overlap the other band's matrix work; against that stand ten launches instead of five, 14 recomputed rows
// and ~17 us of join / fork between consecutive calls.  Net, with the bands' launches free of 4-row tails: -0.8 ... -3.8 % for
// exact-f32 images from 3.5 rounds of tiles on, -0.1 % at 3840x2160; a loss in the split-half mode: hence the rule below.  Costs a
// second set of feature maps (each band's are half the size).
namespace {

// ---- the fork decision measured on the caller's own calls (sr_internal.h ForkTune) ----------------------------------------------
constexpr int kForkTuneBlock = 4;     // calls per plan: one dropped (the workspace meets a new geometry, first-use allocations), three timed
constexpr size_t kForkTuneShapes = 8;  // shapes remembered per context
constexpr float kForkTuneGain = 0.985f;  // the fork must win by 1.5 % to be chosen: it costs a second workspace

void fork_tune_release(sr_ctx::ForkTune& t) {
    for (auto& e : t.ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
}

// The entry of this shape (created, with its two timing events, on first sight; the one used longest ago makes room).  Null: no tuning.
sr_ctx::ForkTune* fork_tune_entry(sr_ctx* c, bool img_u8, bool out_u8, int img_ch, int H, int W, int halo_top, int halo_bot) {
    ++c->fork_tune_clock;
    for (auto& t : c->fork_tune)
        if (t.H == H && t.W == W && t.top == halo_top && t.bot == halo_bot && t.img_u8 == img_u8 && t.out_u8 == out_u8 &&
            t.img_ch == (img_u8 ? img_ch : 3) && t.precision == c->precision) { t.used = c->fork_tune_clock; return &t; }
    if (c->fork_tune.size() >= kForkTuneShapes) {
        size_t oldest = 0;
        for (size_t k = 1; k < c->fork_tune.size(); ++k) if (c->fork_tune[k].used < c->fork_tune[oldest].used) oldest = k;
        fork_tune_release(c->fork_tune[oldest]);  // (an event still in flight is released when it completes: hipEventDestroy's contract)
        c->fork_tune.erase(c->fork_tune.begin() + (long)oldest);
    }
    sr_ctx::ForkTune t;
    t.H = H; t.W = W; t.top = halo_top; t.bot = halo_bot; t.img_u8 = img_u8; t.out_u8 = out_u8; t.img_ch = img_u8 ? img_ch : 3; t.precision = c->precision;
    t.used = c->fork_tune_clock;
    for (auto& e : t.ev)
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); fork_tune_release(t); return nullptr; }
    c->fork_tune.push_back(t);
    return &c->fork_tune.back();
}

// Read the sample in flight if it has finished -- a query, never a wait.  A sample that cannot be read (a capturing stream, a device
// error) ends the measurement in favour of the rule.
void fork_tune_harvest(sr_ctx::ForkTune& t, int rule) {
    if (!t.pending) return;
    const hipError_t q = hipEventQuery(t.ev[1]);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return; }
    float ms = 0.f;
    if (q != hipSuccess || hipEventElapsedTime(&ms, t.ev[0], t.ev[1]) != hipSuccess || !(ms > 0.f)) {
        (void)hipGetLastError();
        t.pending = false; t.decided = rule;
        return;
    }
    t.pending = false;
    const int plan = t.taken < kForkTuneBlock ? 0 : 1;
    if (t.taken % kForkTuneBlock != 0) t.best[plan] = std::min(t.best[plan], ms);
    if (++t.taken >= 2 * kForkTuneBlock) t.decided = t.best[1] < kForkTuneGain * t.best[0] ? 1 : 0;
}

}  // namespace

void sr_fork_tune_clear(sr_ctx* c) {
    for (auto& t : c->fork_tune) fork_tune_release(t);
    c->fork_tune.clear();
}

int sr_ensure_fork_resources(sr_ctx* c) {
    if (sr_capture_refuses(c, !c->stream2 || !c->ev_fork[0] || !c->ev_fork[1])) return SR_E_INVALID;
    if (!c->stream2) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    for (auto& e : c->ev_fork) if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return SR_OK;
}

int sr_run_stack_auto(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int n, int H, int W, int halo_top, int halo_bot,
                      void* d_out, bool out_u8, hipStream_t s, const sr_halo_gate* gate) {
    if (!c || !d_img || !d_out) return SR_E_INVALID;
    c->band_pending = false;  // (the event pairs of an earlier sharded call are not this call's: sr_comm.cpp sets the flag again behind its own)
    int rows_a = 0;
    sr_device_guard restore_device;
    int mode = c->env_fork;
    sr_ctx::ForkTune* tune = nullptr;
    bool sample = false;
    if (c->capturing) {
        // Nothing may be allocated and no event of the tuner's recorded or read (a captured call is no sample: its events never fire, and
        // a replay is not this call).  Decided before the fork event, so that a refusal leaves the capture as it was.
        bool fork = false;
        HIPCHK(c, hipSetDevice(c->device));
        SRCHK(capture_plan(c, img_u8, img_ch, n, H, W, halo_top, halo_bot, &fork, &rows_a));
        mode = fork ? c->env_fork : 0;
    } else if (sr_fork_tunable(*c, n, H, W, halo_top, halo_bot, gate != nullptr)) {
        HIPCHK(c, hipSetDevice(c->device));
        tune = fork_tune_entry(c, img_u8, out_u8, img_ch, H, W, halo_top, halo_bot);
        if (tune) {
            int rows_rule = 0;
            const int rule = sr_plan_fork(*c, -1, img_u8, img_ch, n, H, W, halo_top, halo_bot, &rows_rule) ? 1 : 0;
            if (tune->decided < 0) fork_tune_harvest(*tune, rule);
            if (tune->decided >= 0) {
                mode = tune->decided;
            } else {
                mode = tune->taken < kForkTuneBlock ? 0 : 1;  // this block's plan; timed unless the last sample is still in flight
                sample = !tune->pending;
            }
        }
    }
    if (sample && hipEventRecord(tune->ev[0], s) != hipSuccess) { (void)hipGetLastError(); sample = false; }
    auto sampled = [&](int rc) {  // the closing event of a timed call, on the caller's stream (behind the join of a forked one)
        if (sample && rc == SR_OK) {
            if (hipEventRecord(tune->ev[1], s) == hipSuccess) tune->pending = true; else (void)hipGetLastError();
        }
        return rc;
    };
    if (!sr_plan_fork(*c, mode, img_u8, img_ch, n, H, W, halo_top, halo_bot, &rows_a)) {
        if (tune && tune->decided < 0 && mode == 1) tune->decided = 0;  // (cannot be forked at all)
        if (c->graph == SR_GRAPH_SR_NET) sr_plan_note(c, "fork 0");
        return sampled(sr_run_stack(c, d_img, img_u8, img_ch, n, H, W, halo_top, halo_bot, d_out, out_u8, s, 0, gate));
    }
    HIPCHK(c, hipSetDevice(c->device));
    SRCHK(sr_ensure_fork_resources(c));
    const size_t in_px = img_u8 ? (size_t)img_ch : 3 * sizeof(float), out_px = out_u8 ? 4 : 3 * sizeof(float);
    sr_fork_band fb[2];
    sr_fork_bands(H, halo_top, halo_bot, rows_a, fb);
    StackJob a = stack_job(c, 0, d_img, img_u8, img_ch, 1, fb[0].H, W, fb[0].top, fb[0].bot, d_out, out_u8, s);
    StackJob b = stack_job(c, 1, (const char*)d_img + (size_t)fb[1].first_row * W * in_px, img_u8, img_ch, 1, fb[1].H, W, fb[1].top, fb[1].bot,
                           (char*)d_out + (size_t)rows_a * c->factor * W * c->factor * out_px, out_u8, c->stream2);
    a.forked = b.forked = true;
    if (gate) {  // the first band holds the late rows at the image's top, the second those at its bottom; the caller's stream is the one whose wait is timed
        a.gate = b.gate = gate; a.late_top = gate->top; b.late_bot = gate->bot; a.mark = true;
    }
    HIPCHK(c, hipEventRecord(c->ev_fork[0], s));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork[0], 0));
    // Both bands are planned (and their workspaces allocated) before anything is launched: should the second set of feature maps not fit,
    // the undivided pass on the first workspace still may -- the call must not fail for want of an optimisation's memory.
    SRCHK(a.prepare());  // (the first band's maps do not fit: the undivided pass, which needs larger ones, cannot either)
    int rc = b.prepare();
    if (rc == SR_E_NOMEM) {  // the second workspace is the optimisation's: give back what of it exists and run undivided on the first
        for (auto& p : c->ws[1].d_feat) { if (p) (void)hipFree(p); p = nullptr; }
        c->ws[1].feat_cap_px = 0; c->ws[1].geo_n = 0;
        if (tune && tune->decided < 0) tune->decided = 0;  // (no room for the fork's second workspace)
        sample = false;
        sr_plan_note(c, "fork 0 nomem");
        return sr_run_stack(c, d_img, img_u8, img_ch, n, H, W, halo_top, halo_bot, d_out, out_u8, s, 0, gate);
    }
    sr_plan_note(c, "fork 1 " + std::to_string(rows_a) + "," + std::to_string(H - halo_top - halo_bot - rows_a));
    for (int st = 0; st < 5 && rc == SR_OK; ++st) {
        rc = a.launch(st);
        if (rc == SR_OK) rc = b.launch(st);
    }
    // join also on failure: whatever was queued on the second stream must be ordered before the caller's next work
    const hipError_t e1 = hipEventRecord(c->ev_fork[1], c->stream2);
    const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(s, c->ev_fork[1], 0) : e1;
    if (rc != SR_OK) return rc;
    HIPCHK(c, e1); HIPCHK(c, e2);
    c->last_h = c->last_w = 0;  // each workspace holds one band: sr_read_feature refuses
    return sampled(SR_OK);
}

namespace {

// Host-pointer entry points: upload, conv stack, download -- software-pipelined over chunks on
// three streams.  Issue order is H2D(i+1), kernels(i+1), D2H(i): with pageable caller memory the
// runtime blocks the calling thread inside each copy, and this order keeps kernels queued behind
// it; with pinned memory (sr_host_alloc) all three engines run concurrently.
// reserve: no caller buffers -- everything else of the call happens (allocations, events, the kernels on whatever the
// staging buffers hold), so that the first real call costs what every later one does (sr_reserve_*).
int run_host(sr_ctx* c, const void* in, bool img_u8, int img_ch, sr_deal deal, int h, int w, void* out, bool out_u8, int y_lo = 0,
             int y_hi = -1, bool reserve = false) {
    const int n = deal.count;
    if (!c || ((!in || !out) && !reserve) || n <= 0 || h <= 0 || w <= 0 || deal.first < 0 || deal.stride < 1) return SR_E_INVALID;
    if (img_u8 && img_ch != 3 && img_ch != 4) return SR_E_INVALID;
    if (c->graph == SR_GRAPH_DOWNSAMPLE && (h < 3 || w < 3)) return SR_E_INVALID;
    if (c->graph != SR_GRAPH_SR_NET && img_u8 != out_u8) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    c->band_pending = false;  // (an earlier sharded call's event pairs are not this call's timing)
    c->capturing = false;     // (the context's own streams)
    const size_t in_px = img_u8 ? (size_t)img_ch : 3 * sizeof(float), out_px = out_u8 ? 4 : 3 * sizeof(float);
    if (y_hi < 0) y_hi = h;
    if (y_lo < 0 || y_hi > h || y_lo >= y_hi) return SR_E_INVALID;
    if ((y_lo > 0 || y_hi < h) && (n != 1 || c->graph != SR_GRAPH_SR_NET)) return SR_E_INVALID;
    if (y_lo > 0 && y_lo < SR_HALO) return SR_E_HALO;
    if (y_hi < h && h - y_hi < SR_HALO) return SR_E_HALO;
    sr_domain_set_aside(c);
    bool in_order = false;
    const std::vector<sr_chunk> plan = sr_plan_chunks(*c, deal, h, w, in_px, out_px, y_lo, y_hi, &in_order);
    const int nch = (int)plan.size();
    const int slots = nch > 1 ? 2 : 1;
    {
        // one | batch (images per chunk) | inorder / alternating (band rows, top to bottom); rows=: a share of the image (multi-context calls)
        const bool bands = nch > 1 && (plan[0].halo_top > 0 || plan[0].halo_bot > 0);
        std::string line = std::string("host ") + (nch == 1 ? "one" : !bands ? "batch" : in_order ? "inorder" : "alternating");
        for (int i = 0; i < nch; ++i)
            line += (i ? "," : " ") + std::to_string(bands ? (int)(plan[i].out_bytes / ((size_t)c->factor * c->factor * w * out_px)) : plan[i].n);
        if (y_lo > 0 || y_hi < h) line += " rows=" + std::to_string(y_lo) + ":" + std::to_string(y_hi);
        if (c->graph == SR_GRAPH_SR_NET) sr_plan_note(c, line);
    }
    SRCHK(sr_ensure_streams(c, nch > 1));
    // One chunk: upload, kernels and download in order on `stream`.  Several: chunk i uploads on the stream its kernels
    // follow on (the other compute stream is busy with chunk i-1 meanwhile) -- or, when all chunks compute in order on
    // `stream`, on the idle `stream2` -- and downloads on `copy_out`.
    // A dedicated upload stream (a third hardware queue, 8-40 ms to create) lets chunk i+1 arrive while both compute streams
    // are busy.  Measured A/B (profiles/r2_upload_stream_ab.txt): worth 1-2 % of an exact-f32 1080p call, nothing at 4K, and
    // 2 % SLOWER in the split-half mode (whose calls are download-bound) -- so only exact-f32 contexts get one, and only from
    // their second pipelined call on: a one-shot process never pays for it, a service does once.
    if (nch > 1 && !reserve && c->precision == SR_PRECISION_F32 && ++c->pipelined_calls >= 2 && !c->copy_in)
        HIPCHK(c, hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
    // (pipelined_calls: a frame stream creates copy_in too, sr_yuv.cpp -- that must not move this call's first pipelined pass onto it)
    const bool own_upload = nch > 1 && c->copy_in && c->pipelined_calls >= 2 && c->precision == SR_PRECISION_F32;
    hipStream_t down = nch > 1 ? c->copy_out : c->stream;
    size_t in_max = 0, out_max = 0;
    for (const sr_chunk& k : plan) { in_max = std::max(in_max, k.in_bytes); out_max = std::max(out_max, k.out_bytes); }
    const size_t in1 = slots == 2 ? in_max : 0, out1 = slots == 2 ? out_max : 0;
    SRCHK(sr_ensure_bufs(c, {{&c->d_in[0], in_max}, {&c->d_out[0], out_max}, {&c->d_in[1], in1}, {&c->d_out[1], out1}}));
    // events per chunk: 0 upload begins, 1 upload done, 2 kernels begin, 3 kernels done, 4 download done
    while (c->pool.size() < (size_t)nch * 5) {
        hipEvent_t e = nullptr;
        HIPCHK(c, hipEventCreate(&e));
        c->pool.push_back(e);
    }
    auto ev = [&](int i, int k) { return c->pool[(size_t)i * 5 + k]; };
    const char* src = (const char*)in;
    char* dst = (char*)out;
    // a chunk's images are contiguous on the device; in the caller's buffers they are in_step / out_step apart
    auto copy_images = [&](const sr_chunk& k, bool up, int sl, hipStream_t on) -> int {
        if (reserve) return SR_OK;
        const bool contiguous = k.n == 1 || (up ? k.in_step == k.in_bytes / k.n : k.out_step == k.out_bytes / k.n);
        const int pieces = contiguous ? 1 : k.n;
        const size_t in_img = k.in_bytes / (contiguous ? 1 : k.n), out_img = k.out_bytes / (contiguous ? 1 : k.n);
        for (int j = 0; j < pieces; ++j) {
            if (up) HIPCHK(c, hipMemcpyAsync((char*)c->d_in[sl].p + j * in_img, src + k.in_off + j * k.in_step, in_img, hipMemcpyHostToDevice, on));
            else HIPCHK(c, hipMemcpyAsync(dst + k.out_off + j * k.out_step, (const char*)c->d_out[sl].p + j * out_img, out_img, hipMemcpyDeviceToHost, on));
        }
        return SR_OK;
    };
    // chunk i computes on stream i % 2 with workspace i % 2: consecutive chunks' stage launches overlap (the tail of one
    // launch -- its last, partly filled round of workgroups -- runs beside the head of the other stream's next launch;
    // measured at 1080p, one stream: five bands cost 19 % more kernel time than the undivided pass)
    // (a geometric band plan wants the opposite: band i finished, and downloading, before band i+1 takes the chip)
    auto cstream = [&](int i) { return (slots == 2 && (i & 1) && !in_order) ? c->stream2 : c->stream; };
    auto issue_front = [&](int i) -> int {  // upload + kernels of chunk i
        const sr_chunk& k = plan[i];
        const int sl = i % slots;
        hipStream_t cs = cstream(i);
        hipStream_t upl = own_upload ? c->copy_in : (in_order && nch > 1) ? c->stream2 : cs;
        if (i >= 2) HIPCHK(c, hipStreamWaitEvent(upl, ev(i - 2, 3), 0));  // slot's previous reader
        HIPCHK(c, hipEventRecord(ev(i, 0), upl));
        SRCHK(copy_images(k, true, sl, upl));
        HIPCHK(c, hipEventRecord(ev(i, 1), upl));
        if (upl != cs) HIPCHK(c, hipStreamWaitEvent(cs, ev(i, 1), 0));
        if (i >= 2) HIPCHK(c, hipStreamWaitEvent(cs, ev(i - 2, 4), 0));   // slot's previous download
        HIPCHK(c, hipEventRecord(ev(i, 2), cs));
        SRCHK(sr_run_stack(c, c->d_in[sl].p, img_u8, img_ch, k.n, k.h_ext, w, k.halo_top, k.halo_bot, c->d_out[sl].p, out_u8, cs, sl));
        HIPCHK(c, hipEventRecord(ev(i, 3), cs));
        return SR_OK;
    };
    auto issue_back = [&](int i) -> int {  // download of chunk i
        if (down != cstream(i)) HIPCHK(c, hipStreamWaitEvent(down, ev(i, 3), 0));
        SRCHK(copy_images(plan[i], false, i % slots, down));
        HIPCHK(c, hipEventRecord(ev(i, 4), down));
        return SR_OK;
    };
    int rc = issue_front(0);
    for (int i = 0; i < nch && rc == SR_OK; ++i) {
        if (i + 1 < nch) rc = issue_front(i + 1);
        if (rc == SR_OK) rc = issue_back(i);
    }
    // drain everything before returning, ALSO on failure: copies into / out of the caller's buffers and kernels on
    // the context's stream must not be in flight once the call has returned
    const hipError_t e1 = own_upload ? hipStreamSynchronize(c->copy_in) : hipSuccess, e2 = hipStreamSynchronize(c->stream), e4 = nch > 1 ? hipStreamSynchronize(c->stream2) : hipSuccess,
                     e3 = nch > 1 ? hipStreamSynchronize(c->copy_out) : hipSuccess;
    if (rc != SR_OK) return rc;
    HIPCHK(c, e1); HIPCHK(c, e2); HIPCHK(c, e4); HIPCHK(c, e3);
    double h2d = 0, ker = 0, d2h = 0;
    for (int i = 0; i < nch; ++i) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, ev(i, 0), ev(i, 1))); h2d += ms;
        // chunks overlap on two compute streams: kernel time = first kernel start -> last kernel end
        HIPCHK(c, hipEventElapsedTime(&ms, ev(0, 2), ev(i, 3))); ker = std::max(ker, (double)ms);
        HIPCHK(c, hipEventElapsedTime(&ms, ev(i, 3), ev(i, 4))); d2h += ms;  // includes waiting for the copy engine
    }
    c->h2d_ms = h2d; c->total_ms = ker; c->d2h_ms = d2h; c->band_pending = false;
    if (nch > 1) c->last_h = c->last_w = 0;  // the feature maps hold one chunk only: sr_read_feature refuses
    if (sr_domain_tripped(c)) {  // (every stream has drained: the flag is final) the whole job again in exact f32, as sr_host_call does
        if (reserve) return SR_OK;
        (void)sr_set_precision(c, SR_PRECISION_F32);
        const int rc2 = run_host(c, in, img_u8, img_ch, deal, h, w, out, out_u8, y_lo, y_hi, false);
        (void)sr_set_precision(c, SR_PRECISION_SPLIT_F16);
        return rc2;
    }
    return SR_OK;
}

// Each of `parts` shares on its own host thread -- or, should the system refuse another thread, right here: no exception may cross
// the C ABI with joinable threads behind it.  The first share that failed gives the status.
template <class F>
int run_shares(int parts, F share) {
    std::vector<int> rc(parts, SR_OK);
    std::vector<std::thread> th;
    for (int k = 0; k < parts; ++k) {
        auto fn = [&rc, &share, k] { rc[k] = share(k); };
        try { th.emplace_back(fn); } catch (const std::exception&) { fn(); }
    }
    for (auto& t : th) t.join();
    for (int k = 0; k < parts; ++k)
        if (rc[k] != SR_OK) return rc[k];
    return SR_OK;
}

}  // namespace

// Contexts that cooperate on one call must be distinct objects computing the same function: same graph, factor,
// arithmetic mode and parameters -- or the "bit-identical to the single-device call" guarantee silently breaks
// (a seam between shares), and one context driven from two threads at once races on its workspace.
int sr_check_context_set(sr_ctx* const* ctxs, int n_ctx) {
    if (!ctxs || n_ctx <= 0) return SR_E_INVALID;
    for (int k = 0; k < n_ctx; ++k) {
        if (!ctxs[k] || ctxs[k]->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
        if (ctxs[k]->factor != ctxs[0]->factor || ctxs[k]->precision != ctxs[0]->precision ||
            ctxs[k]->params_hash != ctxs[0]->params_hash) return SR_E_INVALID;
        for (int j = 0; j < k; ++j) if (ctxs[j] == ctxs[k]) return SR_E_INVALID;
    }
    return SR_OK;
}

extern "C" {

int sr_upscale_f32_dev(sr_ctx* c, const float* d_in, int n, int h, int w, float* d_out, void* stream) {
    sr_capture_scope capture(c, stream);
    sr_plan_clear(c);
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    return sr_run_stack_auto(c, d_in, false, 3, n, h, w, 0, 0, d_out, false, (hipStream_t)stream);
}

int sr_upscale_rgba8_dev(sr_ctx* c, const uint8_t* d_in, int in_channels, int n, int h, int w,
                         uint8_t* d_out, void* stream) {
    sr_capture_scope capture(c, stream);
    sr_plan_clear(c);
    if (!sr_dword_aligned(d_out)) return SR_E_INVALID;
    return sr_run_stack_auto(c, d_in, true, in_channels, n, h, w, 0, 0, d_out, true, (hipStream_t)stream);
}

int sr_upscale_band_f32_dev(sr_ctx* c, const float* d_in, int h_ext, int w, int halo_top, int halo_bot,
                            float* d_out, void* stream) {
    sr_capture_scope capture(c, stream);
    sr_plan_clear(c);
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    return sr_run_stack_auto(c, d_in, false, 3, 1, h_ext, w, halo_top, halo_bot, d_out, false, (hipStream_t)stream);
}

int sr_upscale_band_rgba8_dev(sr_ctx* c, const uint8_t* d_in, int in_channels, int h_ext, int w,
                              int halo_top, int halo_bot, uint8_t* d_out, void* stream) {
    sr_capture_scope capture(c, stream);
    sr_plan_clear(c);
    if (!sr_dword_aligned(d_out)) return SR_E_INVALID;
    return sr_run_stack_auto(c, d_in, true, in_channels, 1, h_ext, w, halo_top, halo_bot, d_out, true,
                             (hipStream_t)stream);
}

// ... and what a DEVICE-pointer call of that shape would create on its first use: if it runs as two bands (sr_plan_fork), the second
// stream, the fork / join events and both workspaces at the bands' geometry -- allocations and a stream creation that would
// otherwise happen, synchronously, inside the first "asynchronous" sr_upscale_*_dev call after the reserve.
static int reserve_fork(sr_ctx* c, bool img_u8, int img_ch, int n, int h, int w) {
    int rows_a = 0;
    // (a shape the fork tuner will measure runs both ways: what the forked calls need is created here too)
    if (!sr_plan_fork(*c, sr_fork_tunable(*c, n, h, w, 0, 0, false) ? 1 : c->env_fork, img_u8, img_ch, n, h, w, 0, 0, &rows_a)) return SR_OK;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    SRCHK(sr_ensure_streams(c, false));
    SRCHK(sr_ensure_fork_resources(c));
    sr_fork_band fb[2];
    sr_fork_bands(h, 0, 0, rows_a, fb);
    StackJob a = stack_job(c, 0, nullptr, img_u8, img_ch, 1, fb[0].H, w, fb[0].top, fb[0].bot, nullptr, false, c->stream);
    StackJob b = stack_job(c, 1, nullptr, img_u8, img_ch, 1, fb[1].H, w, fb[1].top, fb[1].bot, nullptr, false, c->stream);
    a.forked = b.forked = true;
    int rc = a.prepare();
    if (rc == SR_OK) rc = b.prepare();
    if (rc == SR_E_NOMEM) return SR_OK;  // the device call will run undivided (sr_run_stack_auto)
    if (rc != SR_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SR_OK;
}

int sr_reserve_f32(sr_ctx* c, int n, int h, int w) {
    sr_plan_clear(c);
    const int rc = run_host(c, nullptr, false, 3, sr_deal{0, 1, n}, h, w, nullptr, false, 0, -1, true);
    return rc == SR_OK ? reserve_fork(c, false, 3, n, h, w) : rc;
}

int sr_reserve_rgba8(sr_ctx* c, int in_channels, int n, int h, int w) {
    sr_plan_clear(c);
    const int rc = run_host(c, nullptr, true, in_channels, sr_deal{0, 1, n}, h, w, nullptr, true, 0, -1, true);
    return rc == SR_OK ? reserve_fork(c, true, in_channels, n, h, w) : rc;
}

int sr_upscale_f32(sr_ctx* c, const float* in, int n, int h, int w, float* out) {
    sr_plan_clear(c);
    return run_host(c, in, false, 3, sr_deal{0, 1, n}, h, w, out, false);
}

int sr_upscale_rgba8(sr_ctx* c, const uint8_t* in, int in_channels, int n, int h, int w, uint8_t* out) {
    sr_plan_clear(c);
    return run_host(c, in, true, in_channels, sr_deal{0, 1, n}, h, w, out, true);
}

// One image, several GPUs, one process: device k produces its share of the rows from the caller's image directly
// (the 7 halo rows either side are just more rows of the same host buffer, so nothing is exchanged between
// devices); one host thread per context drives its pipeline.  Shares are multiples of 8 rows (whole tiles).
static int run_multi(sr_ctx* const* ctxs, int n_ctx, const void* in, bool img_u8, int img_ch, int h, int w, void* out, bool out_u8) {
    if (!in || !out || h <= 0 || w <= 0) return SR_E_INVALID;
    SRCHK(sr_check_context_set(ctxs, n_ctx));
    for (int k = 0; k < n_ctx; ++k) sr_plan_clear(ctxs[k]);
    const std::vector<sr_row_share> share = sr_multi_shares(n_ctx, h);
    const int parts = (int)share.size();
    if (parts == 1) return run_host(ctxs[0], in, img_u8, img_ch, sr_deal{0, 1, 1}, h, w, out, out_u8);
    return run_shares(parts, [&](int k) { return run_host(ctxs[k], in, img_u8, img_ch, sr_deal{0, 1, 1}, h, w, out, out_u8, share[k].lo, share[k].hi); });
}

int sr_upscale_f32_multi(sr_ctx* const* ctxs, int n_ctx, const float* in, int h, int w, float* out) {
    return run_multi(ctxs, n_ctx, in, false, 3, h, w, out, false);
}

int sr_upscale_rgba8_multi(sr_ctx* const* ctxs, int n_ctx, const uint8_t* in, int in_channels, int h, int w, uint8_t* out) {
    return run_multi(ctxs, n_ctx, in, true, in_channels, h, w, out, true);
}

// Many images, several GPUs, one process (throughput mode, BASELINE configs[4]): image i goes to context i mod n_ctx,
// parameters are replicated, nothing is exchanged.  One host thread per context runs that context's images through
// its own upload / compute / download pipeline (chunks of ~1M px, so several small images share a launch).
static int run_batch_multi(sr_ctx* const* ctxs, int n_ctx, const void* in, bool img_u8, int img_ch, int n, int h, int w, void* out,
                           bool out_u8) {
    if (!in || !out || n <= 0 || h <= 0 || w <= 0) return SR_E_INVALID;
    SRCHK(sr_check_context_set(ctxs, n_ctx));
    for (int k = 0; k < n_ctx; ++k) sr_plan_clear(ctxs[k]);
    const int used = std::min(n_ctx, n);
    if (used == 1) return run_host(ctxs[0], in, img_u8, img_ch, sr_deal{0, 1, n}, h, w, out, out_u8);
    return run_shares(used, [&](int k) { return run_host(ctxs[k], in, img_u8, img_ch, sr_deal{k, used, (n - k + used - 1) / used}, h, w, out, out_u8); });
}

int sr_upscale_f32_batch_multi(sr_ctx* const* ctxs, int n_ctx, const float* in, int n, int h, int w, float* out) {
    return run_batch_multi(ctxs, n_ctx, in, false, 3, n, h, w, out, false);
}

int sr_upscale_rgba8_batch_multi(sr_ctx* const* ctxs, int n_ctx, const uint8_t* in, int in_channels, int n, int h, int w,
                                 uint8_t* out) {
    return run_batch_multi(ctxs, n_ctx, in, true, in_channels, n, h, w, out, true);
}

int sr_read_feature(sr_ctx* c, int which, float* out_host, size_t cap_floats) {
    if (!c || which < 0 || which > 3 || !out_host) return SR_E_INVALID;
    const size_t nf = (size_t)c->last_h * c->last_w * 32;
    if (nf == 0 || cap_floats < nf || !c->ws[0].d_feat[which]) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const size_t pitch = (size_t)c->ws[0].pitch;
    if (c->precision == SR_PRECISION_SPLIT_F16) {
        // row-planar map: row y = 8 runs of `pitch` 16-byte groups (4 x 8 hi halves, then their lo halves); whole padded rows come over
        std::vector<_Float16> rows((size_t)c->last_h * pitch * 64);
        HIPCHK(c, hipMemcpy(rows.data(), c->ws[0].d_feat[which] + (size_t)kFeatPad * pitch * 32, rows.size() * sizeof(_Float16), hipMemcpyDeviceToHost));
        for (int y = 0; y < c->last_h; ++y)
            for (int x = 0; x < c->last_w; ++x)
                for (int k = 0; k < 32; ++k) {
                    const _Float16* row = rows.data() + (size_t)y * pitch * 64;
                    const size_t cell = ((size_t)(k >> 3) * pitch + kFeatPad + x) * 8 + (k & 7);
                    out_host[((size_t)y * c->last_w + x) * 32 + k] = (float)row[cell] + (float)row[cell + 4 * pitch * 8] * (1.0f / 2048.0f);
                }
        return SR_OK;
    }
    const float* src = c->ws[0].d_feat[which] + ((size_t)kFeatPad * pitch + kFeatPad) * 32;
    HIPCHK(c, hipMemcpy2D(out_host, (size_t)c->last_w * 128, src, pitch * 128, (size_t)c->last_w * 128,
                          c->last_h, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_check_domain(sr_ctx* c) {
    if (!c) return SR_E_INVALID;
    const bool fault = c->dev_fault || (c->h_domain && *(volatile int*)c->h_domain);
    c->dev_fault = false;
    if (c->h_domain) *(volatile int*)c->h_domain = 0;
    return fault ? SR_E_DOMAIN : SR_OK;
}

int sr_last_timing(sr_ctx* c, double* total_ms, double stage_ms[5], double* h2d_ms, double* d2h_ms) {
    if (!c) return SR_E_INVALID;
    if (c->band_pending) {  // a sharded call (sr_comm.cpp): its whole step on this context -- band copy, halo exchange, conv stack -- waited for here
        float ms = 0;
        HIPCHK(c, hipEventSynchronize(c->ev_band[1]));
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_band[0], c->ev_band[1]));
        c->total_ms = ms;
        for (auto& v : c->stage_ms) v = 0;
        c->h2d_ms = c->d2h_ms = 0;
        c->band_pending = false;
    }
    if (total_ms) *total_ms = c->total_ms;
    if (stage_ms) for (int i = 0; i < 5; ++i) stage_ms[i] = c->stage_ms[i];
    if (h2d_ms) *h2d_ms = c->h2d_ms;
    if (d2h_ms) *d2h_ms = c->d2h_ms;
    return SR_OK;
}

}  // extern "C"
