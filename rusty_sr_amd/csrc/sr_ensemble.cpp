// sr_ensemble.cpp -- geometric self-ensemble (include/srhip.h sr_upscale_ensemble_*): the network is run on the flips and rotations of
// the image a mask names, each output is carried back and the results are averaged.  The reference has no counterpart (main.rs:171 runs
// graph.forward once).  Kernels: sr_ensemble.hip; every pass of the network: sr_run_stack_auto, the device entry points' own path, on the
// caller's stream.
//
// One member k of the mask, in ascending order:
//   1. T_k of the caller's image -> d_ein, f32: a u8 image is converted on the way (byte / 255, alpha dropped: img_to_data), because a
//      member's pass writes f32 and the stage kernels pair f32 output with f32 input; member 0 of an f32 image reads the caller's own;
//   2. the conv stack on it -> d_eout, f32 (members with bit 2: a w x h pass) -- bit for bit the values the plain RGBA8 call quantises;
//   3. acc = acc + T_k^-1(d_eout); the last member stores (acc + ..) * (1 / count) at the caller's output instead, quantised for RGBA8.
// An f32 call accumulates in the caller's output buffer; an RGBA8 call in d_eacc.  A mask of member 0 alone is the plain call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sr_internal.h"

namespace {

// T_k: swap the axes if k & 4, then reverse the rows if k & 2, then the columns if k & 1 -- as the gather of sr_ens_map, whose flips are
// in SOURCE coordinates.  Forward (dst = T_k(src)): without the swap dst row p is src row p or its mirror (bit 1), columns alike (bit 0);
// with it, dst row p came from src COLUMN p, so bit 1 mirrors src columns and bit 0 src rows.  Backward (dst = T_k^-1(src)): the flips
// were applied to src's own rows (bit 1) and columns (bit 0) last, so they are undone there, swap or not.
sr_ens_map member_map(int k, bool inverse, int dst_h, int dst_w) {
    sr_ens_map m{};
    m.DH = dst_h; m.DW = dst_w;
    m.swap = (k >> 2) & 1;
    const int rows = (k >> 1) & 1, cols = k & 1;
    if (inverse || !m.swap) { m.flip_r = rows; m.flip_c = cols; }
    else { m.flip_r = cols; m.flip_c = rows; }
    return m;
}

int check_image_args(const sr_ctx* c, const void* in, const void* out, bool img_u8, int ch, int n, int h, int w, unsigned members) {
    if (!c || !in || !out || n < 1) return SR_E_INVALID;
    if (img_u8 && ch != 3 && ch != 4) return SR_E_INVALID;
    return sr_ensemble_check(c, members, h, w);
}

// n images, one after another, on device buffers: every mask, member 0 alone too (sr_net_queue runs that one as one batch)
int queue_batch(sr_ctx* c, const void* d_in, bool img_u8, int ch, int n, int h, int w, void* d_out, bool out_u8, unsigned members, hipStream_t s) {
    const sr_net_strides at = sr_net_image_strides(c->factor, img_u8, ch, out_u8, h, w);
    for (int i = 0; i < n; ++i)
        SRCHK(sr_ensemble_queue(c, (const char*)d_in + i * at.in_img, img_u8, ch, h, w, (char*)d_out + i * at.out_img, out_u8, members, s));
    return SR_OK;
}

// The host-pointer calls (sr_host_image_call).  sr_last_timing: total = every pass and pixel move of the call; the stage times are the last
// pass's.
int ensemble_host(sr_ctx* c, const void* in, bool img_u8, int ch, int n, int h, int w, void* out, bool out_u8, unsigned members) {
    sr_plan_clear(c);
    SRCHK(check_image_args(c, in, out, img_u8, ch, n, h, w, members));
    const sr_net_strides at = sr_net_image_strides(c->factor, img_u8, ch, out_u8, h, w);
    return sr_host_image_call(c, true, in, n * at.in_img, out, n * at.out_img, [&](const void* d_in, void* d_out, hipStream_t s) {
        return queue_batch(c, d_in, img_u8, ch, n, h, w, d_out, out_u8, members, s);
    });
}

int ensemble_dev(sr_ctx* c, const void* d_in, bool img_u8, int ch, int n, int h, int w, void* d_out, bool out_u8, unsigned members,
                 void* stream) {
    sr_plan_clear(c);
    SRCHK(check_image_args(c, d_in, d_out, img_u8, ch, n, h, w, members));
    if (!sr_dword_aligned(d_out) || (!img_u8 && !sr_dword_aligned(d_in))) return SR_E_INVALID;
    return sr_on_device(c, stream, [&] { return queue_batch(c, d_in, img_u8, ch, n, h, w, d_out, out_u8, members, (hipStream_t)stream); });
}

}  // namespace

void sr_ensemble_release(sr_ctx* c) {
    for (sr_buf* b : {&c->d_ein, &c->d_eout, &c->d_eacc}) sr_free_buf(*b);
}

int sr_ensemble_check(const sr_ctx* c, unsigned members, int h, int w) {
    if (!c || c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    if (members == 0 || members > 255u) return SR_E_INVALID;
    if (h < 1 || w < 1 || h > INT32_MAX / c->factor || w > INT32_MAX / c->factor) return SR_E_INVALID;
    return SR_OK;
}

int sr_ensemble_queue(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int h, int w, void* d_out, bool out_u8, unsigned members,
                      hipStream_t s) {
    if (members == 1u)  // member 0 alone: the plain call, its bits
        return sr_run_stack_auto(c, d_img, img_u8, img_ch, 1, h, w, 0, 0, d_out, out_u8, s);
    const int f = c->factor, OH = f * h, OW = f * w;
    const int count = __builtin_popcount(members);
    // Everything the call needs beside the plain call's workspace, before anything is launched: a grid beyond what a launch takes is
    // refused here, memory by sr_reserve_bufs.
    const size_t map_bytes = (size_t)OH * OW * 3 * sizeof(float);
    const size_t in_bytes = (img_u8 || (members & ~1u)) ? (size_t)h * w * 3 * sizeof(float) : 0;
    const size_t acc_bytes = out_u8 && count > 1 ? map_bytes : 0;
    const size_t blocks = std::max(sr_ens_blocks(OH, OW, false), sr_ens_blocks(OH, OW, true));
    if (blocks > (size_t)INT32_MAX) return SR_E_NOMEM;
    SRCHK(sr_reserve_bufs(c, {{&c->d_ein, in_bytes}, {&c->d_eout, map_bytes}, {&c->d_eacc, acc_bytes}}));
    SRCHK(sr_net_capture_ready(c, false, 3, 1, h, w, members));
    float* acc = out_u8 ? (float*)c->d_eacc.p : (float*)d_out;
    const float scale = 1.0f / (float)count;
    int done = 0;
    for (int k = 0; k < 8; ++k) {
        if (!(members >> k & 1u)) continue;
        const bool swap = (k & 4) != 0;
        const int hk = swap ? w : h, wk = swap ? h : w;
        const void* img = d_img;
        if (k != 0 || img_u8) {
            HIPCHK(c, sr_launch_ens_input(d_img, img_u8, img_ch, c->d_ein.p, member_map(k, false, hk, wk), s));
            img = c->d_ein.p;
        }
        SRCHK(sr_run_stack_auto(c, img, false, 3, 1, hk, wk, 0, 0, c->d_eout.p, false, s));
        ++done;
        HIPCHK(c, sr_launch_ens_accumulate((const float*)c->d_eout.p, acc, d_out, out_u8, done == 1, done == count, scale,
                                           member_map(k, true, OH, OW), s));
    }
    return SR_OK;
}

extern "C" {

int sr_upscale_ensemble_f32_dev(sr_ctx* c, const float* d_in, int n, int h, int w, float* d_out, unsigned members, void* stream) {
    return ensemble_dev(c, d_in, false, 3, n, h, w, d_out, false, members, stream);
}

int sr_upscale_ensemble_rgba8_dev(sr_ctx* c, const uint8_t* d_in, int in_channels, int n, int h, int w, uint8_t* d_out_rgba, unsigned members,
                                  void* stream) {
    return ensemble_dev(c, d_in, true, in_channels, n, h, w, d_out_rgba, true, members, stream);
}

int sr_upscale_ensemble_f32(sr_ctx* c, const float* in, int n, int h, int w, float* out, unsigned members) {
    return ensemble_host(c, in, false, 3, n, h, w, out, false, members);
}

int sr_upscale_ensemble_rgba8(sr_ctx* c, const uint8_t* in, int in_channels, int n, int h, int w, uint8_t* out_rgba, unsigned members) {
    return ensemble_host(c, in, true, in_channels, n, h, w, out_rgba, true, members);
}

}  // extern "C"
