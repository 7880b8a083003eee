// sr_alpha.cpp -- the transparency path (include/srhip.h "Transparency"): the colours of an RGBA8 image are bled under its transparent
// pixels, the bled image is upscaled by the path of the plain or the ensemble call, and the alpha of the ORIGINAL image, interpolated, is
// written into byte 3 of the result.  The reference drops alpha (main.rs:175).  Kernels: sr_alpha.hip; the network: sr_run_stack_auto (the
// plain device call's path) or sr_ensemble_queue (the ensemble's), untouched, on the caller's stream.
#include <hip/hip_runtime.h>

#include "sr_internal.h"

namespace {

bool shape_ok(const sr_ctx* c, int n, int h, int w) {
    return n >= 1 && h >= 1 && w >= 1 && h <= INT32_MAX / c->factor && w <= INT32_MAX / c->factor;
}

// everything sr_upscale_rgba8_alpha[_dev] refuses for its arguments alone
int check_upscale_args(const sr_ctx* c, const void* in, const void* out, int n, int h, int w, int radius, unsigned members) {
    if (!c || !in || !out) return SR_E_INVALID;
    if (c->graph != SR_GRAPH_SR_NET && c->graph != SR_GRAPH_BILINEAR) return SR_E_INVALID;
    if (!shape_ok(c, n, h, w)) return SR_E_INVALID;
    if (radius < 0 || radius > SR_ALPHA_BLEED_MAX) return SR_E_INVALID;
    if (members == 0 || members > 255u) return SR_E_INVALID;
    if (members != 1u && c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    return SR_OK;
}

// bleed -> network -> merge on device buffers, queued on s; the arguments are checked and the context's device is current
int queue_alpha(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, uint8_t* d_out, int radius, unsigned members, hipStream_t s) {
    const size_t f = (size_t)c->factor;
    const size_t in_img = (size_t)h * w * 4, out_img = f * h * f * w * 4;
    // a shape either launch cannot take is refused before anything runs
    if (sr_alpha_bleed_blocks(n, h, w) > (size_t)INT32_MAX || sr_alpha_merge_blocks(c->factor, n, h, w) > (size_t)INT32_MAX) return SR_E_NOMEM;
    const uint8_t* img = d_in;
    if (radius > 0) {
        if ((size_t)n * in_img > c->d_ableed.cap) {  // more than the device has at all: refused by arithmetic, nothing attempted
            if (!c->total_mem) HIPCHK(c, hipDeviceTotalMem(&c->total_mem, c->device));
            if ((size_t)n * (in_img + out_img) > c->total_mem) return SR_E_NOMEM;
        }
        const int rc = sr_ensure_bufs(c, {{&c->d_ableed, (size_t)n * in_img}});
        if (rc != SR_OK) return rc;
        HIPCHK(c, sr_launch_alpha_bleed(d_in, (uint8_t*)c->d_ableed.p, n, h, w, radius, s));
        img = (const uint8_t*)c->d_ableed.p;
    }
    if (members == 1u) {
        const int rc = sr_run_stack_auto(c, img, true, 4, n, h, w, 0, 0, d_out, true, s);
        if (rc != SR_OK) return rc;
    } else {
        for (int i = 0; i < n; ++i) {
            const int rc = sr_ensemble_queue(c, img + i * in_img, true, 4, h, w, d_out + i * out_img, true, members, s);
            if (rc != SR_OK) return rc;
        }
    }
    HIPCHK(c, sr_launch_alpha_merge(c->factor, d_in, d_out, n, h, w, s));
    return SR_OK;
}

// The host-pointer call: one upload, the device call, one download (sr_host_call).  sr_last_timing: total = bleed, every pass of the network
// and the merge; h2d / d2h the two copies.
int alpha_host(sr_ctx* c, const uint8_t* in, int n, int h, int w, uint8_t* out, int radius, unsigned members) {
    sr_plan_clear(c);
    const int rc = check_upscale_args(c, in, out, n, h, w, radius, members);
    if (rc != SR_OK) return rc;
    const size_t f = (size_t)c->factor;
    const size_t in_bytes = (size_t)n * h * w * 4, out_bytes = (size_t)n * f * h * f * w * 4;
    return sr_host_call(
        c, true, SR_TIMES_PARTS, {{&c->d_in[0], in_bytes}, {&c->d_out[0], out_bytes}},
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(c->d_in[0].p, in, in_bytes, hipMemcpyHostToDevice, s));
            return SR_OK;
        },
        [&](hipStream_t s) { return queue_alpha(c, (const uint8_t*)c->d_in[0].p, n, h, w, (uint8_t*)c->d_out[0].p, radius, members, s); },
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(out, c->d_out[0].p, out_bytes, hipMemcpyDeviceToHost, s));
            return SR_OK;
        });
}

}  // namespace

void sr_alpha_release(sr_ctx* c) {
    sr_free_buf(c->d_ableed);
}

extern "C" {

int sr_bleed_rgba8_dev(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, int radius, uint8_t* d_out, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_in || !d_out || n < 1 || h < 1 || w < 1) return SR_E_INVALID;
    if (radius < 0 || radius > SR_ALPHA_BLEED_MAX) return SR_E_INVALID;
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out) || d_in == d_out) return SR_E_INVALID;
    if (sr_alpha_bleed_blocks(n, h, w) > (size_t)INT32_MAX) return SR_E_NOMEM;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sr_launch_alpha_bleed(d_in, d_out, n, h, w, radius, (hipStream_t)stream));
    return SR_OK;
}

int sr_merge_alpha_rgba8_dev(sr_ctx* c, const uint8_t* d_lr, int n, int h, int w, uint8_t* d_out, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_lr || !d_out) return SR_E_INVALID;
    if (c->graph != SR_GRAPH_SR_NET && c->graph != SR_GRAPH_BILINEAR) return SR_E_INVALID;
    if (!shape_ok(c, n, h, w)) return SR_E_INVALID;
    if (!sr_dword_aligned(d_lr) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    if (sr_alpha_merge_blocks(c->factor, n, h, w) > (size_t)INT32_MAX) return SR_E_NOMEM;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sr_launch_alpha_merge(c->factor, d_lr, d_out, n, h, w, (hipStream_t)stream));
    return SR_OK;
}

int sr_upscale_rgba8_alpha_dev(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, uint8_t* d_out, int radius, unsigned members,
                               void* stream) {
    sr_plan_clear(c);
    const int rc = check_upscale_args(c, d_in, d_out, n, h, w, radius, members);
    if (rc != SR_OK) return rc;
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    return queue_alpha(c, d_in, n, h, w, d_out, radius, members, (hipStream_t)stream);
}

int sr_upscale_rgba8_alpha(sr_ctx* c, const uint8_t* in, int n, int h, int w, uint8_t* out, int radius, unsigned members) {
    return alpha_host(c, in, n, h, w, out, radius, members);
}

}  // extern "C"
