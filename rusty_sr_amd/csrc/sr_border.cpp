// sr_border.cpp -- the border modes (include/srhip.h "Borders"): the image is continued by `pad` pixels on every side under wrap,
// replicate or mirror, the padded image is upscaled by the path of the plain or the ensemble call, and the centre f h x f w is cut out
// of the result.  The reference has no counterpart: every layer of its network zero-pads.  Kernels: sr_border.hip; the network:
// sr_run_stack_auto (the plain device call's path) or sr_ensemble_queue (the ensemble's), untouched, on the caller's stream.  The whole
// padded image is run and cropped both ways.  With bleed >= 0 the transparency path's two launches (sr_alpha.hip) run on
// the UNPADDED image, before the pad and behind the crop.
#include <hip/hip_runtime.h>

#include "sr_internal.h"

namespace {

constexpr size_t kPx8 = 4, kPxF = 3 * sizeof(float);

bool mode_ok(int mode) { return mode >= SR_BORDER_WRAP && mode <= SR_BORDER_MIRROR; }

// the sizes the primitives take: the index rule forms 2 size, the padded sizes are ints
bool prim_shape_ok(int n, int h, int w) {
    const int cap = INT32_MAX / 2 - 2 * SR_BORDER_PAD_MAX;
    return n >= 1 && h >= 1 && w >= 1 && h <= cap && w <= cap;
}

// everything the composed calls refuse for their arguments alone; bleed: -1 opaque output, 0.. the transparency path's radius (RGBA8 only)
int check_upscale_args(const sr_ctx* c, const void* in, const void* out, int n, int h, int w, int mode, int pad, unsigned members, int bleed) {
    if (!c || !in || !out) return SR_E_INVALID;
    if (c->graph != SR_GRAPH_SR_NET && c->graph != SR_GRAPH_BILINEAR) return SR_E_INVALID;
    if (n < 1 || h < 1 || w < 1 || h > INT32_MAX / c->factor || w > INT32_MAX / c->factor) return SR_E_INVALID;
    if (!mode_ok(mode) || pad < SR_HALO || pad > SR_BORDER_PAD_MAX) return SR_E_INVALID;
    if (members == 0 || members > 255u) return SR_E_INVALID;
    if (members != 1u && c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    if (bleed < -1 || bleed > SR_ALPHA_BLEED_MAX) return SR_E_INVALID;
    return SR_OK;
}

// [bleed ->] pad -> network -> crop [-> merge] on device buffers, queued on s; the arguments are checked and the context's device is current
int queue_border(sr_ctx* c, const void* d_in, bool u8, int n, int h, int w, void* d_out, int mode, int pad, unsigned members, int bleed,
                 hipStream_t s) {
    const size_t f = (size_t)c->factor, px = u8 ? kPx8 : kPxF;
    // a padded shape the network's size rule or either launch cannot take is refused before anything runs
    if (h > INT32_MAX / c->factor - 2 * pad || w > INT32_MAX / c->factor - 2 * pad) return SR_E_NOMEM;
    const int H = h + 2 * pad, W = w + 2 * pad;
    const int OH = (int)f * H, OW = (int)f * W, oh = (int)f * h, ow = (int)f * w;
    const size_t in_img = (size_t)h * w * px, pad_img = (size_t)H * W * px, big_img = (size_t)OH * OW * px;
    if (pad_img / px / (size_t)W != (size_t)H || big_img / px / (size_t)OW != (size_t)OH) return SR_E_NOMEM;
    if (pad_img > SIZE_MAX / (size_t)n || big_img > SIZE_MAX / (size_t)n) return SR_E_NOMEM;
    if (sr_border_pad_blocks(!u8, n, h, w, pad) > (size_t)INT32_MAX || sr_border_crop_blocks(!u8, n, oh, ow) > (size_t)INT32_MAX) return SR_E_NOMEM;
    const bool alpha = bleed >= 0;
    if (alpha && (sr_alpha_bleed_blocks(n, h, w) > (size_t)INT32_MAX || sr_alpha_merge_blocks(c->factor, n, h, w) > (size_t)INT32_MAX))
        return SR_E_NOMEM;
    const size_t bled_bytes = bleed > 0 ? (size_t)n * in_img : 0;
    if ((size_t)n * pad_img > c->d_bpad.cap || (size_t)n * big_img > c->d_bout.cap || bled_bytes > c->d_ableed.cap) {
        // more than the device has at all: refused by arithmetic, nothing attempted
        if (!c->total_mem) HIPCHK(c, hipDeviceTotalMem(&c->total_mem, c->device));
        const size_t total = c->total_mem;
        if ((size_t)n * big_img > total || (size_t)n * pad_img > total - (size_t)n * big_img) return SR_E_NOMEM;
        if (bled_bytes > total - (size_t)n * big_img - (size_t)n * pad_img) return SR_E_NOMEM;
    }
    SRCHK(sr_ensure_bufs(c, {{&c->d_bpad, (size_t)n * pad_img}, {&c->d_bout, (size_t)n * big_img}, {&c->d_ableed, bled_bytes}}));
    const void* img = d_in;
    if (bleed > 0) {
        HIPCHK(c, sr_launch_alpha_bleed((const uint8_t*)d_in, (uint8_t*)c->d_ableed.p, n, h, w, bleed, s));
        img = c->d_ableed.p;
    }
    HIPCHK(c, sr_launch_border_pad(img, !u8, n, h, w, mode, pad, c->d_bpad.p, s));
    if (members == 1u) {
        SRCHK(sr_run_stack_auto(c, c->d_bpad.p, u8, u8 ? 4 : 3, n, H, W, 0, 0, c->d_bout.p, u8, s));
    } else {
        for (int i = 0; i < n; ++i)
            SRCHK(sr_ensemble_queue(c, (const char*)c->d_bpad.p + i * pad_img, u8, u8 ? 4 : 3, H, W, (char*)c->d_bout.p + i * big_img, u8, members, s));
    }
    HIPCHK(c, sr_launch_border_crop(c->d_bout.p, !u8, n, OH, OW, (int)f * pad, (int)f * pad, oh, ow, d_out, s));
    if (alpha) HIPCHK(c, sr_launch_alpha_merge(c->factor, (const uint8_t*)d_in, (uint8_t*)d_out, n, h, w, s));
    return SR_OK;
}

int border_dev(sr_ctx* c, const void* d_in, bool u8, int n, int h, int w, void* d_out, int mode, int pad, unsigned members, int bleed,
               void* stream) {
    sr_plan_clear(c);
    SRCHK(check_upscale_args(c, d_in, d_out, n, h, w, mode, pad, members, bleed));
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    return queue_border(c, d_in, u8, n, h, w, d_out, mode, pad, members, bleed, (hipStream_t)stream);
}

// The host-pointer calls: one upload, the device call, one download (sr_host_call).  sr_last_timing: total = every launch of the call,
// h2d / d2h the two copies.
int border_host(sr_ctx* c, const void* in, bool u8, int n, int h, int w, void* out, int mode, int pad, unsigned members, int bleed) {
    sr_plan_clear(c);
    SRCHK(check_upscale_args(c, in, out, n, h, w, mode, pad, members, bleed));
    const size_t f = (size_t)c->factor, px = u8 ? kPx8 : kPxF;
    const size_t in_bytes = (size_t)n * h * w * px, out_bytes = (size_t)n * f * h * f * w * px;
    return sr_host_call(
        c, true, SR_TIMES_PARTS, {{&c->d_in[0], in_bytes}, {&c->d_out[0], out_bytes}},
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(c->d_in[0].p, in, in_bytes, hipMemcpyHostToDevice, s));
            return SR_OK;
        },
        [&](hipStream_t s) { return queue_border(c, c->d_in[0].p, u8, n, h, w, c->d_out[0].p, mode, pad, members, bleed, s); },
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(out, c->d_out[0].p, out_bytes, hipMemcpyDeviceToHost, s));
            return SR_OK;
        });
}

int pad_dev(sr_ctx* c, const void* d_in, bool f32, int n, int h, int w, int mode, int pad, void* d_out, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_in || !d_out || !prim_shape_ok(n, h, w)) return SR_E_INVALID;
    if (!mode_ok(mode) || pad < 0 || pad > SR_BORDER_PAD_MAX) return SR_E_INVALID;
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out) || d_in == d_out) return SR_E_INVALID;
    if (sr_border_pad_blocks(f32, n, h, w, pad) > (size_t)INT32_MAX) return SR_E_NOMEM;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sr_launch_border_pad(d_in, f32, n, h, w, mode, pad, d_out, (hipStream_t)stream));
    return SR_OK;
}

int crop_dev(sr_ctx* c, const void* d_in, bool f32, int n, int H, int W, int y0, int x0, int ch, int cw, void* d_out, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_in || !d_out || n < 1 || H < 1 || W < 1 || ch < 1 || cw < 1) return SR_E_INVALID;
    if (y0 < 0 || x0 < 0 || ch > H - y0 || cw > W - x0) return SR_E_INVALID;  // the window lies inside its image
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out) || d_in == d_out) return SR_E_INVALID;
    if (sr_border_crop_blocks(f32, n, ch, cw) > (size_t)INT32_MAX) return SR_E_NOMEM;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sr_launch_border_crop(d_in, f32, n, H, W, y0, x0, ch, cw, d_out, (hipStream_t)stream));
    return SR_OK;
}

}  // namespace

void sr_border_release(sr_ctx* c) {
    sr_free_buf(c->d_bpad);
    sr_free_buf(c->d_bout);
}

extern "C" {

int sr_pad_rgba8_dev(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, int mode, int pad, uint8_t* d_out, void* stream) {
    return pad_dev(c, d_in, false, n, h, w, mode, pad, d_out, stream);
}

int sr_pad_f32_dev(sr_ctx* c, const float* d_in, int n, int h, int w, int mode, int pad, float* d_out, void* stream) {
    return pad_dev(c, d_in, true, n, h, w, mode, pad, d_out, stream);
}

int sr_crop_rgba8_dev(sr_ctx* c, const uint8_t* d_in, int n, int H, int W, int y0, int x0, int ch, int cw, uint8_t* d_out, void* stream) {
    return crop_dev(c, d_in, false, n, H, W, y0, x0, ch, cw, d_out, stream);
}

int sr_crop_f32_dev(sr_ctx* c, const float* d_in, int n, int H, int W, int y0, int x0, int ch, int cw, float* d_out, void* stream) {
    return crop_dev(c, d_in, true, n, H, W, y0, x0, ch, cw, d_out, stream);
}

int sr_upscale_rgba8_border_dev(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, uint8_t* d_out, int mode, int pad, unsigned members,
                                int bleed, void* stream) {
    return border_dev(c, d_in, true, n, h, w, d_out, mode, pad, members, bleed, stream);
}

int sr_upscale_f32_border_dev(sr_ctx* c, const float* d_in, int n, int h, int w, float* d_out, int mode, int pad, unsigned members,
                              void* stream) {
    return border_dev(c, d_in, false, n, h, w, d_out, mode, pad, members, -1, stream);
}

int sr_upscale_rgba8_border(sr_ctx* c, const uint8_t* in, int n, int h, int w, uint8_t* out, int mode, int pad, unsigned members, int bleed) {
    return border_host(c, in, true, n, h, w, out, mode, pad, members, bleed);
}

int sr_upscale_f32_border(sr_ctx* c, const float* in, int n, int h, int w, float* out, int mode, int pad, unsigned members) {
    return border_host(c, in, false, n, h, w, out, mode, pad, members, -1);
}

}  // extern "C"
