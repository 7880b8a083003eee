// sr_border.cpp -- the composed calls around the network: the border modes (include/srhip.h "Borders") and transparency ("Transparency").
// Border: the image is continued by `pad` pixels on every side under wrap, replicate or mirror, the padded image is upscaled by the path
// of the plain or the ensemble call (sr_net_queue), and the centre f h x f w is cut out of the result.  The reference has no counterpart:
// every layer of its network zero-pads.  Kernels: sr_border.hip.  The whole padded image is run and cropped both ways.
// Transparency (bleed >= 0): the colours of the image are bled under its transparent pixels before the pad, and the alpha of the
// ORIGINAL image is merged into the result behind the crop -- the two launches of sr_alpha.hip, on the UNPADDED image.  One composer runs
// both; sr_upscale_rgba8_alpha[_dev] are it without a border: no pad, no crop, the network writes the caller's output.
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

// What a composed call is asked for.  border: false for the transparency calls, whose mode and pad are 0 and whose bleed is >= 0;
// bleed: -1 opaque output, 0.. the transparency path's radius (RGBA8 only).
struct Composed {
    bool border;
    int mode, pad;
    unsigned members;
    int bleed;
};

// everything the composed calls refuse for their arguments alone
int check_upscale_args(const sr_ctx* c, const void* in, const void* out, int n, int h, int w, const Composed& a) {
    SRCHK(sr_net_check(c, in, out, n, h, w, a.members));
    if (a.border && (!mode_ok(a.mode) || a.pad < SR_HALO || a.pad > SR_BORDER_PAD_MAX)) return SR_E_INVALID;
    if (a.bleed < (a.border ? -1 : 0) || a.bleed > SR_ALPHA_BLEED_MAX) return SR_E_INVALID;
    return SR_OK;
}

// either launch queued on s, with its "op" line in the plan record: the grid sr_launch_border_* itself takes
int queue_pad(sr_ctx* c, const void* d_in, bool f32, int n, int h, int w, int mode, int pad, void* d_out, hipStream_t s) {
    unsigned bx = 0, by = 0;
    (void)sr_border_pad_blocks(f32, n, h, w, pad, &bx, &by);
    HIPCHK(c, sr_launch_border_pad(d_in, f32, n, h, w, mode, pad, d_out, s));
    sr_plan_note_op(c, "pad", f32, n, bx, by);
    return SR_OK;
}

int queue_crop(sr_ctx* c, const void* d_in, bool f32, int n, int H, int W, int y0, int x0, int ch, int cw, void* d_out, hipStream_t s) {
    unsigned bx = 0, by = 0;
    (void)sr_border_crop_blocks(f32, n, ch, cw, &bx, &by);
    HIPCHK(c, sr_launch_border_crop(d_in, f32, n, H, W, y0, x0, ch, cw, d_out, s));
    sr_plan_note_op(c, "crop", f32, n, bx, by);
    return SR_OK;
}

// [bleed ->] [pad ->] network [-> crop] [-> merge] on device buffers, queued on s; the arguments are checked and the context's device is
// current.  Without a border the network reads the (bled) image and writes d_out; d_bpad / d_bout are neither sized nor touched.
int queue_composed(sr_ctx* c, const void* d_in, bool u8, int n, int h, int w, void* d_out, const Composed& a, hipStream_t s) {
    const bool border = a.border, alpha = a.bleed >= 0;
    const int pad = a.pad, bleed = a.bleed;
    const size_t f = (size_t)c->factor, px = u8 ? kPx8 : kPxF;
    const int H = h + 2 * pad, W = w + 2 * pad, oh = (int)f * h, ow = (int)f * w;  // (pad <= 32, h and w <= INT32_MAX / f: they fit)
    size_t pad_bytes = 0, big_bytes = 0;
    if (border) {  // a padded shape the network's size rule or either launch cannot take is refused before anything runs
        if (h > INT32_MAX / c->factor - 2 * pad || w > INT32_MAX / c->factor - 2 * pad) return SR_E_NOMEM;
        const size_t OH = f * H, OW = f * W, pad_img = (size_t)H * W * px, big_img = OH * OW * px;
        if (pad_img / px / (size_t)W != (size_t)H || big_img / px / OW != OH) return SR_E_NOMEM;
        if (pad_img > SIZE_MAX / (size_t)n || big_img > SIZE_MAX / (size_t)n) return SR_E_NOMEM;
        if (sr_border_pad_blocks(!u8, n, h, w, pad) > (size_t)INT32_MAX || sr_border_crop_blocks(!u8, n, oh, ow) > (size_t)INT32_MAX) return SR_E_NOMEM;
        pad_bytes = (size_t)n * pad_img;
        big_bytes = (size_t)n * big_img;
    }
    if (alpha && (sr_alpha_bleed_blocks(n, h, w) > (size_t)INT32_MAX || sr_alpha_merge_blocks(c->factor, n, h, w) > (size_t)INT32_MAX))
        return SR_E_NOMEM;
    const size_t bled_bytes = bleed > 0 ? (size_t)n * h * w * kPx8 : 0;
    SRCHK(border ? sr_reserve_bufs(c, {{&c->d_bpad, pad_bytes}, {&c->d_bout, big_bytes}, {&c->d_ableed, bled_bytes}})
                 : sr_reserve_bufs(c, {{&c->d_ableed, bled_bytes}}));
    SRCHK(sr_net_capture_ready(c, u8, u8 ? 4 : 3, n, H, W, a.members));
    const void* img = d_in;
    if (bleed > 0) {
        SRCHK(sr_alpha_queue_bleed(c, (const uint8_t*)d_in, (uint8_t*)c->d_ableed.p, n, h, w, bleed, s));
        img = c->d_ableed.p;
    }
    if (border) SRCHK(queue_pad(c, img, !u8, n, h, w, a.mode, pad, c->d_bpad.p, s));
    SRCHK(sr_net_queue(c, border ? c->d_bpad.p : img, u8, u8 ? 4 : 3, n, H, W, border ? c->d_bout.p : d_out, u8, a.members, s));
    if (border) SRCHK(queue_crop(c, c->d_bout.p, !u8, n, (int)f * H, (int)f * W, (int)f * pad, (int)f * pad, oh, ow, d_out, s));
    if (alpha) SRCHK(sr_alpha_queue_merge(c, (const uint8_t*)d_in, (uint8_t*)d_out, n, h, w, s));
    return SR_OK;
}

int composed_dev(sr_ctx* c, const void* d_in, bool u8, int n, int h, int w, void* d_out, const Composed& a, void* stream) {
    sr_plan_clear(c);
    SRCHK(check_upscale_args(c, d_in, d_out, n, h, w, a));
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    return sr_on_device(c, stream, [&] { return queue_composed(c, d_in, u8, n, h, w, d_out, a, (hipStream_t)stream); });
}

// The host-pointer calls (sr_host_image_call).  sr_last_timing: total = every launch of the call, h2d / d2h the two copies.
int composed_host(sr_ctx* c, const void* in, bool u8, int n, int h, int w, void* out, const Composed& a) {
    sr_plan_clear(c);
    SRCHK(check_upscale_args(c, in, out, n, h, w, a));
    const size_t f = (size_t)c->factor, px = u8 ? kPx8 : kPxF;
    return sr_host_image_call(c, true, in, (size_t)n * h * w * px, out, (size_t)n * f * h * f * w * px, [&](const void* d_in, void* d_out, hipStream_t s) {
        return queue_composed(c, d_in, u8, n, h, w, d_out, a, s);
    });
}

int pad_dev(sr_ctx* c, const void* d_in, bool f32, int n, int h, int w, int mode, int pad, void* d_out, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_in || !d_out || !prim_shape_ok(n, h, w)) return SR_E_INVALID;
    if (!mode_ok(mode) || pad < 0 || pad > SR_BORDER_PAD_MAX) return SR_E_INVALID;
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out) || d_in == d_out) return SR_E_INVALID;
    if (sr_border_pad_blocks(f32, n, h, w, pad) > (size_t)INT32_MAX) return SR_E_NOMEM;
    return sr_on_device(c, stream, [&] { return queue_pad(c, d_in, f32, n, h, w, mode, pad, d_out, (hipStream_t)stream); });
}

int crop_dev(sr_ctx* c, const void* d_in, bool f32, int n, int H, int W, int y0, int x0, int ch, int cw, void* d_out, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_in || !d_out || n < 1 || H < 1 || W < 1 || ch < 1 || cw < 1) return SR_E_INVALID;
    if (y0 < 0 || x0 < 0 || ch > H - y0 || cw > W - x0) return SR_E_INVALID;  // the window lies inside its image
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out) || d_in == d_out) return SR_E_INVALID;
    if (sr_border_crop_blocks(f32, n, ch, cw) > (size_t)INT32_MAX) return SR_E_NOMEM;
    return sr_on_device(c, stream, [&] { return queue_crop(c, d_in, f32, n, H, W, y0, x0, ch, cw, d_out, (hipStream_t)stream); });
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
    return composed_dev(c, d_in, true, n, h, w, d_out, {true, mode, pad, members, bleed}, stream);
}

int sr_upscale_f32_border_dev(sr_ctx* c, const float* d_in, int n, int h, int w, float* d_out, int mode, int pad, unsigned members,
                              void* stream) {
    return composed_dev(c, d_in, false, n, h, w, d_out, {true, mode, pad, members, -1}, stream);
}

int sr_upscale_rgba8_border(sr_ctx* c, const uint8_t* in, int n, int h, int w, uint8_t* out, int mode, int pad, unsigned members, int bleed) {
    return composed_host(c, in, true, n, h, w, out, {true, mode, pad, members, bleed});
}

int sr_upscale_f32_border(sr_ctx* c, const float* in, int n, int h, int w, float* out, int mode, int pad, unsigned members) {
    return composed_host(c, in, false, n, h, w, out, {true, mode, pad, members, -1});
}

int sr_upscale_rgba8_alpha_dev(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, uint8_t* d_out, int radius, unsigned members,
                               void* stream) {
    return composed_dev(c, d_in, true, n, h, w, d_out, {false, 0, 0, members, radius}, stream);
}

int sr_upscale_rgba8_alpha(sr_ctx* c, const uint8_t* in, int n, int h, int w, uint8_t* out, int radius, unsigned members) {
    return composed_host(c, in, true, n, h, w, out, {false, 0, 0, members, radius});
}

}  // extern "C"
