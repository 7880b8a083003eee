// sr_alpha.cpp -- the transparency path's two primitives (include/srhip.h "Transparency"): the colours of an RGBA8 image are bled under its
// transparent pixels, and the alpha of the ORIGINAL image, interpolated, is written into byte 3 of an upscaled one.  The reference drops
// alpha (main.rs:175).  Kernels: sr_alpha.hip.  The composed calls, sr_upscale_rgba8_alpha[_dev]: sr_border.cpp, the composer without a border.
#include <hip/hip_runtime.h>

#include "sr_internal.h"

void sr_alpha_release(sr_ctx* c) {
    sr_free_buf(c->d_ableed);
}

int sr_alpha_queue_bleed(sr_ctx* c, const uint8_t* d_in, uint8_t* d_out, int n, int h, int w, int radius, hipStream_t s) {
    unsigned tx = 0, ty = 0;
    (void)sr_alpha_bleed_blocks(n, h, w, &tx, &ty);
    HIPCHK(c, sr_launch_alpha_bleed(d_in, d_out, n, h, w, radius, s));
    sr_plan_note_op(c, "bleed", false, n, tx, ty);
    return SR_OK;
}

int sr_alpha_queue_merge(sr_ctx* c, const uint8_t* d_lr, uint8_t* d_out, int n, int h, int w, hipStream_t s) {
    unsigned bx = 0, by = 0;
    (void)sr_alpha_merge_blocks(c->factor, n, h, w, &bx, &by);
    HIPCHK(c, sr_launch_alpha_merge(c->factor, d_lr, d_out, n, h, w, s));
    sr_plan_note_op(c, "merge", false, n, bx, by, nullptr, c->factor);
    return SR_OK;
}

extern "C" {

int sr_bleed_rgba8_dev(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, int radius, uint8_t* d_out, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_in || !d_out || n < 1 || h < 1 || w < 1) return SR_E_INVALID;
    if (radius < 0 || radius > SR_ALPHA_BLEED_MAX) return SR_E_INVALID;
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out) || d_in == d_out) return SR_E_INVALID;
    if (sr_alpha_bleed_blocks(n, h, w) > (size_t)INT32_MAX) return SR_E_NOMEM;
    return sr_on_device(c, stream, [&] { return sr_alpha_queue_bleed(c, d_in, d_out, n, h, w, radius, (hipStream_t)stream); });
}

int sr_merge_alpha_rgba8_dev(sr_ctx* c, const uint8_t* d_lr, int n, int h, int w, uint8_t* d_out, void* stream) {
    sr_plan_clear(c);
    SRCHK(sr_net_check(c, d_lr, d_out, n, h, w, 1u));  // (the shapes and graphs of the composed call, no ensemble)
    if (!sr_dword_aligned(d_lr) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    if (sr_alpha_merge_blocks(c->factor, n, h, w) > (size_t)INT32_MAX) return SR_E_NOMEM;
    return sr_on_device(c, stream, [&] { return sr_alpha_queue_merge(c, d_lr, d_out, n, h, w, (hipStream_t)stream); });
}

}  // extern "C"
