// sr_degrade.cpp -- the degradation operator's host side (include/srhip.h "Degradation"): the argument checks, the f64 tables of a
// context and the two entry points that degrade one frame of one image.  The degraded training step is sr_train.cpp's
// (sr_train_step_degrade).  Kernels: sr_degrade.hip.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sr_internal.h"

namespace {

// everything sr_degrade_rgba8[_dev] refuse for their arguments alone; *job is filled where they pass
int plan_degrade(const sr_ctx* c, const uint8_t* hr, int ch, int h, int w, int factor, int y0, int x0, int frame_h, int frame_w, int member,
                 const sr_degrade* deg, const uint8_t* out, sr_degrade_one* job) {
    if (!c || !hr || !deg || !out || (ch != 3 && ch != 4) || h < 1 || w < 1) return SR_E_INVALID;
    if (factor < 2 || factor > 4 || frame_h < factor || frame_w < factor || frame_h % factor || frame_w % factor) return SR_E_INVALID;
    if (member < 0 || member > 7) return SR_E_INVALID;
    SRCHK(sr_degrade_check(*deg));
    job->d = {hr, ch, h, w, y0, x0, member};
    job->g = *deg;
    job->f = factor; job->frame_h = frame_h; job->frame_w = frame_w;
    return SR_OK;
}

int queue_degrade(sr_ctx* c, const sr_degrade_one& job, uint8_t* d_out, hipStream_t s) {
    SRCHK(sr_degrade_ensure_table(c));
    const hipError_t e = sr_launch_degrade(job, c->d_dtab, d_out, s);
    if (e == hipErrorInvalidValue) return SR_E_NOMEM;  // (a grid beyond what a launch takes: the arguments have been checked)
    HIPCHK(c, e);
    return SR_OK;
}

}  // namespace

int sr_degrade_check(const sr_degrade& g) {
    // (written so that a NaN is refused)
    if (!(g.sigma >= 0.0f && g.sigma <= (float)SR_DEGRADE_MAX_SIGMA) || !(g.noise >= 0.0f && g.noise <= (float)SR_DEGRADE_MAX_NOISE)) return SR_E_INVALID;
    if (g.quality < 0 || g.quality > 100) return SR_E_INVALID;
    return SR_OK;
}

int sr_degrade_radius(const sr_degrade& g) {
    return g.sigma > 0.0f ? (int)std::ceil(3.0 * (double)g.sigma) : 0;
}

int sr_degrade_ensure_table(sr_ctx* c) {
    if (c->d_dtab) return SR_OK;
    if (sr_capture_refuses(c, true)) return SR_E_INVALID;  // (the upload is synchronous)
    double tab[256 + 64];
    for (int b = 0; b < 256; ++b) {
        const double s = (double)b / 255.0;
        tab[b] = s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4);
    }
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) {
            const double v = 0.5 * std::cos((double)((2 * x + 1) * u) * 3.14159265358979323846 / 16.0);
            tab[256 + u * 8 + x] = u == 0 ? v / std::sqrt(2.0) : v;
        }
    double* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, sizeof tab));
    const hipError_t e = hipMemcpy(d, tab, sizeof tab, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        HIPCHK(c, e);
    }
    c->d_dtab = d;
    return SR_OK;
}

void sr_degrade_release(sr_ctx* c) {
    if (c->d_dtab) (void)hipFree(c->d_dtab);
    c->d_dtab = nullptr;
}

extern "C" {

int sr_degrade_rgba8_dev(sr_ctx* c, const uint8_t* d_hr, int in_channels, int h, int w, int factor, int y0, int x0, int frame_h, int frame_w,
                         int member, const sr_degrade* deg, uint8_t* d_lr_rgb, void* stream) {
    sr_plan_clear(c);
    sr_degrade_one job;
    SRCHK(plan_degrade(c, d_hr, in_channels, h, w, factor, y0, x0, frame_h, frame_w, member, deg, d_lr_rgb, &job));
    return sr_on_device(c, stream, [&] { return queue_degrade(c, job, d_lr_rgb, (hipStream_t)stream); });
}

int sr_degrade_rgba8(sr_ctx* c, const uint8_t* hr, int in_channels, int h, int w, int factor, int y0, int x0, int frame_h, int frame_w, int member,
                     const sr_degrade* deg, uint8_t* lr_rgb) {
    sr_plan_clear(c);
    sr_degrade_one job;
    SRCHK(plan_degrade(c, hr, in_channels, h, w, factor, y0, x0, frame_h, frame_w, member, deg, lr_rgb, &job));
    const size_t in_bytes = (size_t)h * w * in_channels, out_bytes = (size_t)(frame_h / factor) * (frame_w / factor) * 3;
    return sr_host_image_call(c, false, hr, in_bytes, lr_rgb, out_bytes, [&](const void* d_in, void* d_out, hipStream_t s) {
        job.d.px = (const uint8_t*)d_in;
        return queue_degrade(c, job, (uint8_t*)d_out, s);
    });
}

}  // extern "C"
