// sr_optim.cpp -- host side of the optimiser's additions (include/srhip.h "Optimiser": sr_grad_norm_dev, sr_adam_step_clipped_dev,
// sr_lr_at).  Kernels: sr_optim.hip.  The session's use of them is in sr_train.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sr_internal.h"

void sr_optim_release(sr_ctx* c) { sr_free_buf(c->d_opart); }

bool sr_clip_ok(float clip) { return clip == 0.0f || (std::isfinite(clip) && clip > 0.0f); }
bool sr_ema_decay_ok(float d) { return d == 0.0f || (d > 0.0f && d < 1.0f); }
bool sr_lr_ok(float lr) { return std::isfinite(lr) && lr >= 0.0f; }

// The norm of n floats queued on s (the arguments are the caller's to have checked; the context's device is current).  The partials are
// the context's one buffer, whatever s is: calls on one context must be ordered by the caller, across streams too (srhip.h).
int sr_grad_norm_queue(sr_ctx* c, const float* d_grad, size_t n, float clip, sr_grad_norm* d_out, sr_grad_norm* d_mirror, hipStream_t s) {
    const int rc = sr_ensure_buf(c, c->d_opart, sr_round256(sr_optim_parts(n) * sizeof(double)));
    if (rc != SR_OK) return rc;
    HIPCHK(c, sr_launch_grad_norm(d_grad, n, clip, (double*)c->d_opart.p, d_out, d_mirror, s));
    return SR_OK;
}

extern "C" {

int sr_grad_norm_dev(sr_ctx* c, const float* d_grad, size_t n, float clip, sr_grad_norm* d_out, void* stream) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    sr_plan_clear(c);
    if (!c || !d_grad || !d_out || n == 0 || sr_optim_parts(n) > (size_t)INT32_MAX || !sr_clip_ok(clip)) return SR_E_INVALID;
    if (!sr_dword_aligned(d_grad) || ((uintptr_t)d_out & 7u)) return SR_E_INVALID;
    sr_capture_scope capture(c, stream);
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    return sr_grad_norm_queue(c, d_grad, n, clip, d_out, nullptr, (hipStream_t)stream);
}

int sr_adam_step_clipped_dev(sr_ctx* c, float* d_params, float* d_m, float* d_v, const float* d_grad, size_t n, int step, float lr, float beta1,
                             float beta2, float eps, const sr_grad_norm* d_norm, float* d_ema, float ema_decay, unsigned long long* d_skipped,
                             void* stream) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    sr_plan_clear(c);
    if (!c || !d_params || !d_m || !d_v || !d_grad || n == 0 || step < 1) return SR_E_INVALID;
    if (!sr_dword_aligned(d_params) || !sr_dword_aligned(d_m) || !sr_dword_aligned(d_v) || !sr_dword_aligned(d_grad) || !sr_dword_aligned(d_ema))
        return SR_E_INVALID;
    if (((uintptr_t)d_norm & 7u) || ((uintptr_t)d_skipped & 7u)) return SR_E_INVALID;
    if (!sr_lr_ok(lr) || !sr_ema_decay_ok(ema_decay) || (d_ema != nullptr) != (ema_decay != 0.0f)) return SR_E_INVALID;
    // bias corrections 1 - beta^t, in f32, as sr_adam_step_dev forms them
    const float bc1 = 1.0f - std::pow(beta1, (float)step), bc2 = 1.0f - std::pow(beta2, (float)step);
    const float omd = 1.0f - ema_decay;
    sr_capture_scope capture(c, stream);
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sr_launch_adam_clipped(d_params, d_m, d_v, d_grad, d_ema, n, lr, beta1, beta2, eps, bc1, bc2, ema_decay, omd, d_norm, d_skipped,
                                     (hipStream_t)stream));
    return SR_OK;
}

int sr_lr_at(const sr_lr_schedule* sch, long long step, float* lr) {
    if (!sch || !lr || step < 1) return SR_E_INVALID;
    if (!sr_lr_ok(sch->base) || sch->warmup < 0) return SR_E_INVALID;
    const double base = (double)sch->base, t = (double)step;
    double val;
    switch (sch->kind) {
    case SR_LR_CONSTANT:
        val = base;
        break;
    case SR_LR_STEP:
        if (sch->every < 1 || !std::isfinite(sch->gamma) || !(sch->gamma > 0.0) || sch->gamma > 1.0) return SR_E_INVALID;
        val = base * std::pow(sch->gamma, (double)((step - 1) / sch->every));
        break;
    case SR_LR_COSINE: {
        if (sch->total < 1 || !sr_lr_ok(sch->min_lr) || sch->min_lr > sch->base) return SR_E_INVALID;
        const double T = (double)sch->total, mn = (double)sch->min_lr;
        val = mn + (base - mn) * (0.5 * (1.0 + std::cos(3.14159265358979323846 * std::min(t - 1.0, T) / T)));
        break;
    }
    default:
        return SR_E_INVALID;
    }
    const double warm = sch->warmup ? std::min(1.0, t / (double)sch->warmup) : 1.0;
    *lr = (float)(warm * val);
    return SR_OK;
}

}  // extern "C"
