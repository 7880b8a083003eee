// sr_metrics.cpp -- host side of the Y-channel PSNR / SSIM scores (include/srhip.h, "Metrics"): the window's weights, the partials buffer,
// the two sr_image_metrics_* entry points.  The validation calls that return scores are in sr_valid.cpp; the kernels in sr_metrics.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "sr_internal.h"

namespace {

// the 11-tap Gaussian window, sigma 1.5: g_i = exp(-(i - 5)^2 / 4.5) / sum, in f64 -- computed once, so that every context and device
// filters with the same table
const double* weights() {
    static const struct Table {
        double g[11];
        Table() {
            double sum = 0.0;
            for (int i = 0; i < 11; ++i) sum += g[i] = std::exp(-(double)((i - 5) * (i - 5)) / 4.5);
            for (int i = 0; i < 11; ++i) g[i] /= sum;
        }
    } t;
    return t.g;
}

int check_image_args(const sr_ctx* c, const void* a, int a_ch, const void* b, int b_ch, int h, int w, int shave, int* s_out) {
    if (!c || !a || !b) return SR_E_INVALID;
    if (!sr_hr_channels_ok(true, a_ch) || !sr_hr_channels_ok(true, b_ch) || h < 1 || w < 1) return SR_E_INVALID;
    return sr_metrics_shave(c, shave, s_out);
}

}  // namespace

int sr_metrics_shave(const sr_ctx* c, int shave, int* out) {
    if (shave < -1) return SR_E_INVALID;
    *out = shave < 0 ? c->factor : shave;
    return SR_OK;
}

void sr_metrics_release(sr_ctx* c) {
    sr_free_buf(c->d_mpart);
    sr_free_buf(c->d_mimg);
}

void* sr_metrics_slot(const sr_ctx* c, int H, int W, int shave) {
    return (char*)c->d_mpart.p + 16 * (size_t)sr_metrics_blocks(H, W, shave);
}

void sr_metrics_fill(sr_metrics* m, const void* result16, int H, int W, int shave) {
    const long RH = (long)H - 2L * shave, RW = (long)W - 2L * shave;
    m->y_count = RH > 0 && RW > 0 ? (uint64_t)RH * (uint64_t)RW : 0;
    m->ssim_count = RH >= 11 && RW >= 11 ? (uint64_t)(RH - 10) * (uint64_t)(RW - 10) : 0;
    memcpy(&m->y_sq_err, result16, 8);
    memcpy(&m->ssim_sum, (const char*)result16 + 8, 8);
}

int sr_metrics_reserve(sr_ctx* c, int H, int W, int shave) {
    const long blocks = sr_metrics_blocks(H, W, shave);
    if (blocks > INT32_MAX) return SR_E_INVALID;
    return sr_ensure_bufs(c, {{&c->d_mpart, 16 * (size_t)blocks + 16}});
}

int sr_metrics_queue(sr_ctx* c, const void* d_a, bool a_u8, int a_ch, long pitch_a, const uint8_t* d_b, int b_ch, long pitch_b, int H, int W,
                     const sr_metrics_request& rq, hipStream_t s) {
    const int rc = sr_metrics_reserve(c, H, W, rq.shave);
    if (rc != SR_OK) return rc;
    void* d_result16 = rq.d_result16 ? rq.d_result16 : sr_metrics_slot(c, H, W, rq.shave);
    HIPCHK(c, sr_launch_metrics(d_a, a_u8, a_ch, pitch_a, d_b, b_ch, pitch_b, H, W, rq.shave, weights(), c->d_mpart.p, d_result16, s));
    return SR_OK;
}

extern "C" {

int sr_image_metrics_rgba8_dev(sr_ctx* c, const uint8_t* d_a, int a_channels, const uint8_t* d_b, int b_channels, int h, int w, int shave,
                               void* d_result16, void* stream) {
    sr_plan_clear(c);
    sr_metrics_request rq;
    const int rc = check_image_args(c, d_a, a_channels, d_b, b_channels, h, w, shave, &rq.shave);
    if (rc != SR_OK) return rc;
    if (!d_result16 || !sr_dword_aligned(d_result16)) return SR_E_INVALID;
    rq.d_result16 = d_result16;
    sr_capture_scope capture(c, stream);
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    return sr_metrics_queue(c, d_a, true, a_channels, w, d_b, b_channels, w, h, w, rq, (hipStream_t)stream);
}

int sr_image_metrics_rgba8(sr_ctx* c, const uint8_t* a, int a_channels, const uint8_t* b, int b_channels, int h, int w, int shave,
                           sr_metrics* metrics) {
    sr_plan_clear(c);
    sr_metrics_request rq;
    int rc = check_image_args(c, a, a_channels, b, b_channels, h, w, shave, &rq.shave);
    if (rc != SR_OK) return rc;
    if (!metrics) return SR_E_INVALID;
    const size_t a_bytes = (size_t)h * w * a_channels, b_bytes = (size_t)h * w * b_channels;
    unsigned char result[16] = {0};
    const auto d_b = [&] { return (uint8_t*)c->d_mimg.p + sr_round256(a_bytes); };
    rc = sr_host_call(  // (no network runs: no domain handling)
        c, false, SR_TIMES_NONE, {{&c->d_mimg, sr_round256(a_bytes) + b_bytes}},
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(c->d_mimg.p, a, a_bytes, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(d_b(), b, b_bytes, hipMemcpyHostToDevice, s));
            return SR_OK;
        },
        [&](hipStream_t s) { return sr_metrics_queue(c, c->d_mimg.p, true, a_channels, w, d_b(), b_channels, w, h, w, rq, s); },
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(result, sr_metrics_slot(c, h, w, rq.shave), 16, hipMemcpyDeviceToHost, s));
            return SR_OK;
        });
    if (rc != SR_OK) return rc;
    sr_metrics_fill(metrics, result, h, w, rq.shave);
    return SR_OK;
}

}  // extern "C"
