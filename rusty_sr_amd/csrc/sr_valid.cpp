// sr_valid.cpp -- the validation pass of the reference's `train` (main.rs:220-247): the forward half of
// sr_net(f, Some((0.0, linear_loss))) (network.rs:88-102) on one HR image -- pool, network, loss -- returning the loss as a sum
// and an element count (include/srhip.h sr_validation_error_*).  Kernels: sr_valid.hip; the network: sr_run_stack_auto.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "sr_internal.h"

namespace {

// 512 floats: img_to_data (main.rs:170: byte / 255, an f32 division), then SrgbToLinear of those as the correctly rounded f32 of the
// f64 formula -- computed here, so that every device holds the same table and the tests can restate it bit for bit
int ensure_table(sr_ctx* c) {
    if (c->d_vtab) return SR_OK;
    if (sr_capture_refuses(c, true)) return SR_E_INVALID;  // (the upload is synchronous)
    float tab[512];
    for (int b = 0; b < 256; ++b) {
        const float s = (float)b / 255.0f;
        tab[b] = s;
        tab[256 + b] = (float)(s <= 0.04045f ? (double)s / 12.92 : std::pow(((double)s + 0.055) / 1.055, 2.4));
    }
    float* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, sizeof tab));
    const hipError_t e = hipMemcpy(d, tab, sizeof tab, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        HIPCHK(c, e);
    }
    c->d_vtab = d;
    return SR_OK;
}

// Arguments of every entry point, checked before the GPU is touched.
int check_args(sr_ctx* c, const void* hr, bool hr_u8, int ch, int h, int w) {
    if (!c || !hr) return SR_E_INVALID;
    return sr_check_hr_args(c, hr_u8, ch, 1, h, w);
}

int check_pair_args(sr_ctx* c, const void* lr, bool u8, int lr_ch, const void* hr, int hr_ch, int lh, int lw) {
    if (!c || !lr || !hr) return SR_E_INVALID;
    return sr_check_pair_args(c, u8, lr_ch, hr_ch, 1, lh, lw);
}

// Pool (or, with lr, a paired call's LR image in its place), network, loss on device buffers, queued on s; the sum lands at d_result
// (nullptr: the slot behind the partials, for the host-pointer calls).  members: 0 = the network's output as it is, else the mask of a
// self-ensemble (sr_ensemble.cpp) whose output takes its place.  metrics (u8 HR images only): also score the quantised output against the
// HR crop (sr_metrics.cpp), one more pass behind the loss; without it the call's launches are exactly the loss's.  The context's device
// is current.
int run_validation(sr_ctx* c, const void* d_hr, bool hr_u8, int ch, int h, int w, bool linear, void* d_result, hipStream_t s,
                   const sr_lr_input* lr, unsigned members = 0, const sr_metrics_request* metrics = nullptr) {
    const int f = c->factor, OH = h / f, OW = w / f, HC = f * OH, WC = f * OW;
    const int grid = sr_valid_loss_grid(HC, WC);
    const size_t lr_bytes = (size_t)OH * OW * 3 * sizeof(float), out_bytes = (size_t)HC * WC * 3 * sizeof(float);
    int rc = ensure_table(c);
    if (rc == SR_OK) rc = sr_ensure_bufs(c, {{&c->d_vlr, lr_bytes}, {&c->d_vout, out_bytes}, {&c->d_vpart, (size_t)(grid + 1) * sizeof(double)}});
    if (rc == SR_OK && metrics) rc = sr_metrics_reserve(c, HC, WC, metrics->shave);
    if (rc == SR_OK) rc = sr_net_capture_ready(c, false, 3, 1, OH, OW, members ? members : 1u);
    if (rc != SR_OK && c->capturing) return rc;  // (refused on a capturing stream: nothing was allocated, nothing is given back)
    c->vnode_h = c->vnode_w = 0;
    if (rc != SR_OK) {  // also when it was the scores' partials that did not fit: the job keeps nothing of its two large buffers
        sr_free_buf(c->d_vlr);
        sr_free_buf(c->d_vout);
        return rc;
    }
    if (!d_result) d_result = (double*)c->d_vpart.p + grid;
    if (lr) HIPCHK(c, sr_queue_lr_input(*lr, (long)OH * OW, (float*)c->d_vlr.p, c->d_vtab, s));
    else HIPCHK(c, sr_launch_valid_pool(f, d_hr, hr_u8, ch, w, OH, OW, (float*)c->d_vlr.p, c->d_vtab + 256, s));  // (SrgbToLinear of the bytes)
    if (members) rc = sr_ensemble_queue(c, c->d_vlr.p, false, 3, OH, OW, c->d_vout.p, false, members, s);
    else rc = sr_run_stack_auto(c, c->d_vlr.p, false, 3, 1, OH, OW, 0, 0, c->d_vout.p, false, s);
    if (rc != SR_OK) return rc;
    HIPCHK(c, sr_launch_valid_loss((const float*)c->d_vout.p, d_hr, hr_u8, ch, linear, w, HC, WC, c->d_vtab, (double*)c->d_vpart.p, d_result, s));
    c->vnode_h = OH; c->vnode_w = OW;
    if (metrics) return sr_metrics_queue(c, c->d_vout.p, false, 3, WC, (const uint8_t*)d_hr, ch, w, HC, WC, *metrics, s);
    return SR_OK;
}

// The host-pointer calls: upload, run, download 8 bytes (and the scores' 16), as one sr_host_call.
// lr: nullptr = the pooled form, h x w the HR size; else (pair) h x w is the LR size and lr_ch its channel count.
// ensemble: `members` is a self-ensemble's mask (checked here), else it is not looked at.  metrics (with its shave as the caller gave
// it; u8 only): the scores of the same run of the network, beside the loss.
// sr_last_timing: total = the whole call on the device (upload, pool, network, loss, download); stages: the network's.
int validation_host(sr_ctx* c, const void* lr, int lr_ch, const void* hr, bool hr_u8, int ch, int h, int w, int linear, double* err_sum,
                    size_t* n_elems, bool pair, bool ensemble = false, unsigned members = 0, sr_metrics* metrics = nullptr, int shave = 0) {
    sr_plan_clear(c);
    int rc = pair ? check_pair_args(c, lr, hr_u8, lr_ch, hr, ch, h, w) : check_args(c, hr, hr_u8, ch, h, w);
    if (rc == SR_OK && ensemble) rc = sr_ensemble_check(c, members, pair ? h : h / c->factor, pair ? w : w / c->factor);
    sr_metrics_request rq;
    if (rc == SR_OK && metrics) rc = sr_metrics_shave(c, shave, &rq.shave);
    if (rc != SR_OK) return rc;
    if (!ensemble) members = 0;
    if (!err_sum || !n_elems) return SR_E_INVALID;
    const size_t lr_bytes = pair ? (size_t)h * w * (hr_u8 ? (size_t)lr_ch : 3 * sizeof(float)) : 0;
    if (pair) { h *= c->factor; w *= c->factor; }
    const size_t hr_bytes = (size_t)h * w * (hr_u8 ? (size_t)ch : 3 * sizeof(float));
    const int f = c->factor, HC = f * (h / f), WC = f * (w / f);
    const auto d_lr = [&] { return (char*)c->d_vhr.p + sr_round256(hr_bytes); };  // a pair's LR image, behind the HR image
    double sum = 0.0;
    unsigned char scores[16] = {0};
    rc = sr_host_call(
        c, true, SR_TIMES_TOTAL, {{&c->d_vhr, pair ? sr_round256(hr_bytes) + lr_bytes : hr_bytes}},
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(c->d_vhr.p, hr, hr_bytes, hipMemcpyHostToDevice, s));
            if (pair) HIPCHK(c, hipMemcpyAsync(d_lr(), lr, lr_bytes, hipMemcpyHostToDevice, s));
            return SR_OK;
        },
        [&](hipStream_t s) {
            sr_lr_input in;
            in.d_lr = d_lr(); in.u8 = hr_u8; in.ch = lr_ch;
            return run_validation(c, c->d_vhr.p, hr_u8, ch, h, w, linear != 0, nullptr, s, pair ? &in : nullptr, members, metrics ? &rq : nullptr);
        },
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(&sum, (double*)c->d_vpart.p + sr_valid_loss_grid(HC, WC), sizeof sum, hipMemcpyDeviceToHost, s));
            if (metrics) HIPCHK(c, hipMemcpyAsync(scores, sr_metrics_slot(c, HC, WC, rq.shave), sizeof scores, hipMemcpyDeviceToHost, s));
            return SR_OK;
        });
    if (rc != SR_OK) return rc;
    *err_sum = sum;
    *n_elems = sr_loss_elems(f, 1, h, w);
    if (metrics) sr_metrics_fill(metrics, scores, HC, WC, rq.shave);
    return SR_OK;
}

// The device entry points: the arguments checked, then run_validation on the caller's stream.  pair: h x w is the LR size (else the HR
// size, and d_lr is not looked at).  with_metrics: the scores too, at d_result16 (shave as the caller gave it).
int validation_dev(sr_ctx* c, bool pair, const uint8_t* d_lr, int lr_ch, const uint8_t* d_hr, int ch, int h, int w, int linear, double* d_err_sum,
                   bool with_metrics, int shave, void* d_result16, void* stream) {
    sr_plan_clear(c);
    int rc = pair ? check_pair_args(c, d_lr, true, lr_ch, d_hr, ch, h, w) : check_args(c, d_hr, true, ch, h, w);
    sr_metrics_request rq;
    if (rc == SR_OK && with_metrics) rc = sr_metrics_shave(c, shave, &rq.shave);
    if (rc != SR_OK) return rc;
    if (!d_err_sum || !sr_dword_aligned(d_err_sum)) return SR_E_INVALID;
    if (with_metrics && (!d_result16 || !sr_dword_aligned(d_result16))) return SR_E_INVALID;
    rq.d_result16 = d_result16;
    sr_capture_scope capture(c, stream);
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    sr_lr_input in;
    in.d_lr = d_lr; in.u8 = true; in.ch = lr_ch;
    if (pair) { h *= c->factor; w *= c->factor; }
    return run_validation(c, d_hr, true, ch, h, w, linear != 0, d_err_sum, (hipStream_t)stream, pair ? &in : nullptr, 0, with_metrics ? &rq : nullptr);
}

}  // namespace

int sr_valid_ensure_table(sr_ctx* c) {
    return ensure_table(c);
}

void sr_valid_release(sr_ctx* c) {
    for (sr_buf* b : {&c->d_vhr, &c->d_vlr, &c->d_vout, &c->d_vpart}) sr_free_buf(*b);
    if (c->d_vtab) (void)hipFree(c->d_vtab);
    c->d_vtab = nullptr;
    c->vnode_h = c->vnode_w = 0;
}

extern "C" {

int sr_validation_error_rgba8(sr_ctx* c, const uint8_t* hr, int in_channels, int h, int w, int linear_loss, double* err_sum, size_t* n_elems) {
    return validation_host(c, nullptr, 3, hr, true, in_channels, h, w, linear_loss, err_sum, n_elems, false);
}

int sr_validation_error_f32(sr_ctx* c, const float* hr, int h, int w, int linear_loss, double* err_sum, size_t* n_elems) {
    return validation_host(c, nullptr, 3, hr, false, 3, h, w, linear_loss, err_sum, n_elems, false);
}

int sr_validation_error_rgba8_dev(sr_ctx* c, const uint8_t* d_hr, int in_channels, int h, int w, int linear_loss, double* d_err_sum, void* stream) {
    return validation_dev(c, false, nullptr, 3, d_hr, in_channels, h, w, linear_loss, d_err_sum, false, 0, nullptr, stream);
}

int sr_pair_validation_error_rgba8(sr_ctx* c, const uint8_t* lr, int lr_channels, const uint8_t* hr, int hr_channels, int lh, int lw,
                                   int linear_loss, double* err_sum, size_t* n_elems) {
    return validation_host(c, lr, lr_channels, hr, true, hr_channels, lh, lw, linear_loss, err_sum, n_elems, true);
}

int sr_pair_validation_error_f32(sr_ctx* c, const float* lr, const float* hr, int lh, int lw, int linear_loss, double* err_sum, size_t* n_elems) {
    return validation_host(c, lr, 3, hr, false, 3, lh, lw, linear_loss, err_sum, n_elems, true);
}

int sr_pair_validation_error_rgba8_dev(sr_ctx* c, const uint8_t* d_lr, int lr_channels, const uint8_t* d_hr, int hr_channels, int lh, int lw,
                                       int linear_loss, double* d_err_sum, void* stream) {
    return validation_dev(c, true, d_lr, lr_channels, d_hr, hr_channels, lh, lw, linear_loss, d_err_sum, false, 0, nullptr, stream);
}

int sr_pool_validation_error_ensemble_rgba8(sr_ctx* c, const uint8_t* hr, int in_channels, int h, int w, int linear_loss, unsigned members,
                                       double* err_sum, size_t* n_elems) {
    return validation_host(c, nullptr, 3, hr, true, in_channels, h, w, linear_loss, err_sum, n_elems, false, true, members);
}

int sr_pair_validation_error_ensemble_rgba8(sr_ctx* c, const uint8_t* lr, int lr_channels, const uint8_t* hr, int hr_channels, int lh, int lw,
                                            int linear_loss, unsigned members, double* err_sum, size_t* n_elems) {
    return validation_host(c, lr, lr_channels, hr, true, hr_channels, lh, lw, linear_loss, err_sum, n_elems, true, true, members);
}

int sr_pool_validation_metrics_rgba8(sr_ctx* c, const uint8_t* hr, int in_channels, int h, int w, int linear_loss, unsigned members, int shave,
                                double* err_sum, size_t* n_elems, sr_metrics* metrics) {
    if (!metrics) return SR_E_INVALID;
    return validation_host(c, nullptr, 3, hr, true, in_channels, h, w, linear_loss, err_sum, n_elems, false, members != 0, members, metrics, shave);
}

int sr_pair_validation_metrics_rgba8(sr_ctx* c, const uint8_t* lr, int lr_channels, const uint8_t* hr, int hr_channels, int lh, int lw,
                                     int linear_loss, unsigned members, int shave, double* err_sum, size_t* n_elems, sr_metrics* metrics) {
    if (!metrics) return SR_E_INVALID;
    return validation_host(c, lr, lr_channels, hr, true, hr_channels, lh, lw, linear_loss, err_sum, n_elems, true, members != 0, members, metrics,
                           shave);
}

int sr_pool_validation_metrics_rgba8_dev(sr_ctx* c, const uint8_t* d_hr, int in_channels, int h, int w, int linear_loss, int shave, double* d_err_sum,
                                    void* d_result16, void* stream) {
    return validation_dev(c, false, nullptr, 3, d_hr, in_channels, h, w, linear_loss, d_err_sum, true, shave, d_result16, stream);
}

int sr_pair_validation_metrics_rgba8_dev(sr_ctx* c, const uint8_t* d_lr, int lr_channels, const uint8_t* d_hr, int hr_channels, int lh, int lw,
                                         int linear_loss, int shave, double* d_err_sum, void* d_result16, void* stream) {
    return validation_dev(c, true, d_lr, lr_channels, d_hr, hr_channels, lh, lw, linear_loss, d_err_sum, true, shave, d_result16, stream);
}

int sr_read_validation_nodes(sr_ctx* c, float* lr_out, size_t cap_lr, float* out_out, size_t cap_out) {
    if (!c || (!lr_out && !out_out)) return SR_E_INVALID;
    const size_t n_lr = (size_t)c->vnode_h * c->vnode_w * 3, n_out = n_lr * c->factor * c->factor;
    if (n_lr == 0 || (lr_out && cap_lr < n_lr) || (out_out && cap_out < n_out)) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (lr_out) HIPCHK(c, hipMemcpy(lr_out, c->d_vlr.p, n_lr * sizeof(float), hipMemcpyDeviceToHost));
    if (out_out) HIPCHK(c, hipMemcpy(out_out, c->d_vout.p, n_out * sizeof(float), hipMemcpyDeviceToHost));
    return SR_OK;
}

}  // extern "C"
