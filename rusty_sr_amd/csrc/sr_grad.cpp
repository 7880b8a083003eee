// sr_grad.cpp -- host side of backpropagation through the reference's training graph (network.rs:78-103, `g.backprop` in
// Adam::optimise_from, main.rs:181-257) and of one Adam step (include/srhip.h sr_backprop_*, sr_adam_step_dev).  Kernels: sr_grad.hip;
// the pool and the sum of the loss partials: sr_valid.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "sr_internal.h"

namespace {

// Arguments of every backprop entry point, checked before the GPU is touched.
int check_args(sr_ctx* c, const void* params, const void* hr, bool hr_u8, int ch, int n, int h, int w, const void* grad) {
    if (!c || !params || !hr || !grad) return SR_E_INVALID;
    return sr_check_hr_args(c, hr_u8, ch, n, h, w);
}

size_t lr_floats(int f, int n, int h, int w) { return (size_t)n * (h / f) * (w / f) * 3; }

// A paired call's arguments: the LR batch is n x lh x lw, the HR batch f times that (include/srhip.h, "pairs")
int check_pair_args(sr_ctx* c, const void* params, const void* lr, bool u8, int lr_ch, const void* hr, int hr_ch, int n, int lh, int lw,
                    const void* grad) {
    if (!c || !params || !lr || !hr || !grad) return SR_E_INVALID;
    return sr_check_pair_args(c, u8, lr_ch, hr_ch, n, lh, lw);
}

// The host-pointer calls: upload parameters, HR batch and (pairs) LR batch, run, download err_sum and the gradient, as one sr_host_call.
// lr: nullptr = the pooled form, h x w the HR size; else h x w is the LR size and lr_ch its channel count.
int backprop_host(sr_ctx* c, const float* params, size_t n_params, const void* lr, int lr_ch, const void* hr, bool hr_u8, int ch, int n, int h,
                  int w, int linear, float loss_scale, float l2, double* err_sum, size_t* n_elems, float* grad, bool pair) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    sr_plan_clear(c);
    int rc = pair ? check_pair_args(c, params, lr, hr_u8, lr_ch, hr, ch, n, h, w, grad) : check_args(c, params, hr, hr_u8, ch, n, h, w, grad);
    if (rc != SR_OK) return rc;
    if (!err_sum || !n_elems) return SR_E_INVALID;
    const int np = sr_num_params_factor(c->factor);
    if (np < 0 || n_params != (size_t)np) return SR_E_PARAM_COUNT;
    const size_t lr_bytes = pair ? (size_t)n * h * w * (hr_u8 ? (size_t)lr_ch : 3 * sizeof(float)) : 0;
    if (pair) { h *= c->factor; w *= c->factor; }
    const size_t p_bytes = sr_round256((size_t)np * sizeof(float));
    const size_t hr_bytes = (size_t)n * h * w * (hr_u8 ? (size_t)ch : 3 * sizeof(float));
    // d_gin: the parameters, the gradient, the HR batch, a pair's LR batch
    const auto d_params = [&] { return (float*)c->d_gin.p; };
    const auto d_grad = [&] { return (float*)((char*)c->d_gin.p + p_bytes); };
    const auto d_hr = [&] { return (char*)c->d_gin.p + 2 * p_bytes; };
    const auto d_lr = [&] { return d_hr() + sr_round256(hr_bytes); };
    double* slot = nullptr;
    double sum = 0.0;
    rc = sr_host_call(  // (no conv stack runs: no domain handling; the workspace shares the staging buffer's fate)
        c, false, SR_TIMES_NONE, {{&c->d_gin, 2 * p_bytes + sr_round256(hr_bytes) + sr_round256(lr_bytes)}, {&c->d_gws, 0}},
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(d_params(), params, (size_t)np * sizeof(float), hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(d_hr(), hr, hr_bytes, hipMemcpyHostToDevice, s));
            if (pair) HIPCHK(c, hipMemcpyAsync(d_lr(), lr, lr_bytes, hipMemcpyHostToDevice, s));
            return SR_OK;
        },
        [&](hipStream_t s) {
            sr_lr_input in;
            in.d_lr = d_lr(); in.u8 = hr_u8; in.ch = lr_ch;
            return sr_grad_queue(c, d_params(), d_hr(), hr_u8, ch, n, h, w, linear != 0, loss_scale, l2, nullptr, d_grad(), s, &slot,
                                 pair ? &in : nullptr);
        },
        [&](hipStream_t s) -> int {
            HIPCHK(c, hipMemcpyAsync(&sum, slot, sizeof sum, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(grad, d_grad(), (size_t)np * sizeof(float), hipMemcpyDeviceToHost, s));
            return SR_OK;
        });
    if (rc != SR_OK) return rc;
    *err_sum = sum;
    *n_elems = sr_loss_elems(c->factor, n, h, w);
    return SR_OK;
}

// The device entry points: the arguments checked, then sr_grad_queue on the caller's stream.  pair: h x w is the LR size (else the HR
// size, and d_lr is not looked at).
int backprop_dev(sr_ctx* c, const float* d_params, bool pair, const uint8_t* d_lr, int lr_ch, const uint8_t* d_hr, int ch, int n, int h, int w,
                 int linear, float loss_scale, float l2, double* d_err_sum, float* d_grad, void* stream) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    sr_plan_clear(c);
    const int rc = pair ? check_pair_args(c, d_params, d_lr, true, lr_ch, d_hr, ch, n, h, w, d_grad) : check_args(c, d_params, d_hr, true, ch, n, h, w, d_grad);
    if (rc != SR_OK) return rc;
    if (!d_err_sum || !sr_dword_aligned(d_err_sum) || !sr_dword_aligned(d_params) || !sr_dword_aligned(d_grad)) return SR_E_INVALID;
    sr_capture_scope capture(c, stream);
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    sr_lr_input in;
    in.d_lr = d_lr; in.u8 = true; in.ch = lr_ch;
    if (pair) { h *= c->factor; w *= c->factor; }
    return sr_grad_queue(c, d_params, d_hr, true, ch, n, h, w, linear != 0, loss_scale, l2, d_err_sum, d_grad, (hipStream_t)stream, nullptr,
                         pair ? &in : nullptr);
}

}  // namespace

int sr_grad_input_buffer(sr_ctx* c, int n, int OH, int OW, float** x) {
    const size_t x_bytes = sr_round256((size_t)n * OH * OW * 3 * sizeof(float));
    int rc = sr_valid_ensure_table(c);
    // (the host-pointer calls' staging buffer shares the workspace's fate)
    if (rc == SR_OK) rc = sr_ensure_bufs(c, {{&c->d_gws, x_bytes + sr_grad_workspace_bytes(c->factor, n, OH, OW)}, {&c->d_gin, 0}});
    if (rc != SR_OK) return rc;
    *x = (float*)c->d_gws.p;
    return SR_OK;
}

// The input stage -- the pool, or a paired call's LR batch -- then the backward pass, on device buffers, queued on s.  The workspace is
// grown here.
int sr_grad_queue(sr_ctx* c, const float* d_params, const void* d_hr, bool hr_u8, int ch, int n, int h, int w, bool linear, float loss_scale,
                  float l2, void* d_err, float* d_grad, hipStream_t s, double** result_slot, const sr_lr_input* lr) {
    const int f = c->factor, OH = h / f, OW = w / f;
    const size_t x_bytes = sr_round256(lr_floats(f, n, h, w) * sizeof(float));
    float* x = nullptr;
    const int rc = sr_grad_input_buffer(c, n, OH, OW, &x);
    if (rc != SR_OK) return rc;
    const float* tab_lin = c->d_vtab + 256;
    if (lr) {
        HIPCHK(c, sr_queue_lr_input(*lr, (long)n * OH * OW, x, c->d_vtab, s));
    } else if (h % f == 0) {  // the batch is one image of n h rows
        HIPCHK(c, sr_launch_valid_pool(f, d_hr, hr_u8, ch, w, n * OH, OW, x, tab_lin, s));
    } else {  // each image drops its own last h % f rows
        const size_t img_bytes = (size_t)h * w * (hr_u8 ? (size_t)ch : 3 * sizeof(float));
        for (int b = 0; b < n; ++b)
            HIPCHK(c, sr_launch_valid_pool(f, (const uint8_t*)d_hr + b * img_bytes, hr_u8, ch, w, OH, OW, x + (size_t)b * OH * OW * 3,
                                           tab_lin, s));
    }
    sr_grad_plan p;
    p.factor = f; p.n = n; p.H = OH; p.W = OW;
    p.params = d_params;
    p.x = x;
    p.hr = d_hr; p.hr_u8 = hr_u8; p.hr_ch = ch; p.hr_h = h; p.hr_w = w;
    p.tab = c->d_vtab;
    p.linear = linear; p.loss_scale = loss_scale; p.l2 = l2;
    p.loss_kind = c->loss_kind; p.loss_eps = c->loss_eps;  // the objective in force now: kernel arguments of this pass from here on
    p.ws = (float*)((char*)c->d_gws.p + x_bytes);
    p.err_out = d_err;
    p.grad = d_grad;
    if (result_slot) *result_slot = sr_grad_result_slot(p);
    {  // the plan record: how this pass splits its sums (DESIGN s6), as the layout its launches are sized with gives it
        const sr_grad_split g = sr_grad_split_of(f, n, OH, OW);
        char line[192];
        snprintf(line, sizeof line, "grad n=%d h=%d w=%d conv=%d loss=%d wchunks=%d wchunk=%ld cchunks=%d cchunk=%ld", n, OH, OW, g.conv_grid,
                 g.loss_grid, g.wchunks, g.wchunk, g.cchunks, g.cchunk);
        sr_plan_note(c, line);
    }
    HIPCHK(c, sr_launch_grad(p, s));
    return SR_OK;
}

void sr_grad_release(sr_ctx* c) {
    sr_free_buf(c->d_gws);
    sr_free_buf(c->d_gin);
}

extern "C" {

int sr_backprop_f32(sr_ctx* c, const float* params, size_t n_params, const float* hr, int n, int h, int w, int linear_loss, float loss_scale,
                    float l2, double* err_sum, size_t* n_elems, float* grad) {
    return backprop_host(c, params, n_params, nullptr, 3, hr, false, 3, n, h, w, linear_loss, loss_scale, l2, err_sum, n_elems, grad, false);
}

int sr_backprop_rgba8(sr_ctx* c, const float* params, size_t n_params, const uint8_t* hr, int in_channels, int n, int h, int w, int linear_loss,
                      float loss_scale, float l2, double* err_sum, size_t* n_elems, float* grad) {
    return backprop_host(c, params, n_params, nullptr, 3, hr, true, in_channels, n, h, w, linear_loss, loss_scale, l2, err_sum, n_elems, grad,
                         false);
}

int sr_backprop_rgba8_dev(sr_ctx* c, const float* d_params, const uint8_t* d_hr, int in_channels, int n, int h, int w, int linear_loss,
                          float loss_scale, float l2, double* d_err_sum, float* d_grad, void* stream) {
    return backprop_dev(c, d_params, false, nullptr, 3, d_hr, in_channels, n, h, w, linear_loss, loss_scale, l2, d_err_sum, d_grad, stream);
}

int sr_pair_backprop_f32(sr_ctx* c, const float* params, size_t n_params, const float* lr, const float* hr, int n, int lh, int lw,
                         int linear_loss, float loss_scale, float l2, double* err_sum, size_t* n_elems, float* grad) {
    return backprop_host(c, params, n_params, lr, 3, hr, false, 3, n, lh, lw, linear_loss, loss_scale, l2, err_sum, n_elems, grad, true);
}

int sr_pair_backprop_rgba8(sr_ctx* c, const float* params, size_t n_params, const uint8_t* lr, int lr_channels, const uint8_t* hr,
                           int hr_channels, int n, int lh, int lw, int linear_loss, float loss_scale, float l2, double* err_sum,
                           size_t* n_elems, float* grad) {
    return backprop_host(c, params, n_params, lr, lr_channels, hr, true, hr_channels, n, lh, lw, linear_loss, loss_scale, l2, err_sum, n_elems,
                         grad, true);
}

int sr_pair_backprop_rgba8_dev(sr_ctx* c, const float* d_params, const uint8_t* d_lr, int lr_channels, const uint8_t* d_hr, int hr_channels,
                               int n, int lh, int lw, int linear_loss, float loss_scale, float l2, double* d_err_sum, float* d_grad,
                               void* stream) {
    return backprop_dev(c, d_params, true, d_lr, lr_channels, d_hr, hr_channels, n, lh, lw, linear_loss, loss_scale, l2, d_err_sum, d_grad, stream);
}

// The objective of the backward passes queued from now on (include/srhip.h): host-side state, read by sr_grad_queue.
int sr_set_loss(sr_ctx* c, int kind, float eps) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    sr_plan_clear(c);
    if (!c || c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    if (kind != SR_LOSS_MSE && kind != SR_LOSS_L1 && kind != SR_LOSS_CHARBONNIER) return SR_E_INVALID;
    if (kind == SR_LOSS_CHARBONNIER) {
        if (!(eps > 0.0f && eps <= 1.0f)) return SR_E_INVALID;  // (a NaN fails both comparisons)
        c->loss_eps = eps;
    }
    c->loss_kind = kind;
    return SR_OK;
}

int sr_get_loss(sr_ctx* c, int* kind, float* eps) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    sr_plan_clear(c);
    if (!c || c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    if (kind) *kind = c->loss_kind;
    if (eps) *eps = c->loss_eps;
    return SR_OK;
}

int sr_adam_step_dev(sr_ctx* c, float* d_params, float* d_m, float* d_v, const float* d_grad, size_t n, int step, float lr, float beta1,
                     float beta2, float eps, void* stream) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    sr_plan_clear(c);
    if (!c || !d_params || !d_m || !d_v || !d_grad || n == 0 || step < 1) return SR_E_INVALID;
    if (!sr_dword_aligned(d_params) || !sr_dword_aligned(d_m) || !sr_dword_aligned(d_v) || !sr_dword_aligned(d_grad)) return SR_E_INVALID;
    // bias corrections 1 - beta^t, in f32
    const float bc1 = 1.0f - std::pow(beta1, (float)step), bc2 = 1.0f - std::pow(beta2, (float)step);
    sr_capture_scope capture(c, stream);
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sr_launch_grad_adam(d_params, d_m, d_v, d_grad, n, lr, beta1, beta2, eps, bc1, bc2, (hipStream_t)stream));
    return SR_OK;
}

}  // extern "C"
