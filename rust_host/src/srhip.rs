//! Raw binding of `include/srhip.h` plus a small safe wrapper.  One `extern` line per C
//! declaration; `tests/test_abi.py` keeps the header, the library and the Python table in step,
//! and `tests/test_rust_host.py` checks that every symbol named here is exported.
#![allow(dead_code)]
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_uint, c_void};
use std::ptr;

#[repr(C)]
pub struct SrCtx {
    _private: [u8; 0],
}

#[repr(C)]
pub struct SrTrain {
    _private: [u8; 0],
}

/// `sr_train_pair_crop`: a resident pair id, or -1 and both images' host pixels; the crop origin in LR pixels.
#[repr(C)]
pub struct SrTrainPairCrop {
    pub pair: c_int,
    pub lr_px: *const u8,
    pub hr_px: *const u8,
    pub lr_channels: c_int,
    pub hr_channels: c_int,
    pub lh: c_int,
    pub lw: c_int,
    pub y0: c_int,
    pub x0: c_int,
}

/// `sr_train_crop`: a resident image id, or -1 and host pixels; the crop origin.
#[repr(C)]
pub struct SrTrainCrop {
    pub image: c_int,
    pub px: *const u8,
    pub in_channels: c_int,
    pub h: c_int,
    pub w: c_int,
    pub y0: c_int,
    pub x0: c_int,
}

/// `sr_metrics`: the sums and counts the Y-PSNR and the SSIM of one image are made of.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrMetrics {
    pub y_sq_err: u64,
    pub y_count: u64,
    pub ssim_sum: f64,
    pub ssim_count: u64,
}

#[repr(C)]
pub struct SrVideo {
    _private: [u8; 0],
}

/// `sr_yuv_format`: subsampling (0: 4:2:0, 1: 4:4:4), chroma siting (0: centre, 1: left), matrix (0: BT.601, 1: BT.709), range (0: limited, 1: full).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrYuvFormat {
    pub subsampling: i32,
    pub siting: i32,
    pub matrix: i32,
    pub range: i32,
}

/// `sr_yuv16_format`: a deep frame, samples in little-endian u16.  subsampling (0: 4:2:0, 1: 4:4:4, 2: 4:2:2), siting, matrix (0: BT.601,
/// 1: BT.709, 2: BT.2020 non-constant luminance), range as `sr_yuv_format`; depth 9..=16 bits a sample.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrYuv16Format {
    pub subsampling: i32,
    pub siting: i32,
    pub matrix: i32,
    pub range: i32,
    pub depth: i32,
}

/// `sr_row_band`: LR rows `y0..y1` a frame computes (`sr_video_reuse_plan`).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrRowBand {
    pub y0: i32,
    pub y1: i32,
}

/// `sr_video_reuse_stats`: what a session's row reuse has computed and what it has taken over from the last frame.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrVideoReuseStats {
    pub frames: u64,
    pub frames_reused: u64,
    pub frames_partial: u64,
    pub frames_full: u64,
    pub rows_total: u64,
    pub rows_computed: u64,
    pub bands: u64,
}

/// `sr_degrade`: one item's blur width (HR pixels), noise level (8-bit levels), JPEG quality (0: none) and noise seed.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrDegrade {
    pub sigma: f32,
    pub noise: f32,
    pub quality: c_int,
    pub seed: u64,
}

/// `sr_grad_norm`: the gradient's sum of squares, the clipping scale and the skip flag, as the device writes them.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrGradNorm {
    pub sumsq: f64,
    pub scale: f32,
    pub skip: i32,
}

/// `sr_train_stat`: one step's err_sum, gradient norm, learning rate and clipping scale.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrTrainStat {
    pub err_sum: f64,
    pub grad_norm: f64,
    pub lr: f32,
    pub scale: f32,
}

/// `sr_lr_schedule`: kind (0 constant, 1 step, 2 cosine), base rate, warm-up steps and the kind's own fields.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct SrLrSchedule {
    pub kind: c_int,
    pub base: f32,
    pub warmup: i64,
    pub every: i64,
    pub gamma: f64,
    pub total: i64,
    pub min_lr: f32,
}

pub const SR_OK: c_int = 0;
pub const SR_E_HIP: c_int = -5;
pub const SR_GRAPH_SR_NET: c_int = 0;
pub const SR_GRAPH_BILINEAR: c_int = 1;
pub const SR_GRAPH_DOWNSAMPLE: c_int = 2;
pub const SR_PRECISION_F32: c_int = 0;
pub const SR_PRECISION_SPLIT_F16: c_int = 1;
pub const SR_FACTOR: c_int = 3;
pub const SR_E_COMM: c_int = -9;
pub const SR_E_DOMAIN: c_int = -10;
pub const SR_HALO: c_int = 7;
pub const SR_COMM_ID_BYTES: c_int = 128;
pub const SR_TRAIN_MAX_BATCH: c_int = 64;
pub const SR_TRAIN_RING: c_int = 64;
pub const SR_TRAIN_STORE_AUTO: usize = usize::MAX;
pub const SR_ALPHA_BLEED_DEFAULT: c_int = 8;
pub const SR_ALPHA_BLEED_MAX: c_int = 16;
pub const SR_BORDER_WRAP: c_int = 1;
pub const SR_BORDER_REPLICATE: c_int = 2;
pub const SR_BORDER_MIRROR: c_int = 3;
pub const SR_BORDER_PAD_DEFAULT: c_int = 8;
pub const SR_BORDER_PAD_MAX: c_int = 32;
pub const SR_LOSS_MSE: c_int = 0;
pub const SR_LOSS_L1: c_int = 1;
pub const SR_LOSS_CHARBONNIER: c_int = 2;
pub const SR_VIDEO_REUSE_OFF: c_int = 0;
pub const SR_VIDEO_REUSE_ROWS: c_int = 1;
pub const SR_REUSE_MAX_BANDS: c_int = 4;

extern "C" {
    pub fn sr_rsr_decode(blob: *const u8, len: usize, out: *mut f32, cap: usize, n_out: *mut usize) -> c_int;
    pub fn sr_rsr_encode(params: *const f32, n: usize, out: *mut u8, cap: usize, len_out: *mut usize) -> c_int;
    pub fn sr_create(out: *mut *mut SrCtx, params: *const f32, n_params: usize, factor: c_int, device: c_int) -> c_int;
    pub fn sr_create_graph(out: *mut *mut SrCtx, graph: c_int, params: *const f32, n_params: usize, factor: c_int,
                           device: c_int) -> c_int;
    pub fn sr_num_params(graph: c_int) -> c_int;
    pub fn sr_num_params_factor(factor: c_int) -> c_int;
    pub fn sr_set_precision(ctx: *mut SrCtx, mode: c_int) -> c_int;
    pub fn sr_check_domain(ctx: *mut SrCtx) -> c_int;
    pub fn sr_destroy(ctx: *mut SrCtx);
    pub fn sr_upscale_f32(ctx: *mut SrCtx, input: *const f32, n: c_int, h: c_int, w: c_int, out: *mut f32) -> c_int;
    pub fn sr_upscale_rgba8(ctx: *mut SrCtx, input: *const u8, in_channels: c_int, n: c_int, h: c_int, w: c_int,
                            out_rgba: *mut u8) -> c_int;
    pub fn sr_reserve_f32(ctx: *mut SrCtx, n: c_int, h: c_int, w: c_int) -> c_int;
    pub fn sr_reserve_rgba8(ctx: *mut SrCtx, in_channels: c_int, n: c_int, h: c_int, w: c_int) -> c_int;
    pub fn sr_upscale_f32_dev(ctx: *mut SrCtx, d_in: *const f32, n: c_int, h: c_int, w: c_int, d_out: *mut f32,
                              stream: *mut c_void) -> c_int;
    pub fn sr_upscale_rgba8_dev(ctx: *mut SrCtx, d_in: *const u8, in_channels: c_int, n: c_int, h: c_int, w: c_int,
                                d_out: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_band_f32_dev(ctx: *mut SrCtx, d_in: *const f32, h_ext: c_int, w: c_int, halo_top: c_int,
                                   halo_bot: c_int, d_out: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_band_rgba8_dev(ctx: *mut SrCtx, d_in: *const u8, in_channels: c_int, h_ext: c_int, w: c_int,
                                     halo_top: c_int, halo_bot: c_int, d_out: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_read_feature(ctx: *mut SrCtx, which: c_int, out_host: *mut f32, cap_floats: usize) -> c_int;
    pub fn sr_upscale_f32_multi(ctxs: *const *mut SrCtx, n_ctx: c_int, input: *const f32, h: c_int, w: c_int, out: *mut f32) -> c_int;
    pub fn sr_upscale_rgba8_multi(ctxs: *const *mut SrCtx, n_ctx: c_int, input: *const u8, in_channels: c_int, h: c_int, w: c_int,
                                  out_rgba: *mut u8) -> c_int;
    pub fn sr_upscale_f32_batch_multi(ctxs: *const *mut SrCtx, n_ctx: c_int, input: *const f32, n: c_int, h: c_int, w: c_int,
                                      out: *mut f32) -> c_int;
    pub fn sr_upscale_rgba8_batch_multi(ctxs: *const *mut SrCtx, n_ctx: c_int, input: *const u8, in_channels: c_int, n: c_int,
                                        h: c_int, w: c_int, out_rgba: *mut u8) -> c_int;
    // RCCL communicator inside the library + device-resident row bands (one image over several GPUs)
    pub fn sr_comm_available() -> c_int;
    pub fn sr_comm_unique_id(id: *mut u8, cap: usize) -> c_int;
    pub fn sr_comm_init_rank(ctx: *mut SrCtx, id: *const u8, id_len: usize, rank: c_int, nranks: c_int) -> c_int;
    pub fn sr_comm_init_all(ctxs: *const *mut SrCtx, n: c_int) -> c_int;
    pub fn sr_comm_init_local(ctxs: *const *mut SrCtx, n: c_int) -> c_int;
    pub fn sr_comm_destroy(ctx: *mut SrCtx);
    pub fn sr_comm_rank(ctx: *mut SrCtx, rank: *mut c_int, nranks: *mut c_int) -> c_int;
    pub fn sr_last_comm_error(ctx: *mut SrCtx) -> c_int;
    pub fn sr_last_comm_ms(ctx: *mut SrCtx, comm_ms: *mut f64) -> c_int;
    pub fn sr_last_comm_exposed_ms(ctx: *mut SrCtx, exposed_ms: *mut f64) -> c_int;
    pub fn sr_upscale_sharded_f32_dev(ctx: *mut SrCtx, d_band: *const f32, h_band: c_int, w: c_int, d_out: *mut f32,
                                      stream: *mut c_void) -> c_int;
    pub fn sr_upscale_sharded_rgba8_dev(ctx: *mut SrCtx, d_band: *const u8, in_channels: c_int, h_band: c_int, w: c_int,
                                        d_out: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_sharded_f32_all(ctxs: *const *mut SrCtx, n: c_int, d_bands: *const *const f32, h_bands: *const c_int,
                                      w: c_int, d_outs: *const *mut f32) -> c_int;
    pub fn sr_upscale_sharded_rgba8_all(ctxs: *const *mut SrCtx, n: c_int, d_bands: *const *const u8, in_channels: c_int,
                                        h_bands: *const c_int, w: c_int, d_outs: *const *mut u8) -> c_int;
    pub fn sr_set_pipeline(ctx: *mut SrCtx, enabled: c_int) -> c_int;
    pub fn sr_host_alloc(out: *mut *mut c_void, bytes: usize) -> c_int;  // page-locked host memory
    pub fn sr_host_free(p: *mut c_void);
    pub fn sr_set_profiling(ctx: *mut SrCtx, enabled: c_int) -> c_int;
    pub fn sr_last_timing(ctx: *mut SrCtx, total_ms: *mut f64, stage_ms: *mut f64, h2d_ms: *mut f64, d2h_ms: *mut f64) -> c_int;
    pub fn sr_device_info(ctx: *mut SrCtx, name: *mut c_char, cap: usize, cus: *mut c_int, mhz: *mut c_int) -> c_int;
    pub fn sr_last_hip_error(ctx: *mut SrCtx) -> c_int;
    pub fn sr_strerror(status: c_int) -> *const c_char;
    pub fn sr_validation_error_rgba8(ctx: *mut SrCtx, hr: *const u8, in_channels: c_int, h: c_int, w: c_int, linear_loss: c_int, err_sum: *mut f64, n_elems: *mut usize) -> c_int;
    pub fn sr_validation_error_f32(ctx: *mut SrCtx, hr: *const f32, h: c_int, w: c_int, linear_loss: c_int, err_sum: *mut f64, n_elems: *mut usize) -> c_int;
    pub fn sr_validation_error_rgba8_dev(ctx: *mut SrCtx, d_hr: *const u8, in_channels: c_int, h: c_int, w: c_int, linear_loss: c_int, d_err_sum: *mut f64, stream: *mut c_void) -> c_int;
    pub fn sr_read_validation_nodes(ctx: *mut SrCtx, lr_out: *mut f32, cap_lr: usize, out_out: *mut f32, cap_out: usize) -> c_int;
    pub fn sr_backprop_f32(ctx: *mut SrCtx, params: *const f32, n_params: usize, hr: *const f32, n: c_int, h: c_int, w: c_int, linear_loss: c_int, loss_scale: f32, l2: f32, err_sum: *mut f64, n_elems: *mut usize, grad: *mut f32) -> c_int;
    pub fn sr_backprop_rgba8(ctx: *mut SrCtx, params: *const f32, n_params: usize, hr: *const u8, in_channels: c_int, n: c_int, h: c_int, w: c_int, linear_loss: c_int, loss_scale: f32, l2: f32, err_sum: *mut f64, n_elems: *mut usize, grad: *mut f32) -> c_int;
    pub fn sr_backprop_rgba8_dev(ctx: *mut SrCtx, d_params: *const f32, d_hr: *const u8, in_channels: c_int, n: c_int, h: c_int, w: c_int, linear_loss: c_int, loss_scale: f32, l2: f32, d_err_sum: *mut f64, d_grad: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_adam_step_dev(ctx: *mut SrCtx, d_params: *mut f32, d_m: *mut f32, d_v: *mut f32, d_grad: *const f32, n: usize, step: c_int, lr: f32, beta1: f32, beta2: f32, eps: f32, stream: *mut c_void) -> c_int;
    pub fn sr_init_params(factor: c_int, seed: u64, out: *mut f32, cap: usize) -> c_int;
    pub fn sr_set_params(ctx: *mut SrCtx, params: *const f32, n_params: usize) -> c_int;
    pub fn sr_train_create(out: *mut *mut SrTrain, ctx: *mut SrCtx, start_params: *const f32, n_params: usize, linear_loss: c_int, l2: f32, lr: f32, beta1: f32, beta2: f32, eps: f32, store_bytes: usize) -> c_int;
    pub fn sr_train_add_image(t: *mut SrTrain, px: *const u8, in_channels: c_int, h: c_int, w: c_int, id: *mut c_int) -> c_int;
    pub fn sr_train_step(t: *mut SrTrain, items: *const SrTrainCrop, n: c_int, crop_h: c_int, crop_w: c_int) -> c_int;
    pub fn sr_train_step_aug(t: *mut SrTrain, items: *const SrTrainCrop, members: *const u8, n: c_int, crop_h: c_int, crop_w: c_int) -> c_int;
    pub fn sr_train_sync(t: *mut SrTrain, err_sums: *mut f64, cap: usize, n_steps: *mut usize) -> c_int;
    pub fn sr_train_params(t: *mut SrTrain, out: *mut f32, cap: usize) -> c_int;
    pub fn sr_train_destroy(t: *mut SrTrain);
    pub fn sr_pair_validation_error_rgba8(ctx: *mut SrCtx, lr: *const u8, lr_channels: c_int, hr: *const u8, hr_channels: c_int, lh: c_int, lw: c_int, linear_loss: c_int, err_sum: *mut f64, n_elems: *mut usize) -> c_int;
    pub fn sr_pair_validation_error_f32(ctx: *mut SrCtx, lr: *const f32, hr: *const f32, lh: c_int, lw: c_int, linear_loss: c_int, err_sum: *mut f64, n_elems: *mut usize) -> c_int;
    pub fn sr_pair_validation_error_rgba8_dev(ctx: *mut SrCtx, d_lr: *const u8, lr_channels: c_int, d_hr: *const u8, hr_channels: c_int, lh: c_int, lw: c_int, linear_loss: c_int, d_err_sum: *mut f64, stream: *mut c_void) -> c_int;
    pub fn sr_pair_backprop_f32(ctx: *mut SrCtx, params: *const f32, n_params: usize, lr: *const f32, hr: *const f32, n: c_int, lh: c_int, lw: c_int, linear_loss: c_int, loss_scale: f32, l2: f32, err_sum: *mut f64, n_elems: *mut usize, grad: *mut f32) -> c_int;
    pub fn sr_pair_backprop_rgba8(ctx: *mut SrCtx, params: *const f32, n_params: usize, lr: *const u8, lr_channels: c_int, hr: *const u8, hr_channels: c_int, n: c_int, lh: c_int, lw: c_int, linear_loss: c_int, loss_scale: f32, l2: f32, err_sum: *mut f64, n_elems: *mut usize, grad: *mut f32) -> c_int;
    pub fn sr_pair_backprop_rgba8_dev(ctx: *mut SrCtx, d_params: *const f32, d_lr: *const u8, lr_channels: c_int, d_hr: *const u8, hr_channels: c_int, n: c_int, lh: c_int, lw: c_int, linear_loss: c_int, loss_scale: f32, l2: f32, d_err_sum: *mut f64, d_grad: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_train_add_pair(t: *mut SrTrain, lr_px: *const u8, lr_channels: c_int, hr_px: *const u8, hr_channels: c_int, lh: c_int, lw: c_int, id: *mut c_int) -> c_int;
    pub fn sr_train_step_pairs(t: *mut SrTrain, items: *const SrTrainPairCrop, n: c_int, crop_lh: c_int, crop_lw: c_int) -> c_int;
    pub fn sr_train_step_pairs_aug(t: *mut SrTrain, items: *const SrTrainPairCrop, members: *const u8, n: c_int, crop_lh: c_int, crop_lw: c_int) -> c_int;
    pub fn sr_upscale_ensemble_f32_dev(ctx: *mut SrCtx, d_in: *const f32, n: c_int, h: c_int, w: c_int, d_out: *mut f32, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_ensemble_rgba8_dev(ctx: *mut SrCtx, d_in: *const u8, in_channels: c_int, n: c_int, h: c_int, w: c_int, d_out_rgba: *mut u8, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_ensemble_f32(ctx: *mut SrCtx, input: *const f32, n: c_int, h: c_int, w: c_int, out: *mut f32, members: c_uint) -> c_int;
    pub fn sr_upscale_ensemble_rgba8(ctx: *mut SrCtx, input: *const u8, in_channels: c_int, n: c_int, h: c_int, w: c_int, out_rgba: *mut u8, members: c_uint) -> c_int;
    pub fn sr_pool_validation_error_ensemble_rgba8(ctx: *mut SrCtx, hr: *const u8, in_channels: c_int, h: c_int, w: c_int, linear_loss: c_int, members: c_uint, err_sum: *mut f64, n_elems: *mut usize) -> c_int;
    pub fn sr_pair_validation_error_ensemble_rgba8(ctx: *mut SrCtx, lr: *const u8, lr_channels: c_int, hr: *const u8, hr_channels: c_int, lh: c_int, lw: c_int, linear_loss: c_int, members: c_uint, err_sum: *mut f64, n_elems: *mut usize) -> c_int;
    pub fn sr_image_metrics_rgba8(ctx: *mut SrCtx, a: *const u8, a_channels: c_int, b: *const u8, b_channels: c_int, h: c_int, w: c_int, shave: c_int, metrics: *mut SrMetrics) -> c_int;
    pub fn sr_image_metrics_rgba8_dev(ctx: *mut SrCtx, d_a: *const u8, a_channels: c_int, d_b: *const u8, b_channels: c_int, h: c_int, w: c_int, shave: c_int, d_result16: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn sr_pool_validation_metrics_rgba8(ctx: *mut SrCtx, hr: *const u8, in_channels: c_int, h: c_int, w: c_int, linear_loss: c_int, members: c_uint, shave: c_int, err_sum: *mut f64, n_elems: *mut usize, metrics: *mut SrMetrics) -> c_int;
    pub fn sr_pair_validation_metrics_rgba8(ctx: *mut SrCtx, lr: *const u8, lr_channels: c_int, hr: *const u8, hr_channels: c_int, lh: c_int, lw: c_int, linear_loss: c_int, members: c_uint, shave: c_int, err_sum: *mut f64, n_elems: *mut usize, metrics: *mut SrMetrics) -> c_int;
    pub fn sr_pool_validation_metrics_rgba8_dev(ctx: *mut SrCtx, d_hr: *const u8, in_channels: c_int, h: c_int, w: c_int, linear_loss: c_int, shave: c_int, d_err_sum: *mut f64, d_result16: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn sr_pair_validation_metrics_rgba8_dev(ctx: *mut SrCtx, d_lr: *const u8, lr_channels: c_int, d_hr: *const u8, hr_channels: c_int, lh: c_int, lw: c_int, linear_loss: c_int, shave: c_int, d_err_sum: *mut f64, d_result16: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn sr_bleed_rgba8_dev(ctx: *mut SrCtx, d_in_rgba: *const u8, n: c_int, h: c_int, w: c_int, radius: c_int, d_out_rgba: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_merge_alpha_rgba8_dev(ctx: *mut SrCtx, d_lr_rgba: *const u8, n: c_int, h: c_int, w: c_int, d_out_rgba: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_rgba8_alpha_dev(ctx: *mut SrCtx, d_in_rgba: *const u8, n: c_int, h: c_int, w: c_int, d_out_rgba: *mut u8, radius: c_int, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_rgba8_alpha(ctx: *mut SrCtx, in_rgba: *const u8, n: c_int, h: c_int, w: c_int, out_rgba: *mut u8, radius: c_int, members: c_uint) -> c_int;
    pub fn sr_resize_dev(ctx: *mut SrCtx, d_in: *const c_void, in_pixels: c_int, n: c_int, h: c_int, w: c_int, d_out: *mut c_void, out_pixels: c_int, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_resize_rgba8(ctx: *mut SrCtx, input: *const u8, n: c_int, h: c_int, w: c_int, out: *mut u8, oh: c_int, ow: c_int, filter: c_int, flags: c_uint) -> c_int;
    pub fn sr_upscale_rgba8_sized_dev(ctx: *mut SrCtx, d_in_rgba: *const u8, n: c_int, h: c_int, w: c_int, d_out_rgba: *mut u8, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_rgba8_sized(ctx: *mut SrCtx, in_rgba: *const u8, n: c_int, h: c_int, w: c_int, out_rgba: *mut u8, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, members: c_uint) -> c_int;
    pub fn sr_degrade_rgba8(ctx: *mut SrCtx, hr: *const u8, in_channels: c_int, h: c_int, w: c_int, factor: c_int, y0: c_int, x0: c_int, frame_h: c_int, frame_w: c_int, member: c_int, deg: *const SrDegrade, lr_rgb: *mut u8) -> c_int;
    pub fn sr_degrade_rgba8_dev(ctx: *mut SrCtx, d_hr: *const u8, in_channels: c_int, h: c_int, w: c_int, factor: c_int, y0: c_int, x0: c_int, frame_h: c_int, frame_w: c_int, member: c_int, deg: *const SrDegrade, d_lr_rgb: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_train_step_degrade(t: *mut SrTrain, items: *const SrTrainCrop, members: *const u8, deg: *const SrDegrade, n: c_int, crop_h: c_int, crop_w: c_int) -> c_int;
    pub fn sr_pad_rgba8_dev(ctx: *mut SrCtx, d_in_rgba: *const u8, n: c_int, h: c_int, w: c_int, mode: c_int, pad: c_int, d_out_rgba: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_pad_f32_dev(ctx: *mut SrCtx, d_in: *const f32, n: c_int, h: c_int, w: c_int, mode: c_int, pad: c_int, d_out: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_crop_rgba8_dev(ctx: *mut SrCtx, d_in_rgba: *const u8, n: c_int, big_h: c_int, big_w: c_int, y0: c_int, x0: c_int, ch: c_int, cw: c_int, d_out_rgba: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_crop_f32_dev(ctx: *mut SrCtx, d_in: *const f32, n: c_int, big_h: c_int, big_w: c_int, y0: c_int, x0: c_int, ch: c_int, cw: c_int, d_out: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_rgba8_border_dev(ctx: *mut SrCtx, d_in_rgba: *const u8, n: c_int, h: c_int, w: c_int, d_out_rgba: *mut u8, mode: c_int, pad: c_int, members: c_uint, bleed: c_int, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_f32_border_dev(ctx: *mut SrCtx, d_in: *const f32, n: c_int, h: c_int, w: c_int, d_out: *mut f32, mode: c_int, pad: c_int, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_rgba8_border(ctx: *mut SrCtx, in_rgba: *const u8, n: c_int, h: c_int, w: c_int, out_rgba: *mut u8, mode: c_int, pad: c_int, members: c_uint, bleed: c_int) -> c_int;
    pub fn sr_upscale_f32_border(ctx: *mut SrCtx, input: *const f32, n: c_int, h: c_int, w: c_int, out: *mut f32, mode: c_int, pad: c_int, members: c_uint) -> c_int;
    pub fn sr_yuv_frame_bytes(fmt: *const SrYuvFormat, h: c_int, w: c_int) -> usize;
    pub fn sr_yuv_to_rgb_dev(ctx: *mut SrCtx, d_yuv: *const u8, fmt: *const SrYuvFormat, n: c_int, h: c_int, w: c_int, d_rgb: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_rgb_to_yuv_dev(ctx: *mut SrCtx, d_rgb: *const f32, fmt: *const SrYuvFormat, n: c_int, h: c_int, w: c_int, d_yuv: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_yuv_dev(ctx: *mut SrCtx, d_in: *const u8, fmt: *const SrYuvFormat, n: c_int, h: c_int, w: c_int, d_out: *mut u8, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_yuv(ctx: *mut SrCtx, input: *const u8, fmt: *const SrYuvFormat, n: c_int, h: c_int, w: c_int, out: *mut u8, members: c_uint) -> c_int;
    pub fn sr_video_create(ctx: *mut SrCtx, fmt: *const SrYuvFormat, h: c_int, w: c_int, slots: c_int, members: c_uint, out: *mut *mut SrVideo) -> c_int;
    pub fn sr_video_acquire(v: *mut SrVideo, in_frame: *mut *mut u8) -> c_int;
    pub fn sr_video_submit(v: *mut SrVideo) -> c_int;
    pub fn sr_video_receive(v: *mut SrVideo, out_frame: *mut *const u8) -> c_int;
    pub fn sr_video_pending(v: *const SrVideo) -> c_int;
    pub fn sr_video_destroy(v: *mut SrVideo);
    pub fn sr_rows_differ_dev(ctx: *mut SrCtx, d_a: *const c_void, d_b: *const c_void, rows: usize, row_bytes: usize, d_flags: *mut u32, stream: *mut c_void) -> c_int;
    pub fn sr_video_reuse_plan(plane_flags: *const u32, subsampling: c_int, h: c_int, bands: *mut SrRowBand, max_bands: c_int, n_bands: *mut c_int) -> c_int;
    pub fn sr_video_set_reuse(v: *mut SrVideo, mode: c_int) -> c_int;
    pub fn sr_video_get_reuse_stats(v: *const SrVideo, out: *mut SrVideoReuseStats) -> c_int;
    pub fn sr_yuv16_frame_bytes(fmt: *const SrYuv16Format, h: c_int, w: c_int) -> usize;
    pub fn sr_yuv16_to_rgb_dev(ctx: *mut SrCtx, d_yuv: *const u16, fmt: *const SrYuv16Format, n: c_int, h: c_int, w: c_int, d_rgb: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_rgb_to_yuv16_dev(ctx: *mut SrCtx, d_rgb: *const f32, fmt: *const SrYuv16Format, n: c_int, h: c_int, w: c_int, d_yuv: *mut u16, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_yuv16_dev(ctx: *mut SrCtx, d_in: *const u16, fmt: *const SrYuv16Format, n: c_int, h: c_int, w: c_int, d_out: *mut u16, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_yuv16(ctx: *mut SrCtx, input: *const u16, fmt: *const SrYuv16Format, n: c_int, h: c_int, w: c_int, out: *mut u16, members: c_uint) -> c_int;
    pub fn sr_video_create16(ctx: *mut SrCtx, fmt: *const SrYuv16Format, h: c_int, w: c_int, slots: c_int, members: c_uint, out: *mut *mut SrVideo) -> c_int;
    pub fn sr_resize_to_yuv(ctx: *mut SrCtx, rgb: *const f32, fmt: *const SrYuvFormat, n: c_int, h: c_int, w: c_int, out: *mut u8, oh: c_int, ow: c_int, filter: c_int, flags: c_uint) -> c_int;
    pub fn sr_resize_to_yuv16(ctx: *mut SrCtx, rgb: *const f32, fmt: *const SrYuv16Format, n: c_int, h: c_int, w: c_int, out: *mut u16, oh: c_int, ow: c_int, filter: c_int, flags: c_uint) -> c_int;
    pub fn sr_upscale_yuv_sized(ctx: *mut SrCtx, input: *const u8, fmt: *const SrYuvFormat, n: c_int, h: c_int, w: c_int, out: *mut u8, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, members: c_uint) -> c_int;
    pub fn sr_upscale_yuv16_sized(ctx: *mut SrCtx, input: *const u16, fmt: *const SrYuv16Format, n: c_int, h: c_int, w: c_int, out: *mut u16, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, members: c_uint) -> c_int;
    pub fn sr_video_create_sized(ctx: *mut SrCtx, fmt: *const SrYuvFormat, h: c_int, w: c_int, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, slots: c_int, members: c_uint, out: *mut *mut SrVideo) -> c_int;
    pub fn sr_video_create16_sized(ctx: *mut SrCtx, fmt: *const SrYuv16Format, h: c_int, w: c_int, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, slots: c_int, members: c_uint, out: *mut *mut SrVideo) -> c_int;
    pub fn sr_u16_to_f32_dev(ctx: *mut SrCtx, d_in: *const u16, in_channels: c_int, n: c_int, h: c_int, w: c_int, d_out: *mut f32, stream: *mut c_void) -> c_int;
    pub fn sr_f32_to_u16_dev(ctx: *mut SrCtx, d_in: *const f32, n: c_int, h: c_int, w: c_int, d_out: *mut u16, out_channels: c_int, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_u16_dev(ctx: *mut SrCtx, d_in: *const u16, in_channels: c_int, n: c_int, h: c_int, w: c_int, d_out: *mut u16, out_channels: c_int, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_u16(ctx: *mut SrCtx, input: *const u16, in_channels: c_int, n: c_int, h: c_int, w: c_int, out: *mut u16, out_channels: c_int, members: c_uint) -> c_int;
    pub fn sr_upscale_u16_border_dev(ctx: *mut SrCtx, d_in: *const u16, in_channels: c_int, n: c_int, h: c_int, w: c_int, d_out: *mut u16, out_channels: c_int, mode: c_int, pad: c_int, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_u16_border(ctx: *mut SrCtx, input: *const u16, in_channels: c_int, n: c_int, h: c_int, w: c_int, out: *mut u16, out_channels: c_int, mode: c_int, pad: c_int, members: c_uint) -> c_int;
    pub fn sr_upscale_u16_sized_dev(ctx: *mut SrCtx, d_in: *const u16, in_channels: c_int, n: c_int, h: c_int, w: c_int, d_out: *mut u16, out_channels: c_int, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, members: c_uint, stream: *mut c_void) -> c_int;
    pub fn sr_upscale_u16_sized(ctx: *mut SrCtx, input: *const u16, in_channels: c_int, n: c_int, h: c_int, w: c_int, out: *mut u16, out_channels: c_int, oh: c_int, ow: c_int, filter: c_int, flags: c_uint, members: c_uint) -> c_int;
    pub fn sr_set_loss(ctx: *mut SrCtx, kind: c_int, eps: f32) -> c_int;
    pub fn sr_get_loss(ctx: *mut SrCtx, kind: *mut c_int, eps: *mut f32) -> c_int;
    pub fn sr_grad_norm_dev(ctx: *mut SrCtx, d_grad: *const f32, n: usize, clip: f32, d_out: *mut SrGradNorm, stream: *mut c_void) -> c_int;
    pub fn sr_adam_step_clipped_dev(ctx: *mut SrCtx, d_params: *mut f32, d_m: *mut f32, d_v: *mut f32, d_grad: *const f32, n: usize, step: c_int, lr: f32, beta1: f32, beta2: f32, eps: f32, d_norm: *const SrGradNorm, d_ema: *mut f32, ema_decay: f32, d_skipped: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sr_lr_at(schedule: *const SrLrSchedule, step: i64, lr: *mut f32) -> c_int;
    pub fn sr_train_set_optim(t: *mut SrTrain, clip_norm: f32, ema_decay: f32) -> c_int;
    pub fn sr_train_set_lr(t: *mut SrTrain, lr: f32) -> c_int;
    pub fn sr_train_ema(t: *mut SrTrain, out: *mut f32, cap: usize) -> c_int;
    pub fn sr_train_get_state(t: *mut SrTrain, m: *mut f32, v: *mut f32, e: *mut f32, cap: usize, step: *mut i64, skipped: *mut i64) -> c_int;
    pub fn sr_train_set_state(t: *mut SrTrain, m: *const f32, v: *const f32, e: *const f32, n: usize, step: i64, skipped: i64) -> c_int;
    pub fn sr_train_sync_stats(t: *mut SrTrain, stats: *mut SrTrainStat, cap: usize, n_steps: *mut usize) -> c_int;
}

/// Text of an `sr_status`; for SR_E_PARAM_COUNT / SR_E_BYTEVEC it is the reference's own panic text.
pub fn strerror(rc: c_int) -> String {
    unsafe { CStr::from_ptr(sr_strerror(rc)) }.to_string_lossy().into_owned()
}

/// `<Vec<f32>>::decode::<u32>(&bytes)` of the reference, through the library's parser.
pub fn rsr_decode(blob: &[u8]) -> Result<Vec<f32>, String> {
    let mut n = 0usize;
    let rc = unsafe { sr_rsr_decode(blob.as_ptr(), blob.len(), ptr::null_mut(), 0, &mut n) };
    if rc != SR_OK {
        return Err(strerror(rc));
    }
    let mut out = vec![0f32; n];
    let rc = unsafe { sr_rsr_decode(blob.as_ptr(), blob.len(), out.as_mut_ptr(), n, &mut n) };
    if rc != SR_OK {
        return Err(strerror(rc));
    }
    Ok(out)
}

/// 128 opaque bytes of ncclGetUniqueId for `Engine::comm_init_rank` (rank 0 only).
pub fn comm_unique_id() -> Result<Vec<u8>, String> {
    let mut id = vec![0u8; SR_COMM_ID_BYTES as usize];
    let rc = unsafe { sr_comm_unique_id(id.as_mut_ptr(), id.len()) };
    if rc == SR_OK { Ok(id) } else { Err(strerror(rc)) }
}

/// Owning handle of one engine context: a graph, its parameters, one GPU.
pub struct Engine {
    ctx: *mut SrCtx,
    graph: c_int,
}

impl Engine {
    pub fn new(graph: c_int, params: &[f32], device: c_int) -> Result<Engine, String> {
        let mut ctx = ptr::null_mut();
        let p = if params.is_empty() { ptr::null() } else { params.as_ptr() };
        let rc = unsafe { sr_create_graph(&mut ctx, graph, p, params.len(), SR_FACTOR, device) };
        if rc != SR_OK {
            return Err(strerror(rc));
        }
        Ok(Engine { ctx: ctx, graph: graph })
    }

    /// An sr_net context at factor 2, 3 or 4 (the parameter count must be sr_num_params_factor(factor)).
    pub fn new_factor(params: &[f32], factor: c_int, device: c_int) -> Result<Engine, String> {
        let mut ctx = ptr::null_mut();
        let rc = unsafe { sr_create(&mut ctx, params.as_ptr(), params.len(), factor, device) };
        if rc != SR_OK {
            return Err(strerror(rc));
        }
        Ok(Engine { ctx: ctx, graph: SR_GRAPH_SR_NET })
    }

    /// The validation pass of the reference's `train` (main.rs:220-247) on one RGBA8 HR image: (err_sum, n_elems).
    pub fn validation_error(&mut self, rgba: &[u8], w: u32, h: u32, linear_loss: bool) -> Result<(f64, usize), String> {
        assert_eq!(rgba.len(), w as usize * h as usize * 4);
        let (mut err, mut n) = (0f64, 0usize);
        let rc = unsafe {
            sr_validation_error_rgba8(self.ctx, rgba.as_ptr(), 4, h as c_int, w as c_int, linear_loss as c_int, &mut err, &mut n)
        };
        if rc == SR_OK { Ok((err, n)) } else { Err(strerror(rc)) }
    }

    /// `validation_error` with the benchmark protocol's scores of the same run (sr_pool_validation_metrics_rgba8): shave -1 = the factor.
    pub fn validation_metrics(&mut self, rgba: &[u8], w: u32, h: u32, linear_loss: bool, members: c_uint, shave: c_int)
                              -> Result<(f64, usize, SrMetrics), String> {
        assert_eq!(rgba.len(), w as usize * h as usize * 4);
        let (mut err, mut n, mut m) = (0f64, 0usize, SrMetrics::default());
        let rc = unsafe {
            sr_pool_validation_metrics_rgba8(self.ctx, rgba.as_ptr(), 4, h as c_int, w as c_int, linear_loss as c_int, members, shave, &mut err,
                                        &mut n, &mut m)
        };
        if rc == SR_OK { Ok((err, n, m)) } else { Err(strerror(rc)) }
    }

    pub fn set_precision(&mut self, mode: c_int) -> Result<(), String> {
        let rc = unsafe { sr_set_precision(self.ctx, mode) };
        if rc == SR_OK { Ok(()) } else { Err(strerror(rc)) }
    }

    /// The objective of every backward pass queued on this context from now on (SR_LOSS_*; eps: Charbonnier's, 0 < eps <= 1).
    pub fn set_loss(&mut self, kind: c_int, eps: f32) -> Result<(), String> {
        let rc = unsafe { sr_set_loss(self.ctx, kind, eps) };
        if rc == SR_OK { Ok(()) } else { Err(strerror(rc)) }
    }

    /// Output (width, height) for an input of (w, h): x3, or /3 for the downsample graph.
    pub fn out_dims(&self, w: u32, h: u32) -> (u32, u32) {
        if self.graph == SR_GRAPH_DOWNSAMPLE { (w / 3, h / 3) } else { (w * 3, h * 3) }
    }

    /// img_to_data + graph.forward + data_to_img(..).to_rgba() in one device pass.
    pub fn upscale_rgba8(&mut self, rgba: &[u8], w: u32, h: u32) -> Result<Vec<u8>, String> {
        assert_eq!(rgba.len(), w as usize * h as usize * 4);
        let (ow, oh) = self.out_dims(w, h);
        let mut out = vec![0u8; ow as usize * oh as usize * 4];
        let rc = unsafe { sr_upscale_rgba8(self.ctx, rgba.as_ptr(), 4, 1, h as c_int, w as c_int, out.as_mut_ptr()) };
        if rc == SR_OK {
            Ok(out)
        } else if rc == SR_E_HIP {
            Err(format!("{} (hipError {})", strerror(rc), unsafe { sr_last_hip_error(self.ctx) }))
        } else {
            Err(strerror(rc))
        }
    }

    /// `upscale_rgba8` that keeps the alpha channel (sr_upscale_rgba8_alpha): the colours are bled `bleed` pixels under the transparent
    /// area, the bled image is upscaled, and the interpolated alpha of `rgba` is written into the result.
    pub fn upscale_rgba8_alpha(&mut self, rgba: &[u8], w: u32, h: u32, bleed: c_int) -> Result<Vec<u8>, String> {
        assert_eq!(rgba.len(), w as usize * h as usize * 4);
        let (ow, oh) = self.out_dims(w, h);
        let mut out = vec![0u8; ow as usize * oh as usize * 4];
        let rc = unsafe { sr_upscale_rgba8_alpha(self.ctx, rgba.as_ptr(), 1, h as c_int, w as c_int, out.as_mut_ptr(), bleed, 1) };
        if rc == SR_OK {
            Ok(out)
        } else if rc == SR_E_HIP {
            Err(format!("{} (hipError {})", strerror(rc), unsafe { sr_last_hip_error(self.ctx) }))
        } else {
            Err(strerror(rc))
        }
    }

    /// Same seam as the reference's `graph.forward(1, vec![input], &params)`: NHWC f32 in and out.
    pub fn forward_f32(&mut self, values: &[f32], w: u32, h: u32) -> Result<Vec<f32>, String> {
        assert_eq!(values.len(), w as usize * h as usize * 3);
        let (ow, oh) = self.out_dims(w, h);
        let mut out = vec![0f32; ow as usize * oh as usize * 3];
        let rc = unsafe { sr_upscale_f32(self.ctx, values.as_ptr(), 1, h as c_int, w as c_int, out.as_mut_ptr()) };
        if rc == SR_OK { Ok(out) } else { Err(strerror(rc)) }
    }

    /// One image over several GPUs of this process: image (w x h, RGBA) split into `engines.len()` row shares, one per
    /// engine / device, halo rows read from `rgba` itself (sr_upscale_rgba8_multi).
    pub fn upscale_rgba8_multi(engines: &mut [Engine], rgba: &[u8], w: u32, h: u32) -> Result<Vec<u8>, String> {
        assert_eq!(rgba.len(), w as usize * h as usize * 4);
        let ctxs: Vec<*mut SrCtx> = engines.iter().map(|e| e.ctx).collect();
        let mut out = vec![0u8; w as usize * 3 * h as usize * 3 * 4];
        let rc = unsafe {
            sr_upscale_rgba8_multi(ctxs.as_ptr(), ctxs.len() as c_int, rgba.as_ptr(), 4, h as c_int, w as c_int, out.as_mut_ptr())
        };
        if rc == SR_OK { Ok(out) } else { Err(strerror(rc)) }
    }

    /// A batch dealt round-robin (image i -> engine i mod N), one host thread per engine inside the library.
    pub fn upscale_rgba8_batch_multi(engines: &mut [Engine], rgba: &[u8], n: u32, w: u32, h: u32) -> Result<Vec<u8>, String> {
        assert_eq!(rgba.len(), n as usize * w as usize * h as usize * 4);
        let ctxs: Vec<*mut SrCtx> = engines.iter().map(|e| e.ctx).collect();
        let mut out = vec![0u8; n as usize * w as usize * 3 * h as usize * 3 * 4];
        let rc = unsafe {
            sr_upscale_rgba8_batch_multi(ctxs.as_ptr(), ctxs.len() as c_int, rgba.as_ptr(), 4, n as c_int, h as c_int, w as c_int,
                                         out.as_mut_ptr())
        };
        if rc == SR_OK { Ok(out) } else { Err(strerror(rc)) }
    }

    /// One process per GPU: join the band communicator.  Rank 0 obtains `id` from `comm_unique_id()` and hands it to
    /// the other ranks (file, socket, environment) before every rank calls this.
    pub fn comm_init_rank(&mut self, id: &[u8], rank: c_int, nranks: c_int) -> Result<(), String> {
        let rc = unsafe { sr_comm_init_rank(self.ctx, id.as_ptr(), id.len(), rank, nranks) };
        if rc == SR_OK { Ok(()) } else { Err(format!("{} (ncclResult {})", strerror(rc), unsafe { sr_last_comm_error(self.ctx) })) }
    }

    pub fn last_timing(&mut self) -> (f64, f64, f64) {
        let (mut total, mut h2d, mut d2h) = (0f64, 0f64, 0f64);
        unsafe { sr_last_timing(self.ctx, &mut total, ptr::null_mut(), &mut h2d, &mut d2h) };
        (total, h2d, d2h)
    }
}

impl Drop for Engine {
    fn drop(&mut self) {
        unsafe { sr_destroy(self.ctx) }
    }
}
