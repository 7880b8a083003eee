"""ctypes binding of libsrhip.so (include/srhip.h).  There is no fallback: if
the HIP library is missing or cannot be loaded every engine entry point raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRHIP_LIB", os.path.join(HERE, "libsrhip.so"))  # override: A/B kernel experiments

SR_FACTOR = 3
SR_NUM_PARAMS = 130459
SR_HALO = 7

SR_OK, SR_E_INVALID, SR_E_PARAM_COUNT, SR_E_FACTOR, SR_E_NO_DEVICE = 0, -1, -2, -3, -4
SR_E_HIP, SR_E_NOMEM, SR_E_BYTEVEC, SR_E_HALO, SR_E_COMM, SR_E_DOMAIN = -5, -6, -7, -8, -9, -10
SR_COMM_ID_BYTES = 128
SR_PRECISION_F32, SR_PRECISION_SPLIT_F16 = 0, 1
SR_GRAPH_SR_NET, SR_GRAPH_BILINEAR, SR_GRAPH_DOWNSAMPLE = 0, 1, 2
SR_TRAIN_STORE_AUTO = (1 << (8 * C.sizeof(C.c_size_t))) - 1
SR_TRAIN_MAX_BATCH = 64
SR_TRAIN_RING = 64
SR_ENSEMBLE_ALL, SR_ENSEMBLE_FLIPS, SR_ENSEMBLE_HFLIP = 0xFF, 0x0F, 0x03
SR_ALPHA_BLEED_DEFAULT, SR_ALPHA_BLEED_MAX = 8, 16
SR_ALPHA_BLEED_TILE = 32  # side of the bleed kernel's output tile (the tests put sizes on and across its seams)
SR_FILTER_BOX, SR_FILTER_TRIANGLE, SR_FILTER_CATROM, SR_FILTER_LANCZOS3 = 0, 1, 2, 3
SR_PIXELS_RGBA8, SR_PIXELS_F32 = 0, 1
SR_RESIZE_SRGB_SPACE = 1
SR_DEGRADE_MAX_SIGMA, SR_DEGRADE_MAX_NOISE = 4, 64
SR_BORDER_WRAP, SR_BORDER_REPLICATE, SR_BORDER_MIRROR = 1, 2, 3
SR_BORDER_PAD_DEFAULT, SR_BORDER_PAD_MAX = 8, 32
SR_YUV_420, SR_YUV_444 = 0, 1
SR_YUV_422, SR_YUV_BT2020 = 2, 2  # valid in sr_yuv16_format (Yuv16Format) only
SR_YUV_SITING_CENTER, SR_YUV_SITING_LEFT = 0, 1
SR_YUV_BT601, SR_YUV_BT709 = 0, 1
SR_YUV_LIMITED, SR_YUV_FULL = 0, 1
SR_VIDEO_REUSE_OFF, SR_VIDEO_REUSE_ROWS = 0, 1
SR_REUSE_MAX_BANDS = 4
SR_YUV_SPAN = 1024  # luma columns a workgroup of either conversion takes, two rows at a time (the tests put widths either side of it)
SR_DEEP_SPAN = 2048  # pixels a workgroup of either deep-colour conversion takes, 8 a lane (the tests put counts either side of it)
SR_LOSS_MSE, SR_LOSS_L1, SR_LOSS_CHARBONNIER = 0, 1, 2
SR_LR_CONSTANT, SR_LR_STEP, SR_LR_COSINE = 0, 1, 2
SR_METRICS_TILE = 32  # side of the metrics kernel's tile of region pixels (the tests put sizes either side of its multiples)


class TrainCrop(C.Structure):
    """sr_train_crop (include/srhip.h): a resident image id, or -1 and host pixels; the crop origin."""
    _fields_ = [("image", C.c_int), ("px", C.c_void_p), ("in_channels", C.c_int), ("h", C.c_int), ("w", C.c_int),
                ("y0", C.c_int), ("x0", C.c_int)]


class TrainPairCrop(C.Structure):
    """sr_train_pair_crop (include/srhip.h): a resident pair id, or -1 and both images' host pixels; the crop origin in LR pixels."""
    _fields_ = [("pair", C.c_int), ("lr_px", C.c_void_p), ("hr_px", C.c_void_p), ("lr_channels", C.c_int), ("hr_channels", C.c_int),
                ("lh", C.c_int), ("lw", C.c_int), ("y0", C.c_int), ("x0", C.c_int)]


class Degrade(C.Structure):
    """sr_degrade (include/srhip.h): one item's blur width, noise level, JPEG quality and noise seed."""
    _fields_ = [("sigma", C.c_float), ("noise", C.c_float), ("quality", C.c_int), ("seed", C.c_uint64)]


class Metrics(C.Structure):
    """sr_metrics (include/srhip.h): the sums and counts the Y-PSNR and the SSIM of one image are made of."""
    _fields_ = [("y_sq_err", C.c_uint64), ("y_count", C.c_uint64), ("ssim_sum", C.c_double), ("ssim_count", C.c_uint64)]


class GradNorm(C.Structure):
    """sr_grad_norm (include/srhip.h "Optimiser"): the gradient's sum of squares, the clipping scale and the skip flag."""
    _fields_ = [("sumsq", C.c_double), ("scale", C.c_float), ("skip", C.c_int32)]


class TrainStat(C.Structure):
    """sr_train_stat (include/srhip.h "Optimiser"): one step's err_sum, gradient norm, learning rate and clipping scale."""
    _fields_ = [("err_sum", C.c_double), ("grad_norm", C.c_double), ("lr", C.c_float), ("scale", C.c_float)]


class LrSchedule(C.Structure):
    """sr_lr_schedule (include/srhip.h "Optimiser"): kind, base rate, warm-up steps and the kind's own fields."""
    _fields_ = [("kind", C.c_int), ("base", C.c_float), ("warmup", C.c_longlong), ("every", C.c_longlong), ("gamma", C.c_double),
                ("total", C.c_longlong), ("min_lr", C.c_float)]


class YuvFormat(C.Structure):
    """sr_yuv_format (include/srhip.h "Video"): subsampling, chroma siting, matrix and range of a planar 8-bit YCbCr frame.  The fields
    take the SR_YUV_* numbers; YuvFormat.named("420", "left", "bt709", "limited") takes the names."""
    _fields_ = [("subsampling", C.c_int32), ("siting", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32)]
    SUBSAMPLINGS = {"420": SR_YUV_420, "444": SR_YUV_444}
    SITINGS = {"center": SR_YUV_SITING_CENTER, "left": SR_YUV_SITING_LEFT}
    MATRICES = {"bt601": SR_YUV_BT601, "bt709": SR_YUV_BT709}
    RANGES = {"limited": SR_YUV_LIMITED, "full": SR_YUV_FULL}

    @classmethod
    def named(cls, subsampling="420", siting="center", matrix="bt601", range="limited"):
        return cls(cls.SUBSAMPLINGS[subsampling], cls.SITINGS[siting], cls.MATRICES[matrix], cls.RANGES[range])


class Yuv16Format(C.Structure):
    """sr_yuv16_format (include/srhip.h "Deep video"): a planar YCbCr frame of 9..16-bit samples in little-endian uint16.  The fields take
    the SR_YUV_* numbers and the depth; Yuv16Format.named("422", "left", "bt2020", "limited", 10) takes the names."""
    _fields_ = [("subsampling", C.c_int32), ("siting", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32), ("depth", C.c_int32)]
    SUBSAMPLINGS = {"420": SR_YUV_420, "422": SR_YUV_422, "444": SR_YUV_444}
    SITINGS = YuvFormat.SITINGS
    MATRICES = {"bt601": SR_YUV_BT601, "bt709": SR_YUV_BT709, "bt2020": SR_YUV_BT2020}
    RANGES = YuvFormat.RANGES

    @classmethod
    def named(cls, subsampling="420", siting="left", matrix="bt709", range="limited", depth=10):
        return cls(cls.SUBSAMPLINGS[subsampling], cls.SITINGS[siting], cls.MATRICES[matrix], cls.RANGES[range], int(depth))


class RowBand(C.Structure):
    """sr_row_band (include/srhip.h "Video"): LR rows [y0, y1) a frame computes."""
    _fields_ = [("y0", C.c_int32), ("y1", C.c_int32)]


class VideoReuseStats(C.Structure):
    """sr_video_reuse_stats (include/srhip.h "Video"): what a session's row reuse has computed and what it has taken over."""
    _fields_ = [(name, C.c_uint64) for name in ("frames", "frames_reused", "frames_partial", "frames_full", "rows_total", "rows_computed", "bands")]


# every symbol include/srhip.h declares: (restype, argtypes)
_vp, _fp, _u8p, _dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
_sz, _i = C.c_size_t, C.c_int
_u16p = C.POINTER(C.c_uint16)
SYMBOLS = {
    "sr_rsr_decode": (_i, [_u8p, _sz, _fp, _sz, C.POINTER(_sz)]),
    "sr_rsr_encode": (_i, [_fp, _sz, _u8p, _sz, C.POINTER(_sz)]),
    "sr_create": (_i, [C.POINTER(_vp), _fp, _sz, _i, _i]),
    "sr_create_graph": (_i, [C.POINTER(_vp), _i, _fp, _sz, _i, _i]),
    "sr_num_params": (_i, [_i]),
    "sr_num_params_factor": (_i, [_i]),
    "sr_destroy": (None, [_vp]),
    "sr_upscale_f32": (_i, [_vp, _fp, _i, _i, _i, _fp]),
    "sr_upscale_rgba8": (_i, [_vp, _u8p, _i, _i, _i, _i, _u8p]),
    "sr_reserve_f32": (_i, [_vp, _i, _i, _i]),
    "sr_reserve_rgba8": (_i, [_vp, _i, _i, _i, _i]),
    "sr_upscale_f32_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sr_upscale_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sr_upscale_band_f32_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sr_upscale_band_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "sr_read_feature": (_i, [_vp, _i, _fp, _sz]),
    "sr_set_precision": (_i, [_vp, _i]),
    "sr_check_domain": (_i, [_vp]),
    "sr_upscale_f32_multi": (_i, [C.POINTER(_vp), _i, _fp, _i, _i, _fp]),
    "sr_upscale_rgba8_multi": (_i, [C.POINTER(_vp), _i, _u8p, _i, _i, _i, _u8p]),
    "sr_upscale_f32_batch_multi": (_i, [C.POINTER(_vp), _i, _fp, _i, _i, _i, _fp]),
    "sr_upscale_rgba8_batch_multi": (_i, [C.POINTER(_vp), _i, _u8p, _i, _i, _i, _i, _u8p]),
    "sr_comm_available": (_i, []),
    "sr_comm_unique_id": (_i, [_u8p, _sz]),
    "sr_comm_init_rank": (_i, [_vp, _u8p, _sz, _i, _i]),
    "sr_comm_init_all": (_i, [C.POINTER(_vp), _i]),
    "sr_comm_init_local": (_i, [C.POINTER(_vp), _i]),
    "sr_comm_destroy": (None, [_vp]),
    "sr_comm_rank": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "sr_last_comm_error": (_i, [_vp]),
    "sr_last_comm_ms": (_i, [_vp, _dp]),
    "sr_last_comm_exposed_ms": (_i, [_vp, _dp]),
    "sr_upscale_sharded_f32_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "sr_upscale_sharded_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sr_upscale_sharded_f32_all": (_i, [C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(_i), _i, C.POINTER(_vp)]),
    "sr_upscale_sharded_rgba8_all": (_i, [C.POINTER(_vp), _i, C.POINTER(_vp), _i, C.POINTER(_i), _i, C.POINTER(_vp)]),
    "sr_set_pipeline": (_i, [_vp, _i]),
    "sr_host_alloc": (_i, [C.POINTER(_vp), _sz]),
    "sr_host_free": (None, [_vp]),
    "sr_set_profiling": (_i, [_vp, _i]),
    "sr_last_timing": (_i, [_vp, _dp, _dp, _dp, _dp]),
    "sr_device_info": (_i, [_vp, C.c_char_p, _sz, C.POINTER(_i), C.POINTER(_i)]),
    "sr_last_hip_error": (_i, [_vp]),
    "sr_strerror": (C.c_char_p, [_i]),
    "sr_validation_error_rgba8": (_i, [_vp, _u8p, _i, _i, _i, _i, _dp, C.POINTER(_sz)]),
    "sr_validation_error_f32": (_i, [_vp, _fp, _i, _i, _i, _dp, C.POINTER(_sz)]),
    "sr_validation_error_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sr_read_validation_nodes": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "sr_backprop_f32": (_i, [_vp, _fp, _sz, _fp, _i, _i, _i, _i, C.c_float, C.c_float, _dp, C.POINTER(_sz), _fp]),
    "sr_backprop_rgba8": (_i, [_vp, _fp, _sz, _u8p, _i, _i, _i, _i, _i, C.c_float, C.c_float, _dp, C.POINTER(_sz), _fp]),
    "sr_backprop_rgba8_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_float, C.c_float, _vp, _vp, _vp]),
    "sr_adam_step_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, C.c_float, C.c_float, C.c_float, C.c_float, _vp]),
    "sr_init_params": (_i, [_i, C.c_uint64, _fp, _sz]),
    "sr_set_params": (_i, [_vp, _fp, _sz]),
    "sr_train_create": (_i, [C.POINTER(_vp), _vp, _fp, _sz, _i, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _sz]),
    "sr_train_add_image": (_i, [_vp, _u8p, _i, _i, _i, C.POINTER(_i)]),
    "sr_train_step": (_i, [_vp, C.POINTER(TrainCrop), _i, _i, _i]),
    "sr_train_step_aug": (_i, [_vp, C.POINTER(TrainCrop), _u8p, _i, _i, _i]),
    "sr_train_sync": (_i, [_vp, _dp, _sz, C.POINTER(_sz)]),
    "sr_train_params": (_i, [_vp, _fp, _sz]),
    "sr_train_destroy": (None, [_vp]),
    "sr_pair_validation_error_rgba8": (_i, [_vp, _u8p, _i, _u8p, _i, _i, _i, _i, _dp, C.POINTER(_sz)]),
    "sr_pair_validation_error_f32": (_i, [_vp, _fp, _fp, _i, _i, _i, _dp, C.POINTER(_sz)]),
    "sr_pair_validation_error_rgba8_dev": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sr_pair_backprop_f32": (_i, [_vp, _fp, _sz, _fp, _fp, _i, _i, _i, _i, C.c_float, C.c_float, _dp, C.POINTER(_sz), _fp]),
    "sr_pair_backprop_rgba8": (_i, [_vp, _fp, _sz, _u8p, _i, _u8p, _i, _i, _i, _i, _i, C.c_float, C.c_float, _dp, C.POINTER(_sz), _fp]),
    "sr_pair_backprop_rgba8_dev": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, C.c_float, C.c_float, _vp, _vp, _vp]),
    "sr_train_add_pair": (_i, [_vp, _u8p, _i, _u8p, _i, _i, _i, C.POINTER(_i)]),
    "sr_train_step_pairs": (_i, [_vp, C.POINTER(TrainPairCrop), _i, _i, _i]),
    "sr_train_step_pairs_aug": (_i, [_vp, C.POINTER(TrainPairCrop), _u8p, _i, _i, _i]),
    "sr_upscale_ensemble_f32_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, C.c_uint, _vp]),
    "sr_upscale_ensemble_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, C.c_uint, _vp]),
    "sr_upscale_ensemble_f32": (_i, [_vp, _fp, _i, _i, _i, _fp, C.c_uint]),
    "sr_upscale_ensemble_rgba8": (_i, [_vp, _u8p, _i, _i, _i, _i, _u8p, C.c_uint]),
    "sr_pool_validation_error_ensemble_rgba8": (_i, [_vp, _u8p, _i, _i, _i, _i, C.c_uint, _dp, C.POINTER(_sz)]),
    "sr_pair_validation_error_ensemble_rgba8": (_i, [_vp, _u8p, _i, _u8p, _i, _i, _i, _i, C.c_uint, _dp, C.POINTER(_sz)]),
    "sr_image_metrics_rgba8": (_i, [_vp, _u8p, _i, _u8p, _i, _i, _i, _i, C.POINTER(Metrics)]),
    "sr_image_metrics_rgba8_dev": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sr_pool_validation_metrics_rgba8": (_i, [_vp, _u8p, _i, _i, _i, _i, C.c_uint, _i, _dp, C.POINTER(_sz), C.POINTER(Metrics)]),
    "sr_pair_validation_metrics_rgba8": (_i, [_vp, _u8p, _i, _u8p, _i, _i, _i, _i, C.c_uint, _i, _dp, C.POINTER(_sz), C.POINTER(Metrics)]),
    "sr_pool_validation_metrics_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sr_pair_validation_metrics_rgba8_dev": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sr_bleed_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sr_merge_alpha_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sr_upscale_rgba8_alpha_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, C.c_uint, _vp]),
    "sr_upscale_rgba8_alpha": (_i, [_vp, _u8p, _i, _i, _i, _u8p, _i, C.c_uint]),
    "sr_resize_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, C.c_uint, _vp]),
    "sr_resize_rgba8": (_i, [_vp, _u8p, _i, _i, _i, _u8p, _i, _i, _i, C.c_uint]),
    "sr_upscale_rgba8_sized_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _i, C.c_uint, C.c_uint, _vp]),
    "sr_upscale_rgba8_sized": (_i, [_vp, _u8p, _i, _i, _i, _u8p, _i, _i, _i, C.c_uint, C.c_uint]),
    "sr_degrade_rgba8": (_i, [_vp, _u8p, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(Degrade), _u8p]),
    "sr_degrade_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(Degrade), _vp, _vp]),
    "sr_train_step_degrade": (_i, [_vp, C.POINTER(TrainCrop), _u8p, C.POINTER(Degrade), _i, _i, _i]),
    "sr_pad_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "sr_pad_f32_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "sr_crop_rgba8_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sr_crop_f32_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sr_upscale_rgba8_border_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, C.c_uint, _i, _vp]),
    "sr_upscale_f32_border_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, C.c_uint, _vp]),
    "sr_upscale_rgba8_border": (_i, [_vp, _u8p, _i, _i, _i, _u8p, _i, _i, C.c_uint, _i]),
    "sr_upscale_f32_border": (_i, [_vp, _fp, _i, _i, _i, _fp, _i, _i, C.c_uint]),
    "sr_yuv_frame_bytes": (_sz, [C.POINTER(YuvFormat), _i, _i]),
    "sr_yuv_to_rgb_dev": (_i, [_vp, _vp, C.POINTER(YuvFormat), _i, _i, _i, _vp, _vp]),
    "sr_rgb_to_yuv_dev": (_i, [_vp, _vp, C.POINTER(YuvFormat), _i, _i, _i, _vp, _vp]),
    "sr_upscale_yuv_dev": (_i, [_vp, _vp, C.POINTER(YuvFormat), _i, _i, _i, _vp, C.c_uint, _vp]),
    "sr_upscale_yuv": (_i, [_vp, _u8p, C.POINTER(YuvFormat), _i, _i, _i, _u8p, C.c_uint]),
    "sr_video_create": (_i, [_vp, C.POINTER(YuvFormat), _i, _i, _i, C.c_uint, C.POINTER(_vp)]),
    "sr_video_acquire": (_i, [_vp, C.POINTER(_vp)]),
    "sr_video_submit": (_i, [_vp]),
    "sr_video_receive": (_i, [_vp, C.POINTER(_vp)]),
    "sr_video_pending": (_i, [_vp]),
    "sr_video_destroy": (None, [_vp]),
    "sr_rows_differ_dev": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "sr_video_reuse_plan": (_i, [C.POINTER(C.c_uint32), _i, _i, C.POINTER(RowBand), _i, C.POINTER(_i)]),
    "sr_video_set_reuse": (_i, [_vp, _i]),
    "sr_video_get_reuse_stats": (_i, [_vp, C.POINTER(VideoReuseStats)]),
    "sr_yuv16_frame_bytes": (_sz, [C.POINTER(Yuv16Format), _i, _i]),
    "sr_yuv16_to_rgb_dev": (_i, [_vp, _vp, C.POINTER(Yuv16Format), _i, _i, _i, _vp, _vp]),
    "sr_rgb_to_yuv16_dev": (_i, [_vp, _vp, C.POINTER(Yuv16Format), _i, _i, _i, _vp, _vp]),
    "sr_upscale_yuv16_dev": (_i, [_vp, _vp, C.POINTER(Yuv16Format), _i, _i, _i, _vp, C.c_uint, _vp]),
    "sr_upscale_yuv16": (_i, [_vp, _u16p, C.POINTER(Yuv16Format), _i, _i, _i, _u16p, C.c_uint]),
    "sr_video_create16": (_i, [_vp, C.POINTER(Yuv16Format), _i, _i, _i, C.c_uint, C.POINTER(_vp)]),
    "sr_resize_to_yuv": (_i, [_vp, _vp, C.POINTER(YuvFormat), _i, _i, _i, _u8p, _i, _i, _i, C.c_uint]),
    "sr_resize_to_yuv16": (_i, [_vp, _vp, C.POINTER(Yuv16Format), _i, _i, _i, _u16p, _i, _i, _i, C.c_uint]),
    "sr_upscale_yuv_sized": (_i, [_vp, _u8p, C.POINTER(YuvFormat), _i, _i, _i, _u8p, _i, _i, _i, C.c_uint, C.c_uint]),
    "sr_upscale_yuv16_sized": (_i, [_vp, _u16p, C.POINTER(Yuv16Format), _i, _i, _i, _u16p, _i, _i, _i, C.c_uint, C.c_uint]),
    "sr_video_create_sized": (_i, [_vp, C.POINTER(YuvFormat), _i, _i, _i, _i, _i, C.c_uint, _i, C.c_uint, C.POINTER(_vp)]),
    "sr_video_create16_sized": (_i, [_vp, C.POINTER(Yuv16Format), _i, _i, _i, _i, _i, C.c_uint, _i, C.c_uint, C.POINTER(_vp)]),
    "sr_u16_to_f32_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sr_f32_to_u16_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "sr_upscale_u16_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, C.c_uint, _vp]),
    "sr_upscale_u16": (_i, [_vp, _u16p, _i, _i, _i, _i, _u16p, _i, C.c_uint]),
    "sr_upscale_u16_border_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, C.c_uint, _vp]),
    "sr_upscale_u16_border": (_i, [_vp, _u16p, _i, _i, _i, _i, _u16p, _i, _i, _i, C.c_uint]),
    "sr_upscale_u16_sized_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, C.c_uint, C.c_uint, _vp]),
    "sr_upscale_u16_sized": (_i, [_vp, _u16p, _i, _i, _i, _i, _u16p, _i, _i, _i, _i, C.c_uint, C.c_uint]),
    "sr_set_loss": (_i, [_vp, _i, C.c_float]),
    "sr_get_loss": (_i, [_vp, C.POINTER(_i), _fp]),
    "sr_grad_norm_dev": (_i, [_vp, _vp, _sz, C.c_float, _vp, _vp]),
    "sr_adam_step_clipped_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, C.c_float, _vp, _vp]),
    "sr_lr_at": (_i, [C.POINTER(LrSchedule), C.c_longlong, _fp]),
    "sr_train_set_optim": (_i, [_vp, C.c_float, C.c_float]),
    "sr_train_set_lr": (_i, [_vp, C.c_float]),
    "sr_train_ema": (_i, [_vp, _fp, _sz]),
    "sr_train_get_state": (_i, [_vp, _fp, _fp, _fp, _sz, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "sr_train_set_state": (_i, [_vp, _fp, _fp, _fp, _sz, C.c_longlong, C.c_longlong]),
    "sr_train_sync_stats": (_i, [_vp, C.POINTER(TrainStat), _sz, C.POINTER(_sz)]),
}

# include/srhip_experimental.h: A/B tuning switches (no result bit depends on them), outside the drop-in ABI
EXPERIMENTAL = {
    "sr_set_experiment": (_i, [_vp, C.c_char_p, C.c_char_p]),
    "sr_get_experiment": (_i, [_vp, C.c_char_p, C.c_char_p, _sz]),
}

_lib = None


class SrError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = lib().sr_strerror(status).decode() if _lib is not None else f"status {status}"
        super().__init__(f"{msg}{(' (' + detail + ')') if detail else ''}")


def lib():
    """Load libsrhip.so (built in-tree by rusty_sr_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m rusty_sr_amd.build` "
                "(hipcc --offload-arch=gfx950). rusty_sr_amd has no CPU fallback.")
        # torch ships its own copy of the HIP runtime (SONAME libamdhip64.so.7, found
        # through its RPATH).  Load it FIRST so libsrhip's NEEDED libamdhip64.so.7
        # resolves to that same instance; two HIP runtimes in one process cannot
        # both own the GPU ("No HIP GPUs are available" from whichever comes second).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(EXPERIMENTAL.items()):
            f = getattr(L, name)  # AttributeError if the ABI is incomplete
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def check(status, ctx=None):
    if status != SR_OK:
        detail = ""
        if ctx and status == SR_E_HIP:
            detail = f"hipError {lib().sr_last_hip_error(ctx)}"
        if ctx and status == SR_E_COMM:
            detail = f"ncclResult {lib().sr_last_comm_error(ctx)}"
        raise SrError(status, detail)
