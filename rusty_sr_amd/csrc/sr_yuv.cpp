// sr_yuv.cpp -- the video path (include/srhip.h "Video", "Deep video"): the two colour conversions as entry points, the composed call
//     YCbCr frame -> f32 RGB -> network (sr_net_queue: the plain or the ensemble call's path) -> f32 RGB -> YCbCr frame, quantised once,
// and the frame stream, which keeps that call in flight for a ring of slots.  Kernels: sr_yuv.hip.  The composed calls are their checks,
// their sizes and a work lambda; the stream is the one thing here the scaffold has no form for: a call that returns
// before its work is done.  Frames of bytes and deep frames of uint16 samples are one path, templated on
// the sample type S; the two format structs meet in one sr_yuv_rule (sr_yuv_rule.h), and a session of either kind is one sr_video.  Row
// reuse (sr_video_set_reuse; the compare kernel: sr_reuse.hip, the planner: sr_plan.cpp) is a session's opt-in: it
// computes the row bands a changed input row can reach and takes the other rows from the last frame's output.  The sized calls and
// sessions ("Video at any size") end in the resampler's passes instead of the conversion back: the horizontal pass of
// sr_resize.hip, then the vertical pass that writes the frame (sr_resize_yuv.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sr_internal.h"

namespace {

constexpr size_t kPxF = 3 * sizeof(float);
constexpr int kSideMax = INT32_MAX / 4;  // a side of a frame the conversions take: their column arithmetic is int

// what a sample type's launches are called in the plan record, and the pixels its to-RGB line names (the kernel's input's for bytes,
// the f32 side for deep samples); its frames are aligned to alignof(S)
template <class S>
struct Ops;
template <>
struct Ops<uint8_t> {
    static constexpr const char *to_rgb = "yuv2rgb", *to_yuv = "rgb2yuv";
    static constexpr bool to_rgb_f32 = false;
};
template <>
struct Ops<uint16_t> {
    static constexpr const char *to_rgb = "yuv16_to_rgb", *to_yuv = "rgb_to_yuv16";
    static constexpr bool to_rgb_f32 = true;
};

const char* form_name(const sr_yuv_rule& k) {
    if (k.sub == SR_YUV_444) return "444";
    if (k.sub == SR_YUV_422) return k.left ? "422left" : "422center";
    return k.left ? "420left" : "420center";
}

int check_frames(int n, int h, int w) {
    return n >= 1 && h >= 1 && w >= 1 && h <= kSideMax && w <= kSideMax ? SR_OK : SR_E_INVALID;
}

template <class S>
bool sample_aligned(const void* p) { return ((uintptr_t)p & (alignof(S) - 1)) == 0; }

bool rule_make(const sr_yuv_format* f, sr_yuv_rule* k) { return sr_yuv_rule_make(f, k); }
bool rule_make(const sr_yuv16_format* f, sr_yuv_rule* k) { return sr_yuv16_rule_make(f, k); }

// either launch queued on s, with its "op" line in the plan record: the grid the launcher itself takes
template <class S>
int queue_to_rgb(sr_ctx* c, const S* d_yuv, const sr_yuv_rule& k, int n, int h, int w, float* d_rgb, hipStream_t s) {
    unsigned bx = 0, by = 0;
    if (sr_yuv_blocks(n, h, w, &bx, &by) > (size_t)INT32_MAX) return SR_E_NOMEM;
    HIPCHK(c, sr_launch_yuv_to_rgb(d_yuv, k, n, h, w, d_rgb, s));
    sr_plan_note_op(c, Ops<S>::to_rgb, Ops<S>::to_rgb_f32, n, bx, by, form_name(k));
    return SR_OK;
}

template <class S>
int queue_to_yuv(sr_ctx* c, const float* d_rgb, const sr_yuv_rule& k, int n, int h, int w, S* d_yuv, hipStream_t s) {
    unsigned bx = 0, by = 0;
    if (sr_yuv_blocks(n, h, w, &bx, &by) > (size_t)INT32_MAX) return SR_E_NOMEM;
    HIPCHK(c, sr_launch_rgb_to_yuv(d_rgb, k, n, h, w, d_yuv, s));
    sr_plan_note_op(c, Ops<S>::to_yuv, true, n, bx, by, form_name(k));
    return SR_OK;
}

// everything the composed calls and the frame stream refuse for their context, format, shape and mask alone
template <class Format>
int check_upscale_shape(const sr_ctx* c, const Format* fmt, int n, int h, int w, unsigned members, sr_yuv_rule* k) {
    SRCHK(sr_net_check_shape(c, n, h, w, members));
    if (!rule_make(fmt, k)) return SR_E_INVALID;
    if (h > kSideMax / c->factor || w > kSideMax / c->factor) return SR_E_INVALID;
    return SR_OK;
}

// ... and for their two frame pointers
template <class S, class Format>
int check_upscale_args(const sr_ctx* c, const S* in, const Format* fmt, int n, int h, int w, const S* out, unsigned members, sr_yuv_rule* k) {
    if (!in || !out || !sample_aligned<S>(in) || !sample_aligned<S>(out)) return SR_E_INVALID;
    return check_upscale_shape(c, fmt, n, h, w, members, k);
}

// to RGB -> network -> from RGB on device buffers, queued on s; the arguments are checked and the context's device is current
template <class S>
int queue_upscale(sr_ctx* c, const S* d_in, const sr_yuv_rule& k, int n, int h, int w, S* d_out, unsigned members, hipStream_t s) {
    const size_t f = (size_t)c->factor, in_img = (size_t)h * w * kPxF, out_img = f * h * f * w * kPxF;
    if (out_img / kPxF / (f * w) != f * h || out_img > SIZE_MAX / (size_t)n) return SR_E_NOMEM;
    SRCHK(sr_reserve_bufs(c, {{&c->d_yrgb, (size_t)n * in_img}, {&c->d_ynet, (size_t)n * out_img}}));
    SRCHK(sr_net_capture_ready(c, false, 3, n, h, w, members));
    SRCHK(queue_to_rgb(c, d_in, k, n, h, w, (float*)c->d_yrgb.p, s));
    SRCHK(sr_net_queue(c, c->d_yrgb.p, false, 3, n, h, w, c->d_ynet.p, false, members, s));
    return queue_to_yuv(c, (const float*)c->d_ynet.p, k, n, (int)f * h, (int)f * w, d_out, s);
}

// ---- the entry points of either sample type
template <class Format>
size_t frame_bytes(const Format* fmt, int h, int w, size_t sample) {
    sr_yuv_rule k;
    if (!rule_make(fmt, &k) || h < 1 || w < 1) return 0;
    const size_t samples = sr_yuv_rule_frame_samples(k, h, w);
    return samples > SIZE_MAX / sample ? 0 : sample * samples;
}

template <class S, class Format>
int to_rgb_dev(sr_ctx* c, const S* d_yuv, const Format* fmt, int n, int h, int w, float* d_rgb, void* stream) {
    sr_plan_clear(c);
    sr_yuv_rule k;
    if (!c || !d_yuv || !d_rgb || !rule_make(fmt, &k)) return SR_E_INVALID;
    SRCHK(check_frames(n, h, w));
    if (!sr_dword_aligned(d_rgb) || !sample_aligned<S>(d_yuv)) return SR_E_INVALID;
    return sr_on_device(c, stream, [&] { return queue_to_rgb(c, d_yuv, k, n, h, w, d_rgb, (hipStream_t)stream); });
}

template <class S, class Format>
int to_yuv_dev(sr_ctx* c, const float* d_rgb, const Format* fmt, int n, int h, int w, S* d_yuv, void* stream) {
    sr_plan_clear(c);
    sr_yuv_rule k;
    if (!c || !d_yuv || !d_rgb || !rule_make(fmt, &k)) return SR_E_INVALID;
    SRCHK(check_frames(n, h, w));
    if (!sr_dword_aligned(d_rgb) || !sample_aligned<S>(d_yuv)) return SR_E_INVALID;
    return sr_on_device(c, stream, [&] { return queue_to_yuv(c, d_rgb, k, n, h, w, d_yuv, (hipStream_t)stream); });
}

template <class S, class Format>
int upscale_dev(sr_ctx* c, const S* d_in, const Format* fmt, int n, int h, int w, S* d_out, unsigned members, void* stream) {
    sr_plan_clear(c);
    sr_yuv_rule k;
    SRCHK(check_upscale_args(c, d_in, fmt, n, h, w, (const S*)d_out, members, &k));
    return sr_on_device(c, stream, [&] { return queue_upscale(c, d_in, k, n, h, w, d_out, members, (hipStream_t)stream); });
}

template <class S, class Format>
int upscale_host(sr_ctx* c, const S* in, const Format* fmt, int n, int h, int w, S* out, unsigned members) {
    sr_plan_clear(c);
    sr_yuv_rule k;
    SRCHK(check_upscale_args(c, in, fmt, n, h, w, (const S*)out, members, &k));
    const int f = c->factor;
    const size_t in_bytes = (size_t)n * sizeof(S) * sr_yuv_rule_frame_samples(k, h, w);
    const size_t out_bytes = (size_t)n * sizeof(S) * sr_yuv_rule_frame_samples(k, f * h, f * w);
    return sr_host_image_call(c, true, in, in_bytes, out, out_bytes, [&](const void* d_in, void* d_out, hipStream_t s) {
        return queue_upscale(c, (const S*)d_in, k, n, h, w, (S*)d_out, members, s);
    });
}

// ---- video at any size (include/srhip.h "Video at any size"): the network's f32 output resampled straight to a frame.
// What the calls refuse for the final size beyond the resampler's own refusals
int check_out_size(int oh, int ow) { return oh <= kSideMax && ow <= kSideMax ? SR_OK : SR_E_INVALID; }

// Whether a format class takes the fused vertical pass (resize_v_yuv_kernel) or the chain it equals bit for bit (resize_v_kernel into
// d_yres, then rgb_to_yuv_kernel): by measurement, class by class (profiles/video_sized_rocprof_stats.csv) -- the fused
// kernel where it is not slower than the sum of the two.  At 5760x3240 -> 3840x2160 it is 0.94-0.99 x the sum on 4:4:4 and on centre-sited
// 4:2:0 / 4:2:2, bytes and deep samples alike, and 1.05-1.07 x on the left-sited forms, whose workgroups wait for one thread's second
// walk over the neighbouring column: those go by the chain.  "vyuv" overrides the rule for tests and measurements.
template <class S>
bool fused_pays(const sr_yuv_rule& k) { return !(k.left && k.sub != SR_YUV_444); }

template <class S>
bool takes_fused(const sr_ctx* c, const sr_yuv_rule& k) { return c->env_vyuv_pairs > 0 || (c->env_vyuv_pairs == 0 && fused_pays<S>(k)); }

// The workspace of a resampling to a frame of samples S (and, for the composed calls, rgb_bytes of d_yrgb and net_bytes of d_ynet beside
// it), all or nothing; a grid beyond what a launch takes is refused before an allocation is attempted.  A class that goes by the chain
// holds the resampled f32 image as well.  The context's device is current.
template <class S>
int reserve_sized(sr_ctx* c, sr_resize_job& j, const sr_yuv_rule& k, size_t rgb_bytes, size_t net_bytes) {
    if (!sr_resize_front_fits(j) || sr_resize_yuv_blocks(j.n, j.oh, j.ow, 1) > (size_t)INT32_MAX ||
        sr_resize_v_blocks(j.n, j.oh, j.ow) > (size_t)INT32_MAX)
        return SR_E_NOMEM;
    const size_t res_bytes = takes_fused<S>(c, k) ? 0 : (size_t)j.n * j.oh * j.ow * kPxF;  // (fits a size_t: sr_resize_plan)
    SRCHK(sr_reserve_bufs(c, {{&c->d_rtab, j.tab_bytes}, {&c->d_rmid, j.mid_bytes}, {&c->d_yrgb, rgb_bytes}, {&c->d_ynet, net_bytes},
                              {&c->d_yres, res_bytes}}));
    sr_resize_bind_tables(c, j);
    return SR_OK;
}

// the tap tables, the horizontal pass and the vertical pass that ends in the frame -- fused, or as its two kernels -- queued on s; the
// job's workspace is reserved
template <class S>
int queue_resize_to_yuv(sr_ctx* c, const sr_resize_job& j, const float* d_rgb, const sr_yuv_rule& k, S* d_out, hipStream_t s) {
    unsigned bx = 0, by = 0;
    SRCHK(sr_resize_queue_front(c, j, d_rgb, false, s));
    if (!takes_fused<S>(c, k)) {
        (void)sr_resize_v_blocks(j.n, j.oh, j.ow, &bx, &by);
        HIPCHK(c, sr_launch_resize_v((const float*)c->d_rmid.p, j.n, j.ow, j.y, c->d_yres.p, false, j.linear, s));
        sr_plan_note_op(c, "resize_v", true, j.n, bx, by);
        return queue_to_yuv(c, (const float*)c->d_yres.p, k, j.n, j.oh, j.ow, d_out, s);
    }
    const int pairs = c->env_vyuv_pairs;
    (void)sr_resize_yuv_blocks(j.n, j.oh, j.ow, pairs, &bx, &by);
    HIPCHK(c, sr_launch_resize_v_yuv((const float*)c->d_rmid.p, j.n, j.ow, j.y, k, d_out, j.linear, pairs, s));
    sr_plan_note_op(c, "resize_v_yuv", true, j.n, bx, by, form_name(k));
    return SR_OK;
}

// everything the sized composed calls and the sized frame stream refuse for their context, format, shapes, filter, flags and mask alone
template <class Format>
int plan_upscale_sized(const sr_ctx* c, const Format* fmt, int n, int h, int w, int oh, int ow, int filter, unsigned flags, unsigned members,
                       sr_yuv_rule* k, sr_resize_job* j) {
    SRCHK(check_upscale_shape(c, fmt, n, h, w, members, k));
    SRCHK(check_out_size(oh, ow));
    return sr_resize_plan(n, c->factor * h, c->factor * w, oh, ow, filter, flags, j);
}

// to RGB -> network -> resampling to the frame on device buffers, queued on s; the arguments are checked and the context's device is current
template <class S>
int queue_upscale_sized(sr_ctx* c, const S* d_in, const sr_yuv_rule& k, sr_resize_job& j, int h, int w, S* d_out, unsigned members, hipStream_t s) {
    const int n = j.n;
    const size_t f = (size_t)c->factor, in_img = (size_t)h * w * kPxF, out_img = f * h * f * w * kPxF;  // (n out_img fits: sr_resize_plan)
    SRCHK(reserve_sized<S>(c, j, k, (size_t)n * in_img, (size_t)n * out_img));
    SRCHK(sr_net_capture_ready(c, false, 3, n, h, w, members));
    SRCHK(queue_to_rgb(c, d_in, k, n, h, w, (float*)c->d_yrgb.p, s));
    SRCHK(sr_net_queue(c, c->d_yrgb.p, false, 3, n, h, w, c->d_ynet.p, false, members, s));
    return queue_resize_to_yuv(c, j, (const float*)c->d_ynet.p, k, d_out, s);
}

template <class S, class Format>
int resize_to_yuv_host(sr_ctx* c, const float* rgb, const Format* fmt, int n, int h, int w, S* out, int oh, int ow, int filter, unsigned flags) {
    sr_plan_clear(c);
    sr_yuv_rule k;
    sr_resize_job j;
    if (!c || !rgb || !out || !sample_aligned<S>(out) || !rule_make(fmt, &k)) return SR_E_INVALID;
    SRCHK(check_frames(n, h, w));
    SRCHK(check_out_size(oh, ow));
    SRCHK(sr_resize_plan(n, h, w, oh, ow, filter, flags, &j));
    const size_t in_bytes = (size_t)n * h * w * kPxF, out_bytes = (size_t)n * sizeof(S) * sr_yuv_rule_frame_samples(k, oh, ow);
    return sr_host_image_call(c, false, rgb, in_bytes, out, out_bytes, [&](const void* d_in, void* d_out, hipStream_t s) -> int {
        SRCHK(reserve_sized<S>(c, j, k, 0, 0));
        return queue_resize_to_yuv(c, j, (const float*)d_in, k, (S*)d_out, s);
    });
}

template <class S, class Format>
int upscale_sized_host(sr_ctx* c, const S* in, const Format* fmt, int n, int h, int w, S* out, int oh, int ow, int filter, unsigned flags,
                       unsigned members) {
    sr_plan_clear(c);
    sr_yuv_rule k;
    sr_resize_job j;
    if (!in || !out || !sample_aligned<S>(in) || !sample_aligned<S>(out)) return SR_E_INVALID;
    SRCHK(plan_upscale_sized(c, fmt, n, h, w, oh, ow, filter, flags, members, &k, &j));
    const size_t in_bytes = (size_t)n * sizeof(S) * sr_yuv_rule_frame_samples(k, h, w);
    const size_t out_bytes = (size_t)n * sizeof(S) * sr_yuv_rule_frame_samples(k, oh, ow);
    return sr_host_image_call(c, true, in, in_bytes, out, out_bytes, [&](const void* d_in, void* d_out, hipStream_t s) {
        return queue_upscale_sized(c, (const S*)d_in, k, j, h, w, (S*)d_out, members, s);
    });
}

}  // namespace

void sr_yuv_release(sr_ctx* c) {
    sr_free_buf(c->d_yrgb);
    sr_free_buf(c->d_ynet);
    sr_free_buf(c->d_yres);
}

// ---- the frame stream ------------------------------------------------------------------------------------------------------------------
struct sr_video {
    sr_ctx* c = nullptr;  // nullptr: detached by sr_destroy
    bool failed = false;  // a recomputation in exact f32 could not be queued: what is in flight is lost, every call but destroy is refused
    sr_yuv_rule k{};
    size_t sample = 1;    // bytes of a sample: 2 made by sr_video_create16
    int h = 0, w = 0, slots = 0;
    unsigned members = 1;
    size_t in_bytes = 0, out_bytes = 0;
    bool sized = false;   // made by sr_video_create*_sized: the output frames are job.oh x job.ow
    sr_resize_job job{};  // ... the resampling of the network's output to them (one frame)
    struct Slot {
        uint8_t* h_in = nullptr;   // page-locked
        void* d_in = nullptr;
        void* d_out = nullptr;
        uint8_t* h_out = nullptr;  // where this submission's frame lands: one of outs
        hipEvent_t up = nullptr, done = nullptr, down = nullptr;
    } slot[8];
    uint8_t* outs[9] = {nullptr};  // page-locked output frames, slots + 1 of them: the one the caller holds is never a target
    unsigned long long submitted = 0;  // frames submitted so far: frame i uses slot i mod slots and output i mod (slots + 1)
    int pending = 0;
    bool acquired = false;
    // ---- row reuse (include/srhip.h sr_video_set_reuse): all of it null and unused with the mode off
    int reuse = SR_VIDEO_REUSE_OFF;
    bool have_ref = false;         // d_ref holds the input of the last submitted frame, and that frame's slot its output
    // what the bits of that output depend on besides the frame, as the context had it when the output was computed: rows computed
    // under another precision, other parameters (sr_set_params) or another kernel form ("wino": other last bits) are not reused
    struct Made {
        int precision = 0, wino = 0, wino5 = 0;
        unsigned long long params_hash = 0;
        bool operator==(const Made& o) const { return precision == o.precision && wino == o.wino && wino5 == o.wino5 && params_hash == o.params_hash; }
    } ref_made;
    void* d_ref = nullptr;         // in_bytes
    void* d_band = nullptr;        // out_bytes: a band's output frame before its planes are copied into the slot's
    uint32_t* d_flags = nullptr;   // a word per plane row: Y, Cb, Cr
    uint32_t* h_flags = nullptr;   // page-locked
    hipEvent_t flags_down = nullptr;
    sr_video_reuse_stats stats{};
};

namespace {

// ---- row reuse: the planes of a frame as rows of bytes, the plan of a frame, its launches
// The three planes of one of the session's frames of H x W luma samples: rows, bytes a row, byte offset in the frame
struct Planes {
    size_t rows[3], row_bytes[3], offset[3];
    bool vsub;  // the chroma planes have half the rows
    size_t total_rows() const { return rows[0] + rows[1] + rows[2]; }
};

Planes video_planes(const sr_video* v, size_t H, size_t W) {
    size_t ch, cw;
    sr_yuv_rule_chroma(v->k, H, W, &ch, &cw);
    Planes p{};
    p.vsub = v->k.sub == SR_YUV_420;
    p.rows[0] = H; p.row_bytes[0] = W * v->sample; p.offset[0] = 0;
    for (int k = 1; k < 3; ++k) { p.rows[k] = ch; p.row_bytes[k] = cw * v->sample; p.offset[k] = p.offset[k - 1] + p.rows[k - 1] * p.row_bytes[k - 1]; }
    return p;
}

// the typed call of a session: f(S{}) with S the session's sample type
template <class F>
int by_sample(const sr_video* v, F&& f) { return v->sample == 2 ? f(uint16_t{}) : f(uint8_t{}); }

// the rows of plane k that belong to luma rows [a, b) of its frame: a is even; b is even or the frame's height
void plane_rows(const Planes& p, int k, size_t a, size_t b, size_t* lo, size_t* hi) {
    const bool half = k > 0 && p.vsub;
    *lo = half ? a / 2 : a;
    *hi = half ? (b + 1) / 2 : b;
}

sr_video::Made video_made(const sr_ctx* c) {
    sr_video::Made m;
    m.precision = c->precision;
    m.wino = c->wino;
    m.wino5 = c->wino5;
    m.params_hash = c->params_hash;
    return m;
}

void reuse_free(sr_video* v) {
    if (v->d_ref) (void)hipFree(v->d_ref);
    if (v->d_band) (void)hipFree(v->d_band);
    if (v->d_flags) (void)hipFree(v->d_flags);
    if (v->h_flags) (void)hipHostFree(v->h_flags);
    if (v->flags_down) (void)hipEventDestroy(v->flags_down);
    v->d_ref = v->d_band = nullptr;
    v->d_flags = v->h_flags = nullptr;
    v->flags_down = nullptr;
    v->have_ref = false;
}

// everything the mode's frames need, now: the session's own buffers and the context's workspaces for the whole frame, so that no frame
// allocates (a band pass finds workspace 0's maps large enough whatever the whole frames' passes made of them)
int reuse_reserve(sr_video* v) {
    sr_ctx* c = v->c;
    const size_t f = (size_t)c->factor, words = video_planes(v, (size_t)v->h, (size_t)v->w).total_rows();
    if (!v->d_ref) HIPCHK(c, hipMalloc(&v->d_ref, v->in_bytes));
    if (!v->d_band) HIPCHK(c, hipMalloc(&v->d_band, v->out_bytes));
    if (!v->d_flags) HIPCHK(c, hipMalloc((void**)&v->d_flags, words * sizeof(uint32_t)));
    if (!v->h_flags) HIPCHK(c, hipHostMalloc((void**)&v->h_flags, words * sizeof(uint32_t), hipHostMallocPortable));
    if (!v->flags_down) HIPCHK(c, hipEventCreateWithFlags(&v->flags_down, hipEventDisableTiming));
    SRCHK(sr_reserve_bufs(c, {{&c->d_yrgb, (size_t)v->h * v->w * kPxF}, {&c->d_ynet, f * v->h * f * v->w * kPxF}}));
    if (c->graph == SR_GRAPH_SR_NET) SRCHK(sr_reserve_features(c, v->h, v->w, c->stream));
    return SR_OK;
}

// behind the frame's upload on the upload stream: the compare of its planes with the reference's, the flags' download, the frame as
// the next reference
int reuse_queue_compare(sr_video* v, const void* d_in) {
    sr_ctx* c = v->c;
    if (v->have_ref) {
        const Planes p = video_planes(v, (size_t)v->h, (size_t)v->w);
        sr_rows_differ_args a{};
        a.a = (const uint8_t*)d_in;
        a.b = (const uint8_t*)v->d_ref;
        a.flags = v->d_flags;
        a.n_seg = 3;
        for (int k = 0; k < 3; ++k) a.seg[k] = {p.offset[k], p.rows[k], p.row_bytes[k]};
        a.rows_total = p.total_rows();
        HIPCHK(c, sr_launch_rows_differ(a, c->copy_in));
        sr_plan_note_op(c, "rows_differ", false, 1, (unsigned)sr_rows_differ_blocks(a.rows_total), 1);
        HIPCHK(c, hipMemcpyAsync(v->h_flags, v->d_flags, a.rows_total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->copy_in));
        HIPCHK(c, hipEventRecord(v->flags_down, c->copy_in));
    }
    HIPCHK(c, hipMemcpyAsync(v->d_ref, d_in, v->in_bytes, hipMemcpyDeviceToDevice, c->copy_in));
    return SR_OK;
}

// What a frame computes: *n == 0 nothing, one band [0, h) the whole frame.  The session's first frame has no reference and is whole;
// a call the band form does not exist for is whole unless no row differs.
int reuse_plan(sr_video* v, sr_row_band bands[SR_REUSE_MAX_BANDS], int* n) {
    sr_ctx* c = v->c;
    bands[0] = {0, v->h};
    *n = 1;
    if (!v->have_ref) return SR_OK;
    HIPCHK(c, hipEventSynchronize(v->flags_down));  // the one host wait of the mode (what it costs: DESIGN.md 4v)
    SRCHK(sr_video_reuse_plan(v->h_flags, v->k.sub, v->h, bands, SR_REUSE_MAX_BANDS, n));
    if (*n > 0 && (v->members != 1u || c->graph != SR_GRAPH_SR_NET)) {
        bands[0] = {0, v->h};
        *n = 1;
    }
    return SR_OK;
}

int copy_rows(sr_ctx* c, void* dst, const void* src, size_t row_bytes, size_t lo, size_t hi, size_t src_lo, hipStream_t s) {
    if (lo >= hi) return SR_OK;
    HIPCHK(c, hipMemcpyAsync((char*)dst + lo * row_bytes, (const char*)src + src_lo * row_bytes, (hi - lo) * row_bytes, hipMemcpyDeviceToDevice, s));
    return SR_OK;
}

// the frame's bands on s: the rows between them from the previous frame's output, then band after band
int reuse_queue_bands(sr_video* v, const void* d_in, void* d_out, const void* d_prev_out, const sr_row_band* bands, int n, hipStream_t s) {
    sr_ctx* c = v->c;
    const int h = v->h, w = v->w, f = c->factor;
    const Planes out = video_planes(v, (size_t)f * h, (size_t)f * w);
    if (d_prev_out != d_out)
        for (int i = 0; i <= n; ++i) {  // the clean rows before band i (after the last one: i == n)
            const size_t a = i ? (size_t)f * bands[i - 1].y1 : 0, b = i < n ? (size_t)f * bands[i].y0 : (size_t)f * h;
            if (a >= b) continue;
            for (int k = 0; k < 3; ++k) {
                size_t lo, hi;
                plane_rows(out, k, a, b, &lo, &hi);
                SRCHK(copy_rows(c, (char*)d_out + out.offset[k], (const char*)d_prev_out + out.offset[k], out.row_bytes[k], lo, hi, lo, s));
            }
        }
    if (n == 0) return SR_OK;
    float* rgb = (float*)c->d_yrgb.p;
    float* net = (float*)c->d_ynet.p;
    SRCHK(by_sample(v, [&](auto t) { return queue_to_rgb(c, (const decltype(t)*)d_in, v->k, 1, h, w, rgb, s); }));
    for (int i = 0; i < n; ++i) {
        const int y0 = bands[i].y0, y1 = bands[i].y1, top = y0 > 0 ? SR_HALO : 0, bot = y1 < h ? SR_HALO : 0, bh = f * (y1 - y0);
        float* band_net = net + (size_t)f * y0 * f * w * 3;
        SRCHK(sr_run_stack(c, rgb + (size_t)(y0 - top) * w * 3, false, 3, 1, top + (y1 - y0) + bot, w, top, bot, band_net, false, s));
        SRCHK(by_sample(v, [&](auto t) { return queue_to_yuv(c, band_net, v->k, 1, bh, f * w, (decltype(t)*)v->d_band, s); }));
        const Planes band = video_planes(v, (size_t)bh, (size_t)f * w);
        for (int k = 0; k < 3; ++k) {
            size_t lo, hi;
            plane_rows(out, k, (size_t)f * y0, (size_t)f * y1, &lo, &hi);
            SRCHK(copy_rows(c, (char*)d_out + out.offset[k], (const char*)v->d_band + band.offset[k], out.row_bytes[k], lo, hi, 0, s));
        }
    }
    return SR_OK;
}

// what a session holds on the device and in page-locked memory; its streams have drained
void video_free(sr_video* v) {
    for (auto& s : v->slot) {
        if (s.h_in) (void)hipHostFree(s.h_in);
        if (s.d_in) (void)hipFree(s.d_in);
        if (s.d_out) (void)hipFree(s.d_out);
        for (hipEvent_t e : {s.up, s.done, s.down})
            if (e) (void)hipEventDestroy(e);
        s = sr_video::Slot{};
    }
    for (auto& o : v->outs) {
        if (o) (void)hipHostFree(o);
        o = nullptr;
    }
    reuse_free(v);
}

void video_drain(sr_ctx* c) {
    for (hipStream_t s : {c->copy_in, c->stream, c->stream2, c->copy_out})
        if (s) (void)hipStreamSynchronize(s);
}

// frame number `frame` of the session: upload, the three phases, download, each on its stream, ordered by the slot's events
// (again: the frame is queued a second time, in exact f32, by sr_video_receive -- with row reuse on it is computed whole and neither
// compared nor counted: the reference is the last SUBMITTED frame's input whatever is computed again)
int video_queue(sr_video* v, unsigned long long frame, bool again = false) {
    sr_ctx* c = v->c;
    sr_video::Slot& s = v->slot[frame % (unsigned)v->slots];
    s.h_out = v->outs[frame % (unsigned)(v->slots + 1)];
    HIPCHK(c, hipMemcpyAsync(s.d_in, s.h_in, v->in_bytes, hipMemcpyHostToDevice, c->copy_in));
    HIPCHK(c, hipEventRecord(s.up, c->copy_in));
    sr_row_band bands[SR_REUSE_MAX_BANDS] = {{0, v->h}};
    int n_bands = 1;
    if (v->reuse != SR_VIDEO_REUSE_OFF && !again) {
        if (!(v->ref_made == video_made(c))) v->have_ref = false;  // (sr_set_precision, sr_set_params, "wino" between two frames: the next one is whole)
        SRCHK(reuse_queue_compare(v, s.d_in));
        SRCHK(reuse_plan(v, bands, &n_bands));
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, s.up, 0));
    if (n_bands == 1 && bands[0].y0 == 0 && bands[0].y1 == v->h) {
        SRCHK(by_sample(v, [&](auto t) {
            using S = decltype(t);
            if (v->sized) return queue_upscale_sized(c, (const S*)s.d_in, v->k, v->job, v->h, v->w, (S*)s.d_out, v->members, c->stream);
            return queue_upscale(c, (const S*)s.d_in, v->k, 1, v->h, v->w, (S*)s.d_out, v->members, c->stream);
        }));
    } else {
        SRCHK(reuse_queue_bands(v, s.d_in, s.d_out, v->slot[(frame + (unsigned)v->slots - 1) % (unsigned)v->slots].d_out, bands, n_bands, c->stream));
    }
    if (v->reuse != SR_VIDEO_REUSE_OFF && !again) {
        sr_video_reuse_stats& st = v->stats;
        const bool whole = n_bands == 1 && bands[0].y1 - bands[0].y0 == v->h;
        ++st.frames;
        st.rows_total += (uint64_t)v->h;
        if (n_bands == 0) ++st.frames_reused;
        else if (whole) ++st.frames_full;
        else ++st.frames_partial;
        for (int i = 0; i < n_bands; ++i) st.rows_computed += (uint64_t)(bands[i].y1 - bands[i].y0);
        if (!whole) st.bands += (uint64_t)n_bands;
        v->have_ref = true;
    }
    v->ref_made = video_made(c);
    HIPCHK(c, hipEventRecord(s.done, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->copy_out, s.done, 0));
    HIPCHK(c, hipMemcpyAsync(s.h_out, s.d_out, v->out_bytes, hipMemcpyDeviceToHost, c->copy_out));
    HIPCHK(c, hipEventRecord(s.down, c->copy_out));
    return SR_OK;
}

int video_alloc(sr_video* v) {
    sr_ctx* c = v->c;
    SRCHK(sr_ensure_streams(c, true));
    if (!c->copy_in) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
    if (v->sized) {  // its workspace now, all or nothing, before anything else is allocated: no frame allocates, and a size that cannot fit is refused by arithmetic
        const size_t f = (size_t)c->factor;
        SRCHK(by_sample(v, [&](auto t) { return reserve_sized<decltype(t)>(c, v->job, v->k, (size_t)v->h * v->w * kPxF, f * v->h * f * v->w * kPxF); }));
    }
    for (int i = 0; i < v->slots; ++i) {
        sr_video::Slot& s = v->slot[i];
        HIPCHK(c, hipHostMalloc((void**)&s.h_in, v->in_bytes, hipHostMallocPortable));
        HIPCHK(c, hipMalloc(&s.d_in, v->in_bytes));
        HIPCHK(c, hipMalloc(&s.d_out, v->out_bytes));
        for (hipEvent_t* e : {&s.up, &s.done, &s.down}) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    for (int i = 0; i <= v->slots; ++i) HIPCHK(c, hipHostMalloc((void**)&v->outs[i], v->out_bytes, hipHostMallocPortable));
    if (v->sized && c->graph == SR_GRAPH_SR_NET) SRCHK(sr_reserve_features(c, v->h, v->w, c->stream));
    return SR_OK;
}

// either create call: a session of frames in `fmt` whose samples are `sample` bytes
// (size: of a sized session, else nullptr)
struct VideoSize {
    int oh, ow, filter;
    unsigned flags;
};

template <class Format>
int video_create(sr_ctx* c, const Format* fmt, size_t sample, int h, int w, int slots, unsigned members, sr_video** out,
                 const VideoSize* size = nullptr) {
    sr_plan_clear(c);
    if (out) *out = nullptr;
    sr_yuv_rule k;
    sr_resize_job job;
    if (!out || slots < 1 || slots > 8) return SR_E_INVALID;
    if (size) SRCHK(plan_upscale_sized(c, fmt, 1, h, w, size->oh, size->ow, size->filter, size->flags, members, &k, &job));
    else SRCHK(check_upscale_shape(c, fmt, 1, h, w, members, &k));
    sr_video* v = new sr_video;
    v->sized = size != nullptr;
    v->job = job;
    v->c = c;
    v->k = k;
    v->sample = sample;
    v->h = h;
    v->w = w;
    v->slots = slots;
    v->members = members;
    v->in_bytes = sample * sr_yuv_rule_frame_samples(k, h, w);
    v->out_bytes = sample * (size ? sr_yuv_rule_frame_samples(k, size->oh, size->ow) : sr_yuv_rule_frame_samples(k, c->factor * h, c->factor * w));
    const int rc = sr_on_device(c, [&] { return video_alloc(v); });
    if (rc != SR_OK) {
        video_free(v);
        delete v;
        return rc;
    }
    c->videos.push_back(v);
    *out = v;
    return SR_OK;
}

}  // namespace

void sr_video_detach_all(sr_ctx* c) {
    if (c->videos.empty()) return;
    video_drain(c);
    for (sr_video* v : c->videos) {
        video_free(v);
        v->c = nullptr;
        v->pending = 0;
        v->acquired = false;
    }
    c->videos.clear();
}

extern "C" {

size_t sr_yuv_frame_bytes(const sr_yuv_format* fmt, int h, int w) { return frame_bytes(fmt, h, w, 1); }
size_t sr_yuv16_frame_bytes(const sr_yuv16_format* fmt, int h, int w) { return frame_bytes(fmt, h, w, 2); }

int sr_yuv_to_rgb_dev(sr_ctx* c, const uint8_t* d_yuv, const sr_yuv_format* fmt, int n, int h, int w, float* d_rgb, void* stream) {
    return to_rgb_dev(c, d_yuv, fmt, n, h, w, d_rgb, stream);
}
int sr_yuv16_to_rgb_dev(sr_ctx* c, const uint16_t* d_yuv, const sr_yuv16_format* fmt, int n, int h, int w, float* d_rgb, void* stream) {
    return to_rgb_dev(c, d_yuv, fmt, n, h, w, d_rgb, stream);
}

int sr_rgb_to_yuv_dev(sr_ctx* c, const float* d_rgb, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* d_yuv, void* stream) {
    return to_yuv_dev(c, d_rgb, fmt, n, h, w, d_yuv, stream);
}
int sr_rgb_to_yuv16_dev(sr_ctx* c, const float* d_rgb, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* d_yuv, void* stream) {
    return to_yuv_dev(c, d_rgb, fmt, n, h, w, d_yuv, stream);
}

int sr_upscale_yuv_dev(sr_ctx* c, const uint8_t* d_in, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* d_out, unsigned members,
                       void* stream) {
    return upscale_dev(c, d_in, fmt, n, h, w, d_out, members, stream);
}
int sr_upscale_yuv16_dev(sr_ctx* c, const uint16_t* d_in, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* d_out, unsigned members,
                         void* stream) {
    return upscale_dev(c, d_in, fmt, n, h, w, d_out, members, stream);
}

int sr_upscale_yuv(sr_ctx* c, const uint8_t* in, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* out, unsigned members) {
    return upscale_host(c, in, fmt, n, h, w, out, members);
}
int sr_upscale_yuv16(sr_ctx* c, const uint16_t* in, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* out, unsigned members) {
    return upscale_host(c, in, fmt, n, h, w, out, members);
}

int sr_video_create(sr_ctx* c, const sr_yuv_format* fmt, int h, int w, int slots, unsigned members, sr_video** out) {
    return video_create(c, fmt, 1, h, w, slots, members, out);
}
int sr_video_create16(sr_ctx* c, const sr_yuv16_format* fmt, int h, int w, int slots, unsigned members, sr_video** out) {
    return video_create(c, fmt, 2, h, w, slots, members, out);
}

int sr_resize_to_yuv(sr_ctx* c, const float* rgb, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* out, int oh, int ow, int filter,
                     unsigned flags) {
    return resize_to_yuv_host(c, rgb, fmt, n, h, w, out, oh, ow, filter, flags);
}
int sr_resize_to_yuv16(sr_ctx* c, const float* rgb, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* out, int oh, int ow, int filter,
                       unsigned flags) {
    return resize_to_yuv_host(c, rgb, fmt, n, h, w, out, oh, ow, filter, flags);
}

int sr_upscale_yuv_sized(sr_ctx* c, const uint8_t* in, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* out, int oh, int ow, int filter,
                         unsigned flags, unsigned members) {
    return upscale_sized_host(c, in, fmt, n, h, w, out, oh, ow, filter, flags, members);
}
int sr_upscale_yuv16_sized(sr_ctx* c, const uint16_t* in, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* out, int oh, int ow,
                           int filter, unsigned flags, unsigned members) {
    return upscale_sized_host(c, in, fmt, n, h, w, out, oh, ow, filter, flags, members);
}

int sr_video_create_sized(sr_ctx* c, const sr_yuv_format* fmt, int h, int w, int oh, int ow, int filter, unsigned flags, int slots,
                          unsigned members, sr_video** out) {
    const VideoSize size{oh, ow, filter, flags};
    return video_create(c, fmt, 1, h, w, slots, members, out, &size);
}
int sr_video_create16_sized(sr_ctx* c, const sr_yuv16_format* fmt, int h, int w, int oh, int ow, int filter, unsigned flags, int slots,
                            unsigned members, sr_video** out) {
    const VideoSize size{oh, ow, filter, flags};
    return video_create(c, fmt, 2, h, w, slots, members, out, &size);
}

int sr_video_acquire(sr_video* v, uint8_t** in_frame) {
    if (!v || !v->c || v->failed || !in_frame) return SR_E_INVALID;
    if (v->pending >= v->slots) return SR_E_INVALID;
    v->acquired = true;
    *in_frame = v->slot[v->submitted % (unsigned)v->slots].h_in;
    return SR_OK;
}

int sr_video_submit(sr_video* v) {
    if (!v || !v->c || v->failed || !v->acquired) return SR_E_INVALID;
    sr_ctx* c = v->c;
    sr_plan_clear(c);
    return sr_on_device(c, [&]() -> int {
        if (v->pending == 0) sr_domain_set_aside(c);  // a fault an earlier *_dev call left is that call's, not a frame's
        const int rc = video_queue(v, v->submitted);
        if (rc != SR_OK) {
            video_drain(c);  // nothing of a refused frame stays queued; the slot is still the caller's
            v->have_ref = false;  // (row reuse: the reference may be this frame's already, the outputs are not: the next frame is whole)
            return rc;
        }
        v->acquired = false;
        ++v->submitted;
        ++v->pending;
        return SR_OK;
    });
}

int sr_video_receive(sr_video* v, const uint8_t** out_frame) {
    if (!v || !v->c || v->failed || !out_frame || v->pending < 1) return SR_E_INVALID;
    sr_ctx* c = v->c;
    return sr_on_device(c, [&]() -> int {
        const unsigned long long oldest = v->submitted - (unsigned)v->pending;
        sr_video::Slot& s = v->slot[oldest % (unsigned)v->slots];
        HIPCHK(c, hipEventSynchronize(s.down));
        if (c->precision == SR_PRECISION_SPLIT_F16 && c->h_domain && *(volatile int*)c->h_domain) {
            // Some frame in flight left the split-half mode's domain, and the word does not say which: every one of them, this one
            // included, is computed again in exact f32 from its slot's input, in order.  The context stays in f32.
            video_drain(c);
            (void)sr_domain_tripped(c);
            (void)sr_set_precision(c, SR_PRECISION_F32);
            for (unsigned long long i = oldest; i < v->submitted; ++i) {
                const int rc = video_queue(v, i, true);
                if (rc != SR_OK) {  // some frames are queued again and some are not: none of them may be handed out
                    video_drain(c);
                    v->failed = true;
                    v->pending = 0;
                    v->acquired = false;
                    return rc;
                }
            }
            HIPCHK(c, hipEventSynchronize(s.down));
        }
        --v->pending;
        *out_frame = s.h_out;
        return SR_OK;
    });
}

int sr_video_pending(const sr_video* v) { return v && v->c && !v->failed ? v->pending : -1; }

int sr_rows_differ_dev(sr_ctx* c, const void* d_a, const void* d_b, size_t rows, size_t row_bytes, uint32_t* d_flags, void* stream) {
    sr_plan_clear(c);
    if (!c || !d_a || !d_b || !d_flags || rows == 0 || row_bytes == 0 || !sr_dword_aligned(d_flags)) return SR_E_INVALID;
    if (rows > (size_t)INT32_MAX || row_bytes > SIZE_MAX / rows) return SR_E_INVALID;
    return sr_on_device(c, stream, [&]() -> int {
        sr_rows_differ_args a{};
        a.a = (const uint8_t*)d_a;
        a.b = (const uint8_t*)d_b;
        a.flags = d_flags;
        a.n_seg = 1;
        a.seg[0] = {0, rows, row_bytes};
        a.rows_total = rows;
        HIPCHK(c, sr_launch_rows_differ(a, (hipStream_t)stream));
        sr_plan_note_op(c, "rows_differ", false, 1, (unsigned)sr_rows_differ_blocks(rows), 1);
        return SR_OK;
    });
}

int sr_video_set_reuse(sr_video* v, int mode) {
    if (!v || !v->c || v->failed || v->pending != 0) return SR_E_INVALID;
    if (mode != SR_VIDEO_REUSE_OFF && mode != SR_VIDEO_REUSE_ROWS) return SR_E_INVALID;
    if (v->sized && mode == SR_VIDEO_REUSE_ROWS) return SR_E_INVALID;  // the row bands do not compose with a vertical resampling
    sr_ctx* c = v->c;
    sr_plan_clear(c);
    v->have_ref = false;  // the next frame is computed whole
    const int rc = sr_on_device(c, [&]() -> int {
        if (mode == SR_VIDEO_REUSE_ROWS) return reuse_reserve(v);
        reuse_free(v);  // off: the session owns none of the mode's buffers again (nothing is pending: nothing uses them)
        return SR_OK;
    });
    if (rc != SR_OK) return rc;
    v->reuse = mode;
    return SR_OK;
}

int sr_video_get_reuse_stats(const sr_video* v, sr_video_reuse_stats* out) {
    if (!v || !v->c || !out) return SR_E_INVALID;
    *out = v->stats;
    return SR_OK;
}

void sr_video_destroy(sr_video* v) {
    if (!v) return;
    if (sr_ctx* c = v->c) {
        sr_device_guard restore_device;
        (void)hipSetDevice(c->device);
        video_drain(c);
        video_free(v);
        c->videos.erase(std::remove(c->videos.begin(), c->videos.end(), v), c->videos.end());
    }
    delete v;
}

}  // extern "C"
