// sr_resize.cpp -- resampling to any size (include/srhip.h "Resampling to any size"): sr_resize_* resample an image that is already in
// device or host memory; sr_upscale_rgba8_sized* run the network with f32 output -- the path of sr_upscale_f32_dev or of the f32 ensemble,
// untouched, on the caller's stream -- and resample that, so that the picture is quantised once, at its final size.  The reference has no
// counterpart (main.rs:171-175 writes the factor's size).  Kernels: sr_resize.hip.
//
// Workspace of a context, all grown on first use and freed by sr_destroy: the tap tables of both axes (d_rtab), the horizontal pass's f32
// output (d_rmid), and for the _sized calls the image as f32 (d_rin) and the network's f32 output (d_rnet).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sr_internal.h"

namespace {

// a x b x c x d bytes, or false where that does not fit a size_t
bool bytes_of(size_t a, size_t b, size_t c, size_t d, size_t* out) {
    size_t v = 0;
    return !__builtin_mul_overflow(a, b, &v) && !__builtin_mul_overflow(v, c, &v) && !__builtin_mul_overflow(v, d, out);
}

size_t pixel_bytes(int pixels) { return pixels == SR_PIXELS_RGBA8 ? 4 : 3 * sizeof(float); }

using ResizeJob = sr_resize_job;

// everything sr_resize_* refuse for their arguments alone; *job is filled where they pass
int plan_resize(const void* in, int in_pixels, int n, int h, int w, const void* out, int out_pixels, int oh, int ow, int filter, unsigned flags,
                ResizeJob* job) {
    if (!in || !out) return SR_E_INVALID;
    if ((in_pixels != SR_PIXELS_RGBA8 && in_pixels != SR_PIXELS_F32) || (out_pixels != SR_PIXELS_RGBA8 && out_pixels != SR_PIXELS_F32)) return SR_E_INVALID;
    if (in == out) return SR_E_INVALID;
    return sr_resize_plan(n, h, w, oh, ow, filter, flags, job);
}

// The workspace of a job (and, for the _sized calls, in_bytes of d_rin and net_bytes of d_rnet beside it), all or nothing.  A grid beyond
// what a launch takes is refused before an allocation is attempted, as is memory (sr_reserve_bufs); the context's device is current.
int reserve(sr_ctx* c, ResizeJob& j, size_t in_bytes, size_t net_bytes) {
    if (!sr_resize_front_fits(j) || sr_resize_v_blocks(j.n, j.oh, j.ow) > (size_t)INT32_MAX) return SR_E_NOMEM;
    SRCHK(sr_reserve_bufs(c, {{&c->d_rtab, j.tab_bytes}, {&c->d_rmid, j.mid_bytes}, {&c->d_rin, in_bytes}, {&c->d_rnet, net_bytes}}));
    sr_resize_bind_tables(c, j);
    return SR_OK;
}

// the three launches of a reserved job on s; the two passes leave their "op" lines in the plan record -- the grids and the form
// sr_launch_resize_h / _v themselves take
int queue_resize(sr_ctx* c, const ResizeJob& j, const void* d_in, bool in_u8, void* d_out, bool out_u8, hipStream_t s) {
    unsigned vx = 0, groups = 0;
    (void)sr_resize_v_blocks(j.n, j.oh, j.ow, &vx, &groups);
    SRCHK(sr_resize_queue_front(c, j, d_in, in_u8, s));
    HIPCHK(c, sr_launch_resize_v((const float*)c->d_rmid.p, j.n, j.ow, j.y, d_out, out_u8, j.linear, s));
    sr_plan_note_op(c, "resize_v", !out_u8, j.n, vx, groups);
    return SR_OK;
}

// ---- the network, then the resampling

struct SizedJob {
    ResizeJob resize;  // of the network's output, fh x fw
    size_t in_bytes = 0, net_bytes = 0;
};

// everything sr_upscale_rgba8_sized[_dev] refuse for their arguments alone
int plan_sized(const sr_ctx* c, const void* in, const void* out, int n, int h, int w, int oh, int ow, int filter, unsigned flags, unsigned members,
               SizedJob* job) {
    SRCHK(sr_net_check(c, in, out, n, h, w, members));
    const int fh = c->factor * h, fw = c->factor * w;
    // (the resampling reads the workspace, never the caller's image: `in` stands in for its input so that in == out is refused here too)
    SRCHK(plan_resize(in, SR_PIXELS_F32, n, fh, fw, out, SR_PIXELS_RGBA8, oh, ow, filter, flags, &job->resize));
    if (!bytes_of(n, h, w, 3 * sizeof(float), &job->in_bytes) || !bytes_of(n, fh, fw, 3 * sizeof(float), &job->net_bytes)) return SR_E_INVALID;
    return SR_OK;
}

// byte / 255 -> network (f32 out) -> resampling (RGBA8 out) on device buffers, queued on s; the context's device is current
int queue_sized(sr_ctx* c, SizedJob& j, const uint8_t* d_in, int h, int w, uint8_t* d_out, unsigned members, hipStream_t s) {
    const int n = j.resize.n;
    SRCHK(reserve(c, j.resize, j.in_bytes, j.net_bytes));
    SRCHK(sr_net_capture_ready(c, false, 3, n, h, w, members));
    // img_to_data on the device: the ensemble's input pass with the identity map, the batch as one image of n h rows
    if ((size_t)n * h > (size_t)INT32_MAX) return SR_E_NOMEM;
    const sr_ens_map same{n * h, w, 0, 0, 0};
    if (sr_ens_blocks(same.DH, same.DW, false) > (size_t)INT32_MAX) return SR_E_NOMEM;
    HIPCHK(c, sr_launch_ens_input(d_in, true, 4, c->d_rin.p, same, s));
    SRCHK(sr_net_queue(c, c->d_rin.p, false, 3, n, h, w, c->d_rnet.p, false, members, s));
    return queue_resize(c, j.resize, c->d_rnet.p, false, d_out, true, s);
}

}  // namespace

int sr_resize_plan(int n, int h, int w, int oh, int ow, int filter, unsigned flags, sr_resize_job* job) {
    if (n < 1 || h < 1 || w < 1 || oh < 1 || ow < 1) return SR_E_INVALID;
    if (filter < SR_FILTER_BOX || filter > SR_FILTER_LANCZOS3) return SR_E_INVALID;
    if (flags & ~(unsigned)SR_RESIZE_SRGB_SPACE) return SR_E_INVALID;
    size_t in_bytes = 0, out_bytes = 0, mid_bytes = 0;
    if (!bytes_of(n, h, w, 3 * sizeof(float), &in_bytes) || !bytes_of(n, oh, ow, 3 * sizeof(float), &out_bytes) ||
        !bytes_of(n, h, ow, 3 * sizeof(float), &mid_bytes))
        return SR_E_INVALID;
    job->n = n; job->h = h; job->w = w; job->oh = oh; job->ow = ow; job->filter = filter;
    job->linear = !(flags & SR_RESIZE_SRGB_SPACE);
    job->x = sr_resize_plan_axis(w, ow, filter);
    job->y = sr_resize_plan_axis(h, oh, filter);
    size_t wx = 0, wy = 0;
    if (!bytes_of(job->x.taps, ow, sizeof(float), 1, &wx) || !bytes_of(job->y.taps, oh, sizeof(float), 1, &wy)) return SR_E_INVALID;
    const size_t heads = 2 * sizeof(int) * ((size_t)ow + (size_t)oh);
    if (__builtin_add_overflow(wx, wy, &job->tab_bytes) || __builtin_add_overflow(job->tab_bytes, heads, &job->tab_bytes)) return SR_E_INVALID;
    job->mid_bytes = mid_bytes;
    return SR_OK;
}

bool sr_resize_front_fits(const sr_resize_job& j) { return sr_resize_h_blocks((size_t)j.n * j.h, j.x) <= (size_t)INT32_MAX; }

void sr_resize_bind_tables(sr_ctx* c, sr_resize_job& j) {
    // the tables: [x.lo][x.cnt][y.lo][y.cnt][x.w][y.w]
    int* p = (int*)c->d_rtab.p;
    j.x.lo = p; j.x.cnt = p + j.ow;
    j.y.lo = p + 2 * (size_t)j.ow; j.y.cnt = j.y.lo + j.oh;
    j.x.w = (float*)(j.y.cnt + j.oh);
    j.y.w = j.x.w + (size_t)j.x.taps * j.ow;
}

int sr_resize_queue_front(sr_ctx* c, const sr_resize_job& j, const void* d_in, bool in_u8, hipStream_t s) {
    const size_t rows = (size_t)j.n * j.h;
    unsigned hx = 0;
    int cap = 0;
    const size_t h_blocks = sr_resize_h_blocks(rows, j.x, &hx);
    const int per = sr_resize_h_form(j.x, &cap);
    HIPCHK(c, sr_launch_resize_taps(j.x, j.y, j.filter, s));
    HIPCHK(c, sr_launch_resize_h(d_in, in_u8, j.linear, rows, j.x, (float*)c->d_rmid.p, s));
    sr_plan_note_op(c, "resize_h", !in_u8, j.n, hx, hx ? (unsigned)(h_blocks / hx) : 0u, cap == 0 ? "direct" : per == 1 ? "staged1" : "staged4");
    return SR_OK;
}

sr_resize_axis sr_resize_plan_axis(int n_in, int n_out, int filter) {
    sr_resize_axis a{};
    const double support = filter == SR_FILTER_BOX ? 0.5 : filter == SR_FILTER_TRIANGLE ? 1.0 : filter == SR_FILTER_CATROM ? 2.0 : 3.0;
    a.n_in = n_in;
    a.n_out = n_out;
    a.scale = (double)n_in / (double)n_out;
    a.fs = std::max(a.scale, 1.0);
    a.reach = support * a.fs;
    // hi - lo = trunc(t + 2 reach) - trunc(t) <= floor(2 reach) + 1 for t >= 0 (a negative t is clipped to 0: fewer); one more for the
    // rounding of t; never more than the axis has samples
    a.taps = (int)std::min(std::floor(2.0 * a.reach) + 2.0, (double)n_in);
    return a;
}

void sr_resize_release(sr_ctx* c) {
    for (sr_buf* b : {&c->d_rtab, &c->d_rmid, &c->d_rin, &c->d_rnet}) sr_free_buf(*b);
}

extern "C" {

int sr_resize_dev(sr_ctx* c, const void* d_in, int in_pixels, int n, int h, int w, void* d_out, int out_pixels, int oh, int ow, int filter,
                  unsigned flags, void* stream) {
    sr_plan_clear(c);
    if (!c) return SR_E_INVALID;
    ResizeJob j;
    SRCHK(plan_resize(d_in, in_pixels, n, h, w, d_out, out_pixels, oh, ow, filter, flags, &j));
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    return sr_on_device(c, stream, [&]() -> int {
        SRCHK(reserve(c, j, 0, 0));
        return queue_resize(c, j, d_in, in_pixels == SR_PIXELS_RGBA8, d_out, out_pixels == SR_PIXELS_RGBA8, (hipStream_t)stream);
    });
}

int sr_resize_rgba8(sr_ctx* c, const uint8_t* in, int n, int h, int w, uint8_t* out, int oh, int ow, int filter, unsigned flags) {
    sr_plan_clear(c);
    if (!c) return SR_E_INVALID;
    ResizeJob j;
    SRCHK(plan_resize(in, SR_PIXELS_RGBA8, n, h, w, out, SR_PIXELS_RGBA8, oh, ow, filter, flags, &j));
    const size_t in_bytes = (size_t)n * h * w * pixel_bytes(SR_PIXELS_RGBA8), out_bytes = (size_t)n * oh * ow * pixel_bytes(SR_PIXELS_RGBA8);
    return sr_host_image_call(c, false, in, in_bytes, out, out_bytes, [&](const void* d_in, void* d_out, hipStream_t s) -> int {
        SRCHK(reserve(c, j, 0, 0));
        return queue_resize(c, j, d_in, true, d_out, true, s);
    });
}

int sr_upscale_rgba8_sized_dev(sr_ctx* c, const uint8_t* d_in, int n, int h, int w, uint8_t* d_out, int oh, int ow, int filter, unsigned flags,
                               unsigned members, void* stream) {
    sr_plan_clear(c);
    SizedJob j;
    SRCHK(plan_sized(c, d_in, d_out, n, h, w, oh, ow, filter, flags, members, &j));
    if (!sr_dword_aligned(d_in) || !sr_dword_aligned(d_out)) return SR_E_INVALID;
    return sr_on_device(c, stream, [&] { return queue_sized(c, j, d_in, h, w, d_out, members, (hipStream_t)stream); });
}

int sr_upscale_rgba8_sized(sr_ctx* c, const uint8_t* in, int n, int h, int w, uint8_t* out, int oh, int ow, int filter, unsigned flags,
                           unsigned members) {
    sr_plan_clear(c);
    SizedJob j;
    SRCHK(plan_sized(c, in, out, n, h, w, oh, ow, filter, flags, members, &j));
    const size_t in_bytes = (size_t)n * h * w * 4, out_bytes = (size_t)n * oh * ow * 4;
    return sr_host_image_call(c, true, in, in_bytes, out, out_bytes, [&](const void* d_in, void* d_out, hipStream_t s) {
        return queue_sized(c, j, (const uint8_t*)d_in, h, w, (uint8_t*)d_out, members, s);
    });
}

}  // extern "C"
