// sr_deep.cpp -- deep colour (include/srhip.h "Deep colour"): the two conversions as entry points, and the composed calls
//     16-bit image -> f32 RGB -> network -> f32 RGB -> 16-bit image, quantised once,
// plain (sr_net_queue: the plain or the ensemble call's path), under a border mode (sr_upscale_f32_border_dev on the workspace) and to
// any size (the network's f32 call, then sr_resize_dev from f32 to f32).  The reference has no counterpart: its images are 8 bits wide.
// Kernels: sr_deep.hip.  The composed calls are their checks, their sizes and a work lambda; no stage kernel and no
// existing entry point changes.
//
// Workspace of a context, grown on first use, all or nothing, and freed by sr_destroy: the images as f32 (d_kin), the network's f32
// output (d_knet) and, for the _sized calls, that output resampled (d_kres).  hipMalloc aligns them, so both conversions of a composed
// call run in their wide form on the workspace side.
#include <hip/hip_runtime.h>

#include "sr_internal.h"

namespace {

constexpr size_t kPxF = 3 * sizeof(float);

bool u16_aligned(const void* p) { return ((uintptr_t)p & 1u) == 0; }

// a x b x c pixels and their bytes at `px` bytes a pixel, or false where either does not fit a size_t
bool pixels_of(size_t a, size_t b, size_t c, size_t px, size_t* npx) {
    size_t bytes = 0;
    return !__builtin_mul_overflow(a, b, npx) && !__builtin_mul_overflow(*npx, c, npx) && !__builtin_mul_overflow(*npx, px, &bytes);
}

bool in_channels_ok(int ch) { return ch >= 1 && ch <= 4; }
bool out_channels_ok(int ch) { return ch == 1 || ch == 3 || ch == 4; }

// either launch queued on s, with its "op" line in the plan record: the grid and the form the launcher itself takes (px: the f32 side)
int queue_to_f32(sr_ctx* c, const uint16_t* d_in, int ic, size_t npx, float* d_out, hipStream_t s) {
    const size_t blocks = sr_deep_blocks(npx);
    if (blocks > (size_t)INT32_MAX) return SR_E_NOMEM;
    HIPCHK(c, sr_launch_u16_to_f32(d_in, ic, npx, d_out, s));
    sr_plan_note_op(c, "u16_to_f32", true, 1, (unsigned)blocks, 1, sr_deep_form(d_in, d_out));
    return SR_OK;
}

int queue_to_u16(sr_ctx* c, const float* d_in, size_t npx, uint16_t* d_out, int oc, hipStream_t s) {
    const size_t blocks = sr_deep_blocks(npx);
    if (blocks > (size_t)INT32_MAX) return SR_E_NOMEM;
    HIPCHK(c, sr_launch_f32_to_u16(d_in, npx, d_out, oc, s));
    sr_plan_note_op(c, "f32_to_u16", true, 1, (unsigned)blocks, 1, sr_deep_form(d_in, d_out));
    return SR_OK;
}

// everything the two conversions refuse for their arguments alone; *npx: the batch's pixels
int check_convert(const sr_ctx* c, const void* d_u16, const void* d_f32, bool channels_ok, int n, int h, int w, size_t* npx) {
    if (!c || !d_u16 || !d_f32 || !channels_ok || n < 1 || h < 1 || w < 1) return SR_E_INVALID;
    if (!pixels_of(n, h, w, 4 * sizeof(float), npx)) return SR_E_INVALID;  // (the widest pixel of either side: RGBA16 is 8 bytes)
    if (!u16_aligned(d_u16) || !sr_dword_aligned(d_f32) || d_u16 == d_f32) return SR_E_INVALID;
    return SR_OK;
}

// What a composed call is asked for, and the sizes that follow from it.
struct Job {
    enum Kind { PLAIN, BORDER, SIZED } kind = PLAIN;
    int ic = 3, oc = 3, n = 0, h = 0, w = 0;
    unsigned members = 1;
    int mode = 0, pad = 0;                      // BORDER
    int oh = 0, ow = 0, filter = 0;             // SIZED: the final size
    unsigned flags = 0;
    int nh = 0, nw = 0;                         // the network's output size (filled by check_job)
    size_t in_px = 0, net_px = 0, out_px = 0;   // pixels of the batch: in, behind the network, in the result
};

// everything the composed calls refuse for their arguments alone (SR_E_INVALID); the sizes of *j are filled where they pass
int check_job(const sr_ctx* c, const void* in, const void* out, Job* j) {
    if (!c || !in || !out || !in_channels_ok(j->ic) || !out_channels_ok(j->oc)) return SR_E_INVALID;
    if (!u16_aligned(in) || !u16_aligned(out)) return SR_E_INVALID;
    const bool down = c->graph == SR_GRAPH_DOWNSAMPLE;
    if (down) {  // the plain call alone, with the one member: its f32 call pools 3 x 3 blocks in linear light
        if (j->kind != Job::PLAIN || j->members != 1u || j->n < 1 || j->h < 3 || j->w < 3) return SR_E_INVALID;
    } else {
        SRCHK(sr_net_check_shape(c, j->n, j->h, j->w, j->members));
    }
    j->nh = down ? j->h / 3 : c->factor * j->h;
    j->nw = down ? j->w / 3 : c->factor * j->w;
    if (j->kind == Job::BORDER && (j->mode < SR_BORDER_WRAP || j->mode > SR_BORDER_MIRROR || j->pad < SR_HALO || j->pad > SR_BORDER_PAD_MAX))
        return SR_E_INVALID;
    if (j->kind == Job::SIZED) {
        if (j->oh < 1 || j->ow < 1 || j->filter < SR_FILTER_BOX || j->filter > SR_FILTER_LANCZOS3) return SR_E_INVALID;
        if (j->flags & ~(unsigned)SR_RESIZE_SRGB_SPACE) return SR_E_INVALID;
    } else {
        j->oh = j->nh;
        j->ow = j->nw;
    }
    size_t mid_px = 0;  // (SIZED: the resampler's horizontal pass)
    if (!pixels_of(j->n, j->h, j->w, 4 * sizeof(float), &j->in_px) || !pixels_of(j->n, j->nh, j->nw, kPxF, &j->net_px) ||
        !pixels_of(j->n, j->oh, j->ow, 4 * sizeof(float), &j->out_px) || !pixels_of(j->n, j->nh, j->ow, kPxF, &mid_px))
        return SR_E_INVALID;
    return SR_OK;
}

// A public entry point run as one phase of a composed call: it clears the plan record, so what this call has noted so far is put back
// in front of what it notes.
template <class Call>
int nested(sr_ctx* c, Call&& call) {
    auto before = c->plan_rec;
    const int rc = call();
    c->plan_rec.insert(c->plan_rec.begin(), before.begin(), before.end());
    return rc;
}

// to f32 -> network [under a border | -> resampling] -> to 16 bits on device buffers, queued on s; the arguments are checked and the
// context's device is current.  Nothing is launched before this call's own three buffers stand; the border and the resampling phase
// reserve theirs when they run, behind the first conversion: an SR_E_NOMEM of theirs leaves d_kin written and the caller's output untouched.
int queue_job(sr_ctx* c, const Job& j, const uint16_t* d_in, uint16_t* d_out, hipStream_t s) {
    if (sr_deep_blocks(j.in_px) > (size_t)INT32_MAX || sr_deep_blocks(j.out_px) > (size_t)INT32_MAX) return SR_E_NOMEM;
    SRCHK(sr_reserve_bufs(c, {{&c->d_kin, j.in_px * kPxF}, {&c->d_knet, j.net_px * kPxF}, {&c->d_kres, j.kind == Job::SIZED ? j.out_px * kPxF : 0}}));
    if (c->capturing) {  // on a capturing stream the later phases' buffers stand too before the first launch: nothing can be reserved there
        const size_t H = (size_t)j.h + 2 * (size_t)j.pad, W = (size_t)j.w + 2 * (size_t)j.pad, f = (size_t)c->factor;
        sr_resize_job r;
        if (j.kind == Job::BORDER && (sr_capture_refuses(c, (size_t)j.n * H * W * kPxF > c->d_bpad.cap) || sr_capture_refuses(c, (size_t)j.n * f * H * f * W * kPxF > c->d_bout.cap)))
            return SR_E_INVALID;
        if (j.kind == Job::SIZED && (sr_resize_plan(j.n, j.nh, j.nw, j.oh, j.ow, j.filter, j.flags, &r) != SR_OK ||
                                     sr_capture_refuses(c, r.tab_bytes > c->d_rtab.cap) || sr_capture_refuses(c, r.mid_bytes > c->d_rmid.cap)))
            return SR_E_INVALID;
        SRCHK(sr_net_capture_ready(c, false, 3, j.n, j.kind == Job::BORDER ? (int)H : j.h, j.kind == Job::BORDER ? (int)W : j.w, j.members));
    }
    float* kin = (float*)c->d_kin.p;
    float* knet = (float*)c->d_knet.p;
    SRCHK(queue_to_f32(c, d_in, j.ic, j.in_px, kin, s));
    const float* result = knet;
    if (j.kind == Job::BORDER) {
        SRCHK(nested(c, [&] { return sr_upscale_f32_border_dev(c, kin, j.n, j.h, j.w, knet, j.mode, j.pad, j.members, s); }));
    } else {
        SRCHK(sr_net_queue(c, kin, false, 3, j.n, j.h, j.w, knet, false, j.members, s));
        if (j.kind == Job::SIZED) {
            SRCHK(nested(c, [&] {
                return sr_resize_dev(c, knet, SR_PIXELS_F32, j.n, j.nh, j.nw, c->d_kres.p, SR_PIXELS_F32, j.oh, j.ow, j.filter, j.flags, s);
            }));
            result = (const float*)c->d_kres.p;
        }
    }
    return queue_to_u16(c, result, j.out_px, d_out, j.oc, s);
}

int job_dev(sr_ctx* c, const uint16_t* d_in, uint16_t* d_out, Job j, void* stream) {
    sr_plan_clear(c);
    SRCHK(check_job(c, d_in, d_out, &j));
    return sr_on_device(c, stream, [&] { return queue_job(c, j, d_in, d_out, (hipStream_t)stream); });
}

// The host-pointer calls (sr_host_image_call).  sr_last_timing: total = every launch of the call, h2d / d2h the two copies.
int job_host(sr_ctx* c, const uint16_t* in, uint16_t* out, Job j) {
    sr_plan_clear(c);
    SRCHK(check_job(c, in, out, &j));
    const size_t in_bytes = j.in_px * j.ic * sizeof(uint16_t), out_bytes = j.out_px * j.oc * sizeof(uint16_t);
    return sr_host_image_call(c, true, in, in_bytes, out, out_bytes, [&](const void* d_in, void* d_out, hipStream_t s) {
        return queue_job(c, j, (const uint16_t*)d_in, (uint16_t*)d_out, s);
    });
}

Job plain_job(int ic, int n, int h, int w, int oc, unsigned members) {
    Job j;
    j.ic = ic; j.oc = oc; j.n = n; j.h = h; j.w = w; j.members = members;
    return j;
}

Job border_job(int ic, int n, int h, int w, int oc, int mode, int pad, unsigned members) {
    Job j = plain_job(ic, n, h, w, oc, members);
    j.kind = Job::BORDER; j.mode = mode; j.pad = pad;
    return j;
}

Job sized_job(int ic, int n, int h, int w, int oc, int oh, int ow, int filter, unsigned flags, unsigned members) {
    Job j = plain_job(ic, n, h, w, oc, members);
    j.kind = Job::SIZED; j.oh = oh; j.ow = ow; j.filter = filter; j.flags = flags;
    return j;
}

}  // namespace

void sr_deep_release(sr_ctx* c) {
    for (sr_buf* b : {&c->d_kin, &c->d_knet, &c->d_kres}) sr_free_buf(*b);
}

extern "C" {

int sr_u16_to_f32_dev(sr_ctx* c, const uint16_t* d_in, int in_channels, int n, int h, int w, float* d_out, void* stream) {
    sr_plan_clear(c);
    size_t npx = 0;
    SRCHK(check_convert(c, d_in, d_out, in_channels_ok(in_channels), n, h, w, &npx));
    return sr_on_device(c, stream, [&] { return queue_to_f32(c, d_in, in_channels, npx, d_out, (hipStream_t)stream); });
}

int sr_f32_to_u16_dev(sr_ctx* c, const float* d_in, int n, int h, int w, uint16_t* d_out, int out_channels, void* stream) {
    sr_plan_clear(c);
    size_t npx = 0;
    SRCHK(check_convert(c, d_out, d_in, out_channels_ok(out_channels), n, h, w, &npx));
    return sr_on_device(c, stream, [&] { return queue_to_u16(c, d_in, npx, d_out, out_channels, (hipStream_t)stream); });
}

int sr_upscale_u16_dev(sr_ctx* c, const uint16_t* d_in, int in_channels, int n, int h, int w, uint16_t* d_out, int out_channels,
                       unsigned members, void* stream) {
    return job_dev(c, d_in, d_out, plain_job(in_channels, n, h, w, out_channels, members), stream);
}

int sr_upscale_u16(sr_ctx* c, const uint16_t* in, int in_channels, int n, int h, int w, uint16_t* out, int out_channels, unsigned members) {
    return job_host(c, in, out, plain_job(in_channels, n, h, w, out_channels, members));
}

int sr_upscale_u16_border_dev(sr_ctx* c, const uint16_t* d_in, int in_channels, int n, int h, int w, uint16_t* d_out, int out_channels,
                              int mode, int pad, unsigned members, void* stream) {
    return job_dev(c, d_in, d_out, border_job(in_channels, n, h, w, out_channels, mode, pad, members), stream);
}

int sr_upscale_u16_border(sr_ctx* c, const uint16_t* in, int in_channels, int n, int h, int w, uint16_t* out, int out_channels, int mode,
                          int pad, unsigned members) {
    return job_host(c, in, out, border_job(in_channels, n, h, w, out_channels, mode, pad, members));
}

int sr_upscale_u16_sized_dev(sr_ctx* c, const uint16_t* d_in, int in_channels, int n, int h, int w, uint16_t* d_out, int out_channels,
                             int oh, int ow, int filter, unsigned flags, unsigned members, void* stream) {
    return job_dev(c, d_in, d_out, sized_job(in_channels, n, h, w, out_channels, oh, ow, filter, flags, members), stream);
}

int sr_upscale_u16_sized(sr_ctx* c, const uint16_t* in, int in_channels, int n, int h, int w, uint16_t* out, int out_channels, int oh,
                         int ow, int filter, unsigned flags, unsigned members) {
    return job_host(c, in, out, sized_job(in_channels, n, h, w, out_channels, oh, ow, filter, flags, members));
}

}  // extern "C"
