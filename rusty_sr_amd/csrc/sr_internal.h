// sr_internal.h -- the context behind include/srhip.h's opaque sr_ctx, shared by sr_api.cpp (engine) and
// sr_comm.cpp (RCCL communicator + sharded entry points).  Not installed, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "sr_plan.h"  // (and with it include/srhip.h)
#include "sr_yuv_rule.h"

// 16-channel halves of conv5 (stage 2's 3x3 source) that the exact mode runs as Winograd F(2,3) rows by default: 1.  Both halves would take
// the whole call's direct-FLOP rate to within 1 % of the f32 roof on the fastest boxes, which bench.py's contract asserts it stays below
// (DESIGN.md 4a, item 4); "wino" = "3" runs both, for measurement.
constexpr int kWinoConv5Halves = 1;

// A device buffer that grows on demand (sr_ensure_buf / sr_ensure_bufs) and is never shrunk but by sr_free_buf.
struct sr_buf {
    void* p = nullptr;
    size_t cap = 0;
};

struct sr_ctx : sr_plan_env {  // (the base: what the tile, fork and host-chunk planners read of a context, sr_plan.h)
    int device = 0;
    int clock_mhz = 0;
    char name[128] = {0};
    hipStream_t stream = nullptr;
    float* d_params = nullptr;  // all packed parameters, one allocation
    void* d_qtab = nullptr;     // bilinear_net / downsample_net: data_to_img(LinearToSrgb(l)) as a step table (sr_aux.hip)
    size_t off_w0 = 0, off_w0h = 0, off_w[5] = {0}, off_wh[5] = {0}, off_bias[5] = {0}, off_beta[5] = {0};
    size_t off_wino1 = 0;  // stage 1's weights as Winograd F(2,3) chunks (sr_api.cpp pack_steps_wino)
    size_t off_wino2[3] = {0, 0, 0};  // stage 2's, by wino5: conv2 as Winograd F(2,3) chunks, then conv5's first wino5 halves as 3-tap Winograd chunks, then its other halves' direct chunks
    int wino5 = kWinoConv5Halves;  // exact mode, with stage 2 in its Winograd form (sr_plan_env::wino), the first wino5 halves of conv5 ("wino" = "2": none, the form before; "3": both)
    // Domain of the split-half mode (include/srhip.h, sr_set_precision): values are carried as pairs of HALVES, so every weight, input
    // and activation must be finite and below 65504 in magnitude.  Weights are checked once (split_ok); inputs and activations by the
    // kernels, which raise *h_domain -- one word of mapped host memory, read by the host without a copy once the stream has drained.
    bool split_ok = true;
    int* h_domain = nullptr;   // host address of the flag
    int* d_domain = nullptr;   // the same word as the device sees it
    bool dev_fault = false;    // a fault an earlier *_dev call left in *h_domain, set aside at the start of a host-pointer call: sr_check_domain's
    // Device workspace of one pass of the conv stack.  Two of them: the host pipeline (run_host) alternates chunks between
    // two compute streams so that the tail of one chunk's stage launches overlaps the head of the next chunk's; every
    // other entry point uses ws[0] only (ws[1] is allocated on first use).
    struct Workspace {
        float* d_feat[4] = {nullptr, nullptr, nullptr, nullptr};  // f, l1, l2, l3 (zero-bordered, see sr_kernels.h)
        size_t feat_cap_px = 0;       // allocated padded pixels per map
        int geo_n = 0, geo_h = 0, geo_w = 0;  // geometry the borders were last zeroed for
        bool captured = false;        // a pass on these maps was recorded into a stream capture: a replay writes them behind the host's back, so
                                      // geo_* says nothing any more and every pass from then on clears its borders (ensure_features)
        int pitch = 0; long img_stride = 0;
        int* d_queue = nullptr;       // 5 stages x 8 per-XCD tile-queue heads (persistent kernels)
    } ws[2];
    hipStream_t stream2 = nullptr;    // second compute stream of the host pipeline
    // host-pointer entry points: two in / out slots so that chunk i+1 uploads and chunk i-1
    // downloads while chunk i computes (run_host)
    sr_buf d_in[2], d_out[2];
    hipStream_t copy_out = nullptr;   // downloads of a pipelined host call
    hipStream_t copy_in = nullptr;    // uploads: exact-f32 contexts, from their second pipelined call on (else on the compute streams)
    int pipelined_calls = 0;
    std::vector<hipEvent_t> pool;  // per-chunk timing / ordering events of run_host, grown on demand
    hipEvent_t ev[6] = {nullptr};  // around the five stages of a profiled pass of the conv stack (sr_run_stack)
    double total_ms = 0, stage_ms[5] = {0}, h2d_ms = 0, d2h_ms = 0;
    int last_h = 0, last_w = 0;
    int last_hip = 0;
    // Stream capture (include/srhip.h "Stream capture"): the stream of the *_dev call in progress is being captured (sr_capture_scope).
    // Such a call records its launches and may do nothing else: whatever would allocate, free or upload refuses with SR_E_INVALID
    // (sr_capture_refuses), the fork tuner and the profiling events stand aside.
    bool capturing = false;
    // experiment switches beside the planners' (sr_plan_env), read once at sr_create like them
    int env_bw = -1;                  // tile-order column-block width in tiles (-1: automatic)
    hipEvent_t ev_fork[2] = {nullptr, nullptr};  // fork (caller's stream -> stream2) and join (stream2 -> caller's stream)
    // Mid-size shapes (0.55-12 rounds of 8-row tiles): whether the fork pays depends on how the tiles of the image and of its two bands
    // happen to fill the chip's last round -- -15 ... +20 % from one shape to the next (profiles/r6_fork_tune.txt), which no rule in
    // `rounds` predicts.  So it is MEASURED, per shape and context, on the caller's own calls: a block of undivided calls, then a block of
    // forked ones, each timed by an event pair on the caller's stream that is read -- never waited for -- at a later call of that shape;
    // then the faster plan stays.  Results do not depend on the plan (bit-identical), only the time does.  sr_set_experiment "forktune".
    struct ForkTune {
        int H = 0, W = 0, top = 0, bot = 0, img_ch = 0, precision = 0;
        bool img_u8 = false, out_u8 = false;
        int taken = 0;                    // samples read so far: [0, kForkTuneBlock) undivided, [kForkTuneBlock, 2 kForkTuneBlock) forked; a block's first is dropped (warm-up)
        float best[2] = {1e30f, 1e30f};   // fastest sample of either plan, ms
        int decided = -1;                 // -1: still measuring, 0: undivided, 1: forked
        bool pending = false;             // ev[] bracket a call whose time has not been read yet
        hipEvent_t ev[2] = {nullptr, nullptr};
        unsigned long long used = 0;      // for eviction: the entry used longest ago goes
    };
    std::vector<ForkTune> fork_tune;
    unsigned long long fork_tune_clock = 0;
    int env_vyuv_pairs = 0;           // the vertical pass to a YCbCr frame: 0 the measured rule (sr_yuv.cpp fused_pays), 1 | 2 the fused kernel with that many row pairs a workgroup, -1 the chain; "vyuv"
    int env_auxgrid = 0;              // bilinear_net / downsample_net: at most this many workgroups per launch (0: automatic); "auxgrid"
    unsigned long long params_hash = 0;  // FNV-1a of the parameter vector: contexts of one sharded call must agree
    // ---- multi-GPU (sr_comm.cpp): one RCCL communicator per context, neighbour halo exchange
    void* comm = nullptr;             // ncclComm_t
    bool comm_local = false;          // sr_comm_init_local: neighbours are contexts of this process, halos go by peer copy
    int comm_rank = 0, comm_nranks = 1;
    sr_buf d_ext;  // band + halo rows, the exchange lands here
    hipEvent_t ev_comm[2] = {nullptr, nullptr};  // around the halo exchange of a sharded call, on the stream it runs on (round 6: the context's stream2)
    hipEvent_t ev_wait[2] = {nullptr, nullptr};  // on the band's stream, either side of its wait for the exchange: what of the exchange was NOT hidden
    hipEvent_t ev_xfork = nullptr;               // band's stream -> exchange stream: the caller's band is complete
    bool wait_pending = false;
    double comm_exposed_ms = 0;
    hipEvent_t ev_band[2] = {nullptr, nullptr};  // around the whole sharded step of this context (band copy, exchange, conv stack)
    bool comm_pending = false, band_pending = false;  // the events of the last sharded call have not been read yet (sr_last_comm_ms / sr_last_timing)
    double comm_ms = 0;
    int last_nccl = 0;
    bool comm_broken = false;         // an exchange failed half-posted: the communicator was aborted, sharded calls return SR_E_COMM
    bool layer_halos = false;         // sharded calls exchange FEATURE rows after every stage instead of recomputing the overlap (sr_set_experiment "halo")
    hipEvent_t ev_layer[4] = {nullptr, nullptr, nullptr, nullptr};  // one-process sharded call in that mode: "stage st of this context is done"
    // What the last public call ran (sr_get_experiment "plan", a test hook): the host pipeline's chunk plan, the fork decision of a device
    // call, one line per stage launch -- identical consecutive lines as one, with a count.  Host-side text written where the decisions are
    // made; cleared by every public entry point.  The pixel operators around the network (pad, crop, bleed, merge, the resampler's two
    // passes) write an "op" line per launch -- its grid as the launcher's own *_blocks function gives it (sr_plan_note_op).  A backward
    // pass writes one "grad" line: how it splits its sums over the batch's LR pixels (sr_grad_queue, from sr_grad_split_of).
    std::vector<std::pair<std::string, int>> plan_rec;
    // ---- validation pass (sr_valid.cpp): the forward half of the training graph, grown on demand, freed by sr_destroy
    sr_buf d_vhr;                                   // the HR image of a host-pointer call
    sr_buf d_vlr;                                   // the pooled LR image (the graph's `input` node), f32
    sr_buf d_vout;                                  // the network's f32 output (`output` node)
    sr_buf d_vpart;                                 // the loss kernel's f64 partials, then the host-pointer calls' result
    float* d_vtab = nullptr;                        // 512 floats: byte / 255, then SrgbToLinear of those (sr_valid.cpp)
    int vnode_h = 0, vnode_w = 0;                   // LR size of the last validation call (0: none yet)
    // ---- backpropagation (sr_grad.cpp): grown on demand, freed by sr_destroy
    sr_buf d_gws;                                   // saved forward state, gradients of the nodes, partials (sr_grad_workspace_bytes)
    sr_buf d_gin;                                   // host-pointer calls: params, HR batch, pooled LR batch, gradient
    int loss_kind = SR_LOSS_MSE;                    // sr_set_loss: host-side state, read when a backward pass is queued (sr_grad_queue)
    float loss_eps = 1e-3f;
    // ---- self-ensemble (sr_ensemble.cpp): grown on demand, freed by sr_destroy
    sr_buf d_ein;                                   // T_k of the caller's image, f32 RGB
    sr_buf d_eout;                                  // one member's f32 output map
    sr_buf d_eacc;                                  // the f32 accumulator of a call with RGBA8 output (an f32 call accumulates in its output)
    // ---- metrics (sr_metrics.cpp): grown on demand, freed by sr_destroy
    sr_buf d_mpart;                                 // the tile kernel's partials (f64, then u64), then the host-pointer calls' 16-byte result
    sr_buf d_mimg;                                  // both images of a host-pointer sr_image_metrics_rgba8 call
    // ---- transparency (sr_alpha.cpp): grown on demand, freed by sr_destroy
    sr_buf d_ableed;                                // the bled copy of the caller's RGBA8 image
    size_t total_mem = 0;                           // the device's memory, asked for once: a shape beyond it is refused without an allocation
    // ---- resampling to any size (sr_resize.cpp): grown on demand, freed by sr_destroy
    sr_buf d_rtab;                                  // both axes' tap tables: first tap, tap count, weights (sr_resize_axis)
    sr_buf d_rmid;                                  // the horizontal pass's output, n x h x ow x 3 f32
    sr_buf d_rin;                                   // the _sized calls: byte / 255 of the caller's image, f32 RGB
    sr_buf d_rnet;                                  // the _sized calls: the network's f32 output
    // ---- borders (sr_border.cpp): grown on demand, freed by sr_destroy
    sr_buf d_bpad;                                  // the padded copy of the caller's image, RGBA8 or f32 RGB
    sr_buf d_bout;                                  // the network's output for it, before the crop
    // ---- degradation (sr_degrade.cpp): uploaded on first use, freed by sr_destroy
    double* d_dtab = nullptr;                       // 320 doubles: SrgbToLinear(byte / 255), then the 8 x 8 DCT matrix
    // ---- training sessions on this context (sr_train.cpp): sr_destroy releases what they hold on the device and detaches them
    std::vector<sr_train*> trains;
    // ---- video (sr_yuv.cpp): grown on demand, freed by sr_destroy
    sr_buf d_yrgb;                                  // the frames as the network's input, n x h x w x 3 f32
    sr_buf d_ynet;                                  // the network's f32 output for them, before the conversion back
    sr_buf d_yres;                                  // the sized calls, format classes that go by the chain: the resampled f32 image, oh x ow x 3
    std::vector<sr_video*> videos;                  // frame streams on this context: sr_destroy drains and detaches them
    // ---- deep colour (sr_deep.cpp): grown on demand, freed by sr_destroy
    sr_buf d_kin;                                   // the 16-bit images as the network's input, n x h x w x 3 f32
    sr_buf d_knet;                                  // the network's f32 output for them
    sr_buf d_kres;                                  // the _sized calls: that output resampled, before the conversion back
    // ---- optimiser (sr_optim.cpp): grown on demand, freed by sr_destroy
    sr_buf d_opart;                                 // the gradient norm's f64 partials, one per 256 elements
};

inline void sr_plan_clear(sr_ctx* c) {
    if (c) c->plan_rec.clear();
}

inline void sr_plan_note(sr_ctx* c, const std::string& line) {
    if (!c->plan_rec.empty() && c->plan_rec.back().first == line) ++c->plan_rec.back().second;
    else c->plan_rec.emplace_back(line, 1);
}

// One launch of a pixel operator: "op name=<pad|crop|bleed|merge|resize_h|resize_v|resize_v_yuv|yuv2rgb|rgb2yuv|u16_to_f32|f32_to_u16|yuv16_to_rgb|rgb_to_yuv16|rows_differ> px=<u8|f32> n=.. bx=.. by=.. [form=..] [f=..]".
// px: the pixels the kernel is instantiated on (resize_h, yuv2rgb, rgb2yuv: its input's, resize_v: its output's; the deep-colour and deep video conversions: their f32 side); bx / by: workgroups along a row and along
// the rows of one image (resize_h: of the batch's n h rows; the deep-colour conversions: 1, the batch is one run of pixels), from the
// *_blocks function the launcher itself calls.
inline void sr_plan_note_op(sr_ctx* c, const char* name, bool f32, int n, unsigned bx, unsigned by, const char* form = nullptr, int f = 0) {
    char line[128], tail[48] = "";
    if (form) snprintf(tail, sizeof tail, " form=%s", form);
    else if (f) snprintf(tail, sizeof tail, " f=%d", f);
    snprintf(line, sizeof line, "op name=%s px=%s n=%d bx=%u by=%u%s", name, f32 ? "f32" : "u8", n, bx, by, tail);
    sr_plan_note(c, line);
}

// The device entry points' buffers that the kernels address as 32-bit words (include/srhip.h): every RGBA output -- the final stage
// stores whole dwords (sr_kernels.hip DwordRun) -- and every f32 input and output.  Null passes here: the callers refuse it themselves.
inline bool sr_dword_aligned(const void* p) {
    return ((uintptr_t)p & 3u) == 0;
}

// No HIP device to run on (the runtime reports none, or fails): what an entry point without a context answers SR_E_NO_DEVICE to.
// clear_error: read the runtime's error away, so that no later launch check finds it.  count (optional): the number of devices.
inline bool sr_no_device(bool clear_error = true, int* count = nullptr) {
    int n = 0;
    const bool failed = hipGetDeviceCount(&n) != hipSuccess;
    if (failed && clear_error) (void)hipGetLastError();
    if (count) *count = n;
    return failed || n <= 0;
}

inline void sr_free_buf(sr_buf& b) {
    if (b.p) (void)hipFree(b.p);
    b = sr_buf{};
}

inline size_t sr_round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// ---- the HR images of the training graph (validation, backpropagation, training session): n images of h x w pixels, u8 with 3 or 4
// channels (alpha is ignored) or f32 RGB
inline bool sr_hr_channels_ok(bool hr_u8, int ch) { return hr_u8 ? (ch == 3 || ch == 4) : ch == 3; }

// The HR arguments of an entry point of context c (not null), checked before the GPU is touched.
inline int sr_check_hr_args(const sr_ctx* c, bool hr_u8, int ch, int n, int h, int w) {
    if (c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    if (!sr_hr_channels_ok(hr_u8, ch)) return SR_E_INVALID;
    if (n < 1 || h < c->factor || w < c->factor) return SR_E_INVALID;  // not one f x f pooling block
    return SR_OK;
}

// The arguments of a paired call (include/srhip.h, "pairs"): n LR images of lh x lw (u8 with lr_ch channels, or f32 RGB like the HR batch)
// beside n HR images of exactly f lh x f lw.
inline int sr_check_pair_args(const sr_ctx* c, bool u8, int lr_ch, int hr_ch, int n, int lh, int lw) {
    if (c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    if (!sr_hr_channels_ok(u8, lr_ch) || !sr_hr_channels_ok(u8, hr_ch)) return SR_E_INVALID;
    if (n < 1 || lh < 1 || lw < 1 || lh > INT32_MAX / c->factor || lw > INT32_MAX / c->factor) return SR_E_INVALID;
    return SR_OK;
}

// Elements the loss is summed over: 3 channels of the top-left f floor(h / f) x f floor(w / f) crop of each image.
inline size_t sr_loss_elems(int f, int n, int h, int w) { return (size_t)n * 3 * ((size_t)f * (h / f)) * ((size_t)f * (w / f)); }

// The run-time (hr_u8, ch, linear) of such a call as compile-time constants: fn(bool_constant<HR_U8>, integral_constant<int, CH>,
// bool_constant<LINEAR>), for the combinations sr_hr_channels_ok admits.
template <class Fn>
void sr_dispatch_hr(bool hr_u8, int ch, bool linear, Fn&& fn) {
    auto with_linear = [&](auto u8, auto channels) {
        if (linear) fn(u8, channels, std::true_type{});
        else fn(u8, channels, std::false_type{});
    };
    if (hr_u8 && ch == 3) with_linear(std::true_type{}, std::integral_constant<int, 3>{});
    else if (hr_u8) with_linear(std::true_type{}, std::integral_constant<int, 4>{});
    else with_linear(std::false_type{}, std::integral_constant<int, 3>{});
}

// The library never leaves the calling thread on another device than it found it on: torch (and any HIP host) takes
// "the current device" from hipGetDevice, and the one-process multi-GPU calls walk over every context's device.
// Every extern "C" entry point that may call hipSetDevice holds one of these for its duration.
struct sr_device_guard {
    int saved = -1;
    sr_device_guard() { if (hipGetDevice(&saved) != hipSuccess) { (void)hipGetLastError(); saved = -1; } }
    ~sr_device_guard() { if (saved >= 0) (void)hipSetDevice(saved); }
    sr_device_guard(const sr_device_guard&) = delete;
    sr_device_guard& operator=(const sr_device_guard&) = delete;
};

#define SRCHK(expr) do { const int rc__ = (expr); if (rc__ != SR_OK) return rc__; } while (0)  // a status that is not SR_OK is the caller's
#define HIPCHK(ctx, expr)                         \
    do {                                          \
        hipError_t e__ = (expr);                  \
        if (e__ != hipSuccess) {                  \
            (void)hipGetLastError(); /* the runtime keeps the error until it is read: the next launch check must not find it */ \
            (ctx)->last_hip = (int)e__;           \
            return e__ == hipErrorOutOfMemory ? SR_E_NOMEM : SR_E_HIP; \
        }                                         \
    } while (0)


// Rows of the image that are still on their way when the call is made -- the halo rows of a sharded band, which a neighbour's GPU
// sends while this one already works (sr_comm.cpp): the first `top` and the last `bot` rows of d_img are in place once `ready`
// (recorded on another stream) has fired.  Only stage 0 reads the image's halo rows directly (f rows within 2 of them), so the stack
// launches stage 0 for the rows that need none of them FIRST, waits for the event on its own stream, and then runs stage 0's few
// edge rows and the other stages: the exchange hides under the band copy and the interior of stage 0.  mark[0..1] (optional) are
// recorded on the waiting stream either side of the wait.
struct sr_halo_gate {
    hipEvent_t ready = nullptr;
    int top = 0, bot = 0;
    hipEvent_t mark[2] = {nullptr, nullptr};
};

// The whole conv stack on device buffers (sr_api.cpp): rows [halo_top, H - halo_bot) of each image are produced.
int sr_run_stack(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int n, int H, int W, int halo_top, int halo_bot,
                 void* d_out, bool out_u8, hipStream_t s, int slot = 0, const sr_halo_gate* gate = nullptr);
// ... the same for one image as two row bands forked onto the context's second stream where that pays (the device entry points)
int sr_run_stack_auto(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int n, int H, int W, int halo_top, int halo_bot,
                      void* d_out, bool out_u8, hipStream_t s, const sr_halo_gate* gate = nullptr);
int sr_reserve_features(sr_ctx* c, int H, int W, hipStream_t s);  // workspace 0's maps for one image of H x W, now; the context's device is current
int sr_ensure_fork_resources(sr_ctx* c);  // the second stream + the fork / join events
void sr_fork_tune_clear(sr_ctx* c);      // forget what the fork tuner has measured (its events with it); the context's device is current

// One pass of the conv stack over a band, stage by stage -- for a caller that has something to do BETWEEN the stages (sr_comm.cpp:
// the per-layer feature-halo exchange).  `layers`: every stage computes the band's OWN rows only (no recompute
// margin); the rows of f / l1 / l2 / l3 that the next stage reads beyond them (2 / 1 / 1 / 1 either side) are the caller's to put
// into this context's maps before it launches that stage.
struct sr_band_pass;
int sr_band_pass_begin(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int H, int W, int halo_top, int halo_bot, void* d_out, bool out_u8,
                       hipStream_t s, bool layers, const sr_halo_gate* gate, sr_band_pass** out);
int sr_band_pass_stage(sr_band_pass* p, int st);                 // launch stage st (0..4) on the pass's stream
float* sr_band_pass_row(const sr_band_pass* p, int map, int y);  // row y (the pass's image coordinates) of map 0..3 = f, l1, l2, l3, border columns included
size_t sr_band_pass_row_floats(const sr_band_pass* p);           // ... its length: pitch x 32 floats, contiguous in both map layouts
void sr_band_pass_end(sr_band_pass* p);
int sr_ensure_buf(sr_ctx* c, sr_buf& b, size_t bytes);  // at least `bytes`; what the buffer held is lost when it grows
// The buffers of one job, all or nothing: each is grown to its size; should one not fit, EVERY buffer of the group is freed -- a job that
// does not fit must not keep what of it was allocated (it may be most of the device).  (A size of 0 grows nothing: the buffer only shares
// the group's fate.)
struct sr_buf_want {
    sr_buf* buf;
    size_t bytes;
};
int sr_ensure_bufs(sr_ctx* c, std::initializer_list<sr_buf_want> group);
int sr_ensure_streams(sr_ctx* c, bool pipelined);  // the context's own streams are created on first use

// ---- the split-half mode's domain word (sr_ctx::h_domain) in the synchronous host-pointer calls
// A fault still standing in the word when such a call begins was raised by an EARLIER call -- an unchecked *_dev call (a context has one
// caller: nothing of it is still running once that caller is here) -- and is that call's to report (sr_check_domain); it must not make
// this call, whose values may all be in range, recompute in f32.  Set it aside.
inline void sr_domain_set_aside(sr_ctx* c) {
    if (c->h_domain && *(volatile int*)c->h_domain) { c->dev_fault = true; *(volatile int*)c->h_domain = 0; }
}
// Once every stream of the call has drained: did a value of it leave the split-half mode's domain?  Clears the word.
inline bool sr_domain_tripped(sr_ctx* c) {
    if (c->precision != SR_PRECISION_SPLIT_F16 || !c->h_domain || !*(volatile int*)c->h_domain) return false;
    *(volatile int*)c->h_domain = 0;
    return true;
}

// ---- One synchronous host-pointer call on the context's own stream (sr_api.cpp): every such entry point but the pipelined upscale
// (run_host) is its argument checks and a call of this.  It makes the context's device current (and restores the caller's), creates the
// stream, grows `staging` all or nothing, then runs upload, work, download -- callables that QUEUE on the stream they are given and
// return a status (a HIPCHK inside one returns into this function) -- and drains the stream whatever they returned.
// network: the work runs the conv stack -- a stale domain fault is set aside before it, and in the split-half mode a value that left
// its domain makes all three phases run again in exact f32 (the mode is switched back).  The phases may therefore run twice.
// times, with profiling on (sr_last_timing): PARTS = h2d_ms the upload, total_ms the work, d2h_ms the download; TOTAL = total_ms all three.
enum sr_host_times { SR_TIMES_NONE, SR_TIMES_TOTAL, SR_TIMES_PARTS };
using sr_host_phase = std::function<int(hipStream_t)>;
int sr_host_call(sr_ctx* c, bool network, sr_host_times times, std::initializer_list<sr_buf_want> staging, const sr_host_phase& upload,
                 const sr_host_phase& work, const sr_host_phase& download);

// ---- What a call that wraps the network (ensemble, transparency, borders, any size) or stands beside it (resize, degrade) is made of.
// A new wrapper writes its checks, its sizes and its work lambda, nothing else.
inline int sr_hip_status(sr_ctx* c, hipError_t e) {  // HIPCHK as a value: the status of a lambda that is one runtime call
    HIPCHK(c, e);
    return SR_OK;
}
// Held by every *_dev entry point for its duration: asks the runtime once whether the caller's stream is being captured.  stream = NULL
// is never asked about: a capture that the legacy stream takes part in is not one the library can see (include/srhip.h).
struct sr_capture_scope {
    sr_ctx* c;
    bool outer = false;  // (a composed call makes entry points of its own: what it found comes back when they return)
    sr_capture_scope(sr_ctx* ctx, void* stream) : c(ctx) {
        if (!c) return;
        outer = c->capturing;
        c->capturing = false;
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (!stream) return;
        if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) { (void)hipGetLastError(); return; }
        c->capturing = st != hipStreamCaptureStatusNone;
    }
    ~sr_capture_scope() { if (c) c->capturing = outer; }
    sr_capture_scope(const sr_capture_scope&) = delete;
    sr_capture_scope& operator=(const sr_capture_scope&) = delete;
};
// What a call on a capturing stream answers where it would have to allocate, free, create or upload (`needed`): SR_E_INVALID, before
// it does so.  The remedy: sr_reserve_* or one eager call of that shape first.
inline bool sr_capture_refuses(const sr_ctx* c, bool needed) { return needed && c->capturing; }
// The network on n images of h x w (members: an ensemble's mask, 1: the plain call) needs nothing created for a call on a capturing
// stream -- asked by the composed calls before their first launch; SR_OK off a capture.  The context's device is current.
int sr_net_capture_ready(sr_ctx* c, bool u8, int ch, int n, int h, int w, unsigned members);

// The body of a device-pointer entry point -- a callable that queues on the caller's stream and returns a status -- with the context's
// device current and the caller's restored.  The arguments, the alignment rule of the call included, are checked before it.
template <class Body>
int sr_on_device(sr_ctx* c, Body&& body) {
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    return body();
}
template <class Body>
int sr_on_device(sr_ctx* c, void* stream, Body&& body) {  // ... of a *_dev entry point: its stream may be capturing
    sr_capture_scope capture(c, stream);
    return sr_on_device(c, body);
}
// What every call that runs the network on a batch refuses for its arguments alone (SR_E_INVALID): a null context or image, a graph
// other than sr_net / bilinear, a shape below 1 or beyond INT32_MAX / factor, a mask outside 1..255, a mask other than 1 off sr_net.
int sr_net_check(const sr_ctx* c, const void* in, const void* out, int n, int h, int w, unsigned members);
int sr_net_check_shape(const sr_ctx* c, int n, int h, int w, unsigned members);  // ... all of it but the two image pointers (a call that has no image yet)
// The network on n images on device buffers, queued on s: the plain call's path for the whole batch (members == 1), else the ensemble
// image by image.  u8: ch bytes a pixel in, else f32 RGB; out_u8: RGBA8 out, else f32 RGB.  The context's device is current.
int sr_net_queue(sr_ctx* c, const void* d_in, bool u8, int ch, int n, int h, int w, void* d_out, bool out_u8, unsigned members, hipStream_t s);
// sr_ensure_bufs for a job's workspace, with the refusal by arithmetic before it: wants that all fit what is allocated ask the runtime
// nothing; otherwise a sum of the wanted bytes beyond the device's whole memory (asked for once a context) is SR_E_NOMEM without an
// allocation being attempted.  Only what the context itself allocates counts: a shape that passes and still cannot run beside the
// caller's own buffers is refused with the same status before any launch -- by the staging buffers of a host-pointer call, by hipMalloc
// in sr_ensure_bufs, or by the network's own size rule.  The context's device is current.
int sr_reserve_bufs(sr_ctx* c, std::initializer_list<sr_buf_want> group);
// sr_host_call for a call that uploads one image batch and downloads one: staging d_in[0] / d_out[0], one copy each way, SR_TIMES_PARTS;
// work(d_in, d_out, s) queues everything between the copies on the staged buffers.
using sr_image_work = std::function<int(const void* d_in, void* d_out, hipStream_t s)>;
int sr_host_image_call(sr_ctx* c, bool network, const void* in, size_t in_bytes, void* out, size_t out_bytes, const sr_image_work& work);

void sr_comm_release(sr_ctx* c);  // sr_comm.cpp: destroy the communicator and its buffers (called by sr_destroy)

// ---- validation pass (sr_valid.hip kernels, sr_valid.cpp host side)
void sr_valid_release(sr_ctx* c);  // sr_valid.cpp: free the validation buffers (called by sr_destroy)
int sr_valid_loss_grid(int HC, int WC);  // workgroups (= f64 partials) of the loss kernel for an HC x WC crop: a function of the shape alone
// HR (W px per row, u8 with ch channels or f32 RGB) -> LR image OH x OW x 3 f32 = LinearToSrgb(mean_{f x f}(SrgbToLinear(hr)))
hipError_t sr_launch_valid_pool(int factor, const void* d_hr, bool hr_u8, int ch, int W, int OH, int OW, float* d_lr, const float* d_tab,
                                hipStream_t s);
// LR pixels (u8 with ch channels, any byte offset, npx of them, contiguous) -> npx x 3 f32, img_to_data: byte / 255 (d_tab's first 256 floats)
hipError_t sr_launch_lr_input(const uint8_t* d_lr, int ch, long npx, float* d_x, const float* d_tab, hipStream_t s);
// The LR batch a paired call supplies in place of the pool (include/srhip.h, "pairs"): device memory, u8 (ch 3 or 4) or f32 RGB -- or, with
// in_place, already converted at the input buffer (sr_grad_input_buffer) by the caller.
struct sr_lr_input {
    const void* d_lr = nullptr;
    bool u8 = true;
    int ch = 3;
    bool in_place = false;
};
// queue the conversion (u8) or the copy (f32) of npx LR pixels to d_x
hipError_t sr_queue_lr_input(const sr_lr_input& lr, long npx, float* d_x, const float* d_tab, hipStream_t s);
// sum over the HC x WC crop of (out - hr)^2 (linear: of SrgbToLinear of both) -> one double at d_result (4-byte aligned)
hipError_t sr_launch_valid_loss(const float* d_out, const void* d_hr, bool hr_u8, int ch, bool linear, int W, int HC, int WC, const float* d_tab,
                                double* d_partial, void* d_result, hipStream_t s);
// The f64 partials of a loss kernel -> their sum, one double at d_result (4-byte aligned): one workgroup, a fixed order of additions, so
// the same bits on every run, context and device (also the backward pass's err_sum)
hipError_t sr_launch_loss_sum(const double* d_partial, int n, void* d_result, hipStream_t s);

// ---- metrics (sr_metrics.hip kernels, sr_metrics.cpp host side; include/srhip.h "Metrics")
void sr_metrics_release(sr_ctx* c);  // free the metrics buffers (called by sr_destroy)
long sr_metrics_blocks(int H, int W, int shave);  // workgroups (= partials) of the tile kernel: a function of the shape alone; 0: an empty region
// Scores of A (H x W; u8 with a_ch channels at any byte and pitch_a pixels per row, or the contiguous, 16-byte aligned f32 RGB output, quantised
// on load) against B (u8, b_ch channels, any byte, pitch_b pixels per row) -> 16 bytes at d_result16 (4-byte aligned): u64 y_sq_err, f64
// ssim_sum.  weights: the window's 11 f64 weights (host memory); d_partial: 16 sr_metrics_blocks(..) bytes.
hipError_t sr_launch_metrics(const void* d_a, bool a_u8, int a_ch, long pitch_a, const uint8_t* d_b, int b_ch, long pitch_b, int H, int W,
                             int shave, const double* weights, void* d_partial, void* d_result16, hipStream_t s);
// What a validation call may ask for beside its loss (sr_valid.cpp run_validation): the scores of its quantised output against the HR image.
struct sr_metrics_request {
    int shave = 0;               // >= 0: resolved and checked by sr_metrics_shave
    void* d_result16 = nullptr;  // nullptr: the context's own slot (sr_metrics_slot), for the host-pointer calls
};
int sr_metrics_shave(const sr_ctx* c, int shave, int* out);  // -1 -> the context's factor; below that SR_E_INVALID
int sr_metrics_reserve(sr_ctx* c, int H, int W, int shave);  // grow the partials buffer for such a call (sr_metrics_queue does it too)
// queue the scoring of an H x W image pair on s (the arguments are the caller's to have checked); the context's device is current
int sr_metrics_queue(sr_ctx* c, const void* d_a, bool a_u8, int a_ch, long pitch_a, const uint8_t* d_b, int b_ch, long pitch_b, int H, int W,
                     const sr_metrics_request& rq, hipStream_t s);
void* sr_metrics_slot(const sr_ctx* c, int H, int W, int shave);  // where a request without d_result16 left its 16 bytes
void sr_metrics_fill(sr_metrics* m, const void* result16, int H, int W, int shave);  // the counts, and the two sums from the 16 bytes

// ---- backpropagation (sr_grad.hip kernels, sr_grad.cpp host side)
void sr_grad_release(sr_ctx* c);  // sr_grad.cpp: free the backprop buffers (called by sr_destroy)
// Everything sr_launch_grad reads and writes for one call: a batch of n HR images pooled to n LR images of H x W (already at x).
struct sr_grad_plan {
    int factor = 3, n = 0, H = 0, W = 0;
    const float* params = nullptr;  // the parameters the gradient is taken at, sr_num_params_factor(factor) floats
    const float* x = nullptr;       // the pooled LR batch, n x H x W x 3 f32
    const void* hr = nullptr;       // the HR batch, n images of hr_h x hr_w x hr_ch (u8) or x 3 (f32)
    bool hr_u8 = true;
    int hr_ch = 3, hr_h = 0, hr_w = 0;
    const float* tab = nullptr;     // the validation pass's 512-float table (sr_valid.cpp)
    bool linear = false;
    float loss_scale = 1.0f, l2 = 0.0f;
    int loss_kind = SR_LOSS_MSE;    // the objective (include/srhip.h sr_set_loss), and Charbonnier's eps
    float loss_eps = 1e-3f;
    float* ws = nullptr;            // sr_grad_workspace_bytes(factor, n, H, W), 256-byte aligned
    void* err_out = nullptr;        // sum of squared errors, one double at a 4-byte aligned address (nullptr: sr_grad_result_slot)
    float* grad = nullptr;          // the gradient, .rsr order
};
size_t sr_grad_workspace_bytes(int factor, int n, int H, int W);
double* sr_grad_result_slot(const sr_grad_plan& p);  // the workspace's own slot for err_sum
// How sr_launch_grad splits its sums over the NP = n H W LR pixels (sr_grad.hip layout(): the fields its launches are sized with), for
// the plan record's "grad" line.
struct sr_grad_split {
    int conv_grid, loss_grid;  // workgroups of 128 pixels (beta / bias partials) and of 256 pixels (f64 loss partials)
    int wchunks; long wchunk;  // weight-gradient chunks and their pixels
    int cchunks; long cchunk;  // expand-bias column-sum chunks and their pixels
};
sr_grad_split sr_grad_split_of(int factor, int n, int H, int W);
hipError_t sr_launch_grad(const sr_grad_plan& p, hipStream_t s);
hipError_t sr_launch_grad_adam(float* d_params, float* d_m, float* d_v, const float* d_grad, size_t n, float lr, float beta1, float beta2,
                               float eps, float bc1, float bc2, hipStream_t s);
// The backward pass of a batch of n HR images of h x w on device buffers, queued on s (what sr_backprop_rgba8_dev does after its argument
// checks); lr: nullptr = pool the HR batch, else the LR batch of a paired call (h, w = f x its size).  The context's device is current.
int sr_grad_queue(sr_ctx* c, const float* d_params, const void* d_hr, bool hr_u8, int ch, int n, int h, int w, bool linear, float loss_scale,
                  float l2, void* d_err, float* d_grad, hipStream_t s, double** result_slot, const sr_lr_input* lr);
// Grow the backprop workspace for n LR images of OH x OW; *x: where the pass reads its input batch (n x OH x OW x 3 f32, whole 256 bytes)
int sr_grad_input_buffer(sr_ctx* c, int n, int OH, int OW, float** x);
int sr_valid_ensure_table(sr_ctx* c);  // sr_valid.cpp: the 512-float table behind d_vtab, uploaded on first use

// ---- self-ensemble (sr_ensemble.hip kernels, sr_ensemble.cpp host side; include/srhip.h sr_upscale_ensemble_*)
// One gather of DH x DW pixels: dst[p][q] = src[r][c], (r0, c0) = swap ? (q, p) : (p, q), r / c = r0 / c0 reversed within src if flip_r / flip_c.
struct sr_ens_map {
    int DH, DW, swap, flip_r, flip_c;
};
// workgroups of such a launch (0: an empty shape), a function of the shape alone; the launchers refuse more than INT32_MAX
size_t sr_ens_blocks(int DH, int DW, bool swap, int* lw_out = nullptr, unsigned* blocks_x_out = nullptr);
// the image (u8 with ch channels at any byte, or f32 RGB) -> its transform at d_dst, f32 RGB (u8: byte / 255, alpha dropped)
hipError_t sr_launch_ens_input(const void* d_src, bool u8, int ch, void* d_dst, const sr_ens_map& m, hipStream_t s);
// acc = (first ? 0.0f : acc) + gather(member); the last member stores (that sum) * scale at d_out instead, as f32 (d_out may be d_acc) or RGBA8
hipError_t sr_launch_ens_accumulate(const float* d_member, float* d_acc, void* d_out, bool out_u8, bool first, bool last, float scale,
                                    const sr_ens_map& m, hipStream_t s);
void sr_ensemble_release(sr_ctx* c);  // free the ensemble buffers (called by sr_destroy)
// The ensemble of one image on device buffers, queued on s: the arguments are the caller's to have checked (sr_ensemble_check).  The
// context's device is current.
int sr_ensemble_check(const sr_ctx* c, unsigned members, int h, int w);
int sr_ensemble_queue(sr_ctx* c, const void* d_img, bool img_u8, int img_ch, int h, int w, void* d_out, bool out_u8, unsigned members,
                      hipStream_t s);

// ---- transparency (sr_alpha.hip kernels, sr_alpha.cpp host side; include/srhip.h "Transparency")
// workgroups of either launch (0: an empty shape), functions of the shape alone; the launchers refuse more than INT32_MAX
size_t sr_alpha_bleed_blocks(int n, int h, int w, unsigned* tiles_x_out = nullptr, unsigned* tiles_y_out = nullptr);
size_t sr_alpha_merge_blocks(int factor, int n, int h, int w, unsigned* blocks_x_out = nullptr, unsigned* blocks_y_out = nullptr);
// d_out = bleed(d_in, radius): n RGBA8 images of h x w, both 4-byte aligned and not overlapping
hipError_t sr_launch_alpha_bleed(const uint8_t* d_in, uint8_t* d_out, int n, int h, int w, int radius, hipStream_t s);
// byte 3 of the n images of factor h x factor w at d_out <- the alpha of d_lr (n x h x w RGBA8) interpolated; both 4-byte aligned
hipError_t sr_launch_alpha_merge(int factor, const uint8_t* d_lr, uint8_t* d_out, int n, int h, int w, hipStream_t s);
// ... either launch queued on s with its "op" line in the plan record (sr_alpha.cpp): what the entry points and the composed calls run
int sr_alpha_queue_bleed(sr_ctx* c, const uint8_t* d_in, uint8_t* d_out, int n, int h, int w, int radius, hipStream_t s);
int sr_alpha_queue_merge(sr_ctx* c, const uint8_t* d_lr, uint8_t* d_out, int n, int h, int w, hipStream_t s);
void sr_alpha_release(sr_ctx* c);  // free the bleed buffer (called by sr_destroy)

// ---- borders (sr_border.hip kernels, sr_border.cpp host side; include/srhip.h "Borders")
// workgroups of either launch (0: an empty shape), functions of the shape alone; the launchers refuse more than INT32_MAX
size_t sr_border_pad_blocks(bool f32, int n, int h, int w, int pad, unsigned* blocks_x_out = nullptr, unsigned* blocks_y_out = nullptr);
size_t sr_border_crop_blocks(bool f32, int n, int ch, int cw, unsigned* blocks_x_out = nullptr, unsigned* blocks_y_out = nullptr);
// d_out = the n images of h x w at d_in (RGBA8, or f32 RGB), each continued by `pad` pixels on every side under `mode`; both 4-byte
// aligned and not overlapping
hipError_t sr_launch_border_pad(const void* d_in, bool f32, int n, int h, int w, int mode, int pad, void* d_out, hipStream_t s);
// d_out = the ch x cw window at (y0, x0) of each of the n images of H x W at d_in, contiguous; both 4-byte aligned and not overlapping
hipError_t sr_launch_border_crop(const void* d_in, bool f32, int n, int H, int W, int y0, int x0, int ch, int cw, void* d_out, hipStream_t s);
void sr_border_release(sr_ctx* c);  // free the two buffers (called by sr_destroy)

// ---- resampling to any size (sr_resize.hip kernels, sr_resize.cpp host side; include/srhip.h "Resampling to any size")
// One axis of a resampling, n_in -> n_out samples: the rule's constants (f64, from the host) and where its tables lie in device memory.
// taps: the padded tap count, an upper bound of hi - lo over the axis; w is tap-major, w[k * n_out + o] (taps beyond an index's count: 0).
struct sr_resize_axis {
    int n_in, n_out, taps;
    double scale, fs, reach;  // n_in / n_out, max(scale, 1), S fs
    int* lo;
    int* cnt;
    float* w;
};
sr_resize_axis sr_resize_plan_axis(int n_in, int n_out, int filter);  // everything but the pointers
// The horizontal pass's form for an axis: the input rows a workgroup takes; *cap_out > 0: the staged form, with that many pixels of each row
// in LDS, 0: the direct form (a scale whose run under 256 columns does not fit).
int sr_resize_h_form(const sr_resize_axis& x, int* cap_out);
// workgroups of the two passes (0: an empty shape), functions of the shape alone; the launchers refuse more than INT32_MAX
size_t sr_resize_h_blocks(size_t rows, const sr_resize_axis& x, unsigned* blocks_x_out = nullptr);
size_t sr_resize_v_blocks(int n, int oh, int ow, unsigned* blocks_x_out = nullptr, unsigned* groups_out = nullptr);
hipError_t sr_launch_resize_taps(const sr_resize_axis& x, const sr_resize_axis& y, int filter, hipStream_t s);
// rows (= n h) rows of x.n_in pixels (RGBA8 or f32 RGB; linear: through SrgbToLinear) -> rows x x.n_out x 3 f32 at d_mid
hipError_t sr_launch_resize_h(const void* d_in, bool in_u8, bool linear, size_t rows, const sr_resize_axis& x, float* d_mid, hipStream_t s);
// n images of y.n_in x ow x 3 f32 at d_mid -> n images of y.n_out x ow (RGBA8 or f32 RGB; linear: through LinearToSrgb) at d_out
hipError_t sr_launch_resize_v(const float* d_mid, int n, int ow, const sr_resize_axis& y, void* d_out, bool out_u8, bool linear, hipStream_t s);
// One resampling of n images h x w -> oh x ow: its two axes and what it needs of the workspace (d_rtab, d_rmid).
struct sr_resize_job {
    int n = 0, h = 0, w = 0, oh = 0, ow = 0, filter = 0;
    bool linear = true;
    sr_resize_axis x{}, y{};
    size_t tab_bytes = 0, mid_bytes = 0;
};
// everything a resampling refuses for its shape, filter and flags alone (SR_E_INVALID: sizes below 1, an unknown filter or flag, byte
// counts beyond a size_t); *job is filled where they pass
int sr_resize_plan(int n, int h, int w, int oh, int ow, int filter, unsigned flags, sr_resize_job* job);
bool sr_resize_front_fits(const sr_resize_job& j);           // the horizontal pass's grid is one a launch takes
void sr_resize_bind_tables(sr_ctx* c, sr_resize_job& j);     // the axes' table pointers into d_rtab, once it holds j.tab_bytes
// the tap tables and the horizontal pass of a job whose workspace is reserved and bound, into d_rmid, queued on s, with the pass's "op" line
int sr_resize_queue_front(sr_ctx* c, const sr_resize_job& j, const void* d_in, bool in_u8, hipStream_t s);
// ---- ... that ends in a YCbCr frame (sr_resize_yuv.hip; include/srhip.h "Video at any size")
// workgroups of the launch (0: an empty shape) for `pairs` row pairs a workgroup (1 | 2; anything else: the default), a function of the
// shape alone; the launcher refuses more than INT32_MAX
size_t sr_resize_yuv_blocks(int n, int oh, int ow, int pairs, unsigned* blocks_x_out = nullptr, unsigned* blocks_y_out = nullptr);
// n images of y.n_in x ow x 3 f32 at d_mid -> n frames of y.n_out x ow luma samples S at d_yuv (aligned to a sample): the bits of
// sr_launch_resize_v (f32 out) followed by sr_launch_rgb_to_yuv
template <class S>
hipError_t sr_launch_resize_v_yuv(const float* d_mid, int n, int ow, const sr_resize_axis& y, const sr_yuv_rule& k, S* d_yuv, bool linear,
                                  int pairs, hipStream_t s);
void sr_resize_release(sr_ctx* c);  // free the resampling buffers (called by sr_destroy)

// ---- training session (sr_train.hip crop kernel, sr_train.cpp host side)
// One crop of a step, as the crop kernel reads it: px is device memory, 4-byte aligned when ch = 4 (rows are then read as whole pixels).
// k: the item's member (0..7, include/srhip.h sr_train_step_aug); the source window at (y0, x0) is crop_w x crop_h when k & 4.
struct sr_train_crop_desc {
    const uint8_t* px;
    int ch, h, w, y0, x0;
    int k;
};
struct sr_train_crop_args {  // passed by value: a step whose images are resident uploads nothing
    sr_train_crop_desc d[SR_TRAIN_MAX_BATCH];
    int n, crop_h, crop_w;
};
// One LR / HR pair of a paired step: the LR image is lh x lw, the HR image f lh x f lw; the crop origin in LR pixels.  (Compact: 64 of
// them are one kernel's arguments.)
struct sr_train_pair_desc {
    const uint8_t* lr;
    const uint8_t* hr;
    uint8_t lr_ch, hr_ch, k, pad;  // k: the item's member; (bytes, so that a descriptor stays 40 bytes)
    int lh, lw, y0, x0;
};
static_assert(sizeof(sr_train_pair_desc) == 40 && sizeof(sr_train_crop_desc) == 32, "64 descriptors are one kernel's arguments");
struct sr_train_pair_args {
    sr_train_pair_desc d[SR_TRAIN_MAX_BATCH];
    int n, crop_lh, crop_lw;
    int hr_blocks;  // set by the launcher: blocks of a grid row that cut the HR crop
};
void sr_train_detach_all(sr_ctx* c);  // sr_train.cpp: called by sr_destroy; a detached session refuses every call but sr_train_destroy
// the n crops -> n x crop_h x crop_w x 3 u8 at d_out, whose allocation holds whole dwords (ceil(n crop_h crop_w 3 / 4) of them)
hipError_t sr_launch_train_crop(const sr_train_crop_args& a, uint32_t* d_out, hipStream_t s);
// the n HR crops (f crop_lh x f crop_lw) -> u8 at d_out as above, and the n LR crops -> n x crop_lh x crop_lw x 3 f32 (byte / 255, d_tab)
// at d_x, which is 16-byte aligned and holds whole 16-byte groups
hipError_t sr_launch_train_pair_crop(int factor, sr_train_pair_args a, uint32_t* d_out, float* d_x, const float* d_tab, hipStream_t s);

// ---- degradation (sr_degrade.hip kernels, sr_degrade.cpp host side; include/srhip.h "Degradation")
// One call of the operator: the source image as the crop kernels read it (d.k: the member, d.y0 / d.x0: the frame's origin), its parameters,
// the factor and the frame's size in HR pixels.
struct sr_degrade_one {
    sr_train_crop_desc d;
    sr_degrade g;
    int f, frame_h, frame_w;
};
struct sr_train_degrade_args {  // a degraded step's gather, passed by value like sr_train_crop_args
    sr_train_crop_desc d[SR_TRAIN_MAX_BATCH];
    sr_degrade g[SR_TRAIN_MAX_BATCH];
    int n, crop_h, crop_w, f;
    int hr_blocks;  // set by the launcher: blocks of a grid row that cut the HR crop
};
static_assert(sizeof(sr_degrade) == 24 && sizeof(sr_train_degrade_args) <= 4096 - 4 * sizeof(void*), "one kernel's arguments");
int sr_degrade_check(const sr_degrade& g);  // SR_E_INVALID for parameters out of range
int sr_degrade_radius(const sr_degrade& g);  // ceil(3 sigma): the HR pixels the blur reaches beyond a frame
int sr_degrade_ensure_table(sr_ctx* c);     // the 320 doubles behind d_dtab, uploaded on first use; the context's device is current
void sr_degrade_release(sr_ctx* c);         // free it (called by sr_destroy)
// the LR frame of a.d's window -> frame_h / f x frame_w / f x 3 bytes at d_out (any byte offset); d_tab: the context's d_dtab
hipError_t sr_launch_degrade(const sr_degrade_one& a, const double* d_tab, uint8_t* d_out, hipStream_t s);
// the n HR crops -> u8 at d_batch as sr_launch_train_crop stores them, and their degraded LR frames -> n x crop_h / f x crop_w / f x 3 f32
// (byte / 255, d_ftab's first 256 floats) at d_x
hipError_t sr_launch_train_degrade(sr_train_degrade_args a, uint32_t* d_batch, float* d_x, const float* d_ftab, const double* d_tab,
                                   hipStream_t s);

// ---- video and deep video (sr_yuv.hip kernels, sr_yuv.cpp host side; include/srhip.h "Video", "Deep video")
// The format as the kernels take it, its two validators and its frame size: sr_yuv_rule.h (no HIP).
// workgroups of either launch for n frames of h x w luma samples (0: an empty shape), a function of the shape alone; the launchers refuse
// more than INT32_MAX
size_t sr_yuv_blocks(int n, int h, int w, unsigned* blocks_x_out = nullptr, unsigned* blocks_y_out = nullptr);
// n frames of samples S = uint8_t | uint16_t at d_yuv (aligned to a sample) -> n x h x w x 3 f32 at d_rgb (4-byte aligned), and back;
// a uint8_t launch of a 4:2:2 rule is hipErrorInvalidValue
template <class S>
hipError_t sr_launch_yuv_to_rgb(const S* d_yuv, const sr_yuv_rule& k, int n, int h, int w, float* d_rgb, hipStream_t s);
template <class S>
hipError_t sr_launch_rgb_to_yuv(const float* d_rgb, const sr_yuv_rule& k, int n, int h, int w, S* d_yuv, hipStream_t s);
// The row compare of the frame stream's row reuse (sr_reuse.hip): flags[r] = 1 where row r differs between a and b, else 0.  The rows
// are those of n_seg (1..3) segments one after another -- a frame's planes -- each `rows` rows of `row_bytes` contiguous bytes that
// begin `offset` bytes into a and into b; rows_total is their sum.  a, b: any byte; flags: 4-byte aligned.
struct sr_rows_differ_args {
    const uint8_t* a;
    const uint8_t* b;
    uint32_t* flags;
    struct { size_t offset, rows, row_bytes; } seg[3];
    int n_seg;
    size_t rows_total;
};
size_t sr_rows_differ_blocks(size_t rows_total);  // workgroups of the launch: a function of the row count alone
hipError_t sr_launch_rows_differ(const sr_rows_differ_args& a, hipStream_t s);
void sr_yuv_release(sr_ctx* c);        // free the two buffers (called by sr_destroy)
void sr_video_detach_all(sr_ctx* c);   // called by sr_destroy; a detached stream refuses every call but sr_video_destroy

// ---- deep colour (sr_deep.hip kernels, sr_deep.cpp host side; include/srhip.h "Deep colour")
// workgroups of either launch for npx pixels (0: none): a function of the pixel count alone; the launchers refuse more than INT32_MAX
size_t sr_deep_blocks(size_t npx);
// the form a launch takes for its two pointers: "wide" (both 16-byte aligned), "wide_in", "wide_out" or "narrow"
const char* sr_deep_form(const void* d_in, const void* d_out);
// npx pixels of in_channels (1..4) native-endian 16-bit samples at d_in (2-byte aligned) -> npx x 3 f32 at d_out (4-byte aligned), and
// npx x 3 f32 -> npx pixels of out_channels (1, 3 or 4) samples
hipError_t sr_launch_u16_to_f32(const uint16_t* d_in, int in_channels, size_t npx, float* d_out, hipStream_t s);
hipError_t sr_launch_f32_to_u16(const float* d_in, size_t npx, uint16_t* d_out, int out_channels, hipStream_t s);
void sr_deep_release(sr_ctx* c);  // free the three buffers (called by sr_destroy)

// ---- optimiser (sr_optim.hip kernels, sr_optim.cpp host side; include/srhip.h "Optimiser")
size_t sr_optim_parts(size_t n);  // f64 partials of the norm of n floats: a function of n alone
// S, scale and skip of n floats (4-byte aligned) -> d_out and, if not null, d_mirror (both 8-byte aligned); d_part: sr_optim_parts(n) doubles
hipError_t sr_launch_grad_norm(const float* d_grad, size_t n, float clip, double* d_part, sr_grad_norm* d_out, sr_grad_norm* d_mirror, hipStream_t s);
// Adam on scale g (d_norm null: scale 1, no skip), then e <- d e + omd p' (d_e null: none); 16 bytes a lane when all the pointers allow it
hipError_t sr_launch_adam_clipped(float* d_p, float* d_m, float* d_v, const float* d_g, float* d_e, size_t n, float lr, float b1, float b2, float eps,
                                  float bc1, float bc2, float d, float omd, const sr_grad_norm* d_norm, unsigned long long* d_skipped,
                                  hipStream_t s);
bool sr_clip_ok(float clip);       // 0, or finite and above 0
bool sr_ema_decay_ok(float d);     // 0, or strictly inside (0, 1)
bool sr_lr_ok(float lr);           // finite and at least 0
// sr_grad_norm_dev after its argument checks, with the optional second copy of the result; the context's device is current
int sr_grad_norm_queue(sr_ctx* c, const float* d_grad, size_t n, float clip, sr_grad_norm* d_out, sr_grad_norm* d_mirror, hipStream_t s);
void sr_optim_release(sr_ctx* c);  // free the partials (called by sr_destroy)
