// sr_plan.h -- the tile, fork and host-chunk planners: pure functions of a call's shape and of sr_plan_env, free of HIP (tests/c/plan_check.cpp)
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/srhip.h"

struct sr_plan_env {  // what the planners read of a context: sr_ctx (sr_internal.h) derives from it
    int cus = 0;           // compute units of the device (sr_create)
    int plan_cus = 0;      // > 0: the planners plan as if the device had this many ("cus" switch, at most `cus`; no output byte depends on it)
    int wino = 2;          // exact mode, stages 1 .. wino in their Winograd F(2,3) form ("wino" switch; "0": all direct -- last bits differ)
    int precision = 0;  // SR_PRECISION_F32 / SR_PRECISION_SPLIT_F16
    int graph = SR_GRAPH_SR_NET, factor = SR_FACTOR;
    int pipeline = 1;              // 0: one upload, one pass, one download
    bool profiling = false;
    // experiment switches, read once at sr_create (none changes results but "wino", see wino above): SRHIP_TH, SRHIP_PIPE, SRHIP_TAIL, ...
    int env_th[5] = {0, 0, 0, 0, 0};  // 0: automatic
    int env_pipe = 1;                 // 0: first form everywhere, 1: pipe form except for small launches, 2: pipe form everywhere
    float env_tail = -1.0f;           // 4-row tiles at the end of a launch, in resident workgroups (< 0: automatic = 1 where the tail rule applies, 0: none)
    int env_fork = -1;                // device entry points, one image: two row bands on two streams (sr_run_stack_auto); -1 automatic, 0 never,
                                      // 1 always, > 1: always, with this many rows in the first band
    double fork_min_rounds = 3.5;     //   automatic: fork from this many rounds of 8-row tiles per resident workgroup on ...
    double fork_max_rounds = 1e9;     //   ... and below this many (no upper bound by default)
    double fork_share = 0.5;          //   the first band's share of the rows
    bool fork_autotune = true;        //   mid-size shapes: measured on the caller's own calls ("forktune", sr_internal.h ForkTune)
    int env_bands = 0;                // host pipeline: forced number of row bands (0: automatic)
    std::vector<int> env_rows;        // host pipeline: forced band heights (empty: automatic)
    bool env_rows_two = false;        //   ... computed on alternating streams instead of in order
    bool env_geo = true;              // host pipeline: geometric band plan where the call is compute-bound
};
inline int sr_plan_cus(const sr_plan_env& env) { return env.plan_cus > 0 ? env.plan_cus : env.cus > 0 ? env.cus : 256; }
constexpr int kStageMargin[5] = {5, 3, 2, 1, 0};  // rows stage st computes beyond the band's own, either side: what the later stages read of it
// rounds of 8-row tiles per resident workgroup (2 per CU) of a launch over `rows` rows of n images W wide
inline double sr_rounds(int cus, int W, int rows, int n = 1) { return (double)((long)n * ((W + 31) / 32) * ((rows + 7) / 8)) / (2 * cus); }

// What sr_run_stack, sr_band_pass_begin and the fork rule ask of a pass over rows [halo_top, H - halo_bot) of n images of H x W
inline int sr_check_band_args(bool img_u8, int img_ch, int n, int H, int W, int halo_top, int halo_bot) {
    if (n <= 0 || H <= 0 || W <= 0) return SR_E_INVALID;
    if (img_u8 && img_ch != 3 && img_ch != 4) return SR_E_INVALID;
    if ((halo_top != 0 && halo_top < SR_HALO) || (halo_bot != 0 && halo_bot < SR_HALO)) return SR_E_HALO;
    if (halo_top < 0 || halo_bot < 0 || halo_top + halo_bot >= H) return SR_E_INVALID;
    if ((halo_top || halo_bot) && n != 1) return SR_E_INVALID;
    return SR_OK;
}
struct sr_launch_plan { int y0, y1, ty8, ty4, th, grid; bool pipe; };
// The five launches of a pass over rows [top, bot).  forked: a band of a forked call; layers: no recompute margin (sr_band_pass)
void sr_tile_plan(const sr_plan_env& env, int n, int H, int W, int top, int bot, bool forked, bool layers, sr_launch_plan out[5]);

// Whether a device call of this shape runs as two bands (the automatic rule or sr_set_experiment("fork")), and the first band's rows.
// `mode`: env.env_fork (-1: the automatic rule, 0: never, 1: always, > 1: always, that many rows first) -- or the tuner's 0 / 1.
bool sr_plan_fork(const sr_plan_env& env, int mode, bool img_u8, int img_ch, int n, int H, int W, int halo_top, int halo_bot, int* rows_a_out);
constexpr double kForkTuneMinRounds = 0.55, kForkTuneMaxRounds = 12.0;  // outside: the rule (256x256 = 0.5 rounds: never; 1920x1080 = 15.8: exact f32 always)
bool sr_fork_tunable(const sr_plan_env& env, int n, int H, int W, int halo_top, int halo_bot, bool gated);  // gated: the call has a halo gate
// The two bands of a forked call: each one's first input row in the caller's image, its input rows H, the rows [top, bot) it produces
struct sr_fork_band { int first_row, H, top, bot; };
inline void sr_fork_bands(int H, int halo_top, int halo_bot, int rows_a, sr_fork_band out[2]) {
    const int cut = halo_top + rows_a;  // first row of the second band, in the coordinates of the caller's buffer
    out[0] = {0, cut + SR_HALO, halo_top, cut};
    out[1] = {cut - SR_HALO, H - (cut - SR_HALO), SR_HALO, H - (cut - SR_HALO) - halo_bot};
}

// One unit of the host pipeline: some whole images of a batch, or a row band of a single image
// with the halo rows it needs (band == untiled bit for bit, see sr_upscale_band_*).
struct sr_chunk {
    size_t in_off, in_bytes, out_off, out_bytes;  // of the chunk's FIRST image / of the band, in the caller's buffers
    int n, h_ext, halo_top, halo_bot;
    size_t in_step, out_step;                     // n > 1: distance between consecutive images of the chunk in the caller's
                                                  // buffers (= the image size for a contiguous batch, stride x that for a deal)
};
// Which images of the caller's batch a call processes: first, first + stride, ... (count of them).  A plain call is
// {0, 1, n}; a context's share of a round-robin deal over N contexts is {k, N, ceil((n - k) / N)}.
struct sr_deal { int first, stride, count; };
std::vector<sr_chunk> sr_plan_chunks(const sr_plan_env& env, sr_deal deal, int h, int w, size_t in_px_bytes, size_t out_px_bytes, int y_lo, int y_hi,
                                     bool* in_order);  // *in_order: several bands compute in order on one stream, not on alternating ones
// One image over n_ctx contexts (sr_upscale_*_multi): each share's rows [lo, hi), multiples of 8 (whole tiles).  One share: the whole image.
struct sr_row_share { int lo, hi; };
inline std::vector<sr_row_share> sr_multi_shares(int n_ctx, int h) {
    const int rows = std::max(8, ((h + n_ctx - 1) / n_ctx + 7) / 8 * 8), used = (h + rows - 1) / rows;
    std::vector<sr_row_share> share(used);
    for (int k = 0; k < used; ++k) share[k] = {k * rows, std::min(h, k * rows + rows)};
    // the last share must not be thinner than the halo its neighbour reads from it
    if (used > 1 && share[used - 1].hi - share[used - 1].lo < SR_HALO) { share[used - 2].hi = h; share.pop_back(); }
    return share;
}

// ---- the sizes of a composed call (sr_api.cpp sr_reserve_bufs, sr_net_queue): arithmetic alone, like the planners
// the sum of the `bytes` of a group of wants, or false where it does not fit a size_t
template <class Wants>
bool sr_sum_wants(const Wants& group, size_t* out) {
    *out = 0;
    for (const auto& w : group)
        if (__builtin_add_overflow(*out, (size_t)w.bytes, out)) return false;
    return true;
}
// One image of a batch the network reads (h x w; u8 with ch bytes a pixel, else f32 RGB) and the one it writes (f h x f w; RGBA8, else
// f32 RGB), in bytes: image i of the batch lies i times that far into its buffer.
struct sr_net_strides { size_t in_img, out_img; };
inline sr_net_strides sr_net_image_strides(int factor, bool u8, int ch, bool out_u8, int h, int w) {
    const size_t f = (size_t)factor;
    return {(size_t)h * w * (u8 ? (size_t)ch : 3 * sizeof(float)), f * h * f * w * (out_u8 ? 4 : 3 * sizeof(float))};
}
