// sr_plan.cpp -- the tile, fork and host-chunk planners (sr_plan.h).  Every threshold was measured on an MI355X; its measurement stands beside it.
#include "sr_plan.h"

#include <cstdlib>

void sr_tile_plan(const sr_plan_env& env, int n, int H, int W, int top, int bot, bool forked, bool layers, sr_launch_plan out[5]) {
    const int tiles_x = (W + 31) / 32;
    const int cus = sr_plan_cus(env);
    const int resident = 2 * cus;  // workgroups of a stage kernel that fit the chip at once (2 per CU: 76-78 KB of LDS each)
    for (int st = 0; st < 5; ++st) {
        sr_launch_plan& l = out[st];
        l.y0 = layers ? top : std::max(0, top - kStageMargin[st]);
        l.y1 = layers ? bot : std::min(H, bot + kStageMargin[st]);
        const int rows = l.y1 - l.y0;
        // Tile classes of the launch (sr_kernels.h TileGrid): `ty8` rows of 8-row tiles, then `ty4` rows of 4-row tiles.
        // Measured on MI355X (profiles/r3_tileplans_*, r3_queuefix_*; `rounds` = 8-row tiles per resident workgroup):
        //  * exact f32, a SMALL launch (rounds < 2): 4-row tiles on the first form of the stage kernel -- one tile per
        //    workgroup, no queue (256x256: 0.157 ms against 0.176-0.178 on either tile class of the pipe form);
        //  * split-half mode, small launch: the pipe form all the same (256x256: 0.091 ms against 0.24), 8-row tiles while
        //    they still give every CU one, else 4-row tiles;
        //  * otherwise the pipe form on 8-row tiles, and in exact f32 the LAST tiles of every XCD's queue are 4-row tiles, one per
        //    resident workgroup (sr_set_experiment "tail"): a persistent launch ends when its slowest workgroup does, and with
        //    half-size last tiles (and stealing) the workgroups finish closer together -- also when the tile count is an exact
        //    multiple of the workgroups (1024x768, 6.00 rounds: -4.9 %).  Measured, interleaved A/B (profiles/r3_tail_ab.txt):
        //    800x600 -4.7 %, 1000x600 -4.2 %, 1280x720 -2.4 %, 1920x1200 -1.4 %, the 8- / 4- / 2-way band of 3840x2160 -2.1 /
        //    -0.3 / -0.4 %, 2560x1440 -0.4 %, 3840x2160 0; but 512x512 (2.0 rounds) +5...9 % and 640x480 (2.3) +2 %: the 4-row
        //    tile body is code the launch would otherwise never touch (~30 us of cold instruction fetch per call), so no tail below
        //    3 rounds (round 3 also excluded launches above 14 rounds with a last round more than 70 % full -- 1920x1080, 15.8: 0 then; see below).  The
        //    split-half mode pays 17 % per 4-row tile (its B operands are re-read per tile row) and keeps 8-row tiles.
        //  conv0 and the first form run one class.
        const long tiles8 = (long)n * tiles_x * ((rows + 7) / 8);
        const double rounds = sr_rounds(cus, W, rows, n);
        // (the last stage of factor 4 in the split-half mode exists with 4-row tiles only: two N-tiles of accumulators, sr_kernels.hip kBigTiles)
        // (the exact mode's stages 1 and 2 in their Winograd form: a 4-row tile half-fills the pair dimension, 7 MFMAs per 16 pixels where the
        // direct form issues 5, so a small launch keeps 8-row tiles instead of switching to 4-row ones -- 256x256 stage 1 0.0488 ms with 4-row
        // tiles, 0.0314 with 8-row ones, direct 0.0368; 360x640 0.1515 / 0.0853 / 0.1080: profiles/r7_ab_wino_stage1.txt; stage 2 256x256
        // 0.0658 / 0.0402 / 0.0449, 360x640 0.2188 / 0.1242 / 0.1434: profiles/r8_ab_wino_stage2.txt.  Tile plans change no bit.)
        const bool wino8 = env.precision == SR_PRECISION_F32 && (st == 1 || st == 2) && st <= env.wino;
        const int forced = (st == 4 && env.factor == 4 && env.precision == SR_PRECISION_SPLIT_F16) ? 4 : env.env_th[st];
        const bool small_launch = tiles8 < 2L * resident;
        const bool split = env.precision == SR_PRECISION_SPLIT_F16;
        // (round 4: with the scalar overheads of the pipe form gone it also wins where every workgroup has exactly ONE 4-row tile and the
        // node has several sources -- their tiles arrive under the previous source's taps instead of between them: 256x256 stages 2 / 3
        // 40.5 / 49.0 -> 39.1 / 47.2 us; with more than one round of small tiles the first form still leads, 384x384 0.356 against 0.382 ms:
        // profiles/r4_ab_small_pipe.txt)
        const bool one_small_round = small_launch && (long)n * tiles_x * ((rows + 3) / 4) <= resident;
        l.pipe = st > 0 && env.env_pipe != 0 && (env.env_pipe == 2 || !small_launch || split || (st >= 2 && one_small_round));
        l.ty8 = (rows + 7) / 8; l.ty4 = 0;
        if (forced == 4 || (!forced && small_launch && !wino8 && (!split || tiles8 < cus))) {
            l.ty8 = 0; l.ty4 = (rows + 3) / 4;
        } else if (!forced && l.pipe && !small_launch) {
            float tail = env.env_tail;
            // (round 4, after the matrix stream lost its scalar overheads and 4-row tiles became relatively cheaper -- interleaved A/B,
            // profiles/r4_fork_tail.jsonl: the tail now also pays where round 3 excluded it, above 14 rounds with a nearly full last round
            // (1920x1080 undivided: 4.066 -> 4.052 ms); but NOT in the two bands of a forked call, whose launches run side by side and
            // end staggered anyway: 1920x1080 4.048 -> 4.018, 1600x900 2.853 -> 2.825, 1280x720 1.841 -> 1.834 ms without it)
            // (round 6: not in the exact mode's last stage either -- its 8-row tiles run on 4x4x1 MFMAs with 28 output columns, its 4-row
            // tiles still on 32x32x2 with 32, code the launch would otherwise never touch: 0.7775 -> 0.7695 ms at 1080p, profiles/r6_ab_quad.txt)
            // (nor in stage 2's Winograd form, whose 4-row tiles cost as many MFMAs as 8-row ones for the 5x5 source: 1080p stage 2 0.856 ms
            // with the tail, 0.837 without, profiles/r8_ab_wino_stage2.txt)
            if (tail < 0.0f) tail = (!split && rounds >= 3.0 && !forked && st != 4 && !(st == 2 && wino8)) ? 1.0f : 0.0f;
            if (tail > 0.0f) {
                const long per_row = (long)n * tiles_x;
                const int want = (int)((tail * resident + per_row - 1) / per_row);  // tile rows of small tiles
                l.ty8 = std::max(0, (rows - 4 * want) / 8);
                l.ty4 = std::max(0, (rows - 8 * l.ty8 + 3) / 4);
            }
        }
        if (!forced && l.pipe && !small_launch && !split && l.ty4 == 0 && rounds >= 3.0 && rows % 8 >= 1 && rows % 8 <= 4) {
            // the last 1-4 rows as ONE row of 4-row tiles instead of a mostly empty row of 8-row tiles (a band of a forked call, an image
            // height that is not a multiple of 8): half a tile row of matrix work saved
            l.ty8 = rows / 8; l.ty4 = 1;
        }
        if (l.ty8 > 0 && l.ty4 > 0 && (long)n * tiles_x * (l.ty8 + l.ty4) <= resident) {
            // (cannot happen with the rules above -- a tail is only added to launches of >= 2 rounds -- but a launch with a workgroup
            // per tile hands out tiles by workgroup number alone, which is only a bijection for ONE tile class)
            l.ty8 = 0; l.ty4 = (rows + 3) / 4;
        }
        l.th = l.ty8 > 0 ? 8 : 4;  // the one class of conv0 / the first form
        if (!l.pipe && l.ty8 > 0) { l.ty8 = (rows + 7) / 8; l.ty4 = 0; }
        const int ntiles = n * tiles_x * (l.ty8 + l.ty4);
        // the pipe form is persistent: one workgroup per resident slot, tiles from the queue; the first form one per tile
        l.grid = l.pipe ? std::min(ntiles, resident) : ntiles;
    }
}

bool sr_plan_fork(const sr_plan_env& env, int mode, bool img_u8, int img_ch, int n, int H, int W, int halo_top, int halo_bot, int* rows_a_out) {
    const int own = H - halo_top - halo_bot;
    bool fork = env.graph == SR_GRAPH_SR_NET && n == 1 && !env.profiling && mode != 0 && own >= 4 * SR_HALO &&
                sr_check_band_args(img_u8, img_ch, n, H, W, halo_top, halo_bot) == SR_OK;  // (anything sr_run_stack would refuse is left for it to refuse)
    if (fork && mode < 0) {
        // automatic: where the launches have enough rounds of tiles for two bands to fill the chip each (measured)
        const double rounds = sr_rounds(sr_plan_cus(env), W, own);
        // measured, interleaved in one process (scripts/fork_ab.py).  With the bands' launches free of 4-row tails (sr_tile_plan) the fork
        // wins wherever a band still has a few rounds of tiles, exact f32 (profiles/r4_fork_ab_f32_final_rule.jsonl): 800x600 (3.7 rounds)
        // -3.8 %, 1280x720 -1.6 %, 1920x1080 -0.8 %, 1920x1200 -0.9 %, 2560x1440 -0.4 %, 3840x2160 -0.1 %, a 276-row band of a 3840-wide
        // image -0.4 %; 960x540 (4.0 rounds) ties.  The split-half mode (tiles of 14 us) loses 0.6-2.4 % (r4_fork_ab_split.jsonl).
        fork = env.precision == SR_PRECISION_F32 && rounds >= env.fork_min_rounds && rounds < env.fork_max_rounds;
    }
    if (!fork) return false;
    // The first band's own rows: near the requested share, at the cut (within +-8 rows of it) that wastes the least matrix work in
    // partly filled tile rows.  Stage s of the first band computes rows_a + margin rows from the band's top, of the second band
    // own - rows_a + margin rows; a remainder of 1-4 rows costs a row of 4-row tiles (0.52 of an 8-row one), 5-7 rows a full one.
    int rows_a = mode > 1 ? mode : (int)(own * env.fork_share);
    rows_a = std::max(2 * SR_HALO, std::min(rows_a, own - 2 * SR_HALO));
    if (mode <= 1) {
        static const double weight[5] = {0.0, 25600.0, 34816.0, 44032.0, 28800.0};  // issued MACs per pixel of stages 1-4 (conv0: negligible)
        const bool fours = env.precision == SR_PRECISION_F32;
        auto tile_rows = [&](int rows) { const int r = rows % 8; return rows / 8 + (r == 0 ? 0.0 : (r <= 4 && fours) ? 0.52 : 1.0); };
        double best = 1e300;
        int best_rows = rows_a;
        for (int cand = rows_a - 8; cand <= rows_a + 8; ++cand) {
            if (cand < 2 * SR_HALO || own - cand < 2 * SR_HALO) continue;
            double cost = 0.0;
            for (int st = 1; st < 5; ++st) {
                const int ra = cand + kStageMargin[st] + std::min(halo_top, kStageMargin[st]), rb = own - cand + kStageMargin[st] + std::min(halo_bot, kStageMargin[st]);
                cost += weight[st] * (tile_rows(ra) + tile_rows(rb));
            }
            cost += 1e-3 * std::abs(cand - rows_a);  // ties: the cut nearest the requested share
            if (cost < best) { best = cost; best_rows = cand; }
        }
        rows_a = best_rows;
    }
    *rows_a_out = rows_a;
    return true;
}

bool sr_fork_tunable(const sr_plan_env& env, int n, int H, int W, int halo_top, int halo_bot, bool gated) {
    if (!env.fork_autotune || env.env_fork >= 0 || env.graph != SR_GRAPH_SR_NET || n != 1 || env.profiling || gated || W <= 0) return false;
    const int own = H - halo_top - halo_bot;
    if (own < 4 * SR_HALO) return false;
    const double rounds = sr_rounds(sr_plan_cus(env), W, own);
    return rounds >= kForkTuneMinRounds && rounds < kForkTuneMaxRounds;
}

// Split the job.  Batches go in chunks of ~1M px of whole images.  A single large sr_net image goes as row bands: band k
// owns rows [y0,y1) and carries them plus SR_HALO rows on every side that is not an image edge.  Bands may differ in
// height -- a workspace that meets a new geometry only has its border re-cleared (ensure_features), microseconds.
// [y_lo, y_hi): the image rows this call is to produce (a whole image: 0, h; a device's share of a multi-GPU
// call: its rows, sr_net and n == 1 only).
std::vector<sr_chunk> sr_plan_chunks(const sr_plan_env& env, sr_deal deal, int h, int w, size_t in_px_bytes, size_t out_px_bytes, int y_lo, int y_hi,
                               bool* in_order) {
    std::vector<sr_chunk> plan;
    *in_order = false;
    const int f = env.factor, n = deal.count;
    const size_t in_img = (size_t)h * w * in_px_bytes;
    const size_t out_img = env.graph == SR_GRAPH_DOWNSAMPLE ? (size_t)(h / 3) * (w / 3) * out_px_bytes
                                                           : (size_t)h * f * w * f * out_px_bytes;
    const size_t in_step = in_img * deal.stride, out_step = out_img * deal.stride;
    const bool pipe = env.pipeline && !env.profiling;  // per-stage profiling times one undivided pass
    const int per = (int)std::max<size_t>(1, ((size_t)1 << 20) / ((size_t)h * w));  // images per chunk: ~1M px of work
    if (pipe && n > per) {
        for (int i = 0; i < n; i += per) {
            const int m = std::min(per, n - i);
            const size_t img = (size_t)deal.first + (size_t)i * deal.stride;
            plan.push_back({img * in_img, m * in_img, img * out_img, m * out_img, m, h, 0, 0, in_step, out_step});
        }
        return plan;
    }
    const bool part = y_lo > 0 || y_hi < h;  // a share of the image: always in band form (halo rows from the image itself)
    const int span = y_hi - y_lo;
    std::vector<int> rows;  // rows of each band, top to bottom
    int forced_rows = 0;
    for (int rk : env.env_rows) forced_rows += rk;
    const bool forced_plan = (!env.env_rows.empty() && forced_rows == span) || env.env_bands > 0;  // (sr_set_experiment "rows" / "bands": at any size)
    // Below 2^19 px a lone frame used to go as ONE chunk: upload, kernels, download, nothing overlapping.  Round 6, u8 output, from
    // ~200K px on: TWO bands in order on one stream -- the first band's download runs under the second band's kernels, which is worth more
    // than the second band's 7 recomputed rows and five launches cost (scripts/host_plan_sweep.py, profiles/r6_host_mid_plans.txt: exact f32,
    // 70 / 30: 640x480 0.970 -> 0.873 ms, 854x480 1.311 -> 1.138, 800x600 1.420 -> 1.330, 720x576 1.312 -> 1.186, 960x540 1.479 -> 1.342;
    // the split-half mode, whose kernels are shorter beside the same download, 60 / 40: 640x480 0.536 -> 0.468, 800x600 0.792 -> 0.660,
    // 960x540 0.837 -> 0.701; at 320x320 neither mode gains).  Equal bands on alternating streams are within 2 % of these on most shapes
    // and 6 % better on some (800x600), 6 % worse on others: the in-order plan is the even-tempered one.
    // (from 200K px in exact f32 -- 448x448 -5.4 %, 640x360 -6.5 %, 640x480 -5.5 % against one chunk measured alternately, but 430x419 +3 % -- and
    // from 180K px in the split-half mode: 430x419 -4 %, 448x448 -11 %)
    // f32 OUTPUT (three times the download, as long as the kernels or longer): in-order bands pay more still -- exact f32 60 / 40: 448x448
    // 0.982 -> 0.801 ms, 640x480 1.379 -> 1.143; three equal bands from 400K px: 800x600 2.186 -> 1.556, 960x540 2.253 -> 1.784; split-half
    // two equal bands: 448x448 0.686 -> 0.603, three from 300K px: 640x480 0.974 -> 0.845, 800x600 1.472 -> 1.234, 960x540 1.582 -> 1.328.
    const bool split_mode = env.precision == SR_PRECISION_SPLIT_F16;
    const size_t px_span = (size_t)span * w;
    // (f32 output, smaller frames: exact f32 60 / 40 at 384x384 0.737 -> 0.621, at 320x320 0.578 -> 0.500; split-half 50 / 50 at 384x384 0.523 -> 0.483,
    // at 320x320 -3 %: from 100K / 140K px)
    const size_t mid_lo = out_px_bytes == 4 ? (split_mode ? 180000u : 200000u) : (split_mode ? 140000u : 100000u);
    const bool mid_size = px_span >= mid_lo && px_span < ((size_t)1 << 19);
    if (pipe && n == 1 && env.graph == SR_GRAPH_SR_NET && (forced_plan || mid_size || (size_t)span * w >= ((size_t)1 << 19))) {
        // Kernel and download time per input pixel decide the shape of the plan (measured, page-locked buffers, PCIe 5 x16):
        const double kern_ns = (env.precision == SR_PRECISION_SPLIT_F16 ? 0.9 : 2.0) * (f == 4 ? 1.2 : 1.0);
        const double d2h_ns = (double)out_px_bytes * f * f / 52.0;
        const double rho = kern_ns / d2h_ns;
        if (!env.env_rows.empty() && forced_rows == span) {  // sr_set_experiment("rows"): exactly these bands
            rows = env.env_rows;
            *in_order = !env.env_rows_two;
        } else if (env.env_bands > 0) {  // sr_set_experiment("bands"): that many equal bands
            const int nb = std::min(env.env_bands, span / (2 * SR_HALO));
            for (int k = 0; k < nb; ++k) rows.push_back((span * (k + 1)) / nb - (span * k) / nb);
        } else if (mid_size) {
            const bool u8_out = out_px_bytes == 4;
            if (!u8_out && px_span >= (split_mode ? 300000u : 400000u) && span >= 6 * SR_HALO) {
                const int third = span / 3 / 8 * 8;
                rows = {third, third, span - 2 * third};
            } else {
                const double share = u8_out ? (split_mode ? 0.6 : 0.7) : (split_mode ? 0.5 : 0.6);
                const int first = (int)(span * share) / 8 * 8;
                if (first >= 2 * SR_HALO && span - first >= 2 * SR_HALO) rows = {first, span - first};
            }
            *in_order = !rows.empty();
        } else {
            // Compute-bound (f32 arithmetic, u8 output: rho = 2.9): only the LAST band's download is exposed, and band
            // i's download hides under band i+1's kernels as long as band i+1 is at least 1/rho of it -- bands that
            // shrink geometrically, as many as keep the last one >= 300K px (smaller bands no longer fill the chip: at
            // 1080p the 128-row third band costs more than it hides, 4.95 against 4.85 ms with four equal bands).
            // They compute IN ORDER on one stream: on two, band 1 runs beside band 0, both finish late and the
            // largest download is the exposed one (1080p 5.54 ms).  Measured (scripts/geo_exp.py), geometric
            // against equal bands: 2560x1440 8.17 / 8.37 ms, 3840x2160 17.50 / 17.78 ms.
            const double r = std::min(rho * 0.85, 3.0);
            int nb = 1;
            double sum = 1.0, term = 1.0;
            while (rho >= 2.0 && env.env_geo && nb < 5 && (double)span * w / (sum + term * r) >= 300e3) { term *= r; sum += term; ++nb; }
            if (nb >= 3) {
                int left = span;
                for (int k = 0; k < nb - 1; ++k) {
                    int rk = (int)((double)span * term / sum) / 8 * 8;  // whole 8-row tiles
                    rk = std::max(2 * SR_HALO, std::min(rk, left - 2 * SR_HALO));
                    rows.push_back(rk);
                    left -= rk;
                    term /= r;
                }
                rows.push_back(left);
                *in_order = true;
            } else if (rho >= 2.0 && env.env_geo && (double)span * w >= 800e3) {
                // Compute-bound, but too small for three bands in order (720p .. ~2.8 M px): on alternating streams, two equal
                // bands that keep the chip full, then a tail -- the exposed download is the last band's, so that one is
                // ~150K px (smaller no longer pays its five launches), from 1.8 M px on with a band of 2.5x that in front of
                // it under which the second big band's download finishes.  Measured round 3 (scripts/host_plan_sweep.py,
                // profiles/r3_host_plans.txt), against the equal bands of round 2: 1920x1080 400,400,200,80 = 4.60 against
                // 4.89 ms; 1600x900 3.36 / 3.54; 1280x720 2.22 / 2.36.  2560x1440 is the geometric plan's either way.
                const int last = std::max(16, (int)(150e3 / w + 4.0) / 8 * 8);
                const int mid = (double)span * w >= 1.8e6 ? (5 * last / 2) / 8 * 8 : 0;
                const int big = (span - last - mid) / 2 / 8 * 8;
                if (big >= 2 * last) {
                    rows = {big, span - last - mid - big};
                    if (mid) rows.push_back(mid);
                    rows.push_back(last);
                }
            }
        }
        if (rows.empty() && !mid_size) {
            // Download-bound or balanced (f32 output, the split-half mode): equal bands.  Few expose the first upload
            // and the last download, many pay 14 recomputed rows and five launches each.  Measured, f32 1080p
            // 1 / 2 / 4 / 5 / 8 bands = 5.96 / 5.14 / 4.93 / 5.12 / 5.22 ms; the split-half mode computes 2.2x faster
            // than the bus drains its output and prefers more: 4 / 5 / 6 / 8 bands = 3.77 / 2.7-3.4 / 2.82 / 3.05 ms.
            // Round 6, f32 OUTPUT re-measured on this round's kernels (scripts/host_plan_sweep.py, profiles/r6_host_mid_plans.txt 6.): five equal bands
            // IN ORDER on one stream, eight from 3 M px, beat the equal bands on alternating streams of rounds 2-3 in a process of its own (a C / Rust
            // host) -- exact f32 1280x720 3.53 -> 2.71 ms, 1920x1080 6.25 -> 5.69, 3840x2160 21.1 -> 19.9; split-half 2.29 -> 2.17, 4.74 -> 4.60,
            // 17.8 -> 17.2 -- and are within +-6 % of them inside bench.py's long-lived torch process (exact f32 1920x1080 6.17 against 5.85, split-half
            // 4.60 against 4.93: 7.).
            // The split-half mode with u8 output keeps its equal bands on alternating streams: bands in order that shrink by 0.85 are 3-6 % faster
            // in a fresh process (1920x1080 2.30 -> 2.12 ms) but read 3.37 ms for the first dozens of calls inside bench.py's process -- no overlap at
            // all between the one compute stream and the download stream, which two compute streams never lose entirely (7.); not adopted.
            if (out_px_bytes != 4) {
                const int nb = std::min(px_span < 3000000u ? 5 : 8, std::max(1, span / (2 * SR_HALO)));
                for (int k = 0; k < nb; ++k) rows.push_back((span * (k + 1)) / nb - (span * k) / nb);
                *in_order = true;
            } else {
                int nb = span / (split_mode ? 176 : 256);
                if (nb > 8) nb = 8;
                for (int k = 0; k < nb; ++k) rows.push_back((span * (k + 1)) / nb - (span * k) / nb);
            }
        }
    }
    const size_t img0_in = (size_t)deal.first * in_img, img0_out = (size_t)deal.first * out_img;
    if (rows.size() >= 2) {
        bool ok = true;
        int y0 = y_lo;
        for (int rk : rows) {
            const int y1 = y0 + rk;
            const int start = std::max(0, y0 - SR_HALO), end = std::min(h, y1 + SR_HALO);
            const int ht = y0 - start, hb = end - y1;
            // sr_run_stack's rules: a halo is SR_HALO rows or, at an image edge, none
            ok = ok && rk > 0 && (ht == 0 || ht == SR_HALO) && (hb == 0 || hb == SR_HALO);
            plan.push_back({img0_in + (size_t)start * w * in_px_bytes, (size_t)(end - start) * w * in_px_bytes,
                            img0_out + (size_t)y0 * f * w * f * out_px_bytes, (size_t)rk * f * w * f * out_px_bytes, 1, end - start, ht, hb,
                            0, 0});
            y0 = y1;
        }
        if (ok && y0 == y_hi) return plan;
        plan.clear();
    }
    if (part) {  // one band: the rows themselves plus SR_HALO rows on every side that is not an image edge
        const int start = std::max(0, y_lo - SR_HALO), end = std::min(h, y_hi + SR_HALO);
        plan.push_back({img0_in + (size_t)start * w * in_px_bytes, (size_t)(end - start) * w * in_px_bytes,
                        img0_out + (size_t)y_lo * f * w * f * out_px_bytes, (size_t)span * f * w * f * out_px_bytes, 1, end - start,
                        y_lo - start, end - y_hi, 0, 0});
        return plan;
    }
    plan.push_back({img0_in, (size_t)n * in_img, img0_out, (size_t)n * out_img, n, h, 0, 0, in_step, out_step});
    return plan;
}

// ---- the row-reuse planner of the frame stream (include/srhip.h "Video"; restated in tests/reuse_ref.py) ----
// Which LR rows a frame must compute, from the row flags of the compare against the last frame.  The two constants are reasons, not
// tuned values: a separate band recomputes up to 2 SR_HALO margin rows (its two halos), so a gap of fewer clean rows is cheaper computed
// than skipped, and a plan whose rows plus margins reach the frame is cheaper as the frame; four bands bound the launches of a frame.
extern "C" int sr_video_reuse_plan(const uint32_t* plane_flags, int subsampling, int h, sr_row_band* bands, int max_bands, int* n_bands) {
    if (n_bands) *n_bands = 0;
    if (!plane_flags || !bands || !n_bands || h < 1 || max_bands < 1) return SR_E_INVALID;
    if (subsampling != SR_YUV_420 && subsampling != SR_YUV_444 && subsampling != SR_YUV_422) return SR_E_INVALID;
    const bool sub420 = subsampling == SR_YUV_420;
    const int ch = sub420 ? (h + 1) / 2 : h;
    // needed rows: within SR_HALO of an RGB-dirty row
    std::vector<char> need((size_t)h, 0);
    auto dirty = [&](int lo, int hi) {  // RGB-dirty rows lo .. hi
        for (int y = std::max(0, lo - SR_HALO); y <= std::min(h - 1, hi + SR_HALO); ++y) need[(size_t)y] = 1;
    };
    for (int y = 0; y < h; ++y)
        if (plane_flags[y]) dirty(y, y);
    for (int p = 0; p < 2; ++p)
        for (int c = 0; c < ch; ++c)
            if (plane_flags[(size_t)h + (size_t)p * ch + c]) {
                // 4:2:0: the luma rows whose vertical taps read C[c] -- 2i reads C[i-1], C[i]; 2i + 1 reads C[i], C[i+1]
                if (sub420) dirty(std::max(0, 2 * c - 1), std::min(h - 1, 2 * c + 2));
                else dirty(c, c);
            }
    // maximal runs, edges on even rows (or h) and never inside SR_HALO of an image edge; close runs merged
    std::vector<sr_row_band> run;
    for (int y = 0; y < h;) {
        if (!need[(size_t)y]) { ++y; continue; }
        int e = y;
        while (e < h && need[(size_t)e]) ++e;
        int a = y & ~1, b = std::min(h, (e + 1) & ~1);
        if (a < SR_HALO) a = 0;
        if (h - b < SR_HALO) b = h;
        if (!run.empty() && a - run.back().y1 < 2 * SR_HALO) run.back().y1 = std::max(run.back().y1, b);
        else run.push_back({a, b});
        y = e;
    }
    while ((int)run.size() > SR_REUSE_MAX_BANDS) {  // the smallest gap goes; of equal gaps the one nearer the top
        size_t at = 0;
        for (size_t i = 1; i + 1 < run.size(); ++i)
            if (run[i + 1].y0 - run[i].y1 < run[at + 1].y0 - run[at].y1) at = i;
        run[at].y1 = run[at + 1].y1;
        run.erase(run.begin() + (long)at + 1);
    }
    long cost = 0;
    for (const sr_row_band& r : run) cost += r.y1 - r.y0 + 2 * SR_HALO;
    if (!run.empty() && cost >= h) run.assign(1, sr_row_band{0, h});
    if ((int)run.size() > max_bands) return SR_E_INVALID;
    for (size_t i = 0; i < run.size(); ++i) bands[i] = run[i];
    *n_bands = (int)run.size();
    return SR_OK;
}
