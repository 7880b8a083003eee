/*
 * srhip_experimental.h -- tuning switches of libsrhip.so that are NOT part of the drop-in C ABI (include/srhip.h).
 *
 * Nothing here has a counterpart in the reference (millardjn/rusty_sr has no tuning surface: src/main.rs:33-127 is its
 * whole CLI) and nothing here changes a result bit.  The switches exist for interleaved A/B timing (scripts/ab_libs.py,
 * scripts/fork_ab.py, scripts/band_profile.py) and for the tests that prove bit-identity across kernel forms and tile
 * plans (tests/test_gpu_parity.py).  Keys, values and defaults may change between builds; a host that binds
 * include/srhip.h alone (rust_host/src/srhip.rs, the C++ CLI) never needs this file.
 *
 * Stream capture (include/srhip.h): a captured *_dev call records the plan that the switches stood for when it was captured, and
 * sr_set_experiment is one of the calls after which replaying a graph of this context is undefined ("fork", "forktune" and "cus" can free or
 * re-plan what its nodes point to).  Set the switches first, capture afterwards.
 */
#ifndef SRHIP_EXPERIMENTAL_H
#define SRHIP_EXPERIMENTAL_H

#include "srhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sr_set_experiment(ctx, key, value).  key "th": tile height, value "" (automatic: 8-row tiles ended by 4-row tiles, or 4-row tiles only for
 * small launches), "4" / "8" (all stages) or five digits (one per stage); "tail": how many 4-row tiles end a launch of
 * 8-row tiles, in units of the resident workgroups ("" automatic: 1 where it pays, "0" none); "pipe": "none" forces the first
 * form of the stage kernels (one tile class per launch), "all" the pipe form also for small launches ("" automatic); "bw": width in tiles of the column blocks the tile queue walks
 * ("" automatic, "0" plain row-major); "bands": the host pipeline cuts one large image into that many equal row bands
 * ("" / "0": its own plan); "rows": the bands' heights themselves, "r0,r1,..." top to bottom, computed in order on one stream, or with a
 * leading '=' on alternating streams (used when they add up to the rows of the call); "geo": "0" keeps equal bands where the plan would
 * shrink them geometrically; "halo": what a sharded call (sr_upscale_sharded_*) exchanges -- "" / "input": 7 input rows per
 * neighbour, the overlap recomputed; "layers": additionally the edge rows of every layer's output after its stage
 * (f 2 rows, l1 / l2 / l3 one each), nothing recomputed (8(e)(ii)); every context of a call must say the same.
 * "fork": a lone image through a device entry point as two row bands on two streams -- "" automatic, "0" never, "1" always, N > 1 always
 * with N rows in the first band; "forkshare" / "forkmin": the first band's share of the rows, the automatic rule's threshold in rounds of
 * tiles; "forktune": "" / "1" -- for mid-size shapes (0.55-12 rounds of tiles) the automatic choice is MEASURED on the caller's own calls
 * (four undivided, four forked, timed by event pairs that are queried, never waited for; then the faster plan stays for that shape),
 * "0" -- the rule alone; setting it forgets what was measured.
 * "wino": the exact mode's convolutions as row-direction Winograd F(2,3) -- "": the 5x5 convolutions over f of stages 1 and 2 (conv1,
 * conv2; 7 products per kernel row and output pair instead of 10) and input channels 0-15 of stage 2's 3x3 source (conv5; 4 products
 * instead of 6), whose channels 16-31 stay direct; "2": conv1 and conv2 only, conv5 direct (the form before conv5's: its bits); "3":
 * both halves of conv5 as well (for measurement only, never the default: it takes the call too close to the f32 roof that bench.py's
 * contract holds it below); "1": stage 1's conv1 only; "0": every stage in the direct form.  Unlike the others this switch changes the last bits of f32 results (every setting is
 * held to the same parity bar); every kernel form, tile class and band of one setting stays bit-identical to the others.
 * "auxgrid": the parameter-free graphs (SR_GRAPH_BILINEAR / SR_GRAPH_DOWNSAMPLE) -- "" automatic, "N" (N >= 1): every launch of their kernels
 * takes min(automatic grid, N) workgroups.  The kernels walk their tiles / items with the grid as stride, so a small N reaches their
 * multi-round paths (carries of the item counter, the prefetch of the next round) at tiny shapes and on any CU count; host side only, no
 * output byte depends on it.  Anything but "" or a positive integer: SR_E_INVALID.  (No environment default.)
 * "cus": how many compute units the planners take the device to have -- "" its own count, "N" (1 <= N <= that count, decimal digits only;
 * anything else: SR_E_INVALID): the tile planner (tile classes, first or pipe form, workgroups of a persistent launch = min(tiles, 2 N)),
 * the fork rule and its tuner's range, and conv0's grid (min(tiles, 8 N)) plan as if it had N.  The stage kernels take their tiles from
 * the per-XCD queues whenever a launch has fewer workgroups than tiles, so N of 1-5 reaches the queue, its steals (with fewer than 8
 * workgroups whole queues have no owner and are emptied by steals alone), the change of tile class inside a workgroup, 16 and more tiles
 * through one workgroup and the forked plans on images of a few thousand pixels (tests/test_gpu_tile_queue.py); sr_device_info keeps
 * reporting the device's own count.  Host side only -- no kernel and no launch argument differs while it is unset -- and no output byte
 * depends on it.  Setting it forgets what the fork tuner measured, like "forktune".  (No environment default.)
 * "vyuv": the vertical pass of a resampling that ends in a YCbCr frame (srhip.h "Video at any size") -- "" the measured rule: a format
 * class runs the fused kernel where that is not slower than the two kernels it replaces, else those two; "1" | "2": the
 * fused kernel for every class, with that many row pairs a workgroup; "chain": resize_v + rgb_to_yuv for every class.  For measurement
 * and tests: no output byte depends on it.  Anything else: SR_E_INVALID.  (No environment default.)
 * Every key is host-side state that a call reads when it is QUEUED (launch arguments travel by value): a switch may be set while earlier
 * *_dev calls are still in flight on the caller's stream -- nothing waits, and the calls already queued keep the plan they were queued
 * with (tests/test_gpu_stream_order.py changes "fork", "th" and "pipe" between queued calls).
 * Defaults come from SRHIP_WINO / SRHIP_TH / SRHIP_TAIL / SRHIP_PIPE / SRHIP_BW / SRHIP_BANDS / SRHIP_ROWS / SRHIP_GEO / SRHIP_HALO, read once in sr_create.
 * Unknown key: SR_E_INVALID. */
int sr_set_experiment(sr_ctx* ctx, const char* key, const char* value);

/* What a switch has learned, as text (NUL-terminated, into buf[cap]).  key "forktune": one line per shape the fork tuner has met,
 * "HxW+halo_top+halo_bot precision io state undivided_ms forked_ms" with state measuring | undivided | forked (0.0000: not measured yet).
 * key "plan" (a test hook): what the last call of an entry point on this context ran -- every sr_upscale_* / sr_reserve_* call clears it,
 * the calls over several contexts clear each of theirs.  One line per decision, in the order they were made:
 *   "host KIND s0,s1,... [rows=y0:y1]"  the host pipeline's chunk plan: KIND one | batch (s: images per chunk) | inorder | alternating
 *                                       (s: the row bands' heights, computed in order on one stream / on alternating streams); rows=: the
 *                                       share of the image a multi-context call gave this context;
 *   "fork 0" | "fork 1 a,b"             a device call undivided, or as two bands of a and b rows ("fork 0 nomem": no room for the second);
 *   "launch st=S form=first|pipe ty8=A ty4=B grid=G prec=f32|split_f16 f=F img=u8|f32 out=u8|f32 ch=C"
 *                                       one launch of stage S (0: conv0, 4: the final stage): A rows of 8-row tiles then B rows of 4-row
 *                                       tiles, G workgroups; C: channels of the input image.
 *   "aux graph=bilinear|downsample img=u8|f32 ch=C grid=G units=U"
 *                                       one launch of a parameter-free graph: G workgroups walk U pieces, a workgroup every G-th -- tiles
 *                                       (64 x 16 input pixels, bilinear f32; 64 x 4 output pixels, downsample), or for the u8 bilinear kernel
 *                                       groups of four wave items (an item: 64 16-byte chunks of one input row's three output rows), U =
 *                                       ceil(items / 4).  The launch is multi-round exactly when U > G.
 * Identical lines in a row are one, followed by " xN".  Host-side text written where the decisions are made: no result depends on it.
 * Unknown key, or a buffer too small: SR_E_INVALID. */
int sr_get_experiment(sr_ctx* ctx, const char* key, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SRHIP_EXPERIMENTAL_H */
