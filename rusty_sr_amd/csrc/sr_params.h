// sr_params.h -- the parameter vector of sr_net(f) (the .rsr payload): one table of its 19 segments, in the op insertion order of the
// reference's src/network.rs:33-72.  Everything else -- lengths, offsets, fan-in, the total -- is derived from it.
// Only the expand node depends on the factor f: 3 f^2 channels (network.rs:37), so expand_bias and conv7 / conv9 / conv10 scale with it.
// Host code only; included by .cpp sources and by the host side of .hip sources.
#pragma once
#include <cstddef>

enum sr_seg {
    SR_SEG_CONV0, SR_SEG_F_BIAS, SR_SEG_F_ACTIV, SR_SEG_EXP_BIAS, SR_SEG_L1_BIAS, SR_SEG_L2_BIAS, SR_SEG_L3_BIAS, SR_SEG_L1_ACTIV,
    SR_SEG_L2_ACTIV, SR_SEG_L3_ACTIV, SR_SEG_CONV1, SR_SEG_CONV2, SR_SEG_CONV3, SR_SEG_CONV5, SR_SEG_CONV6, SR_SEG_CONV7, SR_SEG_CONV8,
    SR_SEG_CONV9, SR_SEG_CONV10, SR_SEGS
};

enum sr_seg_kind { SR_KIND_CONV, SR_KIND_BIAS, SR_KIND_BETA };

// A convolution's weights are [cout][ks][ks][cin]; a bias or a BeLU beta has cout values.  cout = kSrExpand: the 3 f^2 expand channels.
// init_mult: the factor on a convolution's He deviation sqrt(2 / fan_in) at initialisation (sr_init_params).
constexpr int kSrExpand = 0;
struct sr_seg_def {
    sr_seg_kind kind;
    int cout, ks, cin;
    double init_mult;
};
constexpr sr_seg_def kSrSegDefs[SR_SEGS] = {
    {SR_KIND_CONV, 32, 5, 3, 1.0},                                                           // conv0
    {SR_KIND_BIAS, 32, 0, 0, 0}, {SR_KIND_BETA, 32, 0, 0, 0},                                // f_bias, f_activ
    {SR_KIND_BIAS, kSrExpand, 0, 0, 0},                                                      // expand_bias
    {SR_KIND_BIAS, 32, 0, 0, 0}, {SR_KIND_BIAS, 32, 0, 0, 0}, {SR_KIND_BIAS, 32, 0, 0, 0},   // l1 .. l3 biases
    {SR_KIND_BETA, 32, 0, 0, 0}, {SR_KIND_BETA, 32, 0, 0, 0}, {SR_KIND_BETA, 32, 0, 0, 0},   // l1 .. l3 activations
    {SR_KIND_CONV, 32, 5, 32, 0.1}, {SR_KIND_CONV, 32, 5, 32, 0.1}, {SR_KIND_CONV, 32, 5, 32, 0.1},  // conv1 .. conv3: f -> l1, l2, l3
    {SR_KIND_CONV, 32, 3, 32, 0.1}, {SR_KIND_CONV, 32, 3, 32, 0.1},                          // conv5, conv6: l1 -> l2, l3
    {SR_KIND_CONV, kSrExpand, 3, 32, 0.1},                                                   // conv7: l1 -> expand
    {SR_KIND_CONV, 32, 3, 32, 0.1},                                                          // conv8: l2 -> l3
    {SR_KIND_CONV, kSrExpand, 3, 32, 0.1}, {SR_KIND_CONV, kSrExpand, 3, 32, 0.1},            // conv9, conv10: l2, l3 -> expand
};

struct sr_param_layout {
    int E;  // expand channels
    size_t off[SR_SEGS], len[SR_SEGS], total;
    explicit sr_param_layout(int f) : E(3 * f * f), total(0) {
        for (int s = 0; s < SR_SEGS; ++s) {
            off[s] = total;
            len[s] = is_conv(s) ? (size_t)cout(s) * fan_in(s) : (size_t)cout(s);
            total += len[s];
        }
    }
    static bool is_conv(int s) { return kSrSegDefs[s].kind == SR_KIND_CONV; }
    static int ks(int s) { return kSrSegDefs[s].ks; }
    static int cin(int s) { return kSrSegDefs[s].cin; }
    static int fan_in(int s) { return ks(s) * ks(s) * cin(s); }
    int cout(int s) const { return kSrSegDefs[s].cout == kSrExpand ? E : kSrSegDefs[s].cout; }
};
