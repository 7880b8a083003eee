// plan_check.cpp -- the tile, fork and host-chunk planners (rusty_sr_amd/csrc/sr_plan.cpp) without a GPU: built by g++ from sr_plan.cpp
// alone, under ASan and UBSan (tests/test_plan_cpu.py) -- that it builds so is the check that the module needs no HIP.
//
// stdin: one call per line, key=value words (tests/plan_cases.py check_line): id cus factor prec call io n h w top bot engines pipeline
// profiling, and the switches as the fields of sr_plan_env they set: [wino] [th=DDDDD] [pipe] [tail] [fork] [forkshare] [forkmin] [bands]
// [rows=R0,R1,..] [rows_two] [geo].  stdout, per call, the planners composed in the order the library composes them:
//     case ID
//     ctx K                           one per context of the call (a context that takes no part: nothing below it)
//     host KIND SIZES [rows=LO:HI]    a host call: its chunks, then each chunk's pass
//     fork 0 | fork 1 ROWS_A,ROWS_B   a device call: undivided, or its two bands' passes interleaved stage by stage
//     launch ST FORM TY8 TY4 GRID
// and, for the test's own checks, "# pass OWN TOP BOT" (a pass over OWN rows with TOP / BOT halo rows) before a pass's first launch and
// "# rows Y0 Y1" (the rows a launch computes) before each launch.
// The "host" and "fork" lines restate what sr_api.cpp writes into the plan record (run_host's "host ..." note: kind, sizes, rows=; the
// "fork 0" / "fork 1 a,b" notes of sr_run_stack_auto): whoever changes that text changes it here (tests/test_gpu_plan_records.py compares).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../rusty_sr_amd/csrc/sr_plan.h"

namespace {

void launch_line(const sr_launch_plan& l, int st) {
    printf("# rows %d %d\nlaunch %d %s %d %d %d\n", l.y0, l.y1, st, l.pipe ? "pipe" : "first", l.ty8, l.ty4, l.grid);
}

// sr_run_stack: one undivided pass
void pass(const sr_plan_env& env, int n, int H, int W, int top, int bot) {
    sr_launch_plan L[5];
    sr_tile_plan(env, n, H, W, top, H - bot, false, false, L);
    printf("# pass %d %d %d\n", H - top - bot, top, bot);
    for (int st = 0; st < 5; ++st) launch_line(L[st], st);
}

// sr_run_stack_auto with the fork tuner off
int device_call(const sr_plan_env& env, bool u8, int n, int H, int W, int top, int bot) {
    if (sr_check_band_args(u8, 3, n, H, W, top, bot) != SR_OK || sr_fork_tunable(env, n, H, W, top, bot, false)) return 1;
    int rows_a = 0;
    if (!sr_plan_fork(env, env.env_fork, u8, 3, n, H, W, top, bot, &rows_a)) {
        printf("fork 0\n");
        pass(env, n, H, W, top, bot);
        return 0;
    }
    printf("fork 1 %d,%d\n", rows_a, H - top - bot - rows_a);
    sr_fork_band fb[2];
    sr_fork_bands(H, top, bot, rows_a, fb);
    sr_launch_plan L[2][5];
    for (int k = 0; k < 2; ++k) {
        const sr_fork_band& b = fb[k];
        sr_tile_plan(env, 1, b.H, W, b.top, b.bot, true, false, L[k]);
        printf("# pass %d %d %d\n", b.bot - b.top, b.top, b.H - b.bot);
    }
    for (int st = 0; st < 5; ++st)
        for (int k = 0; k < 2; ++k) launch_line(L[k][st], st);
    return 0;
}

// run_host: rows [y_lo, y_hi) of the n images
void host_call(const sr_plan_env& env, bool u8, int n, int h, int w, int y_lo, int y_hi) {
    const size_t in_px = u8 ? 3 : 3 * sizeof(float), out_px = u8 ? 4 : 3 * sizeof(float);
    bool in_order = false;
    const std::vector<sr_chunk> plan = sr_plan_chunks(env, sr_deal{0, 1, n}, h, w, in_px, out_px, y_lo, y_hi, &in_order);
    const bool bands = plan.size() > 1 && (plan[0].halo_top > 0 || plan[0].halo_bot > 0);
    printf("host %s", plan.size() == 1 ? "one" : !bands ? "batch" : in_order ? "inorder" : "alternating");
    for (size_t i = 0; i < plan.size(); ++i)
        printf("%c%d", i ? ',' : ' ', bands ? (int)(plan[i].out_bytes / ((size_t)env.factor * env.factor * w * out_px)) : plan[i].n);
    if (y_lo > 0 || y_hi < h) printf(" rows=%d:%d", y_lo, y_hi);
    printf("\n");
    for (const sr_chunk& k : plan) pass(env, k.n, k.h_ext, w, k.halo_top, k.halo_bot);
}

// The sizes of a composed call (sr_plan.h: sr_reserve_bufs' sum, sr_net_queue's strides) at their limits, before any case is read: a sum
// that leaves size_t is reported, not wrapped, and the last image of a batch of 2^31 - 1 lies where 64-bit arithmetic puts it.
struct want { size_t bytes; };
bool sizes_ok() {
    size_t sum = 0;
    const want fits[] = {{SIZE_MAX - 7}, {0}, {7}}, over[] = {{SIZE_MAX - 7}, {0}, {8}}, twice[] = {{SIZE_MAX / 2 + 1}, {SIZE_MAX / 2 + 1}};
    if (!sr_sum_wants(fits, &sum) || sum != SIZE_MAX || sr_sum_wants(over, &sum) || sr_sum_wants(twice, &sum)) return false;
    const int n = INT32_MAX;
    const sr_net_strides u8 = sr_net_image_strides(3, true, 4, true, 9, 7), f32 = sr_net_image_strides(4, false, 3, false, 9, 7), rgb = sr_net_image_strides(2, true, 3, false, 1, 1);
    if (u8.in_img != 252 || u8.out_img != 2268 || f32.in_img != 756 || f32.out_img != 12096 || rgb.in_img != 3 || rgb.out_img != 48) return false;
    return (size_t)(n - 1) * u8.out_img == 4870492909128ull && (size_t)(n - 1) * f32.out_img == 25975962182016ull;
}

}  // namespace

int main() {
    if (!sizes_ok()) { fprintf(stderr, "plan_check: the composed calls' sizes are wrong\n"); return 3; }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::map<std::string, std::string> kv;
        sr_plan_env env;
        env.fork_autotune = false;  // ("forktune" = "0": every case)
        std::istringstream words(line);
        for (std::string word; words >> word;) {
            const size_t eq = word.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "plan_check: no '=' in \"%s\"\n", word.c_str()); return 2; }
            const std::string key = word.substr(0, eq), value = word.substr(eq + 1);
            kv[key] = value;
        }
        auto num = [&](const char* key) { return atoi(kv.at(key).c_str()); };
        env.cus = num("cus");
        env.factor = num("factor");
        env.precision = kv.at("prec") == "split_f16" ? SR_PRECISION_SPLIT_F16 : SR_PRECISION_F32;
        env.pipeline = num("pipeline");
        env.profiling = num("profiling") != 0;
        if (kv.count("wino")) env.wino = num("wino");
        if (kv.count("th")) for (int k = 0; k < 5; ++k) env.env_th[k] = kv.at("th").at(k) - '0';
        if (kv.count("pipe")) env.env_pipe = num("pipe");
        if (kv.count("tail")) env.env_tail = (float)atof(kv.at("tail").c_str());
        if (kv.count("fork")) env.env_fork = num("fork");
        if (kv.count("forkshare")) env.fork_share = atof(kv.at("forkshare").c_str());
        if (kv.count("forkmin")) env.fork_min_rounds = atof(kv.at("forkmin").c_str());
        if (kv.count("bands")) env.env_bands = num("bands");
        if (kv.count("rows")) { std::istringstream rows(kv.at("rows")); for (std::string r; std::getline(rows, r, ',');) env.env_rows.push_back(atoi(r.c_str())); }
        if (kv.count("rows_two")) env.env_rows_two = num("rows_two") != 0;
        if (kv.count("geo")) env.env_geo = num("geo") != 0;
        const bool u8 = kv.at("io") == "u8";
        const std::string call = kv.at("call");
        const int n = num("n"), h = num("h"), w = num("w"), engines = num("engines");
        printf("case %d\n", num("id"));
        if (call == "dev" || call == "band") {
            printf("ctx 0\n");
            if (device_call(env, u8, n, h, w, num("top"), num("bot")) != 0) { fprintf(stderr, "plan_check: case %d is no valid device call\n", num("id")); return 2; }
        } else if (call == "host") {
            printf("ctx 0\n");
            host_call(env, u8, n, h, w, 0, h);
        } else if (call == "multi") {  // run_multi: one share per context, each on its own context
            const std::vector<sr_row_share> share = sr_multi_shares(engines, h);
            for (int k = 0; k < engines; ++k) {
                printf("ctx %d\n", k);
                if (share.size() == 1 && k == 0) host_call(env, u8, 1, h, w, 0, h);
                else if (share.size() > 1 && k < (int)share.size()) host_call(env, u8, 1, h, w, share[k].lo, share[k].hi);
            }
        } else {
            fprintf(stderr, "plan_check: unknown call \"%s\"\n", call.c_str());
            return 2;
        }
    }
    return 0;
}
