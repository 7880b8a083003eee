// train_state.hpp -- the state file `rusty_sr train` writes beside its parameter file (OUT.rsr.state) and --resume reads: what a run needs
// besides the parameters to continue bit for bit.  Host code only: no HIP, no library call (tests/c/train_state.cpp builds it alone).
//
// The file, little-endian, version 1:
//   header (kHeaderBytes): "RSRSTATE", u32 version, u32 header bytes, the fields of State in the order below, the --degrade spec as 128
//     bytes of zero-padded text, and last a u64 FNV-1a of every header byte before it.  One of the fields, params_hash, is the FNV-1a of
//     the parameter file's bytes as they were written beside this state: the two files are written one after the other, never as one, and
//     --resume refuses a parameter file that does not hash to it (a run ended between the two, or a file put there by hand);
//   then n_params f32 of Adam's first moments, n_params of its second moments, and, if the average is on, n_params of averaged parameters.
// A file is refused unless its length is exactly what its header says.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace srstate {

constexpr uint32_t kVersion = 1;
constexpr size_t kDegradeText = 128;
constexpr size_t kHeaderBytes = 8 + 4 + 4 + 4 + 4 + 8 * 12 + 4 * 4 + 8 * 2 + 8 + 8 + 4 * 4 + kDegradeText + 8;

// The settings that determine the trajectory: --resume refuses a run whose options differ from the file's.
struct Settings {
    int32_t factor = 3;
    bool linear = false, augment = false, pairs = false, degrade = false;
    uint64_t seed = 0;
    uint64_t n_files = 0;        // image files listed in the training folder, decodable or not
    int32_t loss_kind = 0;
    float loss_eps = 1e-3f;
    float lr = 2e-3f;            // --lr
    int32_t sched_kind = 0;      // --lr-schedule
    int64_t warmup = 0;          // --warmup
    int64_t every = 0;
    double gamma = 0.0;
    int64_t total = 0;
    float min_lr = 0.0f;
    float clip = 0.0f;           // --clip
    float ema = 0.0f;            // --ema
    std::string degrade_spec;    // --degrade, as given (at most kDegradeText - 1 bytes)
};

struct State {
    Settings set;
    uint64_t n_params = 0;
    int64_t step = 0, skipped = 0;
    // the generators at the draw the GPU consumes next: the crop stream, the --augment stream, the crop stream as it was before the
    // current epoch's shuffle (epoch_valid: an epoch has begun), the position in that shuffle, the --degrade draws made, the validation cursor
    uint64_t rng = 0, aug_rng = 0, epoch_rng = 0, perm_pos = 0, deg_drawn = 0, val_next = 0;
    bool epoch_valid = false;
    uint64_t params_hash = 0;    // checksum() of the parameter file's bytes written with this state
    std::vector<float> m, v, e;  // e: empty unless set.ema > 0
};

uint64_t checksum(const uint8_t* data, size_t len);  // FNV-1a, 64 bit
// State -> file bytes ("" in err), or an empty vector and the reason (sizes that disagree, a spec too long)
std::vector<uint8_t> encode(const State& s, std::string& err);
// file bytes -> State; false and the reason for anything but a well-formed file of exactly its own length
bool parse(const uint8_t* data, size_t len, State& out, std::string& err);
// Write through a temporary file beside `path`, flushed to the disk before it is renamed into place (write_bytes: any file's bytes, the
// parameter files too); read a whole file
bool write_bytes(const std::string& path, const uint8_t* data, size_t len);
bool write_file(const std::string& path, const State& s, std::string& err);
bool read_file(const std::string& path, State& out, std::string& err);
// The option whose value differs between the two ("" if none): "--seed", "--loss", ...
std::string differing(const Settings& file, const Settings& now);

}  // namespace srstate
