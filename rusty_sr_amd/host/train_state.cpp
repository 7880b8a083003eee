// train_state.cpp -- the state file of `rusty_sr train` (train_state.hpp): encode, parse, write through a temporary file, compare settings.
#include "train_state.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

#include <unistd.h>

namespace srstate {

namespace {

const char kMagic[8] = {'R', 'S', 'R', 'S', 'T', 'A', 'T', 'E'};
enum Flags : uint32_t { kLinear = 1, kAugment = 2, kPairs = 4, kDegrade = 8, kEpoch = 16, kKnownFlags = 31 };

// little-endian fields appended to / read from a byte run; a read past the end fails and stays failed
struct Writer {
    std::vector<uint8_t>& b;
    void bytes(const void* p, size_t n) { const uint8_t* q = (const uint8_t*)p; b.insert(b.end(), q, q + n); }
    void u32(uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i))); }
    void u64(uint64_t v) { for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i))); }
    void f32(float v) { uint32_t u; memcpy(&u, &v, 4); u32(u); }
    void f64(double v) { uint64_t u; memcpy(&u, &v, 8); u64(u); }
};

struct Reader {
    const uint8_t* p;
    size_t len, pos = 0;
    bool ok = true;
    bool need(size_t n) { if (!ok || n > len - pos) ok = false; return ok; }
    void bytes(void* out, size_t n) { if (need(n)) { memcpy(out, p + pos, n); pos += n; } else memset(out, 0, n); }
    uint32_t u32() { uint32_t v = 0; if (need(4)) { for (int i = 0; i < 4; ++i) v |= (uint32_t)p[pos + i] << (8 * i); pos += 4; } return v; }
    uint64_t u64() { uint64_t v = 0; if (need(8)) { for (int i = 0; i < 8; ++i) v |= (uint64_t)p[pos + i] << (8 * i); pos += 8; } return v; }
    float f32() { const uint32_t u = u32(); float v; memcpy(&v, &u, 4); return v; }
    double f64() { const uint64_t u = u64(); double v; memcpy(&v, &u, 8); return v; }
};

bool same_f32(float a, float b) { return memcmp(&a, &b, 4) == 0; }

}  // namespace

uint64_t checksum(const uint8_t* data, size_t len) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < len; ++i) h = (h ^ data[i]) * 0x100000001b3ull;
    return h;
}

std::vector<uint8_t> encode(const State& s, std::string& err) {
    err.clear();
    const bool averaged = s.set.ema > 0.0f;
    if (s.m.size() != s.n_params || s.v.size() != s.n_params || s.e.size() != (averaged ? s.n_params : 0)) {
        err = "the moments do not have the parameter count";
        return {};
    }
    if (s.set.degrade_spec.size() >= kDegradeText || s.set.degrade_spec.find('\0') != std::string::npos) {
        err = "the --degrade spec is too long for the state file";
        return {};
    }
    std::vector<uint8_t> b;
    b.reserve(kHeaderBytes + (s.m.size() + s.v.size() + s.e.size()) * 4);
    Writer w{b};
    w.bytes(kMagic, 8);
    w.u32(kVersion);
    w.u32((uint32_t)kHeaderBytes);
    w.u32((uint32_t)s.set.factor);
    w.u32((s.set.linear ? kLinear : 0) | (s.set.augment ? kAugment : 0) | (s.set.pairs ? kPairs : 0) | (s.set.degrade ? kDegrade : 0) |
          (s.epoch_valid ? kEpoch : 0));
    w.u64(s.n_params); w.u64((uint64_t)s.step); w.u64((uint64_t)s.skipped);                                   // 3 of the 12 u64
    w.u64(s.set.seed); w.u64(s.rng); w.u64(s.aug_rng); w.u64(s.epoch_rng); w.u64(s.perm_pos); w.u64(s.deg_drawn);  // 9
    w.u64(s.val_next); w.u64(s.set.n_files); w.u64(s.params_hash);                                             // 12
    w.u32((uint32_t)s.set.loss_kind); w.f32(s.set.loss_eps); w.f32(s.set.lr); w.u32((uint32_t)s.set.sched_kind);
    w.u64((uint64_t)s.set.warmup); w.u64((uint64_t)s.set.every);
    w.f64(s.set.gamma);
    w.u64((uint64_t)s.set.total);
    w.f32(s.set.min_lr); w.f32(s.set.clip); w.f32(s.set.ema); w.u32(0);
    char text[kDegradeText] = {0};
    memcpy(text, s.set.degrade_spec.data(), s.set.degrade_spec.size());
    w.bytes(text, kDegradeText);
    w.u64(checksum(b.data(), b.size()));
    if (b.size() != kHeaderBytes) { err = "internal: header size"; return {}; }
    for (const std::vector<float>* a : {&s.m, &s.v, &s.e})
        for (float x : *a) w.f32(x);
    return b;
}

bool parse(const uint8_t* data, size_t len, State& out, std::string& err) {
    auto fail = [&](const char* why) { err = why; return false; };
    if (!data || len < kHeaderBytes) return fail("the state file is shorter than its header");
    if (memcmp(data, kMagic, 8) != 0) return fail("not a state file of rusty_sr train");
    Reader r{data, kHeaderBytes};
    r.pos = 8;
    if (r.u32() != kVersion) return fail("a state file of another version");
    if (r.u32() != kHeaderBytes) return fail("the state file's header has an unexpected size");
    if (checksum(data, kHeaderBytes - 8) != Reader{data + kHeaderBytes - 8, 8}.u64()) return fail("the state file's header is damaged (checksum)");
    State s;
    s.set.factor = (int32_t)r.u32();
    const uint32_t flags = r.u32();
    s.n_params = r.u64(); s.step = (int64_t)r.u64(); s.skipped = (int64_t)r.u64();
    s.set.seed = r.u64(); s.rng = r.u64(); s.aug_rng = r.u64(); s.epoch_rng = r.u64(); s.perm_pos = r.u64(); s.deg_drawn = r.u64();
    s.val_next = r.u64(); s.set.n_files = r.u64(); s.params_hash = r.u64();
    s.set.loss_kind = (int32_t)r.u32(); s.set.loss_eps = r.f32(); s.set.lr = r.f32(); s.set.sched_kind = (int32_t)r.u32();
    s.set.warmup = (int64_t)r.u64(); s.set.every = (int64_t)r.u64();
    s.set.gamma = r.f64();
    s.set.total = (int64_t)r.u64();
    s.set.min_lr = r.f32(); s.set.clip = r.f32(); s.set.ema = r.f32();
    const uint32_t pad = r.u32();
    char text[kDegradeText];
    r.bytes(text, kDegradeText);
    if (!r.ok || r.pos != kHeaderBytes - 8) return fail("the state file's header is truncated");
    if (text[kDegradeText - 1] != 0 || pad != 0 || (flags & ~(uint32_t)kKnownFlags)) return fail("the state file's header holds unknown fields");
    s.set.degrade_spec = text;
    s.set.linear = flags & kLinear; s.set.augment = flags & kAugment; s.set.pairs = flags & kPairs; s.set.degrade = flags & kDegrade;
    s.epoch_valid = flags & kEpoch;
    if (s.set.factor < 2 || s.set.factor > 4) return fail("the state file names a factor other than 2, 3 or 4");
    if (s.step < 0 || s.step >= INT32_MAX || s.skipped < 0 || s.skipped > s.step) return fail("the state file's step counts are out of range");
    if (!(s.set.ema >= 0.0f && s.set.ema < 1.0f) || !(s.set.clip >= 0.0f) || !std::isfinite(s.set.clip)) return fail("the state file's --clip / --ema are out of range");
    if (s.set.n_files == 0 || s.perm_pos > s.set.n_files) return fail("the state file's shuffle position is out of range");
    const uint64_t arrays = s.set.ema > 0.0f ? 3 : 2;
    // the parameter count is taken from the bytes that are there, never the other way round
    const size_t body = len - kHeaderBytes;
    if (s.n_params == 0 || s.n_params > (uint64_t)(SIZE_MAX / 16) || s.n_params > body / 4) return fail("the state file claims more parameters than it holds");
    if ((uint64_t)body != s.n_params * 4 * arrays) return fail("the state file's length does not match its parameter count");
    Reader a{data + kHeaderBytes, body};
    for (std::vector<float>* dst : {&s.m, &s.v, &s.e}) {
        if (dst == &s.e && arrays == 2) break;
        dst->resize((size_t)s.n_params);
        for (float& x : *dst) x = a.f32();
    }
    if (!a.ok || a.pos != body) return fail("the state file is truncated");
    out = std::move(s);
    err.clear();
    return true;
}

bool write_bytes(const std::string& path, const uint8_t* data, size_t len) {
    const std::string tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    // on the disk before the rename: a machine that stops right after it must not be left with a renamed, short file
    bool ok = fwrite(data, 1, len, f) == len && fflush(f) == 0 && fsync(fileno(f)) == 0;
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) {
        remove(tmp.c_str());
        return false;
    }
    return true;
}

bool write_file(const std::string& path, const State& s, std::string& err) {
    const std::vector<uint8_t> b = encode(s, err);
    if (b.empty()) return false;
    if (!write_bytes(path, b.data(), b.size())) {
        err = "could not write " + path;
        return false;
    }
    return true;
}

bool read_file(const std::string& path, State& out, std::string& err) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { err = "could not open " + path; return false; }
    std::vector<uint8_t> data;
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + n);
    fclose(f);
    return parse(data.data(), data.size(), out, err);
}

std::string differing(const Settings& a, const Settings& b) {
    if (a.seed != b.seed) return "--seed";
    if (a.factor != b.factor) return "--factor";
    if (a.linear != b.linear) return "--linearLoss";
    if (a.loss_kind != b.loss_kind || !same_f32(a.loss_eps, b.loss_eps)) return "--loss";
    if (a.augment != b.augment) return "--augment";
    if (a.pairs != b.pairs) return "--lr_folder";
    if (a.degrade != b.degrade || a.degrade_spec != b.degrade_spec) return "--degrade";
    if (!same_f32(a.lr, b.lr)) return "--lr";
    if (a.sched_kind != b.sched_kind || a.every != b.every || memcmp(&a.gamma, &b.gamma, 8) != 0 || a.total != b.total || !same_f32(a.min_lr, b.min_lr))
        return "--lr-schedule";
    if (a.warmup != b.warmup) return "--warmup";
    if (!same_f32(a.clip, b.clip)) return "--clip";
    if (!same_f32(a.ema, b.ema)) return "--ema";
    if (a.n_files != b.n_files) return "<TRAINING_FOLDER>";
    return "";
}

}  // namespace srstate
