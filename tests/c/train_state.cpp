// The state-file parser of `rusty_sr train` (rusty_sr_amd/host/train_state.cpp) as a program of its own, so that it can run under
// AddressSanitizer + UBSan without the GPU library: round trips, every truncation point, every single-bit flip of the header, parameter
// counts that overflow or exceed the file.  argv[1]: a path to write a state file to and read it back from.  Prints one line per check.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rusty_sr_amd/host/train_state.hpp"

namespace {

srstate::State sample(bool averaged, size_t n) {
    srstate::State s;
    s.set.factor = 4; s.set.linear = true; s.set.augment = true; s.set.degrade = true; s.set.degrade_spec = "blur=0.5:2,jpeg=40:90";
    s.set.seed = 0x0123456789abcdefull; s.set.n_files = 6; s.set.loss_kind = 2; s.set.loss_eps = 0.01f; s.set.lr = 1e-3f;
    s.set.sched_kind = 2; s.set.warmup = 10; s.set.every = 0; s.set.gamma = 0.5; s.set.total = 200; s.set.min_lr = 1e-5f;
    s.set.clip = 0.25f; s.set.ema = averaged ? 0.99f : 0.0f;
    s.n_params = n; s.step = 100; s.skipped = 3;
    s.rng = 11; s.aug_rng = 22; s.epoch_rng = 33; s.perm_pos = 4; s.deg_drawn = 400; s.val_next = 1; s.epoch_valid = true;
    s.params_hash = 0xfedcba9876543210ull;
    for (size_t i = 0; i < n; ++i) {
        s.m.push_back(0.5f * (float)i - 3.0f);
        s.v.push_back(1.0f / (float)(i + 1));
        if (averaged) s.e.push_back(-(float)i);
    }
    return s;
}

bool same(const srstate::State& a, const srstate::State& b) {
    auto bits = [](const std::vector<float>& x, const std::vector<float>& y) {
        return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * 4) == 0);
    };
    return srstate::differing(a.set, b.set).empty() && a.n_params == b.n_params && a.step == b.step && a.skipped == b.skipped && a.rng == b.rng &&
           a.aug_rng == b.aug_rng && a.epoch_rng == b.epoch_rng && a.perm_pos == b.perm_pos && a.deg_drawn == b.deg_drawn &&
           a.val_next == b.val_next && a.epoch_valid == b.epoch_valid && a.params_hash == b.params_hash && bits(a.m, b.m) && bits(a.v, b.v) && bits(a.e, b.e);
}

// a header field overwritten in place, the checksum made good again: only the field's own check can refuse it
std::vector<uint8_t> with_u64(std::vector<uint8_t> b, size_t off, uint64_t v) {
    for (int i = 0; i < 8; ++i) b[off + i] = (uint8_t)(v >> (8 * i));
    const uint64_t h = srstate::checksum(b.data(), srstate::kHeaderBytes - 8);
    for (int i = 0; i < 8; ++i) b[srstate::kHeaderBytes - 8 + i] = (uint8_t)(h >> (8 * i));
    return b;
}

}  // namespace

int main(int argc, char** argv) {
    std::string err;
    for (bool averaged : {true, false}) {
        const srstate::State s = sample(averaged, 37);
        const std::vector<uint8_t> b = srstate::encode(s, err);
        srstate::State back;
        const bool ok = !b.empty() && b.size() == srstate::kHeaderBytes + 37 * 4 * (averaged ? 3 : 2) && srstate::parse(b.data(), b.size(), back, err) &&
                        same(s, back);
        printf("roundtrip %s %s\n", averaged ? "averaged" : "plain", ok ? "ok" : ("FAILED " + err).c_str());
        // every truncation point, from a heap copy of exactly that length (a read past it is the sanitizer's to report), and one byte more
        size_t refused = 0;
        for (size_t len = 0; len < b.size(); ++len) {
            const std::vector<uint8_t> cut(b.begin(), b.begin() + (long)len);
            refused += !srstate::parse(cut.data(), cut.size(), back, err);
        }
        std::vector<uint8_t> longer = b;
        longer.push_back(0);
        refused += !srstate::parse(longer.data(), longer.size(), back, err);
        printf("truncations refused %zu of %zu\n", refused, b.size() + 1);
        // every single-bit flip of the header
        size_t flips = 0, flips_refused = 0;
        for (size_t byte = 0; byte < srstate::kHeaderBytes; ++byte)
            for (int bit = 0; bit < 8; ++bit, ++flips) {
                std::vector<uint8_t> f = b;
                f[byte] ^= (uint8_t)(1u << bit);
                flips_refused += !srstate::parse(f.data(), f.size(), back, err);
            }
        printf("header flips refused %zu of %zu\n", flips_refused, flips);
    }
    {
        const std::vector<uint8_t> b = srstate::encode(sample(true, 37), err);
        srstate::State back;
        const size_t off_n = 8 + 4 + 4 + 4 + 4;  // n_params
        const uint64_t counts[] = {0, 38, 1ull << 30, 1ull << 61, (1ull << 62) + 37, 0x5555555555555555ull + 37, ~0ull};
        for (uint64_t n : counts) {
            const std::vector<uint8_t> f = with_u64(b, off_n, n);
            const bool ok = srstate::parse(f.data(), f.size(), back, err);
            printf("count %llu %s\n", (unsigned long long)n, ok ? "ACCEPTED" : "refused");
        }
        const std::vector<uint8_t> good = with_u64(b, off_n, 37);
        printf("count 37 %s\n", srstate::parse(good.data(), good.size(), back, err) ? "ok" : "REFUSED");
        const std::vector<uint8_t> neg = with_u64(b, off_n + 8, ~0ull);  // step = -1
        printf("step -1 %s\n", srstate::parse(neg.data(), neg.size(), back, err) ? "ACCEPTED" : "refused");
    }
    {
        srstate::State s = sample(true, 5);
        s.m.pop_back();
        printf("encode short moments %s\n", srstate::encode(s, err).empty() ? "refused" : "ACCEPTED");
        s = sample(false, 5);
        s.set.degrade_spec.assign(srstate::kDegradeText, 'x');
        printf("encode long spec %s\n", srstate::encode(s, err).empty() ? "refused" : "ACCEPTED");
    }
    {
        const srstate::Settings a = sample(true, 1).set;
        auto diff = [&](auto change) { srstate::Settings b = a; change(b); return srstate::differing(a, b); };
        printf("differing: '%s' %s %s %s %s %s %s %s\n", srstate::differing(a, a).c_str(), diff([](auto& b) { b.seed ^= 1; }).c_str(),
               diff([](auto& b) { b.loss_kind = 1; }).c_str(), diff([](auto& b) { b.lr = 2e-3f; }).c_str(), diff([](auto& b) { b.total = 100; }).c_str(),
               diff([](auto& b) { b.warmup = 0; }).c_str(), diff([](auto& b) { b.clip = 0.5f; }).c_str(), diff([](auto& b) { b.ema = 0.0f; }).c_str());
    }
    if (argc > 1) {
        const srstate::State s = sample(true, 1000);
        srstate::State back;
        const bool ok = srstate::write_file(argv[1], s, err) && srstate::read_file(argv[1], back, err) && same(s, back);
        FILE* tmp = fopen((std::string(argv[1]) + ".tmp").c_str(), "rb");
        printf("file %s, temporary %s\n", ok ? "ok" : ("FAILED " + err).c_str(), tmp ? "LEFT BEHIND" : "gone");
        if (tmp) fclose(tmp);
        printf("missing file %s\n", srstate::read_file(std::string(argv[1]) + ".nope", back, err) ? "ACCEPTED" : "refused");
    }
    return 0;
}
