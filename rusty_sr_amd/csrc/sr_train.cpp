// sr_train.cpp -- the training session of include/srhip.h (sr_train_*) and the reference's parameter initialisation (sr_init_params): the
// loop of the reference's `train` (main.rs:181-257) without its file handling, which the CLI does.  A step is the crop gather
// (sr_train.hip), sr_backprop_rgba8_dev and sr_adam_step_dev, queued on the context's stream.  With clipping or the
// parameter average on (sr_train_set_optim) the last of them is sr_grad_norm_dev + sr_adam_step_clipped_dev (sr_optim.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "sr_internal.h"
#include "sr_params.h"

namespace {

struct SplitMix64 {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uniform() { return (double)(next() >> 11) * 0x1.0p-53; }  // [0, 1)
};

constexpr int kStage = 2;  // page-locked staging slots of transient images

}  // namespace

struct sr_train {
    sr_ctx* c = nullptr;
    int np = 0;
    bool linear = false;
    float l2 = 0, lr = 0, beta1 = 0, beta2 = 0, eps = 0;
    float* d_state = nullptr;  // parameters, first and second moments, gradient: 4 slices of sr_round256(np floats)
    float *d_p = nullptr, *d_m = nullptr, *d_v = nullptr, *d_g = nullptr;
    // err_sum of each step: a ring of mapped host doubles the backprop's sum kernel writes, each slot free once its step's event has fired
    double* h_err = nullptr;
    double* d_err = nullptr;
    hipEvent_t ring_ev[SR_TRAIN_RING] = {nullptr};
    long long queued = 0, harvested = 0;  // steps issued (= Adam's step count) / whose err_sum has been read
    std::vector<sr_train_stat> done;       // what has been read since the last sync
    // the optimiser's additions (include/srhip.h "Optimiser"): off until sr_train_set_optim, and then the default step's launches stay as they are
    float clip = 0, ema_decay = 0;         // 0: off
    float* d_e = nullptr;                  // the averaged parameters: allocated when first enabled
    sr_grad_norm* d_norm = nullptr;        // the current step's norm, scale and skip flag (in d_state's tail)
    unsigned long long* d_skipped = nullptr;  // steps skipped for a gradient that was not finite (beside it)
    sr_grad_norm* h_norm = nullptr;        // a ring of mapped host copies of d_norm beside the err ring, filled and freed the same way
    sr_grad_norm* d_norm_ring = nullptr;
    float lr_ring[SR_TRAIN_RING] = {0};    // the rate each step in flight was queued with
    bool clip_ring[SR_TRAIN_RING] = {false};  // ... and whether it wrote its slot of the norm ring
    // the image store: one allocation per resident image, within the budget
    // (a pair is one entry: d_lr its LR image of h / f x w / f in the same allocation, nullptr for a plain image)
    struct Img { uint8_t* d; int ch, h, w; uint8_t* d_lr; int lr_ch; };
    std::vector<Img> images;
    size_t store_budget = 0, store_used = 0;
    // per-step buffers, reused in stream order
    sr_buf d_batch;  // the crops, u8
    sr_buf d_trans;  // the rows of transient images a step's crops read
    void* h_stage[kStage] = {nullptr}; size_t stage_cap[kStage] = {0};
    hipEvent_t stage_ev[kStage] = {nullptr};
    bool stage_pending[kStage] = {false};
    int stage_next = 0;
    int last_n = 0, last_h = 0, last_w = 0;  // shape of the last step: another one may grow the backprop workspace
};

namespace {

// A buffer of the session that steps in flight may still read: grown only after the stream has drained.
int grow(sr_ctx* c, hipStream_t s, sr_buf& b, size_t bytes) {
    if (bytes <= b.cap) return SR_OK;
    HIPCHK(c, hipStreamSynchronize(s));
    return sr_ensure_buf(c, b, sr_round256(bytes));
}

// Read the err_sum of the oldest step in flight (waits for it).
int harvest_one(sr_train* t) {
    const int slot = (int)(t->harvested % SR_TRAIN_RING);
    HIPCHK(t->c, hipEventSynchronize(t->ring_ev[slot]));
    sr_train_stat st;
    st.err_sum = ((volatile double*)t->h_err)[slot];
    st.grad_norm = 0.0;
    st.lr = t->lr_ring[slot];
    st.scale = 1.0f;
    if (t->clip_ring[slot]) {
        st.grad_norm = std::sqrt(((volatile sr_grad_norm*)t->h_norm)[slot].sumsq);
        st.scale = ((volatile sr_grad_norm*)t->h_norm)[slot].scale;
    }
    t->done.push_back(st);
    ++t->harvested;
    return SR_OK;
}

int drain(sr_train* t) {
    HIPCHK(t->c, hipStreamSynchronize(t->c->stream));
    while (t->harvested < t->queued) {
        const int rc = harvest_one(t);
        if (rc != SR_OK) return rc;
    }
    return SR_OK;
}

// What every step does before it queues anything: room in the ring, and a drained stream where the backprop workspace may grow.
int begin_step(sr_train* t, int n, int crop_h, int crop_w) {
    sr_ctx* c = t->c;
    if (t->queued - t->harvested >= SR_TRAIN_RING) {  // the ring is full: wait for the oldest step
        const int rc = harvest_one(t);
        if (rc != SR_OK) return rc;
    }
    if (n != t->last_n || crop_h != t->last_h || crop_w != t->last_w) {  // the backprop workspace may grow: nothing in flight may use it
        HIPCHK(c, hipStreamSynchronize(c->stream));
        t->last_n = t->last_h = t->last_w = 0;
    }
    return SR_OK;
}

// The staging slot a step's transient rows go through, trans_bytes of them: free once the copy that read it last has completed.
int acquire_stage(sr_train* t, size_t trans_bytes, int* slot) {
    sr_ctx* c = t->c;
    const int k = t->stage_next;
    *slot = k;
    if (!trans_bytes) return SR_OK;
    if (t->stage_pending[k]) HIPCHK(c, hipEventSynchronize(t->stage_ev[k]));
    t->stage_pending[k] = false;
    if (t->stage_cap[k] < trans_bytes) {
        if (t->h_stage[k]) (void)hipHostFree(t->h_stage[k]);
        t->h_stage[k] = nullptr;
        t->stage_cap[k] = 0;
        HIPCHK(c, hipHostMalloc(&t->h_stage[k], sr_round256(trans_bytes), hipHostMallocPortable));
        t->stage_cap[k] = sr_round256(trans_bytes);
    }
    return SR_OK;
}

int upload_stage(sr_train* t, size_t trans_bytes, int k) {
    sr_ctx* c = t->c;
    if (!trans_bytes) return SR_OK;
    HIPCHK(c, hipMemcpyAsync(t->d_trans.p, t->h_stage[k], trans_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(t->stage_ev[k], c->stream));
    t->stage_pending[k] = true;
    t->stage_next = (k + 1) % kStage;
    return SR_OK;
}

// Backprop on the gathered u8 batch (crop_h x crop_w each; lr: the input the gather has already written, or nullptr: pool), Adam, the ring.
int finish_step(sr_train* t, int n, int crop_h, int crop_w, const sr_lr_input* lr) {
    sr_ctx* c = t->c;
    hipStream_t s = c->stream;
    const size_t n_elems = sr_loss_elems(c->factor, n, crop_h, crop_w);
    const int slot = (int)(t->queued % SR_TRAIN_RING);
    sr_plan_clear(c);
    int rc = sr_grad_queue(c, t->d_p, t->d_batch.p, true, 3, n, crop_h, crop_w, t->linear, (float)(1.0 / (double)n_elems), t->l2, t->d_err + slot,
                           t->d_g, s, nullptr, lr);
    if (rc != SR_OK) return rc;  // (SR_E_NOMEM: the context freed its backprop buffers; the parameters are untouched)
    t->last_n = n; t->last_h = crop_h; t->last_w = crop_w;
    const bool clipped = t->clip > 0.0f, averaged = t->ema_decay > 0.0f;
    if (!clipped && !averaged) {
        rc = sr_adam_step_dev(c, t->d_p, t->d_m, t->d_v, t->d_g, (size_t)t->np, (int)(t->queued + 1), t->lr, t->beta1, t->beta2, t->eps, s);
    } else {
        if (clipped) rc = sr_grad_norm_queue(c, t->d_g, (size_t)t->np, t->clip, t->d_norm, t->d_norm_ring + slot, s);
        if (rc == SR_OK)
            rc = sr_adam_step_clipped_dev(c, t->d_p, t->d_m, t->d_v, t->d_g, (size_t)t->np, (int)(t->queued + 1), t->lr, t->beta1, t->beta2, t->eps,
                                          clipped ? t->d_norm : nullptr, averaged ? t->d_e : nullptr, t->ema_decay, t->d_skipped, s);
    }
    if (rc != SR_OK) return rc;
    t->lr_ring[slot] = t->lr;
    t->clip_ring[slot] = clipped;
    HIPCHK(c, hipEventRecord(t->ring_ev[slot], s));
    ++t->queued;
    return SR_OK;
}

void release(sr_train* t) {
    sr_ctx* c = t->c;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& im : t->images) (void)hipFree(im.d);
    if (t->d_state) (void)hipFree(t->d_state);
    if (t->d_e) (void)hipFree(t->d_e);
    sr_free_buf(t->d_batch);
    sr_free_buf(t->d_trans);
    if (t->h_err) (void)hipHostFree(t->h_err);
    for (int k = 0; k < kStage; ++k) {
        if (t->h_stage[k]) (void)hipHostFree(t->h_stage[k]);
        if (t->stage_ev[k]) (void)hipEventDestroy(t->stage_ev[k]);
    }
    for (auto& e : t->ring_ev) if (e) (void)hipEventDestroy(e);
}

}  // namespace

void sr_train_detach_all(sr_ctx* c) {
    for (sr_train* t : c->trains) {
        release(t);
        t->c = nullptr;
    }
    c->trains.clear();
}

extern "C" {

int sr_init_params(int factor, uint64_t seed, float* out, size_t cap) {
    const int np = sr_num_params_factor(factor);
    if (np < 0) return SR_E_FACTOR;
    if (!out || cap < (size_t)np) return SR_E_INVALID;
    // segment by segment in .rsr order: a bias is 0, a BeLU beta alternates 1, 0, a convolution draws He-normal weights (two uniforms each)
    const sr_param_layout L(factor);
    SplitMix64 rng{seed};
    size_t o = 0;
    for (int sg = 0; sg < SR_SEGS; ++sg) {
        const sr_seg_def& d = kSrSegDefs[sg];
        for (size_t i = 0; i < L.len[sg]; ++i, ++o) {
            if (d.kind == SR_KIND_BIAS) out[o] = 0.0f;
            else if (d.kind == SR_KIND_BETA) out[o] = i % 2 == 0 ? 1.0f : 0.0f;
            else {
                const double std = d.init_mult * std::sqrt(2.0 / L.fan_in(sg));
                const double u1 = rng.uniform(), u2 = rng.uniform();
                out[o] = (float)(std * std::sqrt(-2.0 * std::log(1.0 - u1)) * std::cos(2.0 * 3.14159265358979323846 * u2));
            }
        }
    }
    return o == (size_t)np ? SR_OK : SR_E_INVALID;
}

int sr_train_create(sr_train** out, sr_ctx* c, const float* start_params, size_t n_params, int linear_loss, float l2, float lr, float beta1,
                    float beta2, float eps, size_t store_bytes) {
    if (!c && sr_no_device()) return SR_E_NO_DEVICE;
    if (!out || !c || !start_params) return SR_E_INVALID;
    *out = nullptr;
    if (c->graph != SR_GRAPH_SR_NET) return SR_E_INVALID;
    const int np = sr_num_params_factor(c->factor);
    if (np < 0 || n_params != (size_t)np) return SR_E_PARAM_COUNT;
    sr_train* t = new (std::nothrow) sr_train();
    if (!t) return SR_E_NOMEM;
    t->c = c;
    t->np = np;
    t->linear = linear_loss != 0;
    t->l2 = l2; t->lr = lr; t->beta1 = beta1; t->beta2 = beta2; t->eps = eps;
    sr_device_guard restore_device;
    const int rc = [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        int r = sr_ensure_streams(c, false);
        if (r != SR_OK) return r;
        const size_t slice = sr_round256((size_t)np * sizeof(float));
        HIPCHK(c, hipMalloc((void**)&t->d_state, 4 * slice + 256));  // (the tail: the step's norm and the skipped count)
        t->d_p = t->d_state;
        t->d_m = (float*)((char*)t->d_state + slice);
        t->d_v = (float*)((char*)t->d_state + 2 * slice);
        t->d_g = (float*)((char*)t->d_state + 3 * slice);
        HIPCHK(c, hipMemcpy(t->d_p, start_params, (size_t)np * sizeof(float), hipMemcpyHostToDevice));
        t->d_norm = (sr_grad_norm*)((char*)t->d_state + 4 * slice);
        t->d_skipped = (unsigned long long*)((char*)t->d_state + 4 * slice + 64);
        HIPCHK(c, hipMemset(t->d_m, 0, 2 * slice));
        HIPCHK(c, hipMemset(t->d_norm, 0, 256));
        HIPCHK(c, hipHostMalloc((void**)&t->h_err, SR_TRAIN_RING * (sizeof(double) + sizeof(sr_grad_norm)), hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer((void**)&t->d_err, t->h_err, 0));
        t->h_norm = (sr_grad_norm*)(t->h_err + SR_TRAIN_RING);
        t->d_norm_ring = (sr_grad_norm*)(t->d_err + SR_TRAIN_RING);
        for (auto& e : t->ring_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto& e : t->stage_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (store_bytes == SR_TRAIN_STORE_AUTO) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
            const size_t keep = std::max<size_t>((size_t)8 << 30, free_b / 8);
            store_bytes = free_b > keep ? free_b - keep : 0;
        }
        t->store_budget = store_bytes;
        return SR_OK;
    }();
    if (rc != SR_OK) {
        release(t);
        delete t;
        return rc;
    }
    c->trains.push_back(t);
    *out = t;
    return SR_OK;
}

int sr_train_add_image(sr_train* t, const uint8_t* px, int in_channels, int h, int w, int* id) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !px || !id || (in_channels != 3 && in_channels != 4) || h < 1 || w < 1) return SR_E_INVALID;
    *id = -1;
    sr_ctx* c = t->c;
    const size_t bytes = (size_t)h * w * in_channels, alloc = sr_round256(bytes);
    if (alloc > t->store_budget - std::min(t->store_budget, t->store_used) || t->images.size() >= (size_t)INT32_MAX) return SR_OK;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, alloc) != hipSuccess) {  // the device is fuller than the budget said: no room, not an error
        (void)hipGetLastError();
        return SR_OK;
    }
    const hipError_t e = hipMemcpy(d, px, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        HIPCHK(c, e);
    }
    t->store_used += alloc;
    t->images.push_back({d, in_channels, h, w, nullptr, 0});
    *id = (int)t->images.size() - 1;
    return SR_OK;
}

int sr_train_step(sr_train* t, const sr_train_crop* items, int n, int crop_h, int crop_w) {
    return sr_train_step_aug(t, items, nullptr, n, crop_h, crop_w);
}

int sr_train_step_aug(sr_train* t, const sr_train_crop* items, const uint8_t* members, int n, int crop_h, int crop_w) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !items || n < 1 || n > SR_TRAIN_MAX_BATCH) return SR_E_INVALID;
    sr_ctx* c = t->c;
    if (crop_h < c->factor || crop_w < c->factor) return SR_E_INVALID;
    // every item is checked before anything is launched; the rows of each transient image that its window can reach are what is staged
    // (the window of a member that swaps the axes has crop_w rows)
    auto member = [&](int i) { return members ? (int)members[i] : 0; };
    auto window_rows = [&](int i) { return member(i) & 4 ? crop_w : crop_h; };
    size_t trans_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const sr_train_crop& it = items[i];
        if (member(i) > 7) return SR_E_INVALID;
        if (it.image >= 0) {
            if ((size_t)it.image >= t->images.size() || t->images[(size_t)it.image].d_lr) return SR_E_INVALID;  // (a pair is no plain image)
        } else if (it.image == -1) {
            if (!it.px || (it.in_channels != 3 && it.in_channels != 4) || it.h < 1 || it.w < 1) return SR_E_INVALID;
            const long r0 = std::clamp<long>(it.y0, 0, it.h), r1 = std::clamp<long>((long)it.y0 + window_rows(i), 0, it.h);
            trans_bytes += sr_round256((size_t)(r1 - r0) * it.w * it.in_channels);
        } else {
            return SR_E_INVALID;
        }
    }
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = begin_step(t, n, crop_h, crop_w);
    if (rc != SR_OK) return rc;
    const size_t batch_bytes = (size_t)n * crop_h * crop_w * 3;
    rc = grow(c, s, t->d_batch, batch_bytes + 4);
    if (rc == SR_OK && trans_bytes) rc = grow(c, s, t->d_trans, trans_bytes);
    if (rc != SR_OK) return rc;
    sr_train_crop_args a;
    a.n = n; a.crop_h = crop_h; a.crop_w = crop_w;
    int k = 0;
    rc = acquire_stage(t, trans_bytes, &k);
    if (rc != SR_OK) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const sr_train_crop& it = items[i];
        if (it.image != -1) continue;
        const long r0 = std::clamp<long>(it.y0, 0, it.h), r1 = std::clamp<long>((long)it.y0 + window_rows(i), 0, it.h);
        const size_t row = (size_t)it.w * it.in_channels, bytes = (size_t)(r1 - r0) * row;
        if (bytes) memcpy((char*)t->h_stage[k] + off, it.px + (size_t)r0 * row, bytes);
        // the staged rows as an image of r1 - r0 rows: the crop's rows outside them are outside the source image too
        a.d[i] = {(const uint8_t*)t->d_trans.p + off, it.in_channels, (int)(r1 - r0), it.w, (int)(it.y0 - r0), it.x0, member(i)};
        off += sr_round256(bytes);
    }
    rc = upload_stage(t, trans_bytes, k);
    if (rc != SR_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const sr_train_crop& it = items[i];
        if (it.image < 0) continue;
        const sr_train::Img& im = t->images[(size_t)it.image];
        a.d[i] = {im.d, im.ch, im.h, im.w, it.y0, it.x0, member(i)};
    }
    HIPCHK(c, sr_launch_train_crop(a, (uint32_t*)t->d_batch.p, s));
    return finish_step(t, n, crop_h, crop_w, nullptr);
}

int sr_train_step_degrade(sr_train* t, const sr_train_crop* items, const uint8_t* members, const sr_degrade* deg, int n, int crop_h, int crop_w) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !items || !deg || n < 1 || n > SR_TRAIN_MAX_BATCH) return SR_E_INVALID;
    sr_ctx* c = t->c;
    const int f = c->factor;
    if (crop_h < f || crop_w < f || crop_h % f || crop_w % f) return SR_E_INVALID;
    // every item is checked before anything is launched; the rows of each transient image that its window AND its blur can reach are what
    // is staged (the window of a member that swaps the axes has crop_w rows)
    auto member = [&](int i) { return members ? (int)members[i] : 0; };
    auto reach = [&](int i, long* r0, long* r1) {
        const sr_train_crop& it = items[i];
        const long rows = member(i) & 4 ? crop_w : crop_h, R = sr_degrade_radius(deg[i]);
        *r0 = std::clamp<long>((long)it.y0 - R, 0, it.h);
        *r1 = std::clamp<long>((long)it.y0 + rows + R, 0, it.h);
    };
    size_t trans_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const sr_train_crop& it = items[i];
        if (member(i) > 7 || sr_degrade_check(deg[i]) != SR_OK) return SR_E_INVALID;
        if (it.image >= 0) {
            if ((size_t)it.image >= t->images.size() || t->images[(size_t)it.image].d_lr) return SR_E_INVALID;  // (a pair is no plain image)
        } else if (it.image == -1) {
            if (!it.px || (it.in_channels != 3 && it.in_channels != 4) || it.h < 1 || it.w < 1) return SR_E_INVALID;
            long r0, r1;
            reach(i, &r0, &r1);
            trans_bytes += sr_round256((size_t)(r1 - r0) * it.w * it.in_channels);
        } else {
            return SR_E_INVALID;
        }
    }
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = begin_step(t, n, crop_h, crop_w);
    if (rc != SR_OK) return rc;
    const size_t batch_bytes = (size_t)n * crop_h * crop_w * 3;
    rc = grow(c, s, t->d_batch, batch_bytes + 4);
    if (rc == SR_OK && trans_bytes) rc = grow(c, s, t->d_trans, trans_bytes);
    float* x = nullptr;
    if (rc == SR_OK) rc = sr_grad_input_buffer(c, n, crop_h / f, crop_w / f, &x);  // (the stream has drained if this grows the workspace)
    if (rc == SR_OK) rc = sr_degrade_ensure_table(c);
    if (rc != SR_OK) return rc;
    sr_train_degrade_args a;
    a.n = n; a.crop_h = crop_h; a.crop_w = crop_w; a.f = f; a.hr_blocks = 0;
    int k = 0;
    rc = acquire_stage(t, trans_bytes, &k);
    if (rc != SR_OK) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const sr_train_crop& it = items[i];
        a.g[i] = deg[i];
        if (it.image >= 0) {
            const sr_train::Img& im = t->images[(size_t)it.image];
            a.d[i] = {im.d, im.ch, im.h, im.w, it.y0, it.x0, member(i)};
            continue;
        }
        long r0, r1;
        reach(i, &r0, &r1);
        const size_t row = (size_t)it.w * it.in_channels, bytes = (size_t)(r1 - r0) * row;
        if (bytes) memcpy((char*)t->h_stage[k] + off, it.px + (size_t)r0 * row, bytes);
        // the staged rows as an image of r1 - r0 rows: what the crop and the blur read outside them is outside the source image too
        a.d[i] = {(const uint8_t*)t->d_trans.p + off, it.in_channels, (int)(r1 - r0), it.w, (int)(it.y0 - r0), it.x0, member(i)};
        off += sr_round256(bytes);
    }
    rc = upload_stage(t, trans_bytes, k);
    if (rc != SR_OK) return rc;
    HIPCHK(c, sr_launch_train_degrade(a, (uint32_t*)t->d_batch.p, x, c->d_vtab, c->d_dtab, s));
    sr_lr_input in;
    in.in_place = true;
    return finish_step(t, n, crop_h, crop_w, &in);
}

int sr_train_add_pair(sr_train* t, const uint8_t* lr_px, int lr_channels, const uint8_t* hr_px, int hr_channels, int lh, int lw, int* id) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !lr_px || !hr_px || !id) return SR_E_INVALID;
    sr_ctx* c = t->c;
    const int rc = sr_check_pair_args(c, true, lr_channels, hr_channels, 1, lh, lw);
    if (rc != SR_OK) return rc;
    *id = -1;
    const int f = c->factor;
    const size_t hr_bytes = (size_t)f * lh * f * lw * hr_channels, lr_bytes = (size_t)lh * lw * lr_channels;
    const size_t alloc = sr_round256(hr_bytes) + sr_round256(lr_bytes);  // one entry, both images
    if (alloc > t->store_budget - std::min(t->store_budget, t->store_used) || t->images.size() >= (size_t)INT32_MAX) return SR_OK;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, alloc) != hipSuccess) {  // the device is fuller than the budget said: no room, not an error
        (void)hipGetLastError();
        return SR_OK;
    }
    uint8_t* d_lr = d + sr_round256(hr_bytes);
    hipError_t e = hipMemcpy(d, hr_px, hr_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_lr, lr_px, lr_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        HIPCHK(c, e);
    }
    t->store_used += alloc;
    t->images.push_back({d, hr_channels, f * lh, f * lw, d_lr, lr_channels});
    *id = (int)t->images.size() - 1;
    return SR_OK;
}

int sr_train_step_pairs(sr_train* t, const sr_train_pair_crop* items, int n, int crop_lh, int crop_lw) {
    return sr_train_step_pairs_aug(t, items, nullptr, n, crop_lh, crop_lw);
}

int sr_train_step_pairs_aug(sr_train* t, const sr_train_pair_crop* items, const uint8_t* members, int n, int crop_lh, int crop_lw) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !items || n < 1 || n > SR_TRAIN_MAX_BATCH) return SR_E_INVALID;
    sr_ctx* c = t->c;
    const int f = c->factor;
    if (crop_lh < 1 || crop_lw < 1 || crop_lh > INT32_MAX / f || crop_lw > INT32_MAX / f) return SR_E_INVALID;
    // every item is checked before anything is launched; of a transient pair, the rows its windows can reach are what is staged
    // (the LR window of a member that swaps the axes has crop_lw rows)
    auto member = [&](int i) { return members ? (int)members[i] : 0; };
    auto window_rows = [&](int i) { return member(i) & 4 ? crop_lw : crop_lh; };
    size_t trans_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const sr_train_pair_crop& it = items[i];
        if (member(i) > 7) return SR_E_INVALID;
        if (it.pair >= 0) {
            if ((size_t)it.pair >= t->images.size() || !t->images[(size_t)it.pair].d_lr) return SR_E_INVALID;  // (a plain image is no pair)
        } else if (it.pair == -1) {
            if (!it.lr_px || !it.hr_px || sr_check_pair_args(c, true, it.lr_channels, it.hr_channels, 1, it.lh, it.lw) != SR_OK)
                return SR_E_INVALID;
            const long r0 = std::clamp<long>(it.y0, 0, it.lh), r1 = std::clamp<long>((long)it.y0 + window_rows(i), 0, it.lh);
            trans_bytes += sr_round256((size_t)(r1 - r0) * it.lw * it.lr_channels) +
                           sr_round256((size_t)(r1 - r0) * f * it.lw * f * it.hr_channels);
        } else {
            return SR_E_INVALID;
        }
    }
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int crop_h = f * crop_lh, crop_w = f * crop_lw;
    int rc = begin_step(t, n, crop_h, crop_w);
    if (rc != SR_OK) return rc;
    const size_t batch_bytes = (size_t)n * crop_h * crop_w * 3;
    rc = grow(c, s, t->d_batch, batch_bytes + 4);
    if (rc == SR_OK && trans_bytes) rc = grow(c, s, t->d_trans, trans_bytes);
    float* x = nullptr;
    if (rc == SR_OK) rc = sr_grad_input_buffer(c, n, crop_lh, crop_lw, &x);  // (the stream has drained if this grows the workspace)
    if (rc != SR_OK) return rc;
    sr_train_pair_args a;
    a.n = n; a.crop_lh = crop_lh; a.crop_lw = crop_lw; a.hr_blocks = 0;
    int k = 0;
    rc = acquire_stage(t, trans_bytes, &k);
    if (rc != SR_OK) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const sr_train_pair_crop& it = items[i];
        if (it.pair >= 0) {
            const sr_train::Img& im = t->images[(size_t)it.pair];
            a.d[i] = {im.d_lr, im.d, (uint8_t)im.lr_ch, (uint8_t)im.ch, (uint8_t)member(i), 0, im.h / f, im.w / f, it.y0, it.x0};
            continue;
        }
        // the staged rows as a pair of r1 - r0 LR rows: the crops' rows outside them are outside the source images too
        const long r0 = std::clamp<long>(it.y0, 0, it.lh), r1 = std::clamp<long>((long)it.y0 + window_rows(i), 0, it.lh);
        const size_t lrow = (size_t)it.lw * it.lr_channels, lbytes = (size_t)(r1 - r0) * lrow;
        const size_t hrow = (size_t)f * it.lw * it.hr_channels, hbytes = (size_t)(r1 - r0) * f * hrow;
        if (lbytes) memcpy((char*)t->h_stage[k] + off, it.lr_px + (size_t)r0 * lrow, lbytes);
        const uint8_t* d_lr = (const uint8_t*)t->d_trans.p + off;
        off += sr_round256(lbytes);
        if (hbytes) memcpy((char*)t->h_stage[k] + off, it.hr_px + (size_t)r0 * f * hrow, hbytes);
        a.d[i] = {d_lr, (const uint8_t*)t->d_trans.p + off, (uint8_t)it.lr_channels, (uint8_t)it.hr_channels, (uint8_t)member(i), 0, (int)(r1 - r0), it.lw,
                  (int)(it.y0 - r0), it.x0};
        off += sr_round256(hbytes);
    }
    rc = upload_stage(t, trans_bytes, k);
    if (rc != SR_OK) return rc;
    HIPCHK(c, sr_launch_train_pair_crop(f, a, (uint32_t*)t->d_batch.p, x, c->d_vtab, s));
    sr_lr_input in;
    in.in_place = true;
    return finish_step(t, n, crop_h, crop_w, &in);
}

int sr_train_sync(sr_train* t, double* err_sums, size_t cap, size_t* n_steps) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(t->c, hipSetDevice(t->c->device));
    const int rc = drain(t);
    if (rc != SR_OK) return rc;
    if (err_sums)
        for (size_t i = 0; i < std::min(cap, t->done.size()); ++i) err_sums[i] = t->done[i].err_sum;
    if (n_steps) *n_steps = t->done.size();
    t->done.clear();
    return SR_OK;
}

int sr_train_sync_stats(sr_train* t, sr_train_stat* stats, size_t cap, size_t* n_steps) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(t->c, hipSetDevice(t->c->device));
    const int rc = drain(t);
    if (rc != SR_OK) return rc;
    if (stats) std::copy_n(t->done.begin(), std::min(cap, t->done.size()), stats);
    if (n_steps) *n_steps = t->done.size();
    t->done.clear();
    return SR_OK;
}

int sr_train_set_optim(sr_train* t, float clip_norm, float ema_decay) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !sr_clip_ok(clip_norm) || !sr_ema_decay_ok(ema_decay)) return SR_E_INVALID;
    sr_ctx* c = t->c;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = drain(t);
    if (rc != SR_OK) return rc;
    if (ema_decay > 0.0f && !(t->ema_decay > 0.0f)) {  // enabled: the average starts at the parameters as they are now
        if (!t->d_e) HIPCHK(c, hipMalloc((void**)&t->d_e, sr_round256((size_t)t->np * sizeof(float))));
        HIPCHK(c, hipMemcpy(t->d_e, t->d_p, (size_t)t->np * sizeof(float), hipMemcpyDeviceToDevice));
    }
    t->clip = clip_norm;
    t->ema_decay = ema_decay;
    return SR_OK;
}

int sr_train_set_lr(sr_train* t, float lr) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !sr_lr_ok(lr)) return SR_E_INVALID;
    t->lr = lr;  // (a step's rate is a kernel argument captured when it is queued)
    return SR_OK;
}

int sr_train_ema(sr_train* t, float* out, size_t cap) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !out || cap < (size_t)t->np || !(t->ema_decay > 0.0f)) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(t->c, hipSetDevice(t->c->device));
    HIPCHK(t->c, hipStreamSynchronize(t->c->stream));
    HIPCHK(t->c, hipMemcpy(out, t->d_e, (size_t)t->np * sizeof(float), hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_train_get_state(sr_train* t, float* m, float* v, float* e, size_t cap, long long* step, long long* skipped) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !m || !v || !step || !skipped || cap < (size_t)t->np) return SR_E_INVALID;
    const bool averaged = t->ema_decay > 0.0f;
    if (averaged && !e) return SR_E_INVALID;
    sr_ctx* c = t->c;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)t->np * sizeof(float);
    unsigned long long sk = 0;
    HIPCHK(c, hipMemcpy(m, t->d_m, bytes, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(v, t->d_v, bytes, hipMemcpyDeviceToHost));
    if (averaged) HIPCHK(c, hipMemcpy(e, t->d_e, bytes, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&sk, t->d_skipped, sizeof sk, hipMemcpyDeviceToHost));
    *step = t->queued;
    *skipped = (long long)sk;
    return SR_OK;
}

int sr_train_set_state(sr_train* t, const float* m, const float* v, const float* e, size_t n, long long step, long long skipped) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !m || !v || n != (size_t)t->np || step < 0 || step >= INT32_MAX || skipped < 0) return SR_E_INVALID;
    const bool averaged = t->ema_decay > 0.0f;
    if (averaged && !e) return SR_E_INVALID;
    sr_ctx* c = t->c;
    sr_device_guard restore_device;
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = drain(t);  // (their err_sums stay in the queue of sr_train_sync)
    if (rc != SR_OK) return rc;
    const size_t bytes = (size_t)t->np * sizeof(float);
    const unsigned long long sk = (unsigned long long)skipped;
    HIPCHK(c, hipMemcpy(t->d_m, m, bytes, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(t->d_v, v, bytes, hipMemcpyHostToDevice));
    if (averaged) HIPCHK(c, hipMemcpy(t->d_e, e, bytes, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(t->d_skipped, &sk, sizeof sk, hipMemcpyHostToDevice));
    t->queued = t->harvested = step;  // nothing is in flight: the ring's slots follow the count
    return SR_OK;
}

int sr_train_params(sr_train* t, float* out, size_t cap) {
    if (!t && sr_no_device()) return SR_E_NO_DEVICE;
    if (!t || !t->c || !out || cap < (size_t)t->np) return SR_E_INVALID;
    sr_device_guard restore_device;
    HIPCHK(t->c, hipSetDevice(t->c->device));
    HIPCHK(t->c, hipStreamSynchronize(t->c->stream));
    HIPCHK(t->c, hipMemcpy(out, t->d_p, (size_t)t->np * sizeof(float), hipMemcpyDeviceToHost));
    return SR_OK;
}

void sr_train_destroy(sr_train* t) {
    if (!t) return;
    if (t->c) {  // (a session whose context was destroyed first has released its device memory then: only the shell is left)
        sr_device_guard restore_device;
        if (hipSetDevice(t->c->device) != hipSuccess) (void)hipGetLastError();
        auto& v = t->c->trains;
        v.erase(std::remove(v.begin(), v.end(), t), v.end());
        release(t);
    }
    delete t;
}

}  // extern "C"
