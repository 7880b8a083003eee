/*
 * srhip.h -- C ABI of libsrhip.so, the MI355X (gfx950) engine behind rusty_sr's
 * upscale hot path.
 *
 * The reference (millardjn/rusty_sr v1) has no FFI/plugin seam of its own; the
 * boundary this library replaces is the single call
 *     let output = graph.forward(1, vec![input], &params).remove(0);
 * at reference src/main.rs:171, together with the tensor conversions on either
 * side of it (img_to_data main.rs:170, data_to_img main.rs:175) and the weight
 * decode that feeds it (`<Vec<f32>>::decode::<u32>` main.rs:138,146,149,152).
 * The conventions of that call site are kept: the caller owns `params` and all
 * image buffers, a call is synchronous, a context is single-caller, errors are
 * reported where the reference panics (main.rs:134-138,162,164,175).
 *
 * Everything is plain C: pointers, sizes, ints.  No torch / HIP types appear
 * in a signature (`stream` is an opaque hipStream_t passed as void*; NULL =
 * HIP's default stream).  A Rust host binds this with a 30-line
 * `extern "C"` block (INTEGRATION.md shows it).
 *
 * Tensor layout everywhere: NHWC, channel fastest -- alumina's
 * DataShape::new(channels, &[W, H], n) order (reference main.rs:168).
 * The up-scaling factor of the reference binary is 3 (main.rs:31 `const FACTOR: usize = 3`;
 * the bundled weights only fit factor 3, network.rs:37); the engine also takes 2 and 4.
 */
#ifndef SRHIP_H
#define SRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_FACTOR 3
#define SR_NUM_PARAMS 130459 /* graph.num_params() of sr_net(3, None); main.rs:162 */
/* sr_net(f, None) has 2400 + 64 + 3f^2 + 192 + 3*25600 + 3*9216 + 3*(3f^2*288) parameters */
#define SR_HALO 7            /* receptive-field radius of the conv stack in input px */

typedef struct sr_ctx sr_ctx;

enum sr_status {
    SR_OK = 0,
    SR_E_INVALID = -1,     /* NULL pointer / non-positive dimension / bad channel count */
    SR_E_PARAM_COUNT = -2, /* main.rs:162 assert_eq!(params.len(), graph.num_params()) */
    SR_E_FACTOR = -3,      /* sr_net: factor must be 2, 3 or 4 (the reference ships 3, main.rs:31) */
    SR_E_NO_DEVICE = -4,   /* no gfx950 device visible: the engine has NO CPU fallback */
    SR_E_HIP = -5,         /* a HIP runtime call failed; sr_last_hip_error() has the code */
    SR_E_NOMEM = -6,
    SR_E_BYTEVEC = -7,     /* main.rs:138 "ByteVec conversion failed" */
    SR_E_HALO = -8,        /* band call with a halo that is neither 0 nor >= SR_HALO (or a band thinner than SR_HALO) */
    SR_E_COMM = -9,        /* librccl missing, no communicator on the context, or an RCCL call failed;
                              sr_last_comm_error() has the ncclResult_t */
    SR_E_DOMAIN = -10      /* SR_PRECISION_SPLIT_F16 only: a weight, an input or an activation cannot be carried as a pair of
                              halves (not finite, or 65504 and beyond); see sr_set_precision / sr_check_domain */
};

/* Replaces: `<Vec<f32>>::decode::<u32>(blob)` (bytevec 0.2.0; reference
 * main.rs:138,146,149,152).  Wire format: u32 LE n | n x u32 LE sizes (=4) |
 * n x f32 LE.  Pass out = NULL to query *n_out.  Host-side, no GPU needed. */
int sr_rsr_decode(const uint8_t* blob, size_t len, float* out, size_t cap, size_t* n_out);

/* Replaces: `.encode::<u32>()` (reference main.rs:213), the inverse of the above.
 * Pass out = NULL to query the byte length in *len_out. */
int sr_rsr_encode(const float* params, size_t n, uint8_t* out, size_t cap, size_t* len_out);

/* Replaces: `sr_net(FACTOR, None)` + the parameter-count assert (reference
 * main.rs:146,162; network.rs:16-109).  Validates, selects HIP device
 * `device`, uploads the parameters once re-packed into the MFMA B-operand
 * layout.  Fails with SR_E_NO_DEVICE when no GPU is present. */
int sr_create(sr_ctx** out, const float* params, size_t n_params, int factor, int device);
void sr_destroy(sr_ctx* ctx);

/* The reference's upscale() picks one of three graphs (main.rs:133-158):
 *   SR_GRAPH_SR_NET      sr_net(FACTOR, None)      network.rs:16-109   130459 params
 *   SR_GRAPH_BILINEAR    bilinear_net(FACTOR)      network.rs:111-123  `-p bilinear`, 0 params
 *                        sRGB->linear, bilinear x3, linear->sRGB
 *   SR_GRAPH_DOWNSAMPLE  downsample_net(FACTOR)    network.rs:125-138  `-d`, 0 params
 *                        sRGB->linear, mean over non-overlapping 3x3 blocks, linear->sRGB;
 *                        output (h/3) x (w/3), remainder rows / columns dropped
 * sr_create_graph replaces the `(params, graph)` selection + the count assert
 * (main.rs:162): n_params must equal sr_num_params(graph).  Every sr_upscale_*
 * entry point below then means `graph.forward` for whichever graph the context
 * holds (for SR_GRAPH_DOWNSAMPLE the output is n*(h/3)*(w/3) pixels); the band
 * entry points exist for SR_GRAPH_SR_NET only. */
enum sr_graph { SR_GRAPH_SR_NET = 0, SR_GRAPH_BILINEAR = 1, SR_GRAPH_DOWNSAMPLE = 2 };
int sr_create_graph(sr_ctx** out, int graph, const float* params, size_t n_params, int factor, int device);
int sr_num_params(int graph); /* graph.num_params() at factor 3; -1 for an unknown graph */

/* `sr_net(factor, ..)` takes the factor as an argument (network.rs:16) although main.rs:31
 * hard-wires 3 ("TODO: expose upscaling factor as argument"): sr_create / sr_create_graph accept
 * factor 2, 3 or 4 for SR_GRAPH_SR_NET given a parameter vector of sr_num_params_factor(factor)
 * entries in the same op order (the expand node has 3 f^2 channels, network.rs:37), and every
 * entry point then produces f*h x f*w outputs.  No 2x / 4x weights ship with the reference, so
 * those factors are checked against the CPU restatement only (UNPINNED). */
int sr_num_params_factor(int factor); /* -1 unless 2 <= factor <= 4 */

/* Sizes: nothing but device memory limits an image.  One pass of the conv stack keeps four 32-channel f32 feature maps
 * (512 B per input pixel) beside input and output: 1920x1080 1.1 GB, 3840x2160 4.3 GB, 11 000 x 11 000 62 GB (tested; byte
 * offsets and outputs beyond 4 GiB are fine).  The host-pointer entry points cut large jobs into chunks / row bands, so their
 * workspace is that of a band.  A failed allocation is SR_E_NOMEM and leaves the context usable.
 *
 * Replaces: graph.forward(n, vec![input], &params) (reference main.rs:171).
 * in : n*h*w*3 f32 in [0,1] (what img_to_data produced), host memory.
 * out: n*(3h)*(3w)*3 f32, pre-quantisation, host memory. */
int sr_upscale_f32(sr_ctx* ctx, const float* in, int n, int h, int w, float* out);

/* Replaces: img_to_data + graph.forward + data_to_img(..).to_rgba() (reference
 * main.rs:170-175) as one fused device pass: u8/255 on load, and
 * clamp(floor(255 v + 0.5)) with alpha = 255 on store.
 * in : n*h*w*in_channels u8, in_channels 3 (RGB) or 4 (RGBA, alpha dropped; sr_upscale_rgba8_alpha below keeps it).
 * out: n*(3h)*(3w)*4 u8 RGBA.  Host memory. */
int sr_upscale_rgba8(sr_ctx* ctx, const uint8_t* in, int in_channels, int n, int h, int w,
                     uint8_t* out_rgba);

/* Optional: everything the matching sr_upscale_* call of that shape would do EXCEPT touching caller memory -- the
 * workspace and staging allocations, the events, and one pass of its kernels over whatever the staging buffers hold
 * (code objects load, clocks come up) -- and what a sr_upscale_*_dev call of that shape creates on first use (see there).  The first real call then costs what every later one does; a host calls this at
 * start-up, or -- like the CLI -- on one thread while another still decodes the input file.  The reference has no
 * counterpart (alumina allocates inside graph.forward, main.rs:171). */
int sr_reserve_f32(sr_ctx* ctx, int n, int h, int w);
int sr_reserve_rgba8(sr_ctx* ctx, int in_channels, int n, int h, int w);

/* One image across several GPUs from one process: ctxs[k] (sr_net contexts of the same parameters, normally one
 * per device, created with sr_create(.., device k)) produces a contiguous share of the rows, a multiple of 8.
 * The SR_HALO rows a share needs from its neighbours are read from the caller's image itself, so the devices
 * exchange nothing; results are bit-identical to the single-device call.  This is the host-memory counterpart
 * of the RCCL halo exchange of device-resident bands (sr_upscale_sharded_* below); the reference has neither
 * (one CPU, main.rs:171).  Shares run concurrently, one host thread per context. */
int sr_upscale_f32_multi(sr_ctx* const* ctxs, int n_ctx, const float* in, int h, int w, float* out);
int sr_upscale_rgba8_multi(sr_ctx* const* ctxs, int n_ctx, const uint8_t* in, int in_channels, int h, int w,
                           uint8_t* out_rgba);

/* Many images across several GPUs from one process -- throughput mode: image i goes to ctxs[i mod n_ctx]
 * (contexts of the same parameters and arithmetic mode, one per device), parameters replicated, no exchange;
 * each context runs its images through its own upload / compute / download pipeline on its own host thread.
 * in / out are the whole batch (n images, host memory).  The reference processes one image per process
 * (main.rs:164-171); its users loop over files. */
int sr_upscale_f32_batch_multi(sr_ctx* const* ctxs, int n_ctx, const float* in, int n, int h, int w, float* out);
int sr_upscale_rgba8_batch_multi(sr_ctx* const* ctxs, int n_ctx, const uint8_t* in, int in_channels, int n, int h, int w,
                                 uint8_t* out_rgba);

/* The host-pointer entry points (sr_upscale_f32 / sr_upscale_rgba8 and their _multi forms) run upload / conv stack / download as a software
 * pipeline on up to four HIP streams of the context's own, created on first need (a call that is one chunk uses one): a batch goes in
 * chunks of whole images, one sr_net image of about 200K pixels or more (100K with f32 output) as two or more row bands with SR_HALO
 * halo rows, so that a band's download runs under the next band's kernels (bit-identical to the undivided pass, see sr_upscale_band_*).  Results do not depend on the setting; 0 = one upload, one pass, one download.  The reference has no counterpart
 * (its tensors never leave host memory, main.rs:168-175); buffers from sr_host_alloc are page-locked, which lets the copies run at
 * PCIe rate and truly overlap -- any host memory is accepted.
 * (The device-pointer entry points below run on the CALLER'S stream; where they cut one image into two bands they also use one stream
 * of the context's own and a second set of feature maps, see there.) */
int sr_set_pipeline(sr_ctx* ctx, int enabled);         /* default: enabled */
int sr_host_alloc(void** out, size_t bytes);           /* SR_E_NO_DEVICE without a GPU */
void sr_host_free(void* p);

/* Same two operations on buffers already resident in this context's device
 * memory (HBM); asynchronous on `stream` (opaque hipStream_t; NULL = HIP's
 * default stream, which is also torch's default stream).  The caller orders
 * its own producers / consumers of d_in / d_out on that stream.  These are what bench.py times and what the multi-GPU
 * driver calls after its halo exchange.  One image (n = 1) of enough rows may run as TWO row bands, the second on a stream
 * of the context's own that is forked from `stream` and joined back to it by events (one band's launches drain while the
 * other's fill; bit-identical): the call is still asynchronous and ordered on `stream` alone.  What that costs:
 * a second set of feature maps (each band's are half the size; should they not fit, the call runs undivided), and -- on its first
 * use -- one stream creation and the allocations, inside the call (sr_reserve_* of the same shape does both ahead of time).
 * After such a call sr_read_feature refuses (each workspace holds one band), as it does after a pipelined host call.
 * u8 device images are READ as whole aligned 32-bit words by the parameter-free graphs' kernels: up to 3 bytes in front of the
 * image's first byte and behind its last one -- bytes of the same aligned word, hence of the same allocation granule -- may be
 * read (never written, never used).
 * Alignment: d_out_rgba, and every float* buffer (d_in and d_out of the f32 forms), must be 4-byte aligned -- the kernels store the
 * RGBA output as whole 32-bit words and address f32 buffers as floats.  A pointer that is not is refused with SR_E_INVALID before
 * anything is launched, and the output is left untouched.  No larger alignment is needed (views into a larger allocation are fine),
 * and u8 inputs may start at any byte.  The same holds for the band and sharded forms below. */
int sr_upscale_f32_dev(sr_ctx* ctx, const float* d_in, int n, int h, int w, float* d_out,
                       void* stream);
int sr_upscale_rgba8_dev(sr_ctx* ctx, const uint8_t* d_in, int in_channels, int n, int h, int w,
                         uint8_t* d_out_rgba, void* stream);

/* Stream capture.  Every *_dev entry point of this header may be called while `stream` is being captured (hipStreamBeginCapture,
 * torch.cuda.graph); tests/test_gpu_graph_capture.py holds each of them to the following, on bytes.
 *  1. A *_dev call made on a capturing stream launches nothing: it records its launches into the capture -- the second band of a forked
 *     call included, which joins back to `stream` before the call returns.
 *  2. Every replay gives, byte for byte, what the eager call gives on the buffers' contents at replay time.  Nothing is baked in but the
 *     pointers, the shapes, the mode (sr_set_precision, sr_set_loss and the switches of srhip_experimental.h as they stood at capture) and the
 *     scalar arguments.
 *  3. A graph stays valid while no later call on the context grows or frees a buffer -- no larger shape, no sr_destroy -- and while
 *     sr_set_params, sr_set_precision, sr_set_loss and the setter of srhip_experimental.h are not called.  Replaying a graph after such
 *     a call is UNDEFINED: its nodes may point into freed memory.  Destroy the graph first.
 *  4. Eager calls on the same context, *_dev or host-pointer, of any shape within the reserved capacity may run between replays,
 *     serialised by the caller.  Neither side changes the other's bytes: from its first captured call on, a context clears the borders
 *     of its feature maps with every pass, eager or replayed, instead of trusting the geometry it last saw.
 *  5. A call that would have to allocate, free, create a stream or an event, or upload a first-use table while its stream is capturing
 *     returns SR_E_INVALID before it launches, allocates or frees anything: the capture stays valid and the context usable.  The
 *     remedy: sr_reserve_* or one eager call of that shape (and mode) first.  A forked plan whose second stream or workspace does not
 *     exist yet is recorded undivided instead where the first workspace holds the whole image.  A sharded call of more than one rank
 *     is not recorded at all (SR_E_INVALID): its exchange runs on the communicator's terms.
 *  6. stream = NULL cannot be captured, and the library cannot see such a capture: do not try.
 *  7. sr_check_domain after a replay reports what the replayed kernels saw: the flag lives in mapped host memory.
 *  8. The fork tuner takes no sample from a captured call, and sr_set_profiling times none.  A captured call runs the rule's plan,
 *     whatever the tuner has measured or decided for the shape. */

/* Row-band form for images sharded across GPUs.  d_in holds h_ext = halo_top +
 * h_band + halo_bot input rows of ONE image of width w; halo_top / halo_bot are
 * the rows that belong to the neighbouring bands (0 = this edge is the true
 * image edge, where the reference's per-layer zero padding applies; otherwise
 * must be >= SR_HALO).  d_out receives only the band's 3*h_band output rows.
 * Bit-identical to the corresponding rows of the un-sharded call. */
int sr_upscale_band_f32_dev(sr_ctx* ctx, const float* d_in, int h_ext, int w, int halo_top,
                            int halo_bot, float* d_out, void* stream);
int sr_upscale_band_rgba8_dev(sr_ctx* ctx, const uint8_t* d_in, int in_channels, int h_ext, int w,
                              int halo_top, int halo_bot, uint8_t* d_out_rgba, void* stream);

/* ---- One image sharded over several GPUs, DEVICE-RESIDENT: RCCL halo exchange inside the library ----
 * The reference has no counterpart (one CPU, main.rs:171).  A context can own one RCCL communicator
 * (librccl is dlopen'ed on first use; a host needs no torch and no MPI).  Rank r of n holds a contiguous
 * row band of the image in its GPU's memory (bands in rank order, every band >= SR_HALO rows, same width);
 * sr_upscale_sharded_*_dev sends the band's first / last SR_HALO rows to ranks r-1 / r+1 and receives theirs
 * (one grouped ncclSend / ncclRecv pair per neighbour over xGMI, queued on `stream`), then runs the band form
 * of the conv stack (sr_upscale_band_*_dev) and writes the band's 3*h_band output rows to d_out.  The rows of
 * all ranks together are bit-identical to the single-GPU call.
 * Interior first: the exchange runs on a second stream of the context's own (forked from `stream` by an event and joined back
 * to it by another, like the two-band form above) while `stream` copies the band and computes the first layer on every row that
 * reads no halo row; only then does `stream` wait for the halos.  The call stays asynchronous and ordered on `stream` alone.
 *
 * One process per GPU (the normal form):  rank 0 calls sr_comm_unique_id and hands the 128 bytes to the other
 * ranks by whatever means the host has (a file, a socket, an environment variable, torch.distributed);
 * every rank then calls sr_comm_init_rank (collective: returns when all n ranks have joined).
 * One process, n GPUs: sr_comm_init_all on n contexts of distinct devices (ncclCommInitAll; rank = index), then
 * sr_upscale_sharded_*_all drives all bands from the calling thread (grouped exchange, synchronous).
 * One process, without RCCL: sr_comm_init_local on n contexts (rank = index; the same device may appear more than
 * once).  sr_upscale_sharded_*_all then has every context PULL its two halos from the neighbours' bands with
 * hipMemcpyPeerAsync on its own stream (SDMA over xGMI, peer access enabled where the devices allow it): no
 * rendezvous, no compute unit spent on the exchange.  The *_dev entry points return SR_E_COMM on such a context
 * (a lone rank cannot see its neighbours' buffers). */
#define SR_COMM_ID_BYTES 128
int sr_comm_available(void);                            /* 1 if librccl could be loaded */
int sr_comm_unique_id(uint8_t* id, size_t cap);         /* cap >= SR_COMM_ID_BYTES */
int sr_comm_init_rank(sr_ctx* ctx, const uint8_t* id, size_t id_len, int rank, int nranks);
int sr_comm_init_all(sr_ctx* const* ctxs, int n);
int sr_comm_init_local(sr_ctx* const* ctxs, int n);
void sr_comm_destroy(sr_ctx* ctx);                      /* sr_destroy does this too */
int sr_comm_rank(sr_ctx* ctx, int* rank, int* nranks);  /* 0 of 1 without a communicator */
int sr_last_comm_error(sr_ctx* ctx);                    /* ncclResult_t of the last failed RCCL call */
int sr_last_comm_ms(sr_ctx* ctx, double* comm_ms);      /* device time of the last sharded call's halo exchange (an event pair on the stream
                                                         * it ran on, recorded on every call; waits for the exchange, not for the kernels).
                                                         * sr_last_timing after a sharded call: total_ms = this context's whole step */
int sr_last_comm_exposed_ms(sr_ctx* ctx, double* exposed_ms);  /* ... and how long the band's stream stood waiting for it (an event pair
                                                         * either side of its wait): the part of comm_ms that was NOT hidden under the
                                                         * band copy and the first layer's interior rows */
int sr_upscale_sharded_f32_dev(sr_ctx* ctx, const float* d_band, int h_band, int w, float* d_out, void* stream);
int sr_upscale_sharded_rgba8_dev(sr_ctx* ctx, const uint8_t* d_band, int in_channels, int h_band, int w,
                                 uint8_t* d_out_rgba, void* stream);
int sr_upscale_sharded_f32_all(sr_ctx* const* ctxs, int n, const float* const* d_bands, const int* h_bands, int w,
                               float* const* d_outs);
int sr_upscale_sharded_rgba8_all(sr_ctx* const* ctxs, int n, const uint8_t* const* d_bands, int in_channels,
                                 const int* h_bands, int w, uint8_t* const* d_outs);

/* Arithmetic of the conv stack.
 *   SR_PRECISION_F32       (default) v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulate --
 *                          the same arithmetic class as the reference's f32 CPU path.  Domain: any f32, like
 *                          graph.forward (main.rs:171); infinities and NaNs propagate as IEEE arithmetic has them.
 *   SR_PRECISION_SPLIT_F16 every activation / weight is carried as a pair of halves
 *                          (hi + lo/2048, ~2^-23 relative) and each product is three f16 MFMAs with
 *                          f32 accumulation on the matrix cores; outputs stay within the 1e-4 bar
 *                          (tests/test_gpu_parity.py runs every parity test in both modes).
 *                          DOMAIN: every weight, input value and activation finite and below 65504 in magnitude
 *                          (u8 images through the bundled weights stay below 100).  Nothing outside it is clamped
 *                          silently:
 *                            - sr_set_precision returns SR_E_DOMAIN for a parameter vector with such a weight and leaves
 *                              the context in its previous mode;
 *                            - the kernels notice an input or activation that leaves the domain.  The synchronous
 *                              host-pointer entry points (sr_upscale_f32 / _rgba8 and their _multi / _batch_multi forms) then
 *                              compute the whole call again in SR_PRECISION_F32 and return its result;
 *                            - the asynchronous *_dev entry points cannot: their output is unspecified where the overflow
 *                              reached, and the context keeps a fault that sr_check_domain reports.
 * sr_set_precision is host-side state and no device work, like sr_set_loss: a call reads the mode when it is QUEUED and passes what follows
 * from it to its launches by value, so the mode may be changed while earlier *_dev calls are still in flight on the caller's stream --
 * nothing waits, the calls already queued keep their mode, and the feature-map borders that the other layout needs are cleared by the
 * next call, on that call's stream and in its place there (tests/test_gpu_stream_order.py queues both changes between calls behind a
 * delay).  Not so sr_set_params, which rewrites device memory that calls in flight read: synchronise first, as it says. */
enum sr_precision { SR_PRECISION_F32 = 0, SR_PRECISION_SPLIT_F16 = 1 };
int sr_set_precision(sr_ctx* ctx, int mode);
/* After the stream(s) of earlier *_dev calls have been synchronised: SR_E_DOMAIN if any of them left the domain of
 * SR_PRECISION_SPLIT_F16 since the last check (the fault is cleared), else SR_OK.  No call made in SR_PRECISION_F32 raises a
 * fault; one left by earlier split-mode calls is kept -- across sr_set_precision and across host-pointer calls, which neither
 * report nor act on it -- until it is checked.  (A host-pointer call over several contexts recomputes per context: only the
 * contexts whose rows left the domain return f32-mode rows; both modes meet the same 1e-4 bar.) */
int sr_check_domain(sr_ctx* ctx);

/* (A/B tuning switches that change no result bit, and their environment defaults, are NOT part of this interface:
 * include/srhip_experimental.h.) */

/* Test hook: copy the post-activation feature maps of the most recent call
 * (image 0) to host: which = 0..3 -> f, l1, l2, l3 (h*w*32 f32 each).  The
 * reference exposes the same values as graph node data (network.rs:30,43-48).  Refused (SR_E_INVALID) after a call that ran the image
 * as bands -- a pipelined host call, a forked device call: sr_set_pipeline(ctx, 0) / the undivided device call leave whole maps. */
int sr_read_feature(sr_ctx* ctx, int which, float* out_host, size_t cap_floats);

/* ---- Validation: the loss of a parameter set on an HR image ----
 * Replaces the validation pass of the reference's `train` (main.rs:220-247): the forward half of sr_net(f, Some((0.0, linear_loss)))
 * (network.rs:88-102) on one HR image, and the sums its PSNR is made of.  For the context's factor f (2, 3 or 4):
 *   input  = LinearToSrgb(mean over f x f blocks of SrgbToLinear(hr)), f32 -- NOT quantised to u8 (unlike the downsample graph's output)
 *   output = sr_net(f)(input), f32, no clamp, no quantisation
 *   err    = sum over the compared elements of (output - hr)^2, or with linear_loss != 0 (`-l`, --linearLoss) of
 *            (SrgbToLinear(output) - SrgbToLinear(hr))^2 (the same formula outside [0, 1])
 * hr is what img_to_data makes of the image (byte / 255, RGB, alpha dropped) or an f32 RGB image taken as is.  Each difference is formed
 * in f32, its square summed in f64 (the reference sums in f32).  *n_elems counts the compared elements (pixels x 3): the PSNR of a set of
 * images is -10 log10(sum err_i / sum n_i), the reference's weighting of each image's mean error by flat_size_single (main.rs:236-245).
 * UNPINNED (alumina's source is not at hand): sizes not divisible by f follow the downsample graph -- the LR image is floor(h/f) x
 * floor(w/f), the loss compares the output with the top-left f floor(h/f) x f floor(w/f) crop of hr, and n_elems counts that crop; h < f
 * or w < f is SR_E_INVALID.  alumina's MseLoss normalisation is not reproduced: the sum and the count are what the PSNR needs.
 * SR_GRAPH_SR_NET contexts only (others: SR_E_INVALID); the context's precision applies, and in SR_PRECISION_SPLIT_F16 the host-pointer
 * forms recompute in exact f32 where a value leaves that mode's domain, like sr_upscale_f32.  The result is the same bits from run to
 * run, context to context and device to device (a fixed reduction order, no atomics).  A job that does not fit is SR_E_NOMEM and leaves
 * the context usable.  With sr_set_profiling on, sr_last_timing's total_ms is then the whole host-pointer call on the device (upload,
 * pool, network, loss, download).  Synchronous, host memory: */
int sr_validation_error_rgba8(sr_ctx* ctx, const uint8_t* hr, int in_channels, int h, int w, int linear_loss,
                              double* err_sum, size_t* n_elems);
int sr_validation_error_f32(sr_ctx* ctx, const float* hr, int h, int w, int linear_loss,
                            double* err_sum, size_t* n_elems);
/* ... device memory: ordered on `stream` alone, like every *_dev call; the sum is written to d_err_sum (device memory, 4-byte aligned).
 * d_hr may start at any byte (read as whole aligned 32-bit words, like the parameter-free graphs' u8 inputs).  The element count is
 * 3 f floor(h/f) f floor(w/f). */
int sr_validation_error_rgba8_dev(sr_ctx* ctx, const uint8_t* d_hr, int in_channels, int h, int w, int linear_loss,
                                  double* d_err_sum, void* stream);
/* Test hook, like sr_read_feature: the training graph's `input` node (the pooled LR image, floor(h/f) x floor(w/f) x 3 f32) and `output`
 * node (the f32 network output, f times that size) of the most recent validation call, image 0.  Either pointer may be NULL. */
int sr_read_validation_nodes(sr_ctx* ctx, float* lr_out, size_t cap_lr, float* out_out, size_t cap_out);

/* Backpropagation through the reference's training graph sr_net(f, Some((l2, linear_loss))) (network.rs:78-103; `g.backprop` inside
 * Adam::optimise_from, main.rs:181-257), for a batch of n HR images of h x w -- SR_GRAPH_SR_NET contexts only (else SR_E_INVALID),
 * h, w >= the context's factor f (else SR_E_INVALID):
 *   input  = the validation pass's pooled LR batch (f32, not quantised; the top-left f floor(h/f) x f floor(w/f) crop of each image)
 *   output = sr_net(f)(input), f32;  e = output - hr, or SrgbToLinear(output) - SrgbToLinear(hr) with linear_loss (the formula of
 *            sr_validation_error_*, outside [0, 1] too); hr is byte / 255 (alpha dropped) or the f32 values as they are
 *   err_sum = sum of e^2 over the batch: each difference in f32, the squares summed in f64 -- per image the same as
 *             sr_validation_error_*; n_elems = n 3 f floor(h/f) f floor(w/f)
 *   grad   = d/dp of  loss_scale sum e^2 + l2 sum p^2,  at p = `params` (NOT the context's inference weights: like
 *            backprop(n, input, training_input, params), main.rs:240), sr_num_params_factor(f) floats in the .rsr segment order.
 * UNPINNED (alumina's source is not at hand): MseLoss's normalisation is the caller's `loss_scale` (the Python helper passes
 * 1 / n_elems, alumina's mean over flat_size_all as far as can be told); L2Regularisation is strength x sum p^2 over every parameter.
 * Always exact f32 (v_mfma_f32_32x32x2_f32), whatever sr_set_precision says; no float atomics: the same bits on every run, context and
 * device.  A wrong n_params is SR_E_PARAM_COUNT; with no HIP device present every backprop entry point returns SR_E_NO_DEVICE.  A batch
 * that does not fit returns SR_E_NOMEM and leaves the context usable.  Synchronous, host memory (`hr` n x h x w x in_channels bytes, or
 * n x h x w x 3 floats; `grad` n_params floats): */
int sr_backprop_f32(sr_ctx* ctx, const float* params, size_t n_params, const float* hr, int n, int h, int w, int linear_loss,
                    float loss_scale, float l2, double* err_sum, size_t* n_elems, float* grad);
int sr_backprop_rgba8(sr_ctx* ctx, const float* params, size_t n_params, const uint8_t* hr, int in_channels, int n, int h, int w,
                      int linear_loss, float loss_scale, float l2, double* err_sum, size_t* n_elems, float* grad);
/* ... device memory, ordered on `stream` alone; no host synchronisation (but for the first call of a larger batch, which grows the
 * context's workspace).  d_params and d_grad hold sr_num_params_factor(f) floats and, like d_err_sum (one double), must be 4-byte
 * aligned: a misaligned pointer is SR_E_INVALID before any launch.  16 kernel launches per call (n + 15 when h is not a multiple of f). */
int sr_backprop_rgba8_dev(sr_ctx* ctx, const float* d_params, const uint8_t* d_hr, int in_channels, int n, int h, int w, int linear_loss,
                          float loss_scale, float l2, double* d_err_sum, float* d_grad, void* stream);
/* One Adam step over n parameters in device memory (4-byte aligned), step = 1, 2, ... (UNPINNED: the textbook form, in f32):
 *   m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;  p <- p - lr m^ / (sqrt(v^) + eps),
 *   m^ = m / (1 - beta1^step), v^ = v / (1 - beta2^step).
 * The reference's values: lr 2e-3, beta1 0.95, beta2 0.995, eps 1e-7 (main.rs:199-205).  One launch on `stream`. */
int sr_adam_step_dev(sr_ctx* ctx, float* d_params, float* d_m, float* d_v, const float* d_grad, size_t n, int step, float lr,
                     float beta1, float beta2, float eps, void* stream);

/* ---- Training: the reference's `train` (main.rs:181-257) behind the ABI ----
 * sr_init_params: the reference's g.init_params() for sr_net(factor) -- sr_num_params_factor(factor) floats in the .rsr segment order
 * written to out (cap >= that many, else SR_E_INVALID).  Host only; no device needed.  UNPINNED (alumina's source is not at hand):
 *   convolutions  MSRA normal, std = multiplier sqrt(2 / fan_in), fan_in = ks^2 in_channels, multiplier 1.0 for conv0 and 0.1 for the rest
 *                 (network.rs); biases 0; BeLU beta (init_porque_no_los_dos) 1 on even channels, 0 on odd ones.
 * The generator: SplitMix64 seeded with `seed`; each weight takes two draws u1, u2 = (x >> 11) 2^-53 and is
 * (float)(std sqrt(-2 ln(1 - u1)) cos(2 pi u2)) in double arithmetic (Box-Muller, one value per pair): the same bits on any host whose
 * libm rounds log / cos / sqrt of doubles alike. */
int sr_init_params(int factor, uint64_t seed, float* out, size_t cap);

/* Replace an sr_net context's inference weights: the parameters are packed as sr_create packs them and copied into the context's existing
 * parameter buffer; the split-half mode's weight check is redone (a weight of 65504 or more, or not finite, then makes
 * sr_set_precision(SR_PRECISION_SPLIT_F16) refuse, as after sr_create; a context already in that mode refuses such a vector with
 * SR_E_DOMAIN).  A wrong n_params is SR_E_PARAM_COUNT.  Either refusal leaves the weights unchanged.  Synchronous: waits for the
 * context's own streams.  The caller must have finished (synchronised) its own *_dev work that uses the context before calling. */
int sr_set_params(sr_ctx* ctx, const float* params, size_t n_params);

/* A training session on an sr_net context's device: parameters, Adam moments, gradient, a ring of per-step err_sum values and an
 * image store all live on the device.  One step, queued on the context's own stream without host synchronisation:
 *   1. train_crop_kernel gathers the n crops (crop_h x crop_w, alpha dropped, pixels outside the source image 0 -- y0 / x0 may be
 *      negative or overhang) into one n x crop_h x crop_w x 3 u8 batch;
 *   2. sr_backprop_rgba8_dev on that batch, loss_scale = 1 / n_elems, l2 as given;
 *   3. sr_adam_step_dev with the session's step count (from 1).
 * The same items give the same bits on every run.  An item names a resident image (image >= 0, an id of sr_train_add_image) or carries
 * host pixels (image = -1: px, in_channels 3 or 4, h, w), which pass through page-locked staging that the session reuses only once the
 * copy that read it has completed; sr_train_step returns once it no longer needs px.  Invalid items -- an unknown id, n outside
 * 1 .. SR_TRAIN_MAX_BATCH, a crop smaller than the factor, a channel count other than 3 or 4 -- are SR_E_INVALID before any launch.  A
 * workspace that does not fit is SR_E_NOMEM; the step is not taken and the session stays usable.  At most SR_TRAIN_RING steps are in
 * flight: a step beyond that first waits for the oldest.  The session uses the context's stream and its backprop workspace: while it
 * has steps in flight the context takes no other call (sr_train_params / sr_train_sync wait for them).  sr_destroy of the context
 * waits for its sessions' steps and frees what they hold on the device; such a session refuses every call (SR_E_INVALID) but
 * sr_train_destroy, which a caller still makes.
 * store_bytes: the budget of resident images.  SR_TRAIN_STORE_AUTO: the device's free memory at creation less max(8 GiB, 1/8 of it),
 * which leaves room for the step workspace and for validation passes on large images; 0: every image transient. */
#define SR_TRAIN_STORE_AUTO ((size_t)-1)
#define SR_TRAIN_MAX_BATCH 64
#define SR_TRAIN_RING 64
typedef struct sr_train sr_train;
typedef struct {
    int image;          /* id of a resident image, or -1: the pixels below */
    const uint8_t* px;  /* image = -1: h x w x in_channels u8, host memory */
    int in_channels, h, w;
    int y0, x0;         /* crop origin in the source image */
} sr_train_crop;
int sr_train_create(sr_train** out, sr_ctx* ctx, const float* start_params, size_t n_params, int linear_loss, float l2, float lr,
                    float beta1, float beta2, float eps, size_t store_bytes);
/* Upload an image into the store: *id >= 0 when it is resident from now on, -1 when the store has no room (the image stays the caller's). */
int sr_train_add_image(sr_train* t, const uint8_t* px, int in_channels, int h, int w, int* id);
int sr_train_step(sr_train* t, const sr_train_crop* items, int n, int crop_h, int crop_w);
/* Augmented steps: sr_train_step / sr_train_step_pairs with a member k (0..7) per item, members[i] for items[i]; members == NULL means
 * all 0, and that is what the two plain calls are.  T_k is the self-ensemble's (below): swap the two spatial axes if k & 4, then reverse
 * the rows if k & 2, then the columns if k & 1.  The batch keeps its shape n x crop_h x crop_w x 3: item i of it is T_k(W), W the source
 * window at (y0, x0) -- crop_h x crop_w pixels for k < 4, crop_w x crop_h (rows x columns) for k >= 4 -- cut exactly as the plain
 * call cuts it: alpha dropped, zero outside the image, origins that may be negative or overhang.  k = 0 is the plain call's crop, by the
 * plain call's code.  For pairs, windows and origins are in LR pixels: the LR item is T_k of the LR window (crop_lh x crop_lw, or
 * crop_lw x crop_lh), the HR item T_k of the f x as large HR window at (f y0, f x0); T_k maps f x f blocks onto f x f blocks, so the two
 * stay aligned, and the LR item still goes through the byte / 255 table straight into the backward pass's input (no pool launch, no
 * conversion launch).  The transform is part of the gather: no extra launch, memory or host work.  A step equals sr_backprop_rgba8_dev
 * (sr_pair_backprop_rgba8_dev) + sr_adam_step_dev on the transformed crops, bit for bit.  A member above 7 is SR_E_INVALID before any
 * launch, with the other item checks.  A transient item stages the rows its window can reach (crop_w of them for k >= 4, f x as many HR
 * rows for a pair).  The ring, drain, staging and SR_E_NOMEM rules are those of sr_train_step. */
int sr_train_step_aug(sr_train* t, const sr_train_crop* items, const uint8_t* members, int n, int crop_h, int crop_w);
/* Waits for every queued step; err_sums receives the err_sum of each step since the last sync (at the parameters before that step), in
 * step order, at most cap of them; *n_steps their number.  err_sums may be NULL. */
int sr_train_sync(sr_train* t, double* err_sums, size_t cap, size_t* n_steps);
int sr_train_params(sr_train* t, float* out, size_t cap);  /* waits; the current parameters (cap >= n_params) */
void sr_train_destroy(sr_train* t);

/* ---- Pairs: validation, backpropagation and training on LR / HR image pairs ----
 * The reference's training graph makes its own input, LinearToSrgb(mean_f x f(SrgbToLinear(hr))) (network.rs:87-92): every parameter file
 * it trains is a model of that one degradation.  The sr_pair_* entry points (and the session's sr_train_add_pair / sr_train_step_pairs) take the network's input from the
 * caller instead (the reference's later releases have this as train_prescaled).  For the context's factor f (2, 3 or 4):
 *   The LR image is lh x lw, the HR image exactly f lh x f lw -- the sizes are passed once, as lh, lw; lh < 1 or lw < 1 is SR_E_INVALID
 *   before any launch, and a host whose images have other sizes must refuse them itself (the Python binding and the CLI do).
 *   input  = img_to_data(lr): each byte as (float)b / 255.0f, RGB, alpha dropped (bit-equal to an f32 division for all 256 bytes);
 *            an f32 LR image is taken as is
 *   output = sr_net(f)(input), f32, no clamp;  e = output - hr, or SrgbToLinear(output) - SrgbToLinear(hr) with linear_loss
 *   err_sum, grad: the text of sr_validation_error_* / sr_backprop_* above -- differences formed in f32, squares summed in f64,
 *            n_elems = n 3 f lh f lw, the gradient of loss_scale sum e^2 + l2 sum p^2 at the `params` passed
 * Backpropagation is always exact f32; validation follows the context's precision (and, in SR_PRECISION_SPLIT_F16, the host-pointer forms
 * recompute in exact f32 where a value leaves that mode's domain).  No atomics, a fixed reduction order: the same bits on every run,
 * context and device.  Everything behind the input stage is the code of the pooled calls: a pair whose LR image is the pooled calls' own
 * input gives their result bit for bit.  SR_GRAPH_SR_NET contexts only; the other refusals (SR_E_PARAM_COUNT, SR_E_NOMEM, SR_E_NO_DEVICE)
 * are those of the pooled calls.  u8 forms: lr_channels and hr_channels are 3 or 4, independently.  Synchronous, host memory: */
int sr_pair_validation_error_rgba8(sr_ctx* ctx, const uint8_t* lr, int lr_channels, const uint8_t* hr, int hr_channels, int lh, int lw,
                                   int linear_loss, double* err_sum, size_t* n_elems);
int sr_pair_validation_error_f32(sr_ctx* ctx, const float* lr, const float* hr, int lh, int lw, int linear_loss,
                                 double* err_sum, size_t* n_elems);
/* ... device memory, ordered on `stream` alone.  d_lr, like d_hr, may start at any byte (read as whole aligned 32-bit words);
 * d_err_sum 4-byte aligned.  After any of the three, sr_read_validation_nodes' lr_out is the converted LR image (lh x lw x 3). */
int sr_pair_validation_error_rgba8_dev(sr_ctx* ctx, const uint8_t* d_lr, int lr_channels, const uint8_t* d_hr, int hr_channels, int lh, int lw,
                                       int linear_loss, double* d_err_sum, void* stream);
/* Batches of n pairs (`lr` n x lh x lw x lr_channels bytes or x 3 floats, `hr` n x f lh x f lw x hr_channels bytes or x 3 floats): */
int sr_pair_backprop_f32(sr_ctx* ctx, const float* params, size_t n_params, const float* lr, const float* hr, int n, int lh, int lw,
                         int linear_loss, float loss_scale, float l2, double* err_sum, size_t* n_elems, float* grad);
int sr_pair_backprop_rgba8(sr_ctx* ctx, const float* params, size_t n_params, const uint8_t* lr, int lr_channels, const uint8_t* hr,
                           int hr_channels, int n, int lh, int lw, int linear_loss, float loss_scale, float l2, double* err_sum,
                           size_t* n_elems, float* grad);
/* ... device memory: d_lr and d_hr may start at any byte; d_params, d_grad and d_err_sum must be 4-byte aligned (else SR_E_INVALID before
 * any launch).  16 kernel launches: the LR conversion in the pool's place, then the 15 of the backward pass. */
int sr_pair_backprop_rgba8_dev(sr_ctx* ctx, const float* d_params, const uint8_t* d_lr, int lr_channels, const uint8_t* d_hr, int hr_channels,
                               int n, int lh, int lw, int linear_loss, float loss_scale, float l2, double* d_err_sum, float* d_grad,
                               void* stream);
/* A training session's pairs.  sr_train_add_pair uploads both images as ONE store entry (out of the same budget; *id = -1 when there is
 * no room); ids of pairs and of plain images come from one sequence, and each kind is refused (SR_E_INVALID) where the other is asked
 * for.  sr_train_step_pairs is sr_train_step on pairs: y0 / x0 are in LR pixels, the LR crop is crop_lh x crop_lw there and the HR crop
 * f crop_lh x f crop_lw at (f y0, f x0); pixels outside the images are 0 in both crops, origins may be negative or overhang.  One launch,
 * train_pair_crop_kernel, cuts the HR crops into the u8 batch and the LR crops -- converted, f32 -- straight into the backward pass's input:
 * such a step has no pool launch (crop, the backward pass's 15 launches, Adam).  A transient pair (pair = -1) passes the rows its crops can
 * reach through the session's staging.  The refusals and the ring, drain and SR_E_NOMEM rules of sr_train_step hold; a session may mix both
 * kinds of step. */
typedef struct {
    int pair;              /* id of a resident pair, or -1: the pixels below */
    const uint8_t* lr_px;  /* pair = -1: lh x lw x lr_channels u8, host memory */
    const uint8_t* hr_px;  /*            f lh x f lw x hr_channels u8 */
    int lr_channels, hr_channels, lh, lw;
    int y0, x0;            /* crop origin in the LR image */
} sr_train_pair_crop;
int sr_train_add_pair(sr_train* t, const uint8_t* lr_px, int lr_channels, const uint8_t* hr_px, int hr_channels, int lh, int lw, int* id);
int sr_train_step_pairs(sr_train* t, const sr_train_pair_crop* items, int n, int crop_lh, int crop_lw);
int sr_train_step_pairs_aug(sr_train* t, const sr_train_pair_crop* items, const uint8_t* members, int n, int crop_lh, int crop_lw);  /* (above) */

/* ---- Self-ensemble: the network averaged over flips and rotations of the image ----
 * The reference has no counterpart (main.rs:171 runs graph.forward once); other super-resolution tools call it geometric self-ensemble or
 * test-time augmentation.  Member k (0..7) transforms an h x w x C image, T_k:
 *   if k & 4, swap the two spatial axes;  then, if k & 2, reverse the rows;  then, if k & 1, reverse the columns.
 * T_k^-1 undoes these steps in the opposite order.  For a mask `members` (bits 0..7, not 0, count = its number of set bits):
 *   acc = 0.0f
 *   for k = 0..7 ascending, if members has bit k:  acc = acc + T_k^-1(sr_net(T_k(x)))        plain f32 adds, in this order
 *   out = acc * (1.0f / count)                                                              the reciprocal formed in f32 on the host
 * Each sr_net(.) is exactly what the plain call of that shape computes in the context's precision (members with bit 2 run a w x h pass).
 * u8 input is byte / 255 with alpha dropped, as in the plain call (the bytes are transformed); RGBA8 output is clamp(floor(255 out + 0.5))
 * with alpha 255.  members == 1 gives the plain call's bits.  Any image size, factors 2, 3 and 4, both precisions; no atomics, a grid that
 * depends on the shape alone: the same bits on every run.  n images are handled one after another.
 * Refused with SR_E_INVALID before any launch, the output untouched: a context other than SR_GRAPH_SR_NET, members == 0 or > 255, and (the
 * _dev forms) pointers that break the alignment rules of sr_upscale_*_dev.  Workspace: the plain call's, an f32 copy of the image, one f32 output map and -- for RGBA8
 * output -- one f32 accumulator (an f32 call accumulates in its output buffer), grown on first use; sr_reserve_* knows nothing of them.  A
 * shape that cannot fit is SR_E_NOMEM and leaves the context usable.
 * Quality: +0.06 .. +0.15 dB PSNR on images pooled by 3 with the bundled weights -- but LOWER on an image that is itself
 * this network's output, whose artefacts the identity member reproduces and the others do not.
 * Device memory, asynchronous and ordered on `stream` alone, like sr_upscale_*_dev (a member may run as two bands there, too): */
#define SR_ENSEMBLE_ALL 0xFFu   /* all 8 flips and rotations */
#define SR_ENSEMBLE_FLIPS 0x0Fu /* identity, column flip, row flip, both: every pass is h x w */
#define SR_ENSEMBLE_HFLIP 0x03u /* identity and the column flip */
int sr_upscale_ensemble_f32_dev(sr_ctx* ctx, const float* d_in, int n, int h, int w, float* d_out, unsigned members, void* stream);
int sr_upscale_ensemble_rgba8_dev(sr_ctx* ctx, const uint8_t* d_in, int in_channels, int n, int h, int w, uint8_t* d_out_rgba,
                                  unsigned members, void* stream);
/* ... host memory, synchronous: one upload, the device call on the context's own stream, one download.  In SR_PRECISION_SPLIT_F16 the
 * whole call is computed again in exact f32 where a value left that mode's domain, like sr_upscale_f32 / _rgba8.  With sr_set_profiling on,
 * sr_last_timing's total_ms is every pass and pixel move of the call, h2d / d2h its two copies. */
int sr_upscale_ensemble_f32(sr_ctx* ctx, const float* in, int n, int h, int w, float* out, unsigned members);
int sr_upscale_ensemble_rgba8(sr_ctx* ctx, const uint8_t* in, int in_channels, int n, int h, int w, uint8_t* out_rgba, unsigned members);
/* sr_validation_error_rgba8 ("pool": the input is the pooled HR image) / sr_pair_validation_error_rgba8 with `output` replaced by the
 * ensemble of the network over `input`: pool or LR conversion, loss, f64 sum, n_elems and the crop rule are theirs.
 * sr_read_validation_nodes afterwards returns the ensemble output as `output`. */
int sr_pool_validation_error_ensemble_rgba8(sr_ctx* ctx, const uint8_t* hr, int in_channels, int h, int w, int linear_loss, unsigned members,
                                       double* err_sum, size_t* n_elems);
int sr_pair_validation_error_ensemble_rgba8(sr_ctx* ctx, const uint8_t* lr, int lr_channels, const uint8_t* hr, int hr_channels, int lh,
                                            int lw, int linear_loss, unsigned members, double* err_sum, size_t* n_elems);

/* ---- Metrics: Y-channel PSNR and SSIM, the super-resolution benchmark protocol ----
 * The reference scores a parameter file by one pooled RGB MSE (main.rs:236-246, the validation calls above).  Papers and leaderboards
 * score the 8-bit luma of the saved image, with a border shaved off, per image.  Two operands A (the scored image) and B (the ground
 * truth), both H x W, 8-bit RGB; alpha is dropped, as img_to_data drops it.  Where A is the network's f32 output (the validation forms
 * below) it is quantised on load by data_to_img's rule, clamp(floor(255 v + 0.5), 0, 255) in f32: the scores are exactly those of the
 * pixels `rusty_sr IN OUT` would save, and no u8 copy of the output is written.
 *   Luma      Y = (65481 R + 128553 G + 24966 B + 127500) div 255000 + 16, in integer arithmetic: round(16 + (65.481 R + 128.553 G +
 *             24.966 B) / 255), MATLAB's rgb2ycbcr on uint8, ties upward (194 of the 2^24 colours sit exactly on .5, and the double
 *             formula misses the exact value on 39).  Y is in [16, 235].
 *   Shave     s >= 0 pixels are removed from each border; the scored region is (H - 2s) x (W - 2s).  shave = -1 means the context's
 *             factor f, the protocol's value; anything below is SR_E_INVALID before any launch.  In the validation forms H x W is the
 *             top-left f floor(h/f) x f floor(w/f) crop of the HR image, the one the loss uses.
 *   Y-PSNR    y_sq_err = sum of (Y_A - Y_B)^2 over the region, an exact integer; y_count = the region's pixels.  Per image the PSNR is
 *             10 log10(255^2 y_count / y_sq_err), and inf at zero error.
 *   SSIM      (Wang et al. 2004, as the benchmark scripts apply it.)  Window: 11 x 11 Gaussian, sigma 1.5, g_i = exp(-(i - 5)^2 / 4.5) /
 *             sum, applied separably (rows, then columns); only "valid" positions inside the region count: ssim_count = (H - 2s - 10)
 *             (W - 2s - 10).  C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; mu = filt(Y), var = filt(Y^2) - mu^2, cov = filt(Y_A Y_B) -
 *             mu_A mu_B; the map is ((2 mu_A mu_B + C1)(2 cov + C2)) / ((mu_A^2 + mu_B^2 + C1)(var_A + var_B + C2)); ssim_sum is the
 *             f64 sum of the map, and per image the SSIM is ssim_sum / ssim_count.
 *   Arithmetic  The weights are an f64 table computed once on the host; filters, map and sum are f64 (in f32, filt(Y^2) - mu^2 cancels
 *             at 65 025 and the mean is off by 4e-5 on a bright image).  One partial per workgroup of SR_METRICS_TILE x SR_METRICS_TILE
 *             region pixels, a grid that depends on the shape alone, one workgroup adding the partials in a fixed order, no atomics:
 *             the same bits on every run, context and device.  Identical operands give ssim_sum == ssim_count exactly.
 *   Degenerate sizes are not errors: a region with a side below 11 has ssim_count = 0 and ssim_sum = 0; an empty region also y_count =
 *             0 and y_sq_err = 0.
 * u8 images only: the scores are defined on 8-bit images.  A job that does not fit is SR_E_NOMEM and leaves the context usable. */
#define SR_METRICS_TILE 32
typedef struct sr_metrics { uint64_t y_sq_err, y_count; double ssim_sum; uint64_t ssim_count; } sr_metrics;
/* Two images the caller holds (h x w x a_channels and h x w x b_channels bytes, 3 or 4 channels each); no network runs, and a context of
 * any graph will do -- so a bilinear or foreign upscaler's output can be scored.  Synchronous, host memory: */
int sr_image_metrics_rgba8(sr_ctx* ctx, const uint8_t* a, int a_channels, const uint8_t* b, int b_channels, int h, int w, int shave,
                           sr_metrics* metrics);
/* ... device memory: ordered on `stream` alone, no host synchronisation.  d_a and d_b may start at any byte (read as whole aligned 32-bit
 * words, nothing outside the words of the image).  d_result16 (device memory, 4-byte aligned) receives 16 bytes: the uint64 y_sq_err, then
 * the double ssim_sum; the counts follow from h, w and shave. */
int sr_image_metrics_rgba8_dev(sr_ctx* ctx, const uint8_t* d_a, int a_channels, const uint8_t* d_b, int b_channels, int h, int w, int shave,
                               void* d_result16, void* stream);
/* sr_validation_error_rgba8 / sr_pair_validation_error_rgba8 (members = 0) or their ensemble forms (members = the mask) with the scores
 * of the same run of the network: A = the quantised output, B = the HR crop.  err_sum and n_elems are the bits of those calls; one more
 * pass behind the loss does the scoring.  The context's precision applies, and the split-half mode's recomputation in exact f32. */
int sr_pool_validation_metrics_rgba8(sr_ctx* ctx, const uint8_t* hr, int in_channels, int h, int w, int linear_loss, unsigned members, int shave,
                                double* err_sum, size_t* n_elems, sr_metrics* metrics);
int sr_pair_validation_metrics_rgba8(sr_ctx* ctx, const uint8_t* lr, int lr_channels, const uint8_t* hr, int hr_channels, int lh, int lw,
                                     int linear_loss, unsigned members, int shave, double* err_sum, size_t* n_elems, sr_metrics* metrics);
/* ... device memory, like sr_validation_error_rgba8_dev / sr_pair_validation_error_rgba8_dev (no ensemble): d_err_sum one double,
 * d_result16 the 16 bytes above, both 4-byte aligned. */
int sr_pool_validation_metrics_rgba8_dev(sr_ctx* ctx, const uint8_t* d_hr, int in_channels, int h, int w, int linear_loss, int shave,
                                    double* d_err_sum, void* d_result16, void* stream);
int sr_pair_validation_metrics_rgba8_dev(sr_ctx* ctx, const uint8_t* d_lr, int lr_channels, const uint8_t* d_hr, int hr_channels, int lh, int lw,
                                         int linear_loss, int shave, double* d_err_sum, void* d_result16, void* stream);

/* ---- Transparency: the alpha channel upscaled, the colours bled under it ----
 * The reference drops alpha (data_to_img(..).to_rgba() writes 255, main.rs:175), and so does every call above.  In a straight-alpha image
 * the RGB under alpha == 0 is arbitrary, usually black: the network, whose receptive field reaches SR_HALO pixels, would paint that hard edge
 * as a dark, ringing fringe into pixels that are still partly visible once the alpha is interpolated.  So the call is three passes: bleed
 * the visible colours outward under the transparent area, upscale the bled image, write the interpolated alpha of the ORIGINAL image into
 * the result.  Both rules are integer arithmetic, the same bits on every run and device.  UNPINNED: the reference has nothing to compare with;
 * tests/alpha_ref.py restates both rules in numpy.
 *   Bleed, radius R (0 .. SR_ALPHA_BLEED_MAX), of an h x w RGBA8 image: known_0(p) = alpha(p) > 0, c_0(p) = RGB(p).  For t = 1 .. R every
 *     pixel p that is not known_{t-1} looks at its 8 neighbours inside the image; with N those that are known_{t-1} and N not empty, per
 *     channel c_t(p) = (2 sum_{q in N} c_{t-1}(q) + |N|) div (2 |N|) -- the mean, rounded half up -- and p is known_t.  Each step reads the
 *     step before only, so the result does not depend on any order.  Output: RGB = c_R, alpha = the input's, untouched.  Pixels with
 *     alpha > 0 never change, pixels farther than R (Chebyshev) from every visible one keep their RGB, R = 0 is the identity, and the
 *     images of a batch do not see each other.  The rule commutes with the self-ensemble's eight transforms.
 *   Alpha x f (f = 2, 3, 4): bilinear interpolation with half-pixel centres and clamped edges, the geometry of the bilinear graph, on the
 *     alpha bytes.  Along an axis of length len, output index o: i = o div f, m = 2 (o mod f) + 1 - f; taps (i, i + 1) with weights
 *     (2f - m, m) if m >= 0, else (i - 1, i) with (-m, 2f + m); tap indices clamped to [0, len - 1].  A_out = (sum wy wx a + 2 f^2) div
 *     (4 f^2): the exact bilinear value rounded half up.  A constant alpha stays that constant; an opaque image stays 255.
 * Images are RGBA8 in device memory, 4 bytes a pixel, and BOTH the input and the output pointers must be 4-byte aligned (the kernels move
 * whole dwords; no larger alignment is needed).  Every call is asynchronous and ordered on `stream` alone.
 * sr_bleed_rgba8_dev: d_out = bleed(d_in, radius), n images of h x w; any context.  d_out == d_in is refused (a workgroup reads its
 *   neighbours' pixels), and the two images must not overlap otherwise.
 * sr_merge_alpha_rgba8_dev: byte 3 of every pixel of the f h x f w image at d_out_rgba <- alpha x f of d_lr_rgba (h x w), f the context's
 *   factor; the three colour bytes are left as they are.  SR_GRAPH_SR_NET and SR_GRAPH_BILINEAR contexts.
 * sr_upscale_rgba8_alpha_dev: bleed into a workspace buffer of the context (grown on first use, freed by sr_destroy; radius == 0 launches no
 *   bleed and reads the caller's image), then exactly sr_upscale_rgba8_dev's path (members == 1) or sr_upscale_ensemble_rgba8_dev's
 *   (any other mask) on the bled image, then the merge from the original d_in_rgba.  An opaque image gives the plain call's bytes.
 * sr_upscale_rgba8_alpha: the same on host memory, synchronous: one upload, the device call on the context's own stream, one download; in
 *   SR_PRECISION_SPLIT_F16 the whole call is computed again in exact f32 where a value left that mode's domain.  With sr_set_profiling on,
 *   sr_last_timing's total_ms is the bleed, every pass of the network and the merge, h2d / d2h the two copies.
 * Refused with SR_E_INVALID before any launch, the output untouched: SR_GRAPH_DOWNSAMPLE contexts (merge and upscale calls), a radius outside
 * 0 .. SR_ALPHA_BLEED_MAX, members == 0 or > 255, members != 1 on a context other than SR_GRAPH_SR_NET, a device pointer that is not 4-byte
 * aligned.  A shape whose workspace does not fit is SR_E_NOMEM and leaves the context usable.  Cost at 1920 x 1080: DESIGN.md 4m. */
#define SR_ALPHA_BLEED_DEFAULT 8   /* >= SR_HALO: every visible pixel's receptive field is then bled */
#define SR_ALPHA_BLEED_MAX 16
#define SR_ALPHA_BLEED_TILE 32     /* side of the bleed kernel's output tile (the tests put sizes either side of its multiples) */
int sr_bleed_rgba8_dev(sr_ctx* ctx, const uint8_t* d_in_rgba, int n, int h, int w, int radius, uint8_t* d_out_rgba, void* stream);
int sr_merge_alpha_rgba8_dev(sr_ctx* ctx, const uint8_t* d_lr_rgba, int n, int h, int w, uint8_t* d_out_rgba, void* stream);
int sr_upscale_rgba8_alpha_dev(sr_ctx* ctx, const uint8_t* d_in_rgba, int n, int h, int w, uint8_t* d_out_rgba, int radius, unsigned members,
                               void* stream);
int sr_upscale_rgba8_alpha(sr_ctx* ctx, const uint8_t* in_rgba, int n, int h, int w, uint8_t* out_rgba, int radius, unsigned members);

/* ---- Resampling to any size ----
 * The network upscales by exactly its factor and the downsample graph shrinks by exactly 3; these calls produce any output size, on the
 * device, from values that have not been quantised yet.  UNPINNED: the reference has no counterpart; tests/resize_ref.py restates the rule
 * in numpy (f64) and tests/test_resize_cpu.py holds that restatement to Pillow's Image.resize.
 *   The rule is a separable resampler in Pillow's convention.  Per axis, n_in -> n_out samples: scale = n_in / n_out, fs = max(scale, 1); a
 *     filter F of support S reaches s = S fs.  Output index o has its centre at c = (o + 0.5) scale and the taps i = lo .. hi - 1 with
 *     lo = max(trunc(c - s + 0.5), 0), hi = min(trunc(c + s + 0.5), n_in); w_i = F((i + 0.5 - c) / fs), divided by the sum of the w_i: taps
 *     are clipped at the border and renormalised, never replicated.  Filters: SR_FILTER_BOX, S = 0.5, F = 1 for -0.5 < x <= 0.5;
 *     SR_FILTER_TRIANGLE, S = 1, F = max(0, 1 - |x|); SR_FILTER_CATROM, S = 2, the Keys cubic with a = -0.5; SR_FILTER_LANCZOS3, S = 3,
 *     F = sinc(x) sinc(x / 3) for |x| < 3.  Weights are computed in f64 and stored as f32.
 *   Columns are resampled first (horizontally, over every input row), then rows; sums run in f32 over the taps in ascending index.  Colours
 *     go through SrgbToLinear before the horizontal pass and LinearToSrgb after the vertical one -- the expressions of the bilinear and
 *     downsample graphs; a negative linear value takes the linear branch -- unless SR_RESIZE_SRGB_SPACE is set in `flags`, when neither
 *     is applied.  SR_PIXELS_RGBA8 input is byte / 255 with alpha ignored; SR_PIXELS_RGBA8 output is clamp(floor(255 v + 0.5)) with alpha
 *     255.  SR_PIXELS_F32 is n x h x w x 3 f32.  The images of a batch do not see each other.  SR_FILTER_BOX from h x w to h/3 x w/3
 *     (sizes divisible by 3) is the downsample graph, SR_FILTER_TRIANGLE to 3h x 3w the bilinear graph.
 * sr_resize_dev: n images of h x w at d_in (in_pixels: an sr_pixels) -> n images of oh x ow at d_out (out_pixels), on any context (no
 *   parameters are used).  Three launches on `stream`: the tap tables (computed on the device: no copy from the host), the horizontal and
 *   the vertical pass; the tables and the f32 intermediate (n x h x ow pixels) live in a workspace of the context, grown on first use and
 *   freed by sr_destroy.  Asynchronous and ordered on `stream` alone.  Both pointers 4-byte aligned; the images must not overlap.
 * sr_resize_rgba8: the same from and to RGBA8 in host memory, synchronous: one upload, the device call on the context's stream, one download.
 * sr_upscale_rgba8_sized_dev: the network's path of sr_upscale_f32_dev (members == 1) or sr_upscale_ensemble_f32_dev (any other mask) on
 *   byte / 255 of the image, into a workspace buffer, then sr_resize_dev from that f32 image to RGBA8 of oh x ow: the result is quantised
 *   once, after the resampling.  SR_GRAPH_SR_NET (factors 2-4) and SR_GRAPH_BILINEAR contexts.
 * sr_upscale_rgba8_sized: the same on host memory, synchronous; in SR_PRECISION_SPLIT_F16 the whole call is computed again in exact f32
 *   where a value left that mode's domain.  With sr_set_profiling on, sr_last_timing's total_ms is the network and the three launches of
 *   the resampling, h2d / d2h the two copies.
 * Refused with SR_E_INVALID before any launch, the output untouched: a null pointer; n, h, w, oh or ow below 1; sizes whose byte counts
 * overflow; an unknown filter or pixel kind; a flag bit other than SR_RESIZE_SRGB_SPACE; d_in == d_out; a pointer that is not 4-byte
 * aligned; SR_GRAPH_DOWNSAMPLE contexts, members == 0 or > 255 and members != 1 on a context other than SR_GRAPH_SR_NET (the _sized calls).
 * A shape whose workspace does not fit is SR_E_NOMEM and leaves the context usable.  Cost: DESIGN.md 4n. */
enum sr_filter { SR_FILTER_BOX = 0, SR_FILTER_TRIANGLE = 1, SR_FILTER_CATROM = 2, SR_FILTER_LANCZOS3 = 3 };
enum sr_pixels { SR_PIXELS_RGBA8 = 0, SR_PIXELS_F32 = 1 };
#define SR_RESIZE_SRGB_SPACE 1
int sr_resize_dev(sr_ctx* ctx, const void* d_in, int in_pixels, int n, int h, int w, void* d_out, int out_pixels, int oh, int ow, int filter,
                  unsigned flags, void* stream);
int sr_resize_rgba8(sr_ctx* ctx, const uint8_t* in, int n, int h, int w, uint8_t* out, int oh, int ow, int filter, unsigned flags);
int sr_upscale_rgba8_sized_dev(sr_ctx* ctx, const uint8_t* d_in_rgba, int n, int h, int w, uint8_t* d_out_rgba, int oh, int ow, int filter,
                               unsigned flags, unsigned members, void* stream);
int sr_upscale_rgba8_sized(sr_ctx* ctx, const uint8_t* in_rgba, int n, int h, int w, uint8_t* out_rgba, int oh, int ow, int filter,
                           unsigned flags, unsigned members);

/* ---- Degradation: blur, noise and JPEG made on the device ----
 * The reference trains for one degradation, the f x f mean of linear-light pixels; the pair calls above take any LR image, but made by
 * someone else, once.  Modern training recipes synthesise the LR crop from the HR crop at every draw, each with its own blur width, noise
 * level and JPEG quality: this operator does that on the device.  UNPINNED: the reference has no counterpart; tests/degrade_ref.py restates
 * the rule in numpy (f64), and the kernels are held to it byte for byte.
 *   A call names an image (h x w, 3 or 4 channels, alpha dropped), a factor f (2, 3 or 4), a member k (0..7, T_k of the self-ensemble) and
 *   a frame: frame_h x frame_w HR pixels, multiples of f, at (y0, x0).  As in sr_train_step_aug the frame is T_k(W), W the source window at
 *   (y0, x0) -- frame_h x frame_w pixels for k < 4, frame_w x frame_h (rows x columns) for k >= 4.  Frame pixel (p, q) is defined for ANY
 *   integers p, q by the same mapping (p' = frame_h - 1 - p if k & 2, q' = frame_w - 1 - q if k & 1; source pixel (y0 + p', x0 + q'), or
 *   (y0 + q', x0 + p') if k & 4): the image's RGB byte inside the image, 0 outside, so the blur sees the true neighbours beyond the
 *   frame's edge.  Origins may be negative or overhang.  The output is the LR frame, frame_h / f x frame_w / f x 3 bytes.
 *   All arithmetic is f64.  Every rounding to an integer is R(v) = sign(v) floor(|v| + 0.5 + 2^-30): with integer pixels exact ties are
 *   structural (a DC coefficient is k / 8 over an integer table entry), and the bias keeps them off the boundary.
 *   1. Linearise: SrgbToLinear(byte / 255), s <= 0.04045 ? s / 12.92 : pow((s + 0.055) / 1.055, 2.4), a 256-entry table made on the host.
 *   2. Blur (sigma > 0): separable Gaussian in linear light over the frame, radius ceil(3 sigma), weights exp(-d^2 / (2 sigma^2)) divided
 *      by their sum (taken in tap order); rows first (along q), then columns; sums in tap order.
 *   3. Pool: the mean of each f x f block, summed in row-major order, divided by f^2.
 *   4. Encode: v = 255 LinearToSrgb(mean), l <= 0.0031308 ? 12.92 l : 1.055 pow(l, 1 / 2.4) - 0.055.
 *   5. Noise (noise > 0, in 8-bit levels): value index i = (y lw + x) 3 + c in the LR frame; x1, x2 are outputs number 2i + 1 and 2i + 2
 *      of the SplitMix64 stream seeded with `seed` (output j = mix(seed + j 0x9E3779B97F4A7C15), the generator of sr_init_params);
 *      u = (x >> 11) 2^-53;  v += noise sqrt(-2 ln(1 - u1)) cos(2 pi u2).
 *   6. Quantise: b = clamp(R(v), 0, 255).
 *   7. JPEG round trip (quality 1..100; 0 skips it), 4:4:4: 8 x 8 blocks anchored at the LR frame's origin, ragged edges padded by
 *      replicating the last row / column.  Y = 0.299 R + 0.587 G + 0.114 B, Cb = 128 - 0.168735892 R - 0.331264108 G + 0.5 B,
 *      Cr = 128 + 0.5 R - 0.418687589 G - 0.081312411 B, each clamp(R(.), 0, 255) - 128.  coef = C b C^T with the orthonormal DCT-II
 *      C[u][x] = cos((2x + 1) u pi / 16) / 2, row 0 divided by sqrt 2 (C b first; sums in index order).  Tables: Annex K's luma / chroma
 *      tables, scale = q < 50 ? 5000 / q : 200 - 2 q, t = clamp((base scale + 50) / 100, 1, 255) in integers.  qz = R(coef / t); the
 *      inverse transform of qz t (C^T first), + 128, R() and clamp; R = Y + 1.402 (Cr - 128), G = Y - 0.344136286 (Cb - 128) -
 *      0.714136286 (Cr - 128), B = Y + 1.772 (Cb - 128), R() and clamp.
 *   With sigma = noise = quality = 0 the result is the 8-bit quantisation of the pooled calls' input.  sigma and noise are f32 in the
 *   struct and are widened to f64 as they are.
 * sr_degrade_rgba8: host memory, synchronous: one upload, one launch on the context's stream, one download.  Any graph's context will do;
 *   no network runs.
 * sr_degrade_rgba8_dev: device memory, asynchronous and ordered on `stream` alone; both pointers may start at any byte.
 * Refused with SR_E_INVALID before any launch, the output untouched: a null pointer, in_channels other than 3 or 4, h or w below 1, a
 *   factor outside 2..4, frame sizes that are not multiples of f or are below f, a member above 7, sigma outside [0, SR_DEGRADE_MAX_SIGMA],
 *   noise outside [0, SR_DEGRADE_MAX_NOISE], quality outside 0..100.
 * sr_train_step_degrade: a step of a plain-image session (sr_train_step_aug's items, members and rules) whose network input is the
 *   degraded crop: item i of the u8 HR batch is T_k of its window, as in sr_train_step_aug, and the network's input is the operator's
 *   output for the same window, member and deg[i], as byte / 255 -- what sr_train_step_pairs_aug computes from that LR / HR pair, bit
 *   for bit.  One launch cuts the HR crops and degrades them straight into the backward pass's input: crop, the backward pass's 15
 *   launches, Adam; no extra launch, no host work.  crop_h and crop_w must be multiples of the session's factor.  A transient item stages
 *   the rows its window and its blur radius can reach.  The ring, drain, staging and SR_E_NOMEM rules are those of sr_train_step. */
#define SR_DEGRADE_MAX_SIGMA 4
#define SR_DEGRADE_MAX_NOISE 64
typedef struct sr_degrade {
    float sigma;    /* Gaussian blur, HR pixels; 0: none */
    float noise;    /* standard deviation of the noise, 8-bit levels; 0: none */
    int quality;    /* JPEG quality 1..100; 0: no JPEG */
    uint64_t seed;  /* of the noise stream */
} sr_degrade;
int sr_degrade_rgba8(sr_ctx* ctx, const uint8_t* hr, int in_channels, int h, int w, int factor, int y0, int x0, int frame_h, int frame_w,
                     int member, const sr_degrade* deg, uint8_t* lr_rgb);
int sr_degrade_rgba8_dev(sr_ctx* ctx, const uint8_t* d_hr, int in_channels, int h, int w, int factor, int y0, int x0, int frame_h, int frame_w,
                         int member, const sr_degrade* deg, uint8_t* d_lr_rgb, void* stream);
int sr_train_step_degrade(sr_train* t, const sr_train_crop* items, const uint8_t* members, const sr_degrade* deg, int n, int crop_h, int crop_w);

/* ---- Borders: what lies beyond the edge of the image ----
 * Every layer of sr_net zero-pads its feature maps, so every call above computes an image's left edge without knowing its right edge: a
 * tileable texture comes back with a seam.  These calls let the caller say what continues the image: the image is padded by `pad` pixels
 * on every side under a border mode, the UNCHANGED network runs on the padded image, and the centre f h x f w is cut out of the result.
 * The network's receptive field reaches SR_HALO pixels, so with pad >= SR_HALO the result is exactly what the network computes for the
 * centre of the infinitely continued plane: under SR_BORDER_WRAP, the centre tile of the 3 x 3 tiling, bit for bit on the CPU oracle
 * (tests/test_border_cpu.py; at pad = SR_HALO - 1 it is not).  UNPINNED: the reference has no counterpart; tests/border_ref.py restates
 * the index rule in numpy (np.pad).
 *   The rule is per axis and separable.  Padded index j (0 .. size + 2 pad - 1) of an axis of `size` samples shows sample idx(j - pad):
 *     SR_BORDER_WRAP       idx(i) = i mod size, a true modulo (size may be below pad, and 1)             np.pad mode="wrap"
 *     SR_BORDER_REPLICATE  idx(i) = clamp(i, 0, size - 1)                                                np.pad mode="edge"
 *     SR_BORDER_MIRROR     m = i mod 2 size; idx(i) = m < size ? m : 2 size - 1 - m: a reflection that REPEATS the edge sample
 *                                                                                                        np.pad mode="symmetric"
 *   There is no "zero" mode: padding with zeros is NOT the plain call (the biases make the features of a black border non-zero).  "Off"
 *   is the calls above.  Quality: SR_BORDER_WRAP is for images that tile.  SR_BORDER_REPLICATE and SR_BORDER_MIRROR are NOT a measured
 *   quality gain -- the network was trained with its own zero padding (README.md has the numbers).
 * Images are RGBA8 (4 bytes a pixel, moved as whole dwords: alpha travels with its pixel) or f32 RGB (n x h x w x 3) in device memory;
 * both pointers 4-byte aligned, the images must not overlap.  Asynchronous and ordered on `stream` alone.  Pure data movement: the same
 * bits on every run.
 * sr_pad_*_dev: d_out = the n images of (h + 2 pad) x (w + 2 pad) of the n images of h x w at d_in; pad 0 .. SR_BORDER_PAD_MAX; any context.
 * sr_crop_*_dev: d_out = the ch x cw window at (y0, x0) of each of the n images of H x W at d_in, contiguous; any context.
 * sr_upscale_*_border_dev: pad into a workspace buffer of the context, then exactly sr_upscale_*_dev's path (members == 1) or
 *   sr_upscale_ensemble_*_dev's (any other mask, as in sr_upscale_rgba8_alpha) on the padded image into a second workspace buffer, then
 *   the crop of its centre to d_out: bit for bit the plain (or ensemble) call on the padded image, cropped.  The buffers are grown on
 *   first use, all or nothing, and freed by sr_destroy.  SR_GRAPH_SR_NET (factors 2-4, both precisions) and SR_GRAPH_BILINEAR contexts.
 *   bleed (RGBA8): -1 gives opaque output (alpha 255) like sr_upscale_rgba8; 0 .. SR_ALPHA_BLEED_MAX keeps transparency, in the order
 *   bleed -> pad -> network -> crop -> merge: the bleed and the alpha merge of sr_upscale_rgba8_alpha run on the UNPADDED image (the
 *   alpha is interpolated exactly as there; the bleed does not wrap), so an opaque image gives the bytes of bleed = -1.
 * sr_upscale_*_border: the same on host memory, synchronous: one upload, the device call on the context's own stream, one download; in
 *   SR_PRECISION_SPLIT_F16 the whole call is computed again in exact f32 where a value left that mode's domain.  With sr_set_profiling on,
 *   sr_last_timing's total_ms is every launch of the call, h2d / d2h the two copies.
 * Refused with SR_E_INVALID before any launch, the output untouched: a null pointer; n, h or w below 1; a mode outside 1..3; a pad above
 * SR_BORDER_PAD_MAX or (sr_upscale_*) below SR_HALO or (sr_pad_*) below 0; a crop window that is not inside its image; SR_GRAPH_DOWNSAMPLE
 * contexts, members == 0 or > 255, members != 1 on a context other than SR_GRAPH_SR_NET, a bleed outside -1 .. SR_ALPHA_BLEED_MAX (sr_upscale_*);
 * a device pointer that is not 4-byte aligned; d_in == d_out (sr_pad_*, sr_crop_*).  A shape whose padded size overflows or whose workspace
 * cannot fit the device is SR_E_NOMEM, by arithmetic, and leaves the context usable.  Cost at 1920 x 1080: DESIGN.md 4p. */
#define SR_BORDER_WRAP 1
#define SR_BORDER_REPLICATE 2
#define SR_BORDER_MIRROR 3
#define SR_BORDER_PAD_DEFAULT 8    /* >= SR_HALO; a multiple of 4, so that the crop's source rows keep the output rows' 16-byte phase */
#define SR_BORDER_PAD_MAX 32
int sr_pad_rgba8_dev(sr_ctx* ctx, const uint8_t* d_in_rgba, int n, int h, int w, int mode, int pad, uint8_t* d_out_rgba, void* stream);
int sr_pad_f32_dev(sr_ctx* ctx, const float* d_in, int n, int h, int w, int mode, int pad, float* d_out, void* stream);
int sr_crop_rgba8_dev(sr_ctx* ctx, const uint8_t* d_in_rgba, int n, int H, int W, int y0, int x0, int ch, int cw, uint8_t* d_out_rgba,
                      void* stream);
int sr_crop_f32_dev(sr_ctx* ctx, const float* d_in, int n, int H, int W, int y0, int x0, int ch, int cw, float* d_out, void* stream);
int sr_upscale_rgba8_border_dev(sr_ctx* ctx, const uint8_t* d_in_rgba, int n, int h, int w, uint8_t* d_out_rgba, int mode, int pad,
                                unsigned members, int bleed, void* stream);
int sr_upscale_f32_border_dev(sr_ctx* ctx, const float* d_in, int n, int h, int w, float* d_out, int mode, int pad, unsigned members,
                              void* stream);
int sr_upscale_rgba8_border(sr_ctx* ctx, const uint8_t* in_rgba, int n, int h, int w, uint8_t* out_rgba, int mode, int pad, unsigned members,
                            int bleed);
int sr_upscale_f32_border(sr_ctx* ctx, const float* in, int n, int h, int w, float* out, int mode, int pad, unsigned members);

/* ---- Video: planar YCbCr frames in and out, a frame stream ----
 * The reference takes RGB images (main.rs:164-175); a clip is YCbCr, and converting it on the CPU and quantising it twice costs more
 * than the network.  These calls take and give planar 8-bit frames laid out exactly like a Y4M frame payload: Y (h x w), then Cb, then
 * Cr, each ch x cw -- ch = ceil(h / 2), cw = ceil(w / 2) for SR_YUV_420, h x w for SR_YUV_444 -- contiguous, so a plane may start at
 * any byte.  UNPINNED: the reference has no counterpart; tests/yuv_ref.py states the rule in numpy (f64) and the kernels equal it bit
 * for bit.  The network sees single frames: no motion, no blending across frames.  A frame stream may, as an exact opt-in
 * (sr_video_set_reuse below), take the output rows of the last frame for the rows no changed input row can reach.
 *   Format    subsampling SR_YUV_420 | SR_YUV_444; siting (4:2:0 only) SR_YUV_SITING_CENTER (JPEG, plain C420) | SR_YUV_SITING_LEFT
 *             (MPEG-2: horizontally co-sited with the even columns; vertically centred under both); matrix SR_YUV_BT601 (Kr 0.299,
 *             Kb 0.114) | SR_YUV_BT709 (0.2126, 0.0722); range SR_YUV_LIMITED (Y 16..235, C 16..240) | SR_YUV_FULL.
 *   Constants (f64, formed once on the host): Kg = 1 - Kr - Kb; ib = 1 / (2 (1 - Kb)), ir = 1 / (2 (1 - Kr)), ig = 1 / Kg; sy = 1 / 219,
 *             sc = 1 / 224 (full range: both 1 / 255).  All arithmetic is f64, in the written order, without contraction.
 *   To RGB    4:2:0 chroma is upsampled bilinearly, indices clamped to the plane: vertically, and horizontally under CENTER, luma index
 *             2i takes (C[i-1] + 3 C[i]) / 4 and 2i + 1 takes (3 C[i] + C[i+1]) / 4; horizontally under LEFT an even x takes C[x / 2],
 *             an odd x (C[j] + C[j+1]) / 2.  Both axes together are an integer sum of wy wx C over 16, exact.  Then
 *             y = (Y - 16) sy (full: Y sy), cb = (Cb - 128) sc, cr = (Cr - 128) sc;  r = y + (2 (1 - Kr)) cr;  b = y + (2 (1 - Kb)) cb;
 *             g = ((y - Kr r) - Kb b) ig;  each clamped to [0, 1] and rounded once to f32: the network's input.
 *   From RGB  (the network's UNQUANTISED f32 output) each value clamped to [0, 1] in f64 -- any finite magnitude, and the infinities, are
 *             defined; a NaN counts as 0;  y = (Kr r + Kg g) + Kb b;  cb = (b - y) ib;  cr = (r - y) ir;  Y' = 16 + 219 y, C' = 128 + 224 c
 *             (full: 255 y, 128 + 255 c).  4:2:0 chroma is subsampled at this unrounded level, pixel indices clamped to the image (odd
 *             sizes): CENTER ((p00 + p01) + (p10 + p11)) 0.25 over the 2 x 2 block; LEFT per row ((a + 2 b) + c) 0.25 at columns 2j - 1,
 *             2j, 2j + 1, then (row0 + row1) 0.5.  Finally floor(v + 0.5) clamped to the range's limits is the byte: one quantisation.
 * sr_yuv_frame_bytes: the bytes of one frame; 0 for an invalid format or a shape below 1.  Host only.
 * sr_yuv_to_rgb_dev / sr_rgb_to_yuv_dev: n frames of h x w <-> n x h x w x 3 f32, one launch on `stream`, any graph's context.  The f32
 *   pointer must be 4-byte aligned; the frames may start at any byte.
 * sr_upscale_yuv_dev: to RGB into a workspace buffer of the context, exactly sr_upscale_f32_dev's path (members == 1) or
 *   sr_upscale_ensemble_f32_dev's (any other mask) into a second one, and from RGB into d_out: n frames of f h x f w in the same format.
 *   SR_GRAPH_SR_NET (factors 2-4, both precisions) and SR_GRAPH_BILINEAR contexts.  Asynchronous and ordered on `stream` alone.
 * sr_upscale_yuv: the same on host memory, synchronous: one upload, the device call on the context's own stream, one download; in
 *   SR_PRECISION_SPLIT_F16 the whole call is computed again in exact f32 where a value left that mode's domain.
 * Refused with SR_E_INVALID before any launch, the output untouched: a null pointer, an enum outside its values, n, h or w below 1 or a
 * side beyond INT32_MAX / 4, a misaligned f32 pointer; (sr_upscale_yuv*) SR_GRAPH_DOWNSAMPLE contexts, members == 0 or > 255, members
 * != 1 off SR_GRAPH_SR_NET.  A shape whose workspace cannot fit the device is SR_E_NOMEM and leaves the context usable. */
enum sr_yuv_subsampling { SR_YUV_420 = 0, SR_YUV_444 = 1 };
enum sr_yuv_siting { SR_YUV_SITING_CENTER = 0, SR_YUV_SITING_LEFT = 1 };
enum sr_yuv_matrix { SR_YUV_BT601 = 0, SR_YUV_BT709 = 1 };
enum sr_yuv_range { SR_YUV_LIMITED = 0, SR_YUV_FULL = 1 };
typedef struct sr_yuv_format { int32_t subsampling, siting, matrix, range; } sr_yuv_format;
size_t sr_yuv_frame_bytes(const sr_yuv_format* fmt, int h, int w);
int sr_yuv_to_rgb_dev(sr_ctx* ctx, const uint8_t* d_yuv, const sr_yuv_format* fmt, int n, int h, int w, float* d_rgb, void* stream);
int sr_rgb_to_yuv_dev(sr_ctx* ctx, const float* d_rgb, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* d_yuv, void* stream);
int sr_upscale_yuv_dev(sr_ctx* ctx, const uint8_t* d_in, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* d_out, unsigned members,
                       void* stream);
int sr_upscale_yuv(sr_ctx* ctx, const uint8_t* in, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* out, unsigned members);
/* The frame stream: sr_upscale_yuv of one frame after another with the copies of successive frames under the kernels.  A session owns
 * `slots` (1..8) slots, each a page-locked input frame and a device input and output frame, and slots + 1 page-locked output frames.
 *   sr_video_acquire  the input buffer of the next free slot (sr_yuv_frame_bytes(fmt, h, w) bytes) for the caller to fill; SR_E_INVALID
 *                     if every slot is in flight (nothing is disturbed), the same buffer again if one is already acquired.
 *   sr_video_submit   queues the acquired slot and returns at once: the upload on the context's upload stream, the three phases of
 *                     sr_upscale_yuv_dev on its compute stream, the download on its download stream, ordered by the slot's events.
 *   sr_video_receive  waits for the OLDEST submitted frame and gives its f h x f w frame; the pointer is valid until the next receive or
 *                     destroy.  Frames leave in submission order, each byte for byte sr_upscale_yuv's.  SR_E_INVALID with nothing pending.
 *   sr_video_pending  frames submitted and not yet received (-1: a null, detached or failed session).
 * The network's workspace is the context's own, so the kernels of successive frames run one after another on one stream: only the
 * copies overlap them.  slots == 1 is the serial form.  No graph capture, no host thread.
 * SR_PRECISION_SPLIT_F16: the domain word is the context's, so a fault cannot be pinned to a frame.  sr_video_receive looks at it once
 * the frame's download has completed; if it is set, the session's streams are drained, the word is cleared, the CONTEXT IS SWITCHED TO
 * SR_PRECISION_F32 and stays there, and every frame still in flight -- the one being received included -- is queued again from its
 * slot's input buffer, in order.  No clamped frame is ever handed out.
 * While a session has frames in flight the context takes no other call.  sr_destroy of the context drains and detaches its sessions: a
 * detached session refuses every call (SR_E_INVALID) but sr_video_destroy, which the caller still makes; so does a session whose
 * recomputation in exact f32 could not be queued (sr_video_receive returns that status once, and the frames in flight are lost).
 * sr_video_destroy with frames in flight waits for them.  Refusals of sr_video_create: those of sr_upscale_yuv, slots outside 1..8, a null `out`. */
typedef struct sr_video sr_video;
int sr_video_create(sr_ctx* ctx, const sr_yuv_format* fmt, int h, int w, int slots, unsigned members, sr_video** out);
int sr_video_acquire(sr_video* v, uint8_t** in_frame);
int sr_video_submit(sr_video* v);
int sr_video_receive(sr_video* v, const uint8_t** out_frame);
int sr_video_pending(const sr_video* v);
void sr_video_destroy(sr_video* v);
/* Row reuse: compute only the rows that changed since the last frame.  Letterbox bars, held animation cels and screen recordings repeat
 * whole rows byte for byte, and an output row depends on the input rows within SR_HALO of it alone.  With SR_VIDEO_REUSE_ROWS a submitted
 * frame is compared on the device, row by row and plane by plane, with the last submitted frame; the network runs on the row bands whose
 * dependency cone holds a changed row (the band form, bit-identical to the same rows of the undivided call), and every other output row
 * is the last frame's.  EXACT: every frame received is byte for byte what the session gives with the mode off.  Off by default; with
 * it off the session queues what it always queued and owns none of the buffers below.
 *   sr_rows_differ_dev   d_flags[r] = 1 where the row_bytes bytes of row r differ between a and b (rows contiguous, pitch = row_bytes),
 *                        else 0: one launch on `stream`, every flag written exactly once (no clearing needed), no atomics, the same bits
 *                        on every run.  Bytes are compared, so planes of 8- and 16-bit samples are the same call; a and b may start at
 *                        any byte.  SR_E_INVALID before any launch: a null pointer, rows or row_bytes of 0, rows beyond INT32_MAX,
 *                        d_flags not 4-byte aligned.
 *   sr_video_reuse_plan  host only, no device: the LR row bands [y0, y1) a frame computes, from the flags of its Y rows, then its Cb
 *                        rows, then its Cr rows (subsampling: SR_YUV_420 | SR_YUV_444 | SR_YUV_422; h luma rows).  *n_bands == 0: reuse
 *                        the whole last output; one band [0, h): the whole frame.  The rule (tests/reuse_ref.py restates it):
 *                        1. a differing Y row y is RGB-dirty; so is row y for a differing chroma row y (4:4:4, 4:2:2); a differing 4:2:0
 *                           chroma row c dirties rows max(0, 2c - 1) .. min(h - 1, 2c + 2), the rows whose vertical taps read C[c];
 *                        2. needed are the rows within SR_HALO of a dirty row;
 *                        3. bands are the maximal runs of needed rows, each start rounded down and each end rounded up to an even row
 *                           (or h) -- no 2 x 2 block of the 4:2:0 output straddles an edge -- a start below SR_HALO becoming 0 and an end
 *                           within SR_HALO of h becoming h (SR_E_HALO's rule); bands fewer than 2 SR_HALO rows apart are merged (what a
 *                           separate band recomputes as margin), top to bottom; above SR_REUSE_MAX_BANDS the two with the smallest gap
 *                           are merged, of equal gaps the pair nearer the top, until that many remain;
 *                        4. if the bands' rows plus 2 SR_HALO a band reach h, the plan is the whole frame.
 *                        SR_E_INVALID: a null pointer, h < 1, another subsampling, max_bands below the plan's count (SR_REUSE_MAX_BANDS
 *                        always suffices).
 *   sr_video_set_reuse   SR_VIDEO_REUSE_OFF | SR_VIDEO_REUSE_ROWS, only while nothing is pending (else, and for another mode,
 *                        SR_E_INVALID); the next frame is computed whole.  Turning it on allocates the session's reuse buffers (a device
 *                        copy of the last input frame, a band-sized output frame, the flags) and the context's workspace for the whole
 *                        frame: nothing is allocated per frame.  Turning it off frees the session's reuse buffers again (the context's
 *                        workspaces stay, as after any call).
 *   With the mode on sr_video_submit queues the compare, the copy of the frame to the reference and the flags' download behind the
 *   upload on the upload stream, and WAITS for them -- the one new host wait.  (Measured: the upload stream's work reaches the device
 *   only once the previous frame's kernels have left it, so the wait lasts about a frame period and a clip with nothing to reuse runs
 *   as with one slot)  Then, on the compute stream: the clean row ranges of every plane from the previous frame's slot (one slot: they are in
 *   place), the existing conversion of the whole frame to RGB, and per band the conv stack, the existing conversion of its f (y1 - y0)
 *   rows from RGB, and three row-range copies into the slot's planes.  The download is the whole frame.  Whole-or-nothing: members != 1,
 *   SR_GRAPH_BILINEAR, a session's first frame and the first after sr_video_set_reuse reuse the whole frame if no row differs and are
 *   otherwise computed exactly as with the mode off.  Frames queued again in exact f32 (above) are computed whole; the frame after them
 *   reuses rows again, now of f32 outputs.  A refused submit makes the next frame whole; so do sr_set_precision, sr_set_params
 *   and a change of the kernel form (srhip_experimental.h "wino") between two frames: rows are reused only from an output computed
 *   under the context's present precision, parameters and kernel form.
 *   sr_video_get_reuse_stats  counts since the session was made: frames submitted with the mode on = frames_reused (no launch of the
 *                        network) + frames_partial + frames_full; rows_total = h per such frame, rows_computed = the LR rows the
 *                        network produced (halo rows not counted), bands = band passes (a whole frame counts as none).  Frames queued
 *                        again in exact f32 are not counted a second time. */
#define SR_REUSE_MAX_BANDS 4
enum { SR_VIDEO_REUSE_OFF = 0, SR_VIDEO_REUSE_ROWS = 1 };
typedef struct sr_row_band { int32_t y0, y1; } sr_row_band;   /* LR rows [y0, y1) to compute */
typedef struct sr_video_reuse_stats {
    uint64_t frames, frames_reused, frames_partial, frames_full, rows_total, rows_computed, bands;
} sr_video_reuse_stats;
int sr_rows_differ_dev(sr_ctx* ctx, const void* d_a, const void* d_b, size_t rows, size_t row_bytes, uint32_t* d_flags, void* stream);
int sr_video_reuse_plan(const uint32_t* plane_flags, int subsampling, int h, sr_row_band* bands, int max_bands, int* n_bands);
int sr_video_set_reuse(sr_video* v, int mode);
int sr_video_get_reuse_stats(const sr_video* v, sr_video_reuse_stats* out);

/* ---- Deep video: planar YCbCr frames of 9..16-bit samples, 4:2:0, 4:2:2 and 4:4:4 ----
 * What `ffmpeg -f yuv4mpegpipe` writes for HEVC, AV1 and ProRes sources (C420p10, C422p10, ...): the Video calls above on frames whose
 * samples are little-endian uint16, with a format struct of their own -- sr_yuv_format and its validation are unchanged, and the two
 * enum values added here are valid in sr_yuv16_format only.  A frame is Y (h x w), then Cb, then Cr, each ch x cw samples: SR_YUV_420
 * ceil(h / 2) x ceil(w / 2), SR_YUV_422 h x ceil(w / 2), SR_YUV_444 h x w; contiguous, so a plane may start at any even byte.
 * UNPINNED: tests/yuv16_ref.py states the rule in numpy (f64) and the kernels equal it bit for bit.  It is the 8-bit rule at depth d:
 *   a code is the uint16 as stored, whatever d says -- nothing is masked; the clamp of RGB to [0, 1] defines every input.
 *   Constants, each formed once by a single f64 operation, s = 2^(d - 8).  SR_YUV_LIMITED: oy = 16 s, ky = 219 s, kc = 224 s, mid = 128 s,
 *             limits Y [16 s, 235 s], C [16 s, 240 s].  SR_YUV_FULL: oy = 0, ky = kc = 2^d - 1, mid = 2^(d - 1), limits [0, 2^d - 1].
 *             sy = 1 / ky, sc = 1 / kc; the matrix constants as above, with SR_YUV_BT2020 (non-constant luminance) Kr 0.2627, Kb 0.0593.
 *   To RGB    y = (Y - oy) sy, c = (C - mid) sc, then as above.  4:2:0 chroma: the same exact integer sum over 16, times 0.0625.
 *             4:2:2 chroma: the horizontal taps alone -- an exact integer sum over 4, times 0.25 -- and no vertical tap.
 *   From RGB  as above with Y' = oy + ky y, C' = mid + kc c.  4:2:2 subsampling, at the unrounded level: CENTER (p0 + p1) 0.5; LEFT
 *             ((a + 2 b) + c) 0.25 at columns 2j - 1, 2j, 2j + 1, indices clamped.  Then floor(v + 0.5) clamped to the limits: one uint16.
 *   In limited range the rule on code 2^(d - 8) gives the 8-bit rule's f32 RGB bit for bit: the scale is a power of two.
 * sr_yuv16_frame_bytes: the BYTES of one frame (two a sample); 0 for an invalid format or a shape below 1.  Host only.
 * sr_yuv16_to_rgb_dev / sr_rgb_to_yuv16_dev / sr_upscale_yuv16_dev / sr_upscale_yuv16: as their 8-bit namesakes.  The composed call is
 *   bit-identical to its three device calls chained, the network in between being exactly sr_upscale_f32_dev's or
 *   sr_upscale_ensemble_f32_dev's path.
 * sr_video_create16: a frame stream (above) on deep frames; acquire / submit / receive / pending / destroy are the same calls, the
 *   buffers are bytes (sr_yuv16_frame_bytes of them), and every rule of the 8-bit session holds, the recomputation in exact f32 included.
 * Refused with SR_E_INVALID before any launch, the output untouched: what the 8-bit calls refuse, a depth outside 9..16, a frame pointer
 * that is not 2-byte aligned.  A shape that cannot fit is SR_E_NOMEM. */
enum { SR_YUV_422 = 2 };    /* a subsampling; valid in sr_yuv16_format only */
enum { SR_YUV_BT2020 = 2 }; /* a matrix; valid in sr_yuv16_format only */
typedef struct sr_yuv16_format { int32_t subsampling, siting, matrix, range, depth; } sr_yuv16_format;
size_t sr_yuv16_frame_bytes(const sr_yuv16_format* fmt, int h, int w);
int sr_yuv16_to_rgb_dev(sr_ctx* ctx, const uint16_t* d_yuv, const sr_yuv16_format* fmt, int n, int h, int w, float* d_rgb, void* stream);
int sr_rgb_to_yuv16_dev(sr_ctx* ctx, const float* d_rgb, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* d_yuv, void* stream);
int sr_upscale_yuv16_dev(sr_ctx* ctx, const uint16_t* d_in, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* d_out,
                         unsigned members, void* stream);
int sr_upscale_yuv16(sr_ctx* ctx, const uint16_t* in, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* out, unsigned members);
int sr_video_create16(sr_ctx* ctx, const sr_yuv16_format* fmt, int h, int w, int slots, unsigned members, sr_video** out);

/* ---- Video at any size: the network's frames resampled on the device, quantised once ----
 * `video` writes frames of the weights' factor times the input; what is asked of a video upscaler is 1080p -> 2160p, 720p -> 1080p.  As
 * the image path does ("Resampling to any size"), these calls resample the network's UNQUANTISED f32 output on the device and quantise
 * once, at the final size -- straight to a planar frame of the Video / Deep video formats: the vertical pass of the resampling ends in
 * the YCbCr conversion (one kernel, no oh x ow x 3 f32 image in between, for the format classes on which that is not slower than the
 * two kernels it stands for; the others run those two: the bytes are the same).  All of them are host calls or session calls: host
 * memory, synchronous, none takes a stream.  Every result is defined BIT FOR BIT by the chain of existing device calls:
 *   sr_resize_to_yuv[16]       n f32 RGB images of h x w (any graph's context) -> n frames of oh x ow luma samples in `fmt`: equal to
 *                              sr_resize_dev (SR_PIXELS_F32 -> SR_PIXELS_F32, same filter and flags) followed by sr_rgb_to_yuv[16]_dev.
 *                              One upload, the tap tables, the horizontal pass, the vertical pass to the frame, one download.
 *   sr_upscale_yuv[16]_sized   n frames of h x w -> n frames of oh x ow in the same format: equal to sr_yuv[16]_to_rgb_dev ->
 *                              sr_upscale_f32_dev (members == 1) or sr_upscale_ensemble_f32_dev frame by frame -> sr_resize_dev (f32 ->
 *                              f32) -> sr_rgb_to_yuv[16]_dev.  In SR_PRECISION_SPLIT_F16 a value that leaves the domain makes the whole
 *                              call run again in exact f32, as sr_upscale_yuv does (the context stays in f32).  With sr_set_profiling on,
 *                              sr_last_timing's total_ms is every launch, h2d_ms / d2h_ms the two copies.
 *   sr_video_create[16]_sized  a frame stream (sr_video_create) whose output frames are oh x ow: acquire / submit / receive / pending /
 *                              destroy are the same calls; the slots' output buffers and the page-locked output frames hold
 *                              sr_yuv[16]_frame_bytes(fmt, oh, ow); nothing is allocated per frame -- the workspace is reserved, all or
 *                              nothing, when the session is made; the recomputation in exact f32 works as in the plain session.  Each
 *                              frame is bit-identical to sr_upscale_yuv[16]_sized of it.  sr_video_set_reuse(SR_VIDEO_REUSE_ROWS) on
 *                              such a session is SR_E_INVALID: the row bands do not compose with a vertical resampling.
 * filter: SR_FILTER_*; flags: 0 or SR_RESIZE_SRGB_SPACE.  Refused with SR_E_INVALID before any launch, the output untouched: what
 * sr_upscale_yuv* / sr_video_create* refuse for format, shape, mask and graph (sr_resize_to_yuv*: a null pointer, a misaligned frame
 * pointer, an invalid format, n, h or w below 1); what sr_resize_dev refuses for oh, ow, filter, flags and byte counts beyond a size_t;
 * oh or ow beyond INT32_MAX / 4.  A workspace that cannot fit is SR_E_NOMEM and leaves the context usable. */
int sr_resize_to_yuv(sr_ctx* ctx, const float* rgb, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* out, int oh, int ow, int filter,
                     unsigned flags);
int sr_resize_to_yuv16(sr_ctx* ctx, const float* rgb, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* out, int oh, int ow,
                       int filter, unsigned flags);
int sr_upscale_yuv_sized(sr_ctx* ctx, const uint8_t* in, const sr_yuv_format* fmt, int n, int h, int w, uint8_t* out, int oh, int ow,
                         int filter, unsigned flags, unsigned members);
int sr_upscale_yuv16_sized(sr_ctx* ctx, const uint16_t* in, const sr_yuv16_format* fmt, int n, int h, int w, uint16_t* out, int oh, int ow,
                           int filter, unsigned flags, unsigned members);
int sr_video_create_sized(sr_ctx* ctx, const sr_yuv_format* fmt, int h, int w, int oh, int ow, int filter, unsigned flags, int slots,
                          unsigned members, sr_video** out);
int sr_video_create16_sized(sr_ctx* ctx, const sr_yuv16_format* fmt, int h, int w, int oh, int ow, int filter, unsigned flags, int slots,
                            unsigned members, sr_video** out);

/* ---- Deep colour: 16-bit images in and out ----
 * The reference's images are 8 bits wide (main.rs:164-175), and so is every other integer path here; a 16-bit scan, photograph, height
 * or displacement map would come back with 256 levels a channel.  These calls take and give interleaved 16-bit samples -- native-endian
 * uint16_t, rows and images contiguous -- and quantise the network's f32 output once, to 65536 levels.  UNPINNED: the reference has no
 * counterpart; tests/deep_ref.py states the rule in numpy and the kernels equal it bit for bit.  The rule acts on one pixel at a time:
 * the images of a batch do not see each other and the shape does not enter.
 *   In    x = (float)v / 65535.0f, one correctly rounded IEEE f32 division.  in_channels 1 (grey, copied to R = G = B), 2 (grey + alpha),
 *         3 or 4; alpha is dropped, as sr_upscale_rgba8 drops it.  The result is the network's input, n x h x w x 3 f32.
 *         (float)(257 b) / 65535.0f == (float)b / 255.0f for every byte b: an 8-bit image promoted to 16 bits feeds the network exactly
 *         what the 8-bit path feeds it.
 *   Out   q(v) = (uint16_t) fminf(fmaxf(floorf(65535.0f v + 0.5f), 0.0f), 65535.0f), the product and the sum each rounded to f32 (no
 *         contraction); a NaN gives 0, by fmaxf.  q((float)k / 65535.0f) == k for all 65536 levels.  out_channels 3 writes RGB16, 4
 *         RGBA16 with alpha 65535, 1 grey: q(((r + g) + b) / 3.0f), the sum and the quotient in f32.  2 is refused.
 * sr_u16_to_f32_dev / sr_f32_to_u16_dev: n images of h x w, one launch on `stream`, any graph's context; asynchronous and ordered on
 *   `stream` alone.  A u16 pointer must be 2-byte aligned, an f32 pointer 4-byte aligned; a side whose pointer is 16-byte aligned is
 *   read or written 16 bytes at a time.  d_in == d_out is refused.
 * sr_upscale_u16_dev: to f32 into a workspace buffer of the context (grown on first use, freed by sr_destroy), exactly
 *   sr_upscale_f32_dev's path (members == 1) or sr_upscale_ensemble_f32_dev's (any other mask) into a second one, and to 16 bits into
 *   d_out: n images of f h x f w.  Every graph those f32 calls take: SR_GRAPH_SR_NET (factors 2-4, both precisions), SR_GRAPH_BILINEAR
 *   and, with members == 1, SR_GRAPH_DOWNSAMPLE (h / 3 x w / 3 out: 16-bit images are pooled in linear light too).
 * sr_upscale_u16: the same on host memory, synchronous: one upload, the device call on the context's own stream, one download; in
 *   SR_PRECISION_SPLIT_F16 the whole call is computed again in exact f32 where a value left that mode's domain.  With sr_set_profiling
 *   on, sr_last_timing's total_ms is every launch of the call, h2d / d2h the two copies.
 * sr_upscale_u16_border[_dev]: the same two conversions around sr_upscale_f32_border_dev (mode, pad, members as there).
 * sr_upscale_u16_sized[_dev]: ... around the network's f32 call followed by sr_resize_dev from SR_PIXELS_F32 to SR_PIXELS_F32 (oh, ow,
 *   filter, flags as in sr_upscale_rgba8_sized): n images of oh x ow.  Their graph and mask refusals are those of the 8-bit calls.
 * Refused with SR_E_INVALID before any launch, the output untouched and the context usable: a null pointer; in_channels outside 1..4;
 * out_channels not 1, 3 or 4; n, h or w below 1 (SR_GRAPH_DOWNSAMPLE: h or w below 3); byte counts that overflow; a u16 pointer at an
 * odd address; an f32 pointer that is not 4-byte aligned; members == 0 or > 255; members != 1 on a context other than SR_GRAPH_SR_NET;
 * the refusals of the border and sized calls for their own arguments.  A workspace that does not fit the device is SR_E_NOMEM and
 * leaves the context usable and the output untouched: the call's own three buffers are refused before any launch, the border or
 * resampling phase's behind the first conversion, which writes the context's workspace only.  Transparency at 16 bits, and the multi-GPU, band and sharded forms, do not exist.  Cost:
 * DESIGN.md 4r. */
int sr_u16_to_f32_dev(sr_ctx* ctx, const uint16_t* d_in, int in_channels, int n, int h, int w, float* d_out, void* stream);
int sr_f32_to_u16_dev(sr_ctx* ctx, const float* d_in, int n, int h, int w, uint16_t* d_out, int out_channels, void* stream);
int sr_upscale_u16_dev(sr_ctx* ctx, const uint16_t* d_in, int in_channels, int n, int h, int w, uint16_t* d_out, int out_channels,
                       unsigned members, void* stream);
int sr_upscale_u16(sr_ctx* ctx, const uint16_t* in, int in_channels, int n, int h, int w, uint16_t* out, int out_channels,
                   unsigned members);
int sr_upscale_u16_border_dev(sr_ctx* ctx, const uint16_t* d_in, int in_channels, int n, int h, int w, uint16_t* d_out, int out_channels,
                              int mode, int pad, unsigned members, void* stream);
int sr_upscale_u16_border(sr_ctx* ctx, const uint16_t* in, int in_channels, int n, int h, int w, uint16_t* out, int out_channels,
                          int mode, int pad, unsigned members);
int sr_upscale_u16_sized_dev(sr_ctx* ctx, const uint16_t* d_in, int in_channels, int n, int h, int w, uint16_t* d_out, int out_channels,
                             int oh, int ow, int filter, unsigned flags, unsigned members, void* stream);
int sr_upscale_u16_sized(sr_ctx* ctx, const uint16_t* in, int in_channels, int n, int h, int w, uint16_t* out, int out_channels,
                         int oh, int ow, int filter, unsigned flags, unsigned members);

/* ---- The training objective: squared, L1 or Charbonnier ----
 * The reference trains a sum of squares (network.rs:78-103), and that is the default.  UNPINNED: the other two kinds have no counterpart
 * there; tests/loss_ref.py states them in torch f64 and the tests hold the GPU to it.  With e exactly as in "Backpropagation" above
 * (out - hr, or SrgbToLinear(out) - SrgbToLinear(hr) under linear_loss) the loss is loss_scale * sum rho(e) + l2 * sum p^2:
 *   SR_LOSS_MSE          rho(e) = e^2                          rho'(e) = 2 e: the kernels and the bits of a context that never called this
 *   SR_LOSS_L1           rho(e) = |e|                          rho'(e) = -1, 0 or +1, 0 at e == 0 (the subgradient torch's abs takes)
 *   SR_LOSS_CHARBONNIER  rho(e) = sqrt(e^2 + eps^2) - eps      rho'(e) = e / sqrt(e^2 + eps^2), in f32 with a correctly rounded square
 *                        root and division (no approximate reciprocal): the same bits on every run, context and device
 * sr_set_loss: state of the context, like sr_set_precision; a host-side field and no device work.  Every backward pass queued on the
 *   context afterwards uses it: sr_backprop_* and sr_pair_backprop_* (host and _dev forms) and every step of a training session on the
 *   context (sr_train_step, _aug, _pairs, _pairs_aug, _degrade).  A pass uses the value in force when it was QUEUED: its kernel
 *   arguments are captured then, so changing the objective while earlier steps are in flight neither waits for them nor touches them.
 *   eps is read for SR_LOSS_CHARBONNIER alone (any value passes with the other kinds, and sr_get_loss then keeps reporting the last eps
 *   that was set; 1e-3 on a fresh context).
 * err_sum stays the sum of e^2 under every kind: the PSNR lines and sr_train_sync stay comparable between runs of different objectives.
 *   The value of sum rho(e) is not returned.  sr_validation_error_*, the metrics calls and inference do not look at the objective.
 * Refused, the state unchanged: a null ctx (SR_E_INVALID; SR_E_NO_DEVICE without a device, like the other training entry points); a
 * context that is not SR_GRAPH_SR_NET, a kind outside the three, and for SR_LOSS_CHARBONNIER an eps that is NaN, infinite, <= 0 or > 1
 * (SR_E_INVALID); sr_get_loss: a null ctx likewise, a context that is not SR_GRAPH_SR_NET.  kind / eps of sr_get_loss may be null.  Cost: DESIGN.md 4s. */
enum sr_loss { SR_LOSS_MSE = 0, SR_LOSS_L1 = 1, SR_LOSS_CHARBONNIER = 2 };
int sr_set_loss(sr_ctx* ctx, int kind, float eps);
int sr_get_loss(sr_ctx* ctx, int* kind, float* eps);

/* ---- Optimiser: learning-rate schedules, gradient clipping, averaged parameters, exact resume ----
 * What a long run needs beyond the reference's fixed Adam (main.rs:199-205).  UNPINNED: the reference has no counterpart; tests/optim_ref.py
 * restates every rule in numpy and the tests hold the GPU to it bit for bit.  All of it is off by default: a session that never calls
 * sr_train_set_optim / sr_train_set_lr queues the launches and computes the bits it did before these entry points existed.
 *
 * sr_grad_norm_dev: S = sum (double)g (double)g over the n floats of d_grad (4-byte aligned), each square exact in f64, in an order of
 *   additions that depends on n alone: partial b = the workgroup sum (the butterfly v + v[i ^ off], off = 32 .. 1, over each 64 lanes,
 *   then ((w0 + w1) + w2) + w3) of elements 256 b .. 256 b + 255 (0.0 past n); a lane t of one workgroup then adds partials t, t + 256,
 *   ... in order and the same workgroup sum gives S.  No atomics: the same bits on every run and device.  From S, on the device:
 *     sumsq = S;  norm = sqrt(S) in f64;  scale = clip > 0 && norm > clip ? (float)((double)clip / norm) : 1.0f;
 *     skip  = S is not finite -- exactly when some element of d_grad is NaN or infinite (every square is >= 0).
 *   d_out (8-byte aligned) receives the struct.  clip = 0: no clipping (scale 1.0f), sumsq and skip still computed.  Two launches on
 *   `stream`, no host synchronisation; the partials live in ONE buffer of the context (grown when a call needs more, the earlier one
 *   freed), so calls on one context are the caller's to order -- ACROSS STREAMS TOO: `stream` says where this call's launches go, it does
 *   not give the call partials of its own.  Two calls on different streams of one context, neither ordered after the other's launches
 *   (an event, a synchronisation), race on the partials and may free them under each other; use one stream, or order them, or a context
 *   each.  Works in any graph's context.
 * sr_adam_step_clipped_dev: sr_adam_step_dev's arithmetic, in its written order, on gc = scale g (one f32 product), scale and skip read
 *   from d_norm in device memory (NULL: scale 1.0f, never skipped).  With scale == 1.0f the p, m, v written are sr_adam_step_dev's bits.
 *   d_ema (NULL: off, and ema_decay must then be 0): e <- ema_decay e + (1.0f - ema_decay) p' in f32, p' the parameter just written,
 *   1.0f - ema_decay formed once on the host.  A skipped step (skip != 0) writes nothing to p, m, v or e and adds 1 to *d_skipped
 *   (8-byte aligned, may be NULL).  The caller's step count -- and with it the bias correction 1 - beta^step -- still advances over a
 *   skipped step: the moments simply miss one update.  16 bytes a lane where all the pointers are 16-byte aligned, dwords otherwise;
 *   the bits do not depend on which.  One launch on `stream`.
 * sr_lr_at: the learning rate of step t = 1, 2, ..., host only, no device needed; everything in double, rounded once to f32:
 *     warm = warmup ? min(1, t / warmup) : 1
 *     SR_LR_CONSTANT  base
 *     SR_LR_STEP      base gamma^floor((t - 1) / every)                                      every >= 1, 0 < gamma <= 1
 *     SR_LR_COSINE    min_lr + (base - min_lr) 0.5 (1 + cos(pi min(t - 1, total) / total))   total >= 1, 0 <= min_lr <= base
 *     *lr = (float)(warm * that value)
 *   pow and cos are the host libm's: two hosts may differ in the last bit of the f32.  Fields a kind does not use are not read.
 * The session:
 *   sr_train_set_optim(t, clip_norm, ema_decay): clip_norm 0 (off) or finite and > 0; ema_decay 0 (off) or strictly inside (0, 1).  Waits
 *     for the steps in flight.  The EMA slice is allocated when first enabled and initialised from the parameters as they are then;
 *     turned off and on again it is initialised anew.  With either on, a step is the gather, the backward pass, sr_grad_norm_dev (only
 *     with clip_norm > 0) and sr_adam_step_clipped_dev; with both off it is the step of sr_train_step, by the same launches.
 *   sr_train_set_lr(t, lr): the rate of the steps queued afterwards (finite, >= 0); no synchronisation, steps in flight keep theirs.
 *   sr_train_ema(t, out, cap): waits; the averaged parameters (cap >= n_params).  SR_E_INVALID while the EMA is off.
 *   sr_train_get_state / sr_train_set_state: what a run needs besides the parameters to continue bit for bit: m, v, e (NULL / ignored
 *     while the EMA is off; required while it is on), the step count (= steps queued so far) and the skipped count.  Both wait for the
 *     steps in flight.  The parameters themselves travel through sr_train_params and sr_train_create.  set_state refuses n != n_params, a
 *     negative step or skipped count, a null m or v, and a null e while the EMA is on (SR_E_INVALID), and then leaves the session as it was.
 *   sr_train_sync_stats: sr_train_sync with {err_sum, grad_norm, lr, scale} per step; grad_norm = sqrt(sumsq) (NaN or inf on a skipped
 *     step), 0 with scale 1 while clipping is off.  It shares sr_train_sync's queue: a step is reported by whichever is called first.
 * Refused with SR_E_INVALID before any launch, outputs untouched: nulls (but where noted), misaligned pointers, n == 0, step < 1, a clip,
 * decay, lr or schedule field out of range, d_ema without ema_decay or the reverse, a session whose context is gone.  A null context or
 * session with no device present is SR_E_NO_DEVICE, as for sr_adam_step_dev (sr_lr_at: SR_E_INVALID, it needs none).  Cost: DESIGN.md 4t. */
typedef struct {
    double sumsq;   /* S */
    float scale;    /* what the update multiplies the gradient by */
    int32_t skip;   /* 1: S is not finite */
} sr_grad_norm;
typedef struct {
    double err_sum, grad_norm;
    float lr, scale;
} sr_train_stat;
enum sr_lr_kind { SR_LR_CONSTANT = 0, SR_LR_STEP = 1, SR_LR_COSINE = 2 };
typedef struct {
    int kind;            /* SR_LR_* */
    float base;          /* finite, >= 0 */
    long long warmup;    /* N steps of linear warm-up, 0: none */
    long long every;     /* SR_LR_STEP */
    double gamma;        /* SR_LR_STEP */
    long long total;     /* SR_LR_COSINE */
    float min_lr;        /* SR_LR_COSINE */
} sr_lr_schedule;
int sr_grad_norm_dev(sr_ctx* ctx, const float* d_grad, size_t n, float clip, sr_grad_norm* d_out, void* stream);
int sr_adam_step_clipped_dev(sr_ctx* ctx, float* d_params, float* d_m, float* d_v, const float* d_grad, size_t n, int step, float lr,
                             float beta1, float beta2, float eps, const sr_grad_norm* d_norm, float* d_ema, float ema_decay,
                             unsigned long long* d_skipped, void* stream);
int sr_lr_at(const sr_lr_schedule* schedule, long long step, float* lr);
int sr_train_set_optim(sr_train* t, float clip_norm, float ema_decay);
int sr_train_set_lr(sr_train* t, float lr);
int sr_train_ema(sr_train* t, float* out, size_t cap);
int sr_train_get_state(sr_train* t, float* m, float* v, float* e, size_t cap, long long* step, long long* skipped);
int sr_train_set_state(sr_train* t, const float* m, const float* v, const float* e, size_t n, long long step, long long skipped);
int sr_train_sync_stats(sr_train* t, sr_train_stat* stats, size_t cap, size_t* n_steps);

/* Device time of the most recent call, measured with HIP events on the stream
 * the kernels ran on.  stage_ms[5] = conv0, l1, l2, l3, expand stage kernels
 * (enable with sr_set_profiling; off by default -- it inserts events, and the host-pointer
 * entry points then run undivided).  After a pipelined host call total = first kernel start to last
 * kernel end (chunks overlap on two compute streams), h2d / d2h = sums over the chunks, and
 * sr_read_feature refuses (the maps hold the last chunks only).
 * h2d / d2h are zero for the *_dev entry points. */
int sr_set_profiling(sr_ctx* ctx, int enabled);
int sr_last_timing(sr_ctx* ctx, double* total_ms, double stage_ms[5], double* h2d_ms,
                   double* d2h_ms);

/* Device facts for reports: name (e.g. "gfx950..."), CU count, clock MHz. */
int sr_device_info(sr_ctx* ctx, char* name, size_t cap, int* compute_units, int* clock_mhz);

int sr_last_hip_error(sr_ctx* ctx);
const char* sr_strerror(int status);

#ifdef __cplusplus
}
#endif
#endif /* SRHIP_H */
