/*
 * include/dss_hip.h -- C ABI of libdss_hip.so, the MI355X (gfx950) hot path of
 * cronelab/delayed-speech-synthesis: LPCNet vocoder + high-gamma (HGA) feature extractor.
 *
 * Plain C, plain pointers and sizes; no torch / C++ types.  Every entry point names the reference
 * interface it replaces (file:line relative to the reference repository).
 *
 * Part 1 exports every xiph/LPCNet symbol the reference's Cython wrapper binds (extensions/lpcnet/cLPCNet.pxd:10-19):
 * the four decoder entry points are implemented, the five feature-ENCODER entry points (corpus preparation, outside
 * the accelerated path) are present and fail cleanly (create returns NULL -> the wrapper's MemoryError,
 * LPCNet.pyx:53-56).  The reference's own LPCNet.pyx therefore compiles and links against this library with the two
 * shim headers under include/compat/ (tests/test_cpu_boundary.py does exactly that; INTEGRATION.md shows the recipe).
 * Part 2 is the batched form of the same operator (what AsynchronousSynthesisQueue's process pool,
 * local/training.py:165-207, and the north-star batch configs need).
 * Part 3 is the HGA operator (extensions/hga/hga_optimized.pyx and HighGammaExtractor,
 * local/units.py:97-161).
 * Parts 4-6 are the speech gate and the two recurrent models of the online path, Part 7 the acoustic labels of a
 * training corpus, Part 8 the two recurrent models over the trials of such a corpus (the validation passes of the
 * reference's training scripts), Part 9 the training of the neural detector, Part 10 that of the decoder, Part 11 the
 * spectrograms behind the reference's spectral analyses, Part 13 several decoders trained side by side, Part 14 the trainers'
 * dropout masks drawn on the device, Part 15 several detectors trained side by side, Part 16 the LPC feature encoder behind a
 * training corpus' `lpc_coefficients`, Part 17 the models of a group of trainers over one trial list, Part 18 that encoder on streams
 * with its state carried between pushes, each described at its declarations.
 *
 * Error convention: functions returning int return 0 on success and a negative DSS_E* code on failure;
 * dss_last_error() gives a thread-local message.  Creators return NULL on failure (the reference's
 * wrapper turns NULL into MemoryError, LPCNet.pyx:16-17).  There is NO CPU fallback: without a HIP
 * device every compute entry point fails with DSS_ENODEV.
 *
 * Threading (same contract as the reference): one state is used by one thread at a time;
 * different states may be used from different threads.  Do not fork() after the first call.
 */
#ifndef DSS_HIP_H
#define DSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSS_OK        0
#define DSS_EINVAL   -1   /* bad argument / shape */
#define DSS_ENODEV   -2   /* no HIP device, or HIP runtime error (see dss_last_error) */
#define DSS_ENOMODEL -3   /* no LPCNet weight blob loaded */
#define DSS_ENOMEM   -4

const char *dss_last_error(void);
/* Library version and the device it runs on ("gfx950 ..."); never NULL. */
const char *dss_version(void);
int dss_device_count(void);
/* Select the HIP device used by objects created afterwards on this thread (default 0 / LOCAL_RANK). */
int dss_set_device(int device);
/* The device objects created next on this thread will live on (>= 0), or DSS_ENODEV.  Every object keeps the device
 * it was created on and runs its kernels there; device pointers handed to *_dev entry points must belong to it. */
int dss_current_device(void);

/* ------------------------------------------------------------------------------------------------
 * Part 0 -- streams, events and page-locked host memory as plain handles, for hosts that keep several calls of this
 * library in flight at once (the asynchronous segment synthesis of the gated streaming mode) without binding a HIP
 * runtime themselves.  A stream handle is what every *_dev entry point takes as `hip_stream` (a hipStream_t); streams
 * created here do not synchronise with the null stream.  Nothing in the reference corresponds to these: its one stream
 * blocks while it vocodes (local/units.py:531-538).
 * ---------------------------------------------------------------------------------------------- */
void *dss_stream_create(void);
void dss_stream_destroy(void *hip_stream);
int dss_stream_synchronize(void *hip_stream);
void *dss_event_create(void);
void dss_event_destroy(void *event);
int dss_event_record(void *event, void *hip_stream);
int dss_event_query(void *event);                 /* 1 = finished, 0 = not yet, < 0 = error */
int dss_event_synchronize(void *event);
int dss_stream_wait_event(void *hip_stream, void *event);
/* Page-locked host memory (results that arrive by asynchronous copy).  cached != 0: ordinary cacheable pages
 * (hipHostMallocNonCoherent), valid to read once an event from dss_event_create, recorded on the copy's stream behind the copy,
 * has completed (dss_event_query == 1 or dss_event_synchronize), or after dss_stream_synchronize on that stream.  Events from
 * dss_event_create carry hipEventReleaseToSystem, which is what HIP requires for device stores into such pages to be visible
 * to the host at the event; a host that brings events of its own must create them with that flag.  0: coherent pages. */
void *dss_host_alloc(size_t bytes, int cached);
void dss_host_free(void *p);
/* Device -> page-locked host memory (from dss_host_alloc), ordered on hip_stream; both pointers 16-byte aligned.  Runs as a
 * small kernel that stores into the mapped host pages, NOT as a DMA copy: a DMA copy queued behind a long kernel holds up
 * every other copy of the process (the tick's packet upload) until that kernel has finished.  A null or misaligned pointer
 * or a destination that is not page-locked gives DSS_EINVAL; nothing is enqueued and the HIP runtime's last error stays clear. */
int dss_memcpy_d2h_async(void *host_dst, const void *d_src, size_t bytes, void *hip_stream);
/* Explicitly coherent (fine-grained) page-locked memory (hipHostMallocCoherent): the device's stores reach it while a kernel
 * is still running.  The only memory dss_lpcnet_batch_synthesize_ragged_progress_dev accepts.  Freed with dss_host_free. */
void *dss_host_alloc_fine(size_t bytes);
/* Reads n counters of a progressive call (host_frames_done) with acquire loads: once out[i] = v, the first v*160 samples of
 * row i are in host_pcm.  For C hosts that do not want to reason about the memory model themselves. */
int dss_progress_read(const int *host_frames_done, int n, int *out);

/* ------------------------------------------------------------------------------------------------
 * Part 1 -- xiph LPCNet decoder symbols, as bound by extensions/lpcnet/cLPCNet.pxd:10-13
 * ---------------------------------------------------------------------------------------------- */
typedef struct LPCNetState LPCNetState;

/* cLPCNet.pxd:10.  Allocates one decoder state (device resident) bound to the process-wide model.
 * The model is the blob given to dss_lpcnet_load_model*, else the file named by $DSS_LPCNET_WEIGHTS.
 * NULL if neither exists or no device is available. */
LPCNetState *lpcnet_create(void);
/* cLPCNet.pxd:11.  Zeroes the state, last_exc = ulaw(0), RNG re-seeded with "LPCNet". Returns 0. */
int lpcnet_init(LPCNetState *st);
/* cLPCNet.pxd:12 */
void lpcnet_destroy(LPCNetState *st);
/* cLPCNet.pxd:13.  One 10 ms frame: features[0..19] (host) -> output[0..N-1] (host), N must be 160
 * (LPCNet.pyx:10,39).  Runs the frame-rate network once, then N autoregressive sample steps. */
void lpcnet_synthesize(LPCNetState *st, const float *features, short *output, int N);
/* xiph lpcnet.h: size of the opaque state (reported for completeness; states live on the device). */
int lpcnet_get_size(void);
/* lpcnet_synthesize has no error channel (void).  It never aborts the process: on failure (N != 160, HIP error,
 * NULL argument) the frame is zero-filled, the reason is left in dss_last_error(), and this process-wide counter is
 * incremented (first failure and every 1000th are also printed to stderr). */
long dss_error_count(void);

/* cLPCNet.pxd:15-19 -- feature encoder (prepare_corpus.py:72-73 drives it 160 samples at a time on one state).  Bound to the
 * encoder of Parts 16 and 18 ONLY where the environment holds DSS_LPCNET_ENCODER=1 when lpcnet_encoder_create() is called: that
 * encoder is this project's statement of the published method, its parity with xiph's code is unpinned, and it must not stand
 * in for xiph's silently (the decoder likewise refuses to run without named weights).
 *   Without the opt-in: create returns NULL with "encoder" in dss_last_error() (the reference's LPCFeatureEncoder.__cinit__
 * raises MemoryError, LPCNet.pyx:53-56), the others return -1 and zero their output.
 *   With it: create returns a state that wraps a one-stream handle of Part 18 (NULL, "encoder" in the message, when no device
 * is usable); lpcnet_encoder_init resets it and returns 0; lpcnet_compute_single_frame_features pushes pcm[160] and writes 36
 * floats, returning 0, or on failure -1 with the features zeroed and dss_error_count() incremented; the state carries from call
 * to call, so a 160-sample loop gives the bits of Part 16 on the whole signal.
 *   lpcnet_compute_features is a failing stub either way (-1, 4 x 36 zeros): its published form quantises four frames through
 * packet codebooks that are not at hand, and the reference never calls it. */
typedef struct LPCNetEncState LPCNetEncState;
LPCNetEncState *lpcnet_encoder_create(void);
int lpcnet_encoder_init(LPCNetEncState *st);
void lpcnet_encoder_destroy(LPCNetEncState *st);
int lpcnet_compute_features(LPCNetEncState *st, const short *pcm, float features[4][36]);
int lpcnet_compute_single_frame_features(LPCNetEncState *st, const short *pcm, float features[36]);
/* The batched form on the same xiph state: n_frames frames of pcm[160 n_frames] in one push, out36 (n_frames, 36).  Returns
 * the number of frames, DSS_EINVAL for a NULL state or buffers.  Equal bits to n_frames single-frame calls. */
long long dss_lpcnet_encoder_frames(LPCNetEncState *st, const short *pcm, int n_frames, float *out36);

/* Weights are data in this build (include/dss_lpcnet_blob.h); xiph compiles them in (nnet_data.c,
 * extensions/lpcnet/setup.py:34-36). */
int dss_lpcnet_load_model(const void *blob, size_t len);
int dss_lpcnet_load_model_file(const char *path);
/* SURVEY.md 8(d) algorithmic bytes per output sample for the loaded model (0 if none). */
double dss_lpcnet_bytes_per_sample(void);
/* Which sample-rate kernel the loaded model runs on, and why (any pointer may be NULL):
 *   fast_path     1 = CU-resident kernel, all weights in VGPRs/LDS; 2 = the same kernel with its extended paths (a model
 *                 with skewed sparsity: some row groups keep z/r blocks beyond their wave's register slots as LDS
 *                 records, or h lists longer than 28 -- a few per cent to tens of per cent slower, same results);
 *                 0 = generic kernel (GRU A blocks streamed from L2, several times slower) because the model exceeds
 *                 an outer capacity below;
 *   zr_slots_max  largest z- or r-gate block count of a row group (register slots: 12 on 16 groups, 8 on the other
 *                 32; outer capacity: 16 more per group);
 *   h_slots_max   largest h-gate block count of a row group (28, or 32 in the extended instantiation, with register-held column ids; outer capacity 64);
 *   h_lds_bytes   LDS image: h-gate blocks, z/r tail blocks and their tables (capacity 151 552 B);
 *   gru_a_order   dss_blob_header.gru_a_order of the model. */
int dss_lpcnet_model_info(int *fast_path, int *zr_slots_max, int *h_slots_max, int *h_lds_bytes, int *gru_a_order);

/* ------------------------------------------------------------------------------------------------
 * Part 2 -- batched decoder: B independent utterances / streams, one persistent workgroup each.
 * Replaces the one-process-per-file pool of local/training.py:165-207 and the per-row Python loop of
 * DelayedLPCNetVocoder.synthesize (local/units.py:531-538).  State persists across calls exactly like
 * a vector of LPCNetState (so it also serves 128 concurrent streams, 1 frame per call).
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_lpcnet_batch dss_lpcnet_batch;

dss_lpcnet_batch *dss_lpcnet_batch_create(int max_utts, int max_frames);
void dss_lpcnet_batch_destroy(dss_lpcnet_batch *b);
/* A lane: a second launch context on the decoder slots of `parent` (which must not itself be a lane).  It owns the per-call
 * scratch for max_rows x max_frames and nothing else; its calls are ragged calls whose slot list names the parent's slots.
 * Calls on DIFFERENT lanes (and on the parent) may be in flight on different streams at the same time as long as no slot
 * is in two of them at once -- the caller orders a slot's calls (an event between them).  That is the many-stream form
 * of the reference's one vocoder whose state carries from segment to segment (local/units.py:524,531-538): segments that
 * close on different streams are synthesised side by side, a stream's own segments one after the other.  Destroy with
 * dss_lpcnet_batch_destroy; a parent destroyed first is released with its last lane. */
dss_lpcnet_batch *dss_lpcnet_batch_create_lane(dss_lpcnet_batch *parent, int max_rows, int max_frames);
/* lpcnet_init() on every slot (or on slot `utt` only when utt >= 0). */
int dss_lpcnet_batch_reset(dss_lpcnet_batch *b, int utt);
/* Same, enqueued on `hip_stream` without waiting (for device-resident pipelines and timed loops). */
int dss_lpcnet_batch_reset_async(dss_lpcnet_batch *b, int utt, void *hip_stream);
/* Host buffers.  features: [n_utts][n_frames][feat_stride] float32 (feat_stride >= 20, first 20 used,
 * e.g. 36 for xiph .f32 feature files, LPCNet.pyx:97,115).  pcm: [n_utts][n_frames*160] int16. */
int dss_lpcnet_batch_synthesize(dss_lpcnet_batch *b, const float *features, int n_utts, int n_frames,
                                int feat_stride, short *pcm);
/* Device buffers (same shapes), asynchronous on `hip_stream` (a hipStream_t, or NULL for the default
 * stream).  Nothing is copied to or from the host. */
int dss_lpcnet_batch_synthesize_dev(dss_lpcnet_batch *b, const float *d_features, int n_utts, int n_frames,
                                    int feat_stride, short *d_pcm, void *hip_stream);
/* Ragged / slot-indexed form.  Row i of the call (features [n_utts][n_frames][feat_stride], pcm
 * [n_utts][n_frames*160]) continues the decoder state of slot slots[i] (NULL: slot i) and synthesizes
 * only its first counts[i] <= n_frames frames (NULL: n_frames); its workgroup then retires, pcm beyond
 * counts[i]*160 is left untouched and a count of 0 leaves the slot exactly as it was.  `slots` and
 * `counts` are HOST arrays of n_utts ints, validated (range; a slot may appear once per call, a decoder is
 * sequential) and uploaded on the stream.  This is the shape of the reference's real callers: .npy files
 * of different lengths with a fresh decoder each (local/training.py:182-198), and speech segments of
 * different lengths finishing on some of the 128 streams whose vocoder state carries across segments
 * (local/units.py:524,531-538).  With counts, workgroups take the rows by decreasing frame count whatever order the
 * caller used (the library sorts a dispatch list; results do not depend on it), so that short rows fill in behind the
 * long ones when n_utts exceeds the number of CUs.  Calls on one batch object must be issued on one stream at a time. */
int dss_lpcnet_batch_synthesize_ragged_dev(dss_lpcnet_batch *b, const float *d_features, const int *slots,
                                           const int *counts, int n_utts, int n_frames, int feat_stride,
                                           short *d_pcm, void *hip_stream);
int dss_lpcnet_batch_synthesize_ragged(dss_lpcnet_batch *b, const float *features, const int *slots,
                                       const int *counts, int n_utts, int n_frames, int feat_stride, short *pcm);
/* Progressive form of the ragged call (opt-in; the whole-segment contract above stays the default).  Same rows, slots and
 * counts as dss_lpcnet_batch_synthesize_ragged_dev; the PCM goes straight into host_pcm ([n_utts][n_frames*160] int16) while
 * the kernel runs, and host_frames_done[i] counts the frames of row i already there: the bytes SoX receives, in order
 * (local/units.py:531-538,550-552), a 10 ms frame at a time instead of a whole segment.  Read the counters with
 * dss_progress_read (or acquire loads); counters only grow, and a row of count 0 stays at 0.  The library zeroes
 * host_frames_done[0..n_utts) on the host before it enqueues anything.  Both host pointers must lie in blocks from
 * dss_host_alloc_fine (host_pcm 16-byte aligned); pageable, cached page-locked or short buffers, null pointers, and a batch
 * with trace or teacher forcing on give DSS_EINVAL, and nothing is enqueued.  Neither buffer may belong to a call that is
 * still in flight.  Always one utterance per workgroup (the pair kernel has no progressive form). */
int dss_lpcnet_batch_synthesize_ragged_progress_dev(dss_lpcnet_batch *b, const float *d_features, const int *slots,
                                                    const int *counts, int n_utts, int n_frames, int feat_stride,
                                                    short *host_pcm, int *host_frames_done, void *hip_stream);
/* Kernel choice (uniform and ragged calls).  0 (default): one utterance per workgroup (csrc/lpcnet_sample.hip) while the
 * call has at most one row per CU, two utterances per workgroup -- carried as the two halves of packed fp32 instructions,
 * csrc/lpcnet_sample_pair.hip -- beyond (a uniform call is split: full rounds of two rows per CU on the pair kernel, a
 * remainder of at most one row per CU as one round of the one-utterance kernel); 1 or -1: always one per workgroup; 2:
 * always two (fails with DSS_EINVAL for a
 * model whose CU-resident layout leaves no room for the second utterance).  In a ragged call the two rows of a workgroup
 * are neighbours in the dispatch list (near-equal length); they run packed over the frames both have and the longer one
 * finishes alone.  Models on the extended / generic paths always run one utterance per workgroup.  Results are
 * bit-identical either way, and a decoder state written by one form is continued by the other. */
int dss_lpcnet_batch_set_multi(dss_lpcnet_batch *b, int utterances_per_workgroup);
/* Test taps (device -> host): frame-rate network outputs of the LAST call, per utterance and frame:
 * which = 0: gru_a_condition [n_frames][3*gru_a]; 1: gru_b_condition [n_frames][3*gru_b]; 2: lpc [n_frames][16].
 * which = 3: per-sample excitation index (uint8 stored as float) [n_frames*160]; 4: pre-de-emphasis pcm float.
 * (3 and 4 need dss_lpcnet_batch_enable_trace(b, 1) before the call.) */
int dss_lpcnet_batch_tap(dss_lpcnet_batch *b, int utt, int which, float *out, size_t n_floats);
/* on: 0 = off, 1 = trace on the kernel the model selects, 17 = trace on the generic kernel. */
int dss_lpcnet_batch_enable_trace(dss_lpcnet_batch *b, int on);
/* Teacher forcing (test instrument; needs trace enabled): in the following calls sample k of row u takes the excitation
 * index exc[u*n_frames*160 + k] (host array) instead of the sampled one -- the RNG advances as usual -- and tap 5
 * returns the pre-threshold logits of all 255 tree nodes per sample, [n_frames*160][256] ([.][0] unused).  The calls
 * must have this n_frames.  exc == NULL switches back to free running. */
int dss_lpcnet_batch_force_excitation(dss_lpcnet_batch *b, const unsigned char *exc, int n_utts, int n_frames);
/* Self-test of the only transcendental evaluated on the device on this path: out[i] = (float)(pow(10.0, x[i]) *
 * comp[i]), the expression of freq.c lpc_from_cepstrum (host buffers).  See DESIGN.md section 2. */
int dss_selftest_exp10(const float *x, const float *comp, float *out, long n);
/* Self-test of the device's lin2ulaw (xiph common.h; evaluated in a shorter instruction sequence):
 * out[i] = lin2ulaw(x) for the fp32 x whose bit pattern is start_bits + i * stride (wrapping), i < n (host buffer). */
int dss_selftest_lin2ulaw(unsigned start_bits, unsigned stride, long n, unsigned char *out);
/* Self-test of the short table activations of the CU-resident sample kernel (csrc/lpcnet_device.h) against the forms they
 * replace, on the device: pattern k < n (n <= 2^32) is the fp32 x with bits start_bits + k (wrapping).  which 0: tanh,
 * 1: sigmoid, 2: a * tanh(x) with the sign folded into a pseudo-random factor a.  res[0] = number of patterns whose two
 * results differ in any bit (two NaNs are equal), res[1] = the smallest such k (all ones when there is none). */
int dss_selftest_tansig(int which, unsigned start_bits, unsigned long long n, unsigned long long *res);
/* Host-only (no GPU): the activation tables a loaded model carries, out[0..201) = y, out[208..409) = 1 - y*y as two
 * separately rounded fp32 operations; n must be 409. */
int dss_selftest_tansig_table(float *out, int n);
/* Host-only (no GPU): lays the model out for the CU-resident sample kernel and walks every lane's z, r and h block lists
 * through that layout as the kernel indexes it.  info[8]: fast_path (0/1/2 as in dss_lpcnet_model_info), zr blocks max,
 * h blocks max, LDS bytes, register slots per gate on waves 4-5, tail blocks, mismatching rows, out-of-range reads. */
int dss_selftest_fast_layout(const void *blob, size_t len, int *info);
/* Average device time (ms) of the sample-rate kernel over the calls since the last query, measured with
 * HIP events on the stream the kernel was launched on; resets the accumulator.  Needs
 * dss_lpcnet_batch_enable_timing(b, 1). */
int dss_lpcnet_batch_enable_timing(dss_lpcnet_batch *b, int on);
double dss_lpcnet_batch_kernel_ms(dss_lpcnet_batch *b, int which /*0 = sample kernel, 1 = frame kernels*/);

/* ------------------------------------------------------------------------------------------------
 * Part 3 -- HGA: IIR cascade + warm-start frame buffer + log power, float64
 * ---------------------------------------------------------------------------------------------- */
/* compute_log_power_features(data, sr, window_length, window_shift)  hga_optimized.pyx:27-47.
 * data: host (T, C) float64 row-major.  out: host (W, C), W = dss_hga_num_windows(T, ...).
 * Windowed mean power runs on the device; the final log() is applied by the host libm while copying
 * out, which is what makes the result bit-identical to the reference on any host. */
int dss_hga_num_windows(int T, int sr, float window_length, float window_shift);
int dss_hga_log_power(const double *data, int T, int C, int sr, float window_length, float window_shift,
                      double *out);

/* Stateful extractor for n_streams independent streams of n_channels each: the GPU counterpart of
 * HighGammaExtractor (local/units.py:97-161) without the Python pre/post transforms.
 * sos_hg / sos_fh: (n_sections, 6) band-pass and band-stop second-order sections (units.py:124-126);
 * zi_hg / zi_fh: (n_sections, 2) scipy.signal.sosfilt_zi(sos), replicated over channels as
 * units.py:128-132 does.  Holds per-channel filter state and the last `overlap` filtered rows
 * (WarmStartFrameBuffer, hga_optimized.pyx:50-131) on the device. */
typedef struct dss_hga dss_hga;
dss_hga *dss_hga_create(int n_streams, int n_channels, int fs, float window_length, float window_shift,
                        int n_sections, const double *sos_hg, const double *sos_fh,
                        const double *zi_hg, const double *zi_fh);
void dss_hga_destroy(dss_hga *h);
int dss_hga_reset(dss_hga *h);
/* Frames the next extract call with n new samples per stream will emit. */
int dss_hga_frames_for(const dss_hga *h, int n);
/* extract_features (units.py:145-161): data host (n_streams, n, C) float64 -> out host (n_streams, W, C).
 * Returns W (>= 0) or a negative error.  All streams advance by the same n. */
int dss_hga_extract(dss_hga *h, const double *data, int n, double *out);
/* Fused front end: the pre-transforms decode_online.py:65-97 puts in front of the filters --
 * column reorder (local/common.py:31-32), per-grid common average referencing with excluded channels
 * (common.py:338-345) and channel selection (common.py:54-55) -- collapse to: output channel c =
 * raw[src_col[c]] - mean_g(c), where mean_g is the SEQUENTIAL sum (numpy reduces the fancy-indexed, Fortran-ordered
 * view one column at a time) of raw[comp_cols[comp_off[g] .. comp_off[g+1])] divided by their count, g = grid_of[c]
 * (-1: no referencing).  After this call dss_hga_extract_raw* take raw amplifier packets (n, c_raw). */
int dss_hga_set_frontend(dss_hga *h, int c_raw, const int *src_col, const int *grid_of, int n_grids,
                         const int *comp_cols, const int *comp_off);
int dss_hga_extract_raw(dss_hga *h, const double *raw, int n, double *out);
int dss_hga_extract_raw_dev(dss_hga *h, const double *d_raw, int n, double *d_out, int apply_log, void *hip_stream);
/* Device-resident form: d_data / d_out device pointers; log applied on the device (OCML log, <= 1 ulp
 * from the host's) when apply_log != 0, else out = mean power + 0.01. */
int dss_hga_extract_dev(dss_hga *h, const double *d_data, int n, double *d_out, int apply_log, void *hip_stream);
/* The same from payloads in WIRE format: d_payload (n_streams, c_in, n) float32, channel-major -- the body of the amplifier's
 * packets behind their 7-byte header (local/units.py:78-82: '=BBB HH' + float32[n_channels x n_samples];
 * development_amplifier.py:14-25), c_in = c_raw when a front end is configured, else n_channels.  One more small launch does on
 * the device what ZMQConnector.interpret_bytes does per packet on the host (reshape, transpose, astype(float64)); float32 ->
 * float64 is exact, the frames are those of dss_hga_extract_raw_dev / dss_hga_extract_dev on the converted rows, bit for bit.
 * Half the bytes cross the bus and no stream's packet is touched by the host. */
int dss_hga_extract_wire_dev(dss_hga *h, const float *d_payload, int n, double *d_out, int apply_log, void *hip_stream);
/* Optional last step of the reference's feature chain inside the extractor's launch: ZScoreNormalization,
 * (frame - means[c]) / stds[c] (local/common.py:367-376; decode_online.py:88-97 puts it behind HighGammaActivity as a
 * post-transform).  means / stds: host arrays of n_channels doubles, both NULL to clear.  The device-resident entry
 * points then return z-scored frames (hga_fused_kernel's epilogue, or hga_window_kernel's in the three-launch form); the
 * host-buffer ones apply it on the host after their host-libm log. */
int dss_hga_set_zscore(dss_hga *h, const double *means, const double *stds);
/* ---- a session's trials in one call (baseline_offline.py:45-60, prepare_corpus.py:42-52,179-199) ----
 * The reference builds a FRESH HighGammaExtractor per trial and feeds it rows start .. start+len of one recording as a single
 * chunk.  These entry points do that for a whole trial list with one extractor launch: filters, front end and z-score are the
 * handle's, every trial starts from the unit-step filter state and an empty frame buffer (CASE 1 when len >= one frame,
 * CASE 2 -- left zero pad to one frame -- when frame shift < len < frame; len <= frame shift is an error, pyx:57), and the
 * handle's streaming state (dss_hga_extract*) is neither read nor written.  rec: (T_rec, c_in) float64 row-major, c_in = c_raw
 * with a front end configured, else n_channels; trial ranges may overlap.  out: (sum of W_i, n_channels), trial after trial in
 * list order.  Every range and length is checked on the host before anything is launched.  Returns the number of frames
 * written or a negative error. */
/* Frames of one trial of `len` rows; negative for a rejected length.  The _for form needs no handle (and no device). */
int dss_hga_trial_frames(const dss_hga *h, int len);
int dss_hga_trial_frames_for(int fs, float window_length, float window_shift, int len);
/* The argument checks of the two extract_trials entry points on their own: frames of the whole list, or a negative error. */
int dss_hga_check_trials(int fs, float window_length, float window_shift, long long T_rec, int n_trials,
                         const long long *start, const int *len);
/* Host buffers; host libm log, then patch and z-score on the host: bit-identical to the reference chain. */
int dss_hga_extract_trials(dss_hga *h, const double *rec, long long T_rec, int n_trials, const long long *start,
                           const int *len, double *out);
/* Device-resident; OCML log (<= 1 ulp, as dss_hga_extract_dev), patch and z-score on the device.  start / len are HOST arrays.
 * The call returns once the launches are queued on hip_stream; one call per handle may be in flight. */
int dss_hga_extract_trials_dev(dss_hga *h, const double *d_rec, long long T_rec, int n_trials, const long long *start,
                               const int *len, double *d_out, int apply_log, void *hip_stream);
/* BadChannelCorrection (local/common.py:220-305) on the frames of the trial entry points, after the log and before the
 * z-score, trial by trial as the reference's post-transform runs: column dst_col[k] = mean of columns
 * nb_cols[nb_off[k] .. nb_off[k+1]) in the order numpy's np.mean(data[:, neighbours], axis=1) adds them -- the SEQUENTIAL sum
 * in list order when the trial has two or more frames (for 8 neighbours too), numpy's pairwise kernel (eight running sums,
 * ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), remainder in order; sequential below 8 elements) when it has ONE frame -- and one
 * division.  Neighbours are read from the uncorrected frame: a neighbour that is itself a patched column is an error, as are
 * columns >= n_channels and lists of 128 or more.  NULL / 0 clears. */
int dss_hga_set_patches(dss_hga *h, int n_patches, const int *dst_col, const int *nb_cols, const int *nb_off);
int dss_hga_check_patches(int n_channels, int n_patches, const int *dst_col, const int *nb_cols, const int *nb_off);
/* The same patch on the host frames (N, C) of ONE call of the reference's class, in place (N == 1: the one-frame rule);
 * needs no handle. */
int dss_hga_apply_patches(double *frames, long long N, int C, int n_patches, const int *dst_col, const int *nb_cols,
                          const int *nb_off);
/* out (2, C) = vstack([np.mean(frames, axis=0), np.std(frames, axis=0)]) in numpy's summation order for a C-contiguous
 * (N, C) array: rows added one after the other, / N; std from d = x - mean, d * d, summed the same way, / N, sqrt.  Bit-identical
 * to numpy on the same frames, on the host and on the device (one lane per column walks the rows: the order is the contract).
 * C == 1 is one contiguous run, which numpy sums with its pairwise kernel instead (eight running sums up to 128 elements,
 * halves beyond); both forms follow it there, for the sum and for the sum of squares. */
int dss_hga_column_stats(const double *frames, long long N, int C, double *out);
int dss_hga_column_stats_dev(const double *d_frames, long long N, int C, double *d_out, void *hip_stream);
/* Which form serves a window shape, without a handle or a device: out = {frame_length, shift, overlap, ring_rows, ring_bytes,
 * fused}.  frame_length and shift are the float32 products of hga_optimized.pyx:72-74; ring_rows = (frame_length + shift + 66
 * + 7) & ~7 rows of 16 float64 columns is the LDS ring of the one-launch kernels, ring_bytes = 128 ring_rows; fused = 1 iff
 * ring_bytes <= 40960: dss_hga_extract* then run hga_fused_kernel and the trial entry points are serviceable; with 0 the
 * extractor runs its three-launch form and a trial list is refused.  The launch code takes the same values from the same
 * helper.  Returns 0, or DSS_EINVAL for a shape without a positive shift no longer than the frame. */
int dss_hga_plan(int fs, float window_length, float window_shift, int out[6]);
/* Tests and A/B timing only: which kernel form serves this extractor.  0 = choose (default: hga_fused_kernel; three
 * launches when its ring does not fit LDS), 1 = hga_fused_kernel, 2 = the three-launch form. */
int dss_selftest_hga_force_path(dss_hga *h, int path);

/* ------------------------------------------------------------------------------------------------
 * Part 4 -- speech-segment gate for n_streams streams: the two ring buffers the
 * reference chains behind its neural VAD in FilterSpeechSegments.process (local/units.py:432-447):
 * VoiceActivityDetectionSmoothing (local/common.py:106-153; window 2*smoothing_context+1 <= 64 labels,
 * a frame is speech when the proportion of raw speech labels in the window >= proportion_threshold) and
 * SpeechSegmentHistory (local/common.py:156-215; ring of buffer_size float32 frames, a segment is the
 * speech run plus `context` frames on both sides, emitted on the context-th non-speech frame after it).
 * The VAD network itself stays on PyTorch-ROCm (north_star); its per-frame decisions come in as int32.
 * decode_online.py:115-121 uses smoothing_context 5 (units.py:416), threshold 0.6, buffer 2000, context 50.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_gate dss_gate;
dss_gate *dss_gate_create(int n_streams, int nb_features, int smoothing_context, double proportion_threshold,
                          int buffer_size, int context, int max_frames /* per push */);
void dss_gate_destroy(dss_gate *g);
int dss_gate_reset(dss_gate *g, int stream /* -1: all */);
/* Segments one stream can complete within one push of max_frames frames (E below). */
int dss_gate_max_events(const dss_gate *g);
/* All streams advance by n_frames: frames (n_streams, n_frames, nb_features) float64 (msg.data as the unit
 * receives it; stored as float32 like the numpy rings), labels (n_streams, n_frames) int32, nonzero = the
 * VAD's argmax said speech.  events (HOST out, n_streams x (2+E) ints): per stream [number of segments
 * completed in this push, number of frames the smoothing labelled speech in this push (units.py:445 needs
 * it for previous_frames), length of segment 0, ...].  Returns the total number of completed segments
 * (>= 0) or a negative error.  _dev: device pointers, enqueued on hip_stream, which is synchronised
 * before returning (the caller needs the event counts to go on). */
int dss_gate_push(dss_gate *g, const double *frames, const int *labels, int n_frames, int *events);
int dss_gate_push_dev(dss_gate *g, const double *d_frames, const int *d_labels, int n_frames, int *events,
                      void *hip_stream);
/* Copy segment `event` that `stream` completed in the LAST push: (length, nb_features) float32, at most
 * cap_frames rows.  Returns its length.  A segment of 0 rows (a speech run of buffer_size - 2 * context frames, modulo
 * buffer_size) copies nothing and takes a null destination. */
int dss_gate_segment(dss_gate *g, int stream, int event, float *dst, int cap_frames);
int dss_gate_segment_dev(dss_gate *g, int stream, int event, float *d_dst, int cap_frames, void *hip_stream);
/* The same for n segments of the LAST push in one launch: segment (streams[i], events[i]) goes to row dst_rows[i] of d_dst, a
 * device buffer of row_frames frames per row ((rows, row_frames, nb_features) float32: a pool of segment buffers that outlive
 * the next push).  streams / events / dst_rows are HOST arrays.  Returns n. */
int dss_gate_collect_dev(dss_gate *g, int n, const int *streams, const int *events, const int *dst_rows, float *d_dst,
                         int row_frames, void *hip_stream);
/* Frames this stream has been pushed since the last reset (FilterSpeechSegments' frame_counter). */
int dss_gate_frames_seen(dss_gate *g, int stream);

/* ------------------------------------------------------------------------------------------------
 * Part 5 -- the neural voice-activity detector in front of the gate, for n_streams streams:
 * UnidirectionalVoiceActivityDetector (local/models.py:11-33: LSTM(n_inputs -> H) -> LSTM(H -> H) -> Linear(H -> 2)) as
 * FilterSpeechSegments.process calls it (local/units.py:432-434): every frame of a packet, (h, c) of both layers carried
 * across packets, label = argmax of the two logits.  One launch per call (csrc/vad_lstm.hip).  The reference's arithmetic
 * here is torch.nn.LSTM's: results agree with it to ~1e-6 on the logits (tested at 2e-5), not bit for bit.
 * decode_online.py:115-121 builds the model with 2 layers x 150 hidden units over 64 high-gamma features.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_vad dss_vad;
dss_vad *dss_vad_create(int n_streams, int n_inputs, int hidden_units /* <= 160 */);
void dss_vad_destroy(dss_vad *v);
/* Host arrays in torch.nn.LSTM's own layout (state_dict of the reference class, gate order i, f, g, o):
 * lstm.weight_ih_l0 [4H][n_inputs], lstm.weight_hh_l0 [4H][H], lstm.bias_ih_l0 / bias_hh_l0 [4H], the same four for l1
 * ([4H][H]), classifier.weight [2][H], classifier.bias [2]. */
int dss_vad_load_weights(dss_vad *v, const float *w_ih0, const float *w_hh0, const float *b_ih0, const float *b_hh0,
                         const float *w_ih1, const float *w_hh1, const float *b_ih1, const float *b_hh1,
                         const float *cls_w, const float *cls_b);
/* Zero state (create_new_initial_state, models.py:22-24) of one stream, or of all (stream < 0).  dss_vad_reset runs on the
 * null stream and waits: it is ordered against steps issued on a blocking stream only.  dss_vad_reset_async is enqueued on
 * `hip_stream` -- pass the stream the steps run on. */
int dss_vad_reset(dss_vad *v, int stream);
int dss_vad_reset_async(dss_vad *v, int stream, void *hip_stream);
/* All streams advance by n_frames.  Device pointers, enqueued on hip_stream: d_frames (n_streams, n_frames, n_inputs)
 * float64 (frames_are_f64 != 0: as dss_hga_extract_dev returns them; cast to float32 like units.py:433) or float32;
 * d_labels (n_streams, n_frames) int32, 1 = speech -- what dss_gate_push_dev takes; d_logits (n_streams, n_frames, 2)
 * float32 or NULL. */
int dss_vad_step_dev(dss_vad *v, const void *d_frames, int frames_are_f64, int n_frames, int *d_labels, float *d_logits,
                     void *hip_stream);
/* Host copies of the recurrent state, [2 layers][n_streams][H] each, either may be NULL; set == 0 reads, else writes. */
int dss_vad_state(dss_vad *v, float *h, float *c, int set);

/* ------------------------------------------------------------------------------------------------
 * Part 6 -- the bidirectional recurrent decoder between the extractor and the vocoder:
 * BidirectionalSpeechSynthesisModel (local/models.py:36-58: LSTM(n_inputs -> H, 2 layers, bidirectional) ->
 * Linear(2H -> 20)) as DecodingModel.process calls it (local/units.py:499-508): all frames of a segment (or of a
 * packet, in the chunk-wise streaming mode), zero initial state per call, frames cast to float32.  Three launches per
 * call (csrc/bilstm_decoder.hip: one per layer with both directions side by side, one for the regressor) instead of
 * MIOpen's chain of ~20.  The reference's arithmetic here is torch.nn.LSTM's: results agree with it to ~1e-6 on the
 * features (tested at 2e-5 against the reference-generated golden vector), not bit for bit.  A decoder of another
 * architecture stays a PyTorch-ROCm module (dss_amd/pipeline.py falls back to it).
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_dec dss_dec;
dss_dec *dss_dec_create(int max_streams, int max_frames, int n_inputs /* <= 256 */, int hidden_units /* <= 128 */, int n_outputs /* <= 32 */);
void dss_dec_destroy(dss_dec *v);
/* w: 18 host arrays in torch.nn.LSTM's own layout (state_dict of the reference class, gate order i, f, g, o):
 * for layer l in (0, 1), for (forward, reverse): lstm.weight_ih_l{l}[_reverse] [4H][Cin], lstm.weight_hh_l{l}[_reverse] [4H][H],
 * lstm.bias_ih_l{l}[_reverse] [4H], lstm.bias_hh_l{l}[_reverse] [4H] (Cin = n_inputs for l = 0, 2H for l = 1); then
 * regressor.weight [n_outputs][2H], regressor.bias [n_outputs]. */
int dss_dec_load_weights(dss_dec *v, const float *const *w);
/* Device pointers, enqueued on hip_stream: d_frames (n_streams, n_frames, n_inputs) float64 (frames_are_f64 != 0: as
 * dss_hga_extract_dev returns them) or float32; d_feats (n_streams, n_frames, n_outputs) float32 -- what
 * dss_lpcnet_batch_synthesize_dev takes. */
int dss_dec_forward_dev(dss_dec *v, const void *d_frames, int frames_are_f64, int n_streams, int n_frames, float *d_feats,
                        void *hip_stream);
/* Ragged form -- the segments that closed on one tick, each decoded as a whole from a fresh state (units.py:499-508), in one
 * call: stream i has counts[i] <= n_frames frames, read from row in_rows[i] (NULL: i) of d_frames, a buffer of row_frames >=
 * n_frames frames per row (what dss_gate_collect_dev fills); its backward direction starts at its OWN last frame.  counts /
 * in_rows are HOST arrays.  d_feats is (n_streams, n_frames, n_outputs); rows beyond counts[i] are left untouched. */
int dss_dec_forward_rows_dev(dss_dec *v, const void *d_frames, int frames_are_f64, int row_frames, const int *in_rows,
                             const int *counts, int n_streams, int n_frames, float *d_feats, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 7 -- acoustic voice-activity labels for the trials of a recording session: the `vad_labels` array of the training
 * corpus (prepare_corpus.get_vad_labels, prepare_corpus.py:78-116), which the neural detector of Part 5 is trained on.  Per
 * trial the reference builds a fresh EnergyBasedVad (local/common.py:556-649) and runs from_wav on int16 audio: frames of
 * `window` samples every `shift`, W = floor((n - window) / shift) + 1; x / 2^15 times the window, |real DFT|, the mel filter
 * bank (MelFilterBank, common.py:475-514), log(mel + 1e-7); the frame's log energy is coefficient 0 of scipy's type-2 DCT over
 * the bands, 2 * sum; threshold = energy_threshold + energy_mean_scale * sum(log energy) / W (the mean term is skipped when
 * the scale is 0); frame i is voiced iff, over the frames t in [i - frames_context, i + frames_context) inside the trial,
 * (number with log energy > threshold) >= (number of frames) * proportion_threshold in float64.
 * Here a whole trial list runs in two launches (csrc/acoustic_vad.hip).  The audio is taken AS THE CALLER HANDS IT OVER by
 * dss_avad_labels_trials*: the reference's per-trial loudness normalisation through pydub (prepare_corpus._normalize_audio) is
 * opt-in, through dss_avad_set_gain and dss_avad_prepare_trials* at the end of this part.
 * Trial i is `lead[i]` zero samples followed by audio[first[i] .. first[i] + len[i] - lead[i]): len[i] samples in all, which
 * is the reference's 16 ms shift (prepare_corpus.py:91-93) with lead = 256.  Ranges may overlap.  A trial shorter than one
 * window has no frame (the reference divides by zero there) and is refused.  silence[i] != 0 gives the trial all-zero labels
 * (prepare_corpus.py:99-100).  The reference's arithmetic is numpy's FFT and BLAS: log energies agree with it to ~1e-12, not
 * bit for bit; the same trial gives the same bits alone or inside any list, on every run.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_avad_params {
    int window, shift;                 /* samples per frame (a multiple of 4), samples between frames: 800, 160 at 16 kHz */
    int n_bins, n_bands;               /* window / 2 + 1 spectrum bins, mel bands (<= 64) */
    int frames_context, reserved;      /* EnergyBasedVad's vad_frames_context (5) */
    double energy_threshold;           /* 4 */
    double energy_mean_scale;          /* 1; >= 0 */
    double proportion_threshold;       /* 0.6; inside (0, 1) */
} dss_avad_params;
typedef struct dss_avad dss_avad;
/* The checks of dss_avad_create on their own (no device needed). */
int dss_avad_check_params(const dss_avad_params *p);
/* window_fn: `window` doubles (numpy.hanning(window) in the reference); mel: the (n_bins, n_bands) row-major filter matrix
 * (MelFilterBank.melMatrix).  Both are data the caller computes (dss_amd.acoustic_vad).  NULL on failure. */
dss_avad *dss_avad_create(const dss_avad_params *p, const double *window_fn, const double *mel);
void dss_avad_destroy(dss_avad *h);
/* Frames of a trial of n samples, or DSS_EINVAL when n < window (no device needed). */
int dss_avad_trial_frames_for(int n, int window, int shift);
/* The argument checks of the two labels_trials entry points on their own (no device needed): frames of the whole list, or
 * DSS_EINVAL with the reason in dss_last_error() -- NULL arrays, a negative count, first < 0, len < 0, lead < 0, lead > len,
 * a range that ends behind the audio, len < window, more than 2^31 - 1 frames. */
int dss_avad_check_trials(long long n_audio, int n_trials, const long long *first, const int *len, const int *lead, int window,
                          int shift);
/* Host buffers: audio int16[n_audio]; silence (n_trials bytes) may be NULL; labels uint8[sum W], trial after trial in list
 * order; log_energy double[sum W] and threshold double[n_trials] may be NULL.  Returns the number of frames. */
int dss_avad_labels_trials(dss_avad *h, const int16_t *audio, long long n_audio, int n_trials, const long long *first,
                           const int *len, const int *lead, const unsigned char *silence, unsigned char *labels,
                           double *log_energy, double *threshold);
/* Device-resident: d_audio, d_labels, d_log_energy (or NULL), d_threshold (or NULL) are device pointers; first / len / lead /
 * silence are HOST arrays.  Returns once the launches are queued on hip_stream; one call per handle may be in flight. */
int dss_avad_labels_trials_dev(dss_avad *h, const int16_t *d_audio, long long n_audio, int n_trials, const long long *first,
                               const int *len, const int *lead, const unsigned char *silence, unsigned char *d_labels,
                               double *d_log_energy, double *d_threshold, void *hip_stream);
/* Threshold and vote of ONE trial on the host from its W log energies (no device needed).  The vote's comparison is the
 * reference's; the sum behind the mean is taken in the device kernel's order (256 strided running sums, then a halving
 * tree), not numpy's pairwise one.  labels: W bytes; threshold may be NULL. */
int dss_avad_vote_host(const double *log_energy, int W, const dss_avad_params *p, unsigned char *labels, double *threshold);
/* Opt-in: the trial's audio as prepare_corpus.py prepares it (prepare_corpus.py:33-40, 58-69, 84-93), which the entry points
 * above leave out.  Every trial whose stimulus is not SILENCE goes through pydub there: effects.normalize, then apply_gain(-3),
 * each one audioop.mul over the int16 samples.  Here, for a trial with normalize[i] != 0:
 *   peak      = max |x| over the cut audio[first .. first + len) (where the audio ends before that, over what is there), 0 ..
 *               32768 (-32768 counts as 32768); the last `lead` samples count although the shift drops them;
 *   scale(x, f) = (int16) floor(v), v = (double) x * f, v > 32767 -> 32767, v < -32767 -> -32768 (audioop's fbound);
 *   prepared  = scale(scale(x, gain_by_peak[peak]), post_gain): two roundings, never one folded product;
 * and the prepared trial is `lead` zeros followed by the first len - lead prepared samples.  A trial with normalize[i] == 0 (a
 * SILENCE trial) keeps its samples.  gain_by_peak is DATA: the library evaluates no log and no pow (dss_amd.trial_audio
 * computes pydub's table).  Labels, log energies and thresholds of a normalised call are, bit for bit, those of the plain call
 * on the prepared audio. */
/* The two functions the kernels share with the host (csrc/avad_gain.h); no device needed.  Peak of n samples; DSS_EINVAL for
 * a NULL array. */
int dss_avad_peak_host(const int16_t *x, long long n);
/* out[i] = scale(x[i], factor); a non-finite factor is refused. */
int dss_avad_scale_host(const int16_t *x, long long n, double factor, int16_t *out);
/* Samples one workgroup of the peak kernel takes (a trial's tiles are joined by an integer atomic max). */
int dss_avad_peak_tile(void);
/* Uploads gain_by_peak[32769] (index = peak) and the post gain into the handle, once; both stay until set again.  Refuses a
 * negative or non-finite entry (before it looks at the handle: the refusals need no device).  Waits for the handle's device. */
int dss_avad_set_gain(dss_avad *h, const double *gain_by_peak, double post_gain);
/* The arguments of dss_avad_labels_trials plus: normalize (n_trials bytes, NULL = no trial), prepared (int16[sum len]: the
 * prepared trials, leading zeros included, trial i from sum(len[:i]) on; may be NULL), peaks (int32[n_trials], the peak of
 * EVERY trial, normalised or not; may be NULL).  labels may be NULL as well -- then log_energy and threshold must be, the energy
 * and vote launches are skipped, a trial shorter than one window is allowed, and 0 is returned.  At least one output must be
 * asked for.  A call that normalises a trial before dss_avad_set_gain fails with the reason in dss_last_error().  Launches:
 * peak, energy, vote, and a fourth for `prepared`. */
int dss_avad_prepare_trials(dss_avad *h, const int16_t *audio, long long n_audio, int n_trials, const long long *first,
                            const int *len, const int *lead, const unsigned char *silence, const unsigned char *normalize,
                            unsigned char *labels, double *log_energy, double *threshold, int16_t *prepared, int *peaks);
/* Device-resident form: d_audio and the five outputs are device pointers, the lists HOST arrays; nothing waits for the device
 * between the launches; one call per handle may be in flight. */
int dss_avad_prepare_trials_dev(dss_avad *h, const int16_t *d_audio, long long n_audio, int n_trials, const long long *first,
                                const int *len, const int *lead, const unsigned char *silence, const unsigned char *normalize,
                                unsigned char *d_labels, double *d_log_energy, double *d_threshold, int16_t *d_prepared,
                                int *d_peaks, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 8 -- the two recurrent models over the trials of a corpus, and their validation scores.  A corpus is concatenated
 * arrays cut into trials (hga_activity (N, C), vad_labels, lpc_coefficients, trial_ids: prepare_corpus.py:218-234); the
 * reference's training scripts run every validation trial through the model from a fresh state once per epoch and score it:
 * train_unidirectional_vad.py:181-215 (per-trial nn.CrossEntropyLoss summed over the trials, softmax / argmax per frame, frame
 * accuracy against vad_labels) and train_bidirectional_model.py:165-188 (per-trial nn.MSELoss, averaged over the trials).
 * Here a whole trial list is one call.  Trial k is rows first[k] .. first[k] + len[k] of d_frames, (N, n_inputs) float64
 * (frames_are_f64 != 0) or float32; ranges may overlap and come in any order; first / len are HOST arrays.  Outputs are
 * concatenated in list order: row sum(len[:k]) + t is frame t of trial k (the convention of dss_hga_extract_trials).  Every
 * trial starts from the zero state (create_new_initial_state).  The detector's training is Part 9, the decoder's Part 10.
 * On one handle, trial-list calls are issued on one stream, or one after the other has finished: the handle keeps the
 * call's trial table.
 * ---------------------------------------------------------------------------------------------- */
/* The argument checks of the two forward entry points on their own (no device needed): DSS_EINVAL with the reason in
 * dss_last_error() for a NULL pointer, a negative count, len < 1, first < 0 or first + len > N; else 0 and *total = sum(len). */
int dss_trials_check(long long N, int n_trials, const long long *first, const int *len, long long *total);
/* The detector of Part 5 on every trial, one launch for any n_trials (it need not fit the handle's n_streams): a workgroup
 * per trial, longest first.  d_labels int32[sum len]; d_logits float32[sum len][2] or NULL.  The handle's streaming state
 * (dss_vad_step_dev, dss_vad_state) is neither read nor written.  A trial's labels and logits are bit-identical to
 * dss_vad_step_dev on a one-stream handle that is given the trial's len[k] frames in one call from the zero state. */
int dss_vad_forward_trials_dev(dss_vad *v, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                               const long long *first, const int *len, int *d_labels, float *d_logits, void *hip_stream);
/* Scores of such logits and labels against d_targets, uint8[sum len] (0 / 1, vad_labels) in the same concatenated order; len is
 * a HOST array.  Per frame, evaluated in float64 from the float32 logits z: d_prob[i] = softmax(z)[1] as float32 (or NULL).
 * Per trial: d_loss[k] = the mean over its frames of logsumexp(z) - z[target], summed in frame order in float64 (the
 * reference's cfunc on one trial); d_correct[k] = the number of its frames with label == target. */
int dss_vad_score_trials_dev(const float *d_logits, const int *d_labels, const unsigned char *d_targets, int n_trials,
                             const int *len, double *d_loss /* [n_trials] */, int *d_correct /* [n_trials] */,
                             float *d_prob /* [sum len] or NULL */, void *hip_stream);
/* The decoder of Part 6 on every trial, each as a whole from a fresh state (its backward direction starts at its own last
 * frame): d_feats float32[sum len][n_outputs].  Lists longer than the handle's max_streams run in chunks inside the call; a
 * trial longer than max_frames is an error (nothing is truncated); first[k] must be below 2^31.  A trial's features are
 * bit-identical to dss_dec_forward_rows_dev on the same frames. */
int dss_dec_forward_trials_dev(dss_dec *v, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                               const long long *first, const int *len, float *d_feats, void *hip_stream);
/* d_mse[k] = the mean over trial k's len[k] x n_outputs elements of (d_feats - d_targets)^2, both float32[sum len][n_outputs],
 * accumulated in float64 in a fixed order (256 strided running sums, then a halving tree). */
int dss_dec_mse_trials_dev(const float *d_feats, const float *d_targets, int n_outputs, int n_trials, const int *len,
                           double *d_mse /* [n_trials] */, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 9 -- training the neural detector of Part 5: the loop of train_unidirectional_vad.py:135-175 (truncated backpropagation
 * through time with k1 == k2, batch size 1, torch.optim.RMSprop) as two launches per window (csrc/vad_train.hip).  A window is T
 * frames of one trial (1 <= T <= max_window; the script uses 50) with 0 / 1 targets: forward from the carried state,
 * nn.CrossEntropyLoss (the mean over the T frames), the gradient of that loss with respect to all ten parameter tensors,
 * backpropagated through the window's T steps and stopped at its initial state (state.detach(), line 173), then
 *     sq <- alpha sq + (1 - alpha) g^2;   p <- p - lr g / (sqrt(sq) + eps)       (momentum 0, not centred, no weight decay)
 * per element; bias_ih and bias_hh have equal gradients and each its own square average.  The final (h, c) of both layers is
 * carried to the next window.  Dropout (nn.LSTM(dropout = p) in train mode) multiplies layer 0's output, as layer 1 reads it, by a
 * mask of 0 or 1 / (1 - p) -- not layer 1's output, not the h layer 0 carries to its own next step; the mask is an INPUT here,
 * float32 (T, H) multipliers or NULL for none, and the backward pass uses the same one.  The kernels hold no generator.
 * Every reduction has a fixed order: the same call from the same state gives the same bits.  Fused multiply-adds are used.
 *
 * Flat arrays (dss_vad_trainer_read) hold the ten tensors in state_dict order, each in torch's layout:
 *     lstm.weight_ih_l0 [4H][C], lstm.weight_hh_l0 [4H][H], lstm.bias_ih_l0 [4H], lstm.bias_hh_l0 [4H],
 *     lstm.weight_ih_l1 [4H][H], lstm.weight_hh_l1 [4H][H], lstm.bias_ih_l1 [4H], lstm.bias_hh_l1 [4H],
 *     classifier.weight [2][H], classifier.bias [2]                  -- dss_vad_trainer_param_count(C, H) floats in all.
 * Calls on one trainer are issued on one stream, or one after the other has finished.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_vad_trainer dss_vad_trainer;
/* The argument checks of this part on their own (no device needed): DSS_EINVAL with the reason in dss_last_error() for sizes that
 * are not positive or beyond the kernels' capacities (hidden_units <= 160, n_inputs <= 128, max_window <= 4096), a window of T < 1
 * or T > max_window frames, a trial of len < 1 frames, or trial windows of window < 1 or > max_window frames; else 0.  A caller
 * that has no trial (or no single window) in hand passes 1 for the arguments it does not mean. */
int dss_vad_trainer_check(int n_inputs, int hidden_units, int max_window, int T, int len, int window);
long dss_vad_trainer_param_count(int n_inputs, int hidden_units);
dss_vad_trainer *dss_vad_trainer_create(int n_inputs, int hidden_units, int max_window);
void dss_vad_trainer_destroy(dss_vad_trainer *tr);
/* The ten host arrays of dss_vad_load_weights.  Zeroes the square averages, the gradients and the carried state. */
int dss_vad_trainer_load(dss_vad_trainer *tr, const float *w_ih0, const float *w_hh0, const float *b_ih0, const float *b_hh0,
                         const float *w_ih1, const float *w_hh1, const float *b_ih1, const float *b_hh1,
                         const float *cls_w, const float *cls_b);
/* One flat host array (see above): what = 0 the parameters, 1 the gradients of the last window, 2 the square averages.  Waits
 * for the device. */
int dss_vad_trainer_read(dss_vad_trainer *tr, int what, float *out);
/* Host copies of the carried state, [2 layers][H] each, either may be NULL; set == 0 reads, else writes.  Waits for the device.
 * dss_vad_trainer_reset_state zeroes it (create_new_initial_state: a new trial), enqueued on hip_stream. */
int dss_vad_trainer_state(dss_vad_trainer *tr, float *h, float *c, int set);
int dss_vad_trainer_reset_state(dss_vad_trainer *tr, void *hip_stream);
/* One window, enqueued on hip_stream.  Device pointers: d_frames (T, n_inputs) float64 (frames_are_f64 != 0; cast to float32
 * like the script's .float()) or float32; d_targets uint8[T] (0 / 1); d_mask float32 (T, H) or NULL; *d_loss receives the
 * window's loss (float64, from the float32 logits).  Always computes the loss and the gradients and advances the carried state;
 * parameters, square averages and the packed copies the forward pass reads change only if apply_step != 0. */
int dss_vad_trainer_window_dev(dss_vad_trainer *tr, const void *d_frames, int frames_are_f64, int T, const unsigned char *d_targets,
                               const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss,
                               void *hip_stream);
/* One trial (the script's lines 146-175), enqueued on hip_stream with no host synchronisation between the windows: the state is
 * reset, then windows of `window` frames are stepped in order, the last one being the remainder (len mod window, possibly one
 * frame), each with apply_step.  d_frames (len, n_inputs), d_targets uint8[len], d_masks float32 (len, H) or NULL, d_losses
 * float64[ceil(len / window)].  Returns the number of windows.  Bit-identical to dss_vad_trainer_reset_state followed by
 * dss_vad_trainer_window_dev on the same slices. */
int dss_vad_trainer_trial_dev(dss_vad_trainer *tr, const void *d_frames, int frames_are_f64, int len, const unsigned char *d_targets,
                              const float *d_masks, int window, double lr, double alpha, double eps, double *d_losses,
                              void *hip_stream);
/* Copies the current weights, in the packed form the forward kernels read (b = bias_ih + bias_hh in float32), device to device
 * into an inference handle of the same n_inputs and hidden_units that has weights loaded; enqueued on hip_stream.  After it Part 5
 * and Part 8 run on the trained weights with no host round trip.  The handle's recurrent state is not touched. */
int dss_vad_trainer_publish(dss_vad_trainer *tr, dss_vad *v, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 10 -- training the decoder of Part 6: the loop of train_bidirectional_model.py:134-152 (batch size 1, one trial is one
 * update step, torch.optim.RMSprop) as seven launches per trial on one stream (csrc/dec_train.hip).  A trial is T frames
 * (1 <= T <= max_frames) with float32 targets (T, n_outputs): forward from the zero state through both layers and directions,
 * nn.MSELoss (the mean over the T x n_outputs elements), the gradient of that loss with respect to all eighteen parameter tensors,
 * backpropagated through the whole trial in both directions, then RMSprop per element as in Part 9; bias_ih and bias_hh have
 * equal gradients and each its own square average.  Dropout (nn.LSTM(dropout = p) in train mode) multiplies layer 0's
 * concatenated output [h_forward(t) | h_backward(t)], as layer 1 reads it, by a mask of 0 or 1 / (1 - p) -- not layer 1's
 * output, not the h a direction carries to its own next step; the mask is an INPUT, float32 (T, 2H) multipliers or NULL for
 * none, and the backward pass uses the same one.  The kernels hold no generator.  Every reduction has a fixed order: the same
 * call from the same state gives the same bits.  Fused multiply-adds are used.  Without a mask the forward half computes the
 * features of dss_dec_forward_dev on one stream, bit for bit.
 *
 * Flat arrays (dss_dec_trainer_read) hold the eighteen tensors in state_dict order, each in torch's layout:
 *     for layer in (0, 1), for direction in (forward, reverse): weight_ih [4H][Cin], weight_hh [4H][H], bias_ih [4H], bias_hh [4H]
 *     (Cin = n_inputs for layer 0, 2H for layer 1), then regressor.weight [O][2H], regressor.bias [O]
 *                                                        -- dss_dec_trainer_param_count(C, H, O) floats in all.
 * Calls on one trainer are issued on one stream, or one after the other has finished.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_dec_trainer dss_dec_trainer;
/* The argument checks of this part on their own (no device needed): DSS_EINVAL with the reason in dss_last_error() for sizes that
 * are not positive or beyond the kernels' capacities (hidden_units <= 128, n_inputs <= 256, n_outputs <= 32, max_frames <= 4096)
 * or a trial of T < 1 or T > max_frames frames; else 0. */
int dss_dec_trainer_check(int n_inputs, int hidden_units, int n_outputs, int max_frames, int T);
long dss_dec_trainer_param_count(int n_inputs, int hidden_units, int n_outputs);
/* The workspace of a trial takes about (34 H + C + 3 O) x max_frames floats of device memory (13 MB at H 100, 1500 frames). */
dss_dec_trainer *dss_dec_trainer_create(int n_inputs, int hidden_units, int n_outputs, int max_frames);
void dss_dec_trainer_destroy(dss_dec_trainer *tr);
/* The eighteen host arrays of dss_dec_load_weights.  Zeroes the square averages and the gradients. */
int dss_dec_trainer_load(dss_dec_trainer *tr, const float *const *w);
/* One flat host array (see above): what = 0 the parameters, 1 the gradients of the last trial, 2 the square averages.  Waits
 * for the device. */
int dss_dec_trainer_read(dss_dec_trainer *tr, int what, float *out);
/* The features (T, n_outputs) the forward half of the last trial of T frames computed, to a host array.  Waits for the device. */
int dss_dec_trainer_features(dss_dec_trainer *tr, int T, float *out);
/* One trial, enqueued on hip_stream with no host synchronisation between its launches.  Device pointers: d_frames (T, n_inputs)
 * float64 (frames_are_f64 != 0; cast to float32 like the script's .float()) or float32; d_targets float32 (T, n_outputs); d_mask
 * float32 (T, 2H) or NULL; *d_loss receives the trial's loss (float64, from the float32 features).  Always computes the loss and
 * the gradients; parameters, square averages and the packed copies the forward pass reads change only if apply_step != 0. */
int dss_dec_trainer_trial_dev(dss_dec_trainer *tr, const void *d_frames, int frames_are_f64, int T, const float *d_targets,
                              const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss,
                              void *hip_stream);
/* Copies the current weights, in the packed form the forward kernels read (b = bias_ih + bias_hh in float32), device to device
 * into an inference handle of the same n_inputs, hidden_units and n_outputs that has weights loaded; enqueued on hip_stream.
 * After it Part 6 and Part 8 run on the trained weights with no host round trip. */
int dss_dec_trainer_publish(dss_dec_trainer *tr, dss_dec *v, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 11 -- spectrograms over the trials of a recording, and the two reductions the reference's per-electrode spectral analysis
 * takes of them (eval/suppl_fig_2.py:41-92; eval/figure_2ab.py:30-31 needs the same operator on audio).  The reference calls
 * scipy.signal.spectrogram once per trial and channel; here a trial list and all channels are one call (csrc/spectral.hip).
 * The signals are a row-major (n_rows, ld) float64 array of which the first C <= ld columns are channels (the layout of
 * dss_hga_extract_trials: a 129-column recording needs no copy).  Trial i is rows first[i] .. first[i] + length[i]; trials may
 * overlap and differ in length; first / length are HOST arrays in every form.  Frame w of a trial is its rows w * hop ..
 * w * hop + nperseg - 1, W = (length - nperseg) / hop + 1 frames, no padding and no boundary extension.  Per frame and channel:
 * the frame's mean is removed (detrend = 1; scipy's detrend='constant'), the frame is multiplied by the window (data of the
 * caller) and transformed at bins 0 .. nfft / 2, zero-padded to nfft >= nperseg.  DSS_SPEC_PSD gives (re^2 + im^2) /
 * (fs * sum window^2), doubled except at bin 0 and, for even nfft, the last bin; DSS_SPEC_MAGNITUDE gives sqrt(re^2 + im^2) /
 * sqrt(fs * sum window^2), scipy's mode='magnitude' with its default scaling='density'.  scipy's arithmetic is pocketfft: results
 * agree with it within 2 (nperseg + 8) sqrt(nperseg) 2^-53 of the frame's largest bin (PSD; half that for the magnitude), not bit
 * for bit; fused multiply-adds are used; the same frame gives the same bits alone or inside any list, in all three operations.
 * Limits: nperseg >= 2, hop >= 1, nperseg <= nfft <= 2048, C >= 1.
 * ---------------------------------------------------------------------------------------------- */
#define DSS_SPEC_PSD 0
#define DSS_SPEC_MAGNITUDE 1
typedef struct dss_spec_params {
    int nperseg, hop, nfft;            /* rows per frame, rows between frames (nperseg - noverlap), transform length */
    int mode, detrend, reserved;       /* DSS_SPEC_PSD or DSS_SPEC_MAGNITUDE; 1 removes every frame's mean, 0 does not */
    double fs;                         /* sampling rate */
} dss_spec_params;
typedef struct dss_spec dss_spec;
/* The checks of dss_spec_create on their own (no device needed). */
int dss_spec_check_params(const dss_spec_params *p);
/* Frames of a trial of n rows, or DSS_EINVAL when n < nperseg, nperseg < 2 or hop < 1 (no device needed). */
long long dss_spec_trial_frames_for(long long n, int nperseg, int hop);
/* The argument checks of the trial-list entry points on their own (no device needed): frames of the whole list, or DSS_EINVAL
 * with the reason in dss_last_error() -- NULL arrays, a negative count, first < 0, length < 0, a range that ends behind the
 * signals, length < nperseg. */
long long dss_spec_check_trials(long long n_rows, int n_trials, const long long *first, const long long *length, int nperseg, int hop);
/* The checks of the onset-locked mean on their own (no device needed): pre + post, or DSS_EINVAL naming the trial whose onset
 * frame has fewer than `pre` frames before it (onset - pre < 0) or fewer than `post` frames from it on (onset + post > W).  The
 * reference slices Sxx[:, onset - pre : onset + post] there and silently gets a wrong or short slice. */
int dss_spec_check_locked(int n_trials, const long long *length, const int *onset, int pre, int post, int nperseg, int hop);
/* How a call with these parameters and n_channels channels will cut its workgroups (no device needed): the very choice the
 * launches make, for tests that must know which shape a case runs.  kind: 0 spectrograms (dss_spec_trials), 1 onset-locked mean
 * (dss_spec_locked), 2 mean spectrum (dss_spec_mean).  out = F frames, CG channels, NB blocks of 16 bins per workgroup, the
 * number of 16-bin blocks of nfft / 2 + 1 bins, bytes of LDS per workgroup.  0, or DSS_EINVAL with the reason in
 * dss_last_error(): what dss_spec_check_params refuses, n_channels < 1, an unknown kind. */
int dss_spec_geometry(const dss_spec_params *p, int n_channels, int kind, int out[5]);
/* window: nperseg doubles (scipy.signal.get_window('hann', nperseg) in the reference; dss_amd.spectral.hann_periodic).  NULL on
 * failure. */
dss_spec *dss_spec_create(const dss_spec_params *p, const double *window);
void dss_spec_destroy(dss_spec *h);
/* Spectrograms: out is (sum W_i, C, nfft / 2 + 1) float64, frame after frame, trial after trial in list order.  Returns the
 * number of frames.  Host buffers; only the rows the trials span are copied to the device. */
long long dss_spec_trials(dss_spec *h, const double *x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                          const long long *length, double *out);
/* Device-resident: d_x and d_out are device pointers.  Returns once the launch is queued on hip_stream; one call per handle may
 * be in flight. */
long long dss_spec_trials_dev(dss_spec *h, const double *d_x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                              const long long *length, double *d_out, void *hip_stream);
/* The mean over the trials of the frames around each trial's own onset frame, without storing any spectrogram: out is
 * (C, nfft / 2 + 1, pre + post) float64, column j the mean over i of frame onset[i] - pre + j of trial i -- the trials' values
 * added in list order, then divided by n_trials.  onset is a HOST array.  Returns pre + post. */
int dss_spec_locked(dss_spec *h, const double *x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                    const long long *length, const int *onset, int pre, int post, double *out);
int dss_spec_locked_dev(dss_spec *h, const double *d_x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                        const long long *length, const int *onset, int pre, int post, double *d_out, void *hip_stream);
/* The mean spectrum over ALL frames of all trials: out is (C, nfft / 2 + 1) float64 -- every trial's frames added in frame order,
 * the trials' sums added in list order, divided by the number of frames (two launches).  Returns 0. */
int dss_spec_mean(dss_spec *h, const double *x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                  const long long *length, double *out);
int dss_spec_mean_dev(dss_spec *h, const double *d_x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                      const long long *length, double *d_out, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 12 -- the lagged audio-ECoG spectrogram correlation sums of the acoustic contamination analysis (stage 1 of the reference's
 * replicate.sh; eval/contamination/run_contamination_analysis.m drives a MATLAB toolbox after Roussel et al. that the reference
 * does not ship, so the definition is this project's own restatement of the published method: DESIGN.md and
 * tests/contamination_reference.py; parity with the toolbox's output is not pinned).  The brain signals are a row-major
 * (n_rows, ld) float64 array of which the first C <= ld columns are channels, the audio n_rows float64 values at the same rate.
 * Frame t is rows t * hop .. t * hop + nperseg - 1, W = (n_rows - nperseg) / hop + 1 frames, no padding; per frame the rows
 * times the window (data of the caller), the DFT of length nperseg, the magnitude at bins bin_lo .. bin_lo + n_bins - 1, no
 * detrending and no scale factor (a Pearson correlation does not see one).  With A[t][i] the audio's magnitudes less shift[i],
 * N_c[t][j] those of channel c, keep[t] the frame mask, a call gives for every lag l in -max_lag .. max_lag, over the frames t
 * with 0 <= t + l < W, keep[t] and keep[t + l]:
 *     n[l] the number of such frames, sa[l][i] = sum A[t+l][i], saa[l][i] = sum A[t+l][i]^2,
 *     sb[l][c][j] = sum N_c[t][j], sbb[l][c][j] = sum N_c[t][j]^2, sab[l][c][i][j] = sum A[t+l][i] N_c[t][j],
 * and shift[i], the mean of the audio's bin i over the kept frames, which the library subtracts so that sab - sa sb / n does not
 * cancel.  The result is ONE float64 array: n (2 max_lag + 1), shift (n_bins), sa, saa (lags, n_bins), sb, sbb (lags, C, n_bins),
 * sab (lags, C, n_bins, n_bins), at the offsets dss_contam_result_size reports.  No spectrogram of a channel is ever stored.
 * No atomics; every sum has one fixed order: the same call gives the same bits, from host or device buffers.  Fused multiply-adds
 * are used.  A lag with |l| >= W has n = 0 and sums of 0.
 * Limits: 2 <= nperseg <= 2048, hop >= 1, 1 <= n_bins <= 31, 0 <= max_lag <= 4096, C <= 65535, and 32 frames of one channel
 * (31 min(hop, nperseg) + nperseg rows) beside the tables within the kernel's 80 KB of LDS.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_contam_params {
    int nperseg, hop;                  /* rows per frame (also the transform length), rows between frames */
    int bin_lo, n_bins;                /* kept DFT bins bin_lo .. bin_lo + n_bins - 1 */
    int max_lag, reserved;             /* lags -max_lag .. max_lag, in frames */
} dss_contam_params;
typedef struct dss_contam dss_contam;
/* The checks of dss_contam_create on their own (no device needed). */
int dss_contam_check_params(const dss_contam_params *p);
/* Those, and the window's own: nperseg finite doubles, not all zero (no device needed; dss_contam_create runs it first). */
int dss_contam_check_window(const dss_contam_params *p, const double *window);
/* Frames of a recording of n_rows rows, or DSS_EINVAL: n_rows < nperseg, nperseg < 2, hop < 1, max_lag < 0, or frames plus lags
 * beyond the kernels' 32-bit frame index (no device needed).  max_lag >= the frame count is allowed: the outer lags are empty. */
long long dss_contam_frames_for(long long n_rows, int nperseg, int hop, int max_lag);
/* The checks both calls make of their sizes before they touch the device, on their own: what dss_contam_check_params and
 * dss_contam_frames_for refuse, n_channels < 1, ld < n_channels, n_channels > 65535.  The number of frames, or DSS_EINVAL (no
 * device needed). */
long long dss_contam_check_call(const dss_contam_params *p, long long n_rows, int ld, int n_channels);
/* Doubles of the result for n_channels channels, and (offsets != NULL) where n, shift, sa, saa, sb, sbb, sab start in it (no
 * device needed).  DSS_EINVAL for n_channels outside 1 .. 65535. */
long long dss_contam_result_size(const dss_contam_params *p, int n_channels, long long offsets[7]);
/* How a call on n_rows rows of n_channels channels is cut into workgroups, as the calls themselves decide it (no device needed):
 * plan = {frames W, tiles of 32 frames, chunks (the grid's x), tiles per chunk (the last chunk may hold fewer), lag groups Z (the
 * grid's z), lags per wave}.  Each workgroup (chunk, channel, lag group) walks its chunk's tiles with 4 x lags-per-wave lags in
 * registers.  Returns 0, or DSS_EINVAL for what dss_contam_check_call(p, n_rows, n_channels, n_channels) refuses. */
int dss_contam_plan(const dss_contam_params *p, long long n_rows, int n_channels, int plan[6]);
/* window: nperseg doubles (dss_amd.contamination.hamming_symmetric).  NULL on failure. */
dss_contam *dss_contam_create(const dss_contam_params *p, const double *window);
void dss_contam_destroy(dss_contam *h);
/* Host buffers.  keep_frames: W bytes, 0 drops the frame, or NULL for all frames (a HOST array in both forms).  Returns 0. */
int dss_contam_moments(dss_contam *h, const double *brain, long long n_rows, int ld, int C, const double *audio,
                       const unsigned char *keep_frames, double *out);
/* Device-resident: d_brain, d_audio and d_out are device pointers.  Returns once the launches are queued on hip_stream; one call
 * per handle may be in flight. */
int dss_contam_moments_dev(dss_contam *h, const double *d_brain, long long n_rows, int ld, int C, const double *d_audio,
                           const unsigned char *keep_frames, double *d_out, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 13 -- several decoders of Part 10 trained side by side: the folds of train_bidirectional_model.py:65-68 (one decoder per
 * held-out day), seeds, learning rates.  Batch size 1 is a property of one training run; the runs are independent.  A group is
 * n_models trainers of equal sizes, and a step is one trial for each of them in ONE set of Part 10's seven launches with a model
 * axis on the grid (csrc/dec_train.hip), so the serial chains of all models run at the same time on different compute units.
 * The arithmetic is Part 10's, shared term for term: after any sequence of steps, every model's loss, features, gradients,
 * square averages, parameters and packed copies are bit for bit those of a dss_dec_trainer given the same weights and the same
 * trials in the same order, whatever n_models is, wherever the model sits in the group and whatever the others do.
 * 1 <= n_models <= 64: with 64 models every serial workgroup of a launch is resident at once on 256 compute units; more models
 * are more groups.  Calls on one group are issued on one stream, or one after the other has finished.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_dec_group dss_dec_group;
/* One model's part of a step.  T == 0: the model sits the step out -- its parameters, square averages, gradients, packed copies,
 * workspace, the features of its last trial and its loss slot all stay as they were, and its pointers are not looked at.
 * Else Part 10's trial: device pointers d_frames (T, n_inputs), d_targets float32 (T, n_outputs), d_mask float32 (T, 2H) or NULL. */
typedef struct {
    const void *d_frames;
    int T;
    const float *d_targets;
    const float *d_mask;
    int apply_step;
    double lr, alpha, eps;
} dss_dec_group_trial;
/* The argument checks on their own (no device needed): Part 10's limits on the sizes, and 1 <= n_models <= 64. */
int dss_dec_group_check(int n_models, int n_inputs, int hidden_units, int n_outputs, int max_frames);
/* n_models times Part 10's device memory, plus the tables. */
dss_dec_group *dss_dec_group_create(int n_models, int n_inputs, int hidden_units, int n_outputs, int max_frames);
void dss_dec_group_destroy(dss_dec_group *g);
/* dss_dec_trainer_load / _read / _features / _publish for model m (0 <= m < n_models). */
int dss_dec_group_load(dss_dec_group *g, int m, const float *const *w);
int dss_dec_group_read(dss_dec_group *g, int m, int what, float *out);
int dss_dec_group_features(dss_dec_group *g, int m, int T, float *out);
int dss_dec_group_publish(dss_dec_group *g, int m, dss_dec *dec, void *hip_stream);
/* One step: trials is a HOST array of n_models entries, read before the call returns; the frames of all models have one dtype
 * (frames_are_f64).  d_losses is a device array of n_models float64; entry m is written only if trials[m].T > 0.  Seven launches
 * on hip_stream with no host synchronisation: the entries travel in a ring of eight page-locked tables, copied in stream order,
 * so steps may be enqueued back to back (the ninth step in flight waits for the first to finish).  DSS_EINVAL before any launch
 * for a model with T > 0 that has no parameters loaded, T < 0 or T > max_frames, null frames or targets on a model with T > 0, or
 * a call in which every T is 0. */
int dss_dec_group_step_dev(dss_dec_group *g, const dss_dec_group_trial *trials, int frames_are_f64, double *d_losses,
                           void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 14 -- the trainers' dropout masks drawn on the device (csrc/dropout.hip): the (T, H) / (T, 2H) multipliers that Parts 9, 10
 * and 13 take as d_mask, from a stateless counter-based generator, so that no mask is drawn on the host and uploaded.  A mask is a
 * pure function of (seed, draw, rows, width, p): it depends neither on the number of entries of a call, nor on an entry's place
 * among them, nor on the order of calls, and a run is reproducible from its seed with no generator state to keep.
 *
 * The definition.  The block function is Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2,
 * 3", SC'11): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments 0x9E3779B9 (k0), 0xBB67AE85 (k1); ten rounds, each
 *   (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
 * the key moved on by its increments after every round.  Known answers (counter / key -> block):
 *   00000000 x 4 / 00000000 x 2                               -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   ffffffff x 4 / ffffffff x 2                               -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *   243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0   -> d16cfe09 94fdcceb 5001e420 24126ea1
 * A mask of rows x width float32, row-major: element e = t * width + j takes word e & 3 of the block with counter
 * (lo32(e >> 2), hi32(e >> 2), lo32(draw), hi32(draw)) and key (lo32(seed), hi32(seed)); u = (float)(word >> 8) * 2^-24, exact in
 * float32; the element is scale if u >= p, else 0.0f.  scale is the caller's float32 1 / (float32)(1.0 - p), an IEEE division
 * done once on the host (2.0 at p = 0.5): the kernel only selects.  p == 0 is no mask at all (d_mask == NULL in Parts 9, 10, 13).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    float *d_mask;                  /* rows * width float32; 4-byte aligned (16-byte aligned masks are written in 16-byte stores) */
    int rows, width;                /* rows == 0 (or width == 0): the entry is left alone and its pointer is not looked at */
    unsigned long long seed, draw;
    float p, scale;
} dss_dropout_entry;
/* The argument checks on their own (no device needed).  DSS_EINVAL with the reason in dss_last_error() for n_entries outside
 * 1 .. 64, a NULL table, a negative size, and on an entry that is not empty: a null or not 4-byte aligned pointer, rows * width
 * >= 2^31, p outside (0, 1) (NaN included), a scale that is not positive and finite; and for a table whose entries are all empty. */
int dss_dropout_check(int n_entries, const dss_dropout_entry *e);
/* Fills the masks of entries[0 .. n_entries), a HOST array read before the call returns, in ONE launch on hip_stream (the entry is
 * blockIdx.y and travels with the kernel arguments); d_mask are device pointers.  No host synchronisation: calls may be enqueued
 * back to back.  Nothing outside [d_mask, d_mask + rows * width) is written.  What dss_dropout_check refuses is refused before any
 * launch. */
int dss_dropout_masks_dev(const dss_dropout_entry *entries, int n_entries, void *hip_stream);
/* The same masks, bit for bit, computed on the CPU (no device needed): d_mask are host pointers. */
int dss_dropout_masks_host(const dss_dropout_entry *entries, int n_entries);
/* Self-test of the block function on the CPU: out[4] = Philox4x32-10(counter[4], key[2]). */
int dss_selftest_philox(const unsigned *counter, const unsigned *key, unsigned *out);

/* ------------------------------------------------------------------------------------------------
 * Part 15 -- several detectors of Part 9 trained side by side: the day split of train_unidirectional_vad.py:81-93, seeds,
 * learning rates.  Batch size 1 is a property of one training run; the runs are independent.  A group is n_models trainers of
 * equal sizes, and a window is one window for each of them in ONE pair of Part 9's launches with a model axis on the grid
 * (csrc/vad_train.hip), so the serial workgroups of all models run at the same time on different compute units.  The arithmetic
 * is Part 9's, shared term for term: after any sequence of steps, every model's losses, gradients, square averages, parameters,
 * packed copies and carried state are bit for bit those of a dss_vad_trainer given the same weights and the same windows in the
 * same order, whatever n_models is, wherever the model sits in the group and whatever the others do.
 * 1 <= n_models <= 64; more models are more groups.  Calls on one group are issued on one stream, or one after the other has
 * finished.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_vad_group dss_vad_group;
/* One model's part of a step.  len == 0: the model sits the step out -- its parameters, square averages, gradients, packed
 * copies, workspace, carried state and loss slots all stay as they were, and its pointers are not looked at.  Else device
 * pointers as in Part 9: d_frames (len, n_inputs), d_targets uint8[len], d_mask float32 (len, H) or NULL, d_losses float64, one
 * slot per window of the model (dss_vad_group_window_dev: one; dss_vad_group_trial_dev: ceil(len / window)). */
typedef struct {
    const void *d_frames;
    const unsigned char *d_targets;
    const float *d_mask;
    double *d_losses;
    double lr, alpha, eps;
    int len, apply_step;
} dss_vad_group_trial;
/* The argument checks on their own (no device needed): Part 9's limits on the sizes, and 1 <= n_models <= 64. */
int dss_vad_group_check(int n_models, int n_inputs, int hidden_units, int max_window);
/* n_models times Part 9's device memory, plus the tables. */
dss_vad_group *dss_vad_group_create(int n_models, int n_inputs, int hidden_units, int max_window);
void dss_vad_group_destroy(dss_vad_group *g);
/* dss_vad_trainer_load / _read / _state / _publish for model m (0 <= m < n_models). */
int dss_vad_group_load(dss_vad_group *g, int m, const float *w_ih0, const float *w_hh0, const float *b_ih0, const float *b_hh0,
                       const float *w_ih1, const float *w_hh1, const float *b_ih1, const float *b_hh1,
                       const float *cls_w, const float *cls_b);
int dss_vad_group_read(dss_vad_group *g, int m, int what, float *out);
int dss_vad_group_state(dss_vad_group *g, int m, float *h, float *c, int set);
int dss_vad_group_publish(dss_vad_group *g, int m, dss_vad *v, void *hip_stream);
/* Both step functions: trials is a HOST array of n_models entries, read before the call returns; the frames of all models have
 * one dtype (frames_are_f64).  Launches on hip_stream with no host synchronisation: the entries travel in a ring of eight
 * page-locked tables, copied in stream order, so steps may be enqueued back to back (the ninth step in flight waits for the
 * first to finish).  DSS_EINVAL before any launch, with a message that names the model, for a model with len > 0 that has no
 * parameters loaded, len < 0, null frames, targets or losses on a model with len > 0, and for a call in which every len is 0.
 *
 * dss_vad_group_window_dev: one window for each model, len <= max_window frames, from the model's carried state (no reset), as
 * dss_vad_trainer_window_dev; apply_step is honoured; the loss goes to d_losses[0].  Also refuses len > max_window. */
int dss_vad_group_window_dev(dss_vad_group *g, const dss_vad_group_trial *trials, int frames_are_f64, void *hip_stream);
/* dss_vad_group_trial_dev: one trial for each model, as dss_vad_trainer_trial_dev: the carried state of every model with
 * len > 0 is zeroed (one launch), then window w = 0, 1, ... of every model is stepped by one pair of launches -- frames
 * w * window .. of its trial, the last window being the remainder -- until the longest trial has run out; a model whose trial
 * is over is left alone by the later pairs.  Window w's loss goes to d_losses[w]; apply_step is taken as 1.  Also refuses a
 * window outside 1 .. max_window.  Returns the number of pairs launched, max over the models of ceil(len / window). */
int dss_vad_group_trial_dev(dss_vad_group *g, const dss_vad_group_trial *trials, int window, int frames_are_f64, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 16 -- LPC feature encoder: the `lpc_coefficients` of a training corpus (prepare_corpus.py:55-76 runs xiph's
 * LPCFeatureEncoder over every trial's int16 audio, LPCNet.pyx:65-87).  The method here is THIS PROJECT'S STATEMENT of the
 * published encoder (the binding definition is tests/feature_encoder_reference.py); parity with xiph's code
 * is not pinned, no copy of it being at hand.  Per 160-sample frame 36 float32 values: 18 Bark cepstral coefficients, the pitch
 * feature (18) and correlation (19) as the decoder of Part 1 reads them, and the 16 LPC taps (20..35) the decoder derives from
 * that cepstrum (the same device code).  One fresh encoder per trial; a whole trial list runs in three launches on one stream
 * with no host synchronisation between them (csrc/feature_encoder.hip).  No LPCNet model is needed.
 *
 * A trial list is an int16 concatenation and n_trials + 1 ascending offsets (a HOST array; what session_trial_audio
 * returns): trial i is samples offsets[i] .. offsets[i + 1] and gives (offsets[i + 1] - offsets[i]) / 160 frames; a trial
 * shorter than 160 samples gives none.  Audio that arrives in pieces, and the xiph encoder symbols of Part 1, go through the
 * state-carrying form of Part 18, which gives these bits for any chunking.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_fenc dss_fenc;
dss_fenc *dss_fenc_create(void);
void dss_fenc_destroy(dss_fenc *f);
/* Pure host function: out[0 .. n_trials] = the first output frame of every trial and, last, the total, which is also
 * returned (out may be NULL).  DSS_EINVAL for a negative first offset or offsets that decrease. */
long long dss_fenc_frame_offsets(const long long *offsets, int n_trials, long long *out);
/* Host buffers: audio int16[n], out36 float32 (total frames, 36).  Returns the total number of frames.  An empty list
 * (n_trials == 0) or one without a whole frame is a no-op that returns 0.  DSS_EINVAL, before anything is launched, for
 * offsets that decrease or run past n. */
long long dss_fenc_features_trials(dss_fenc *f, const short *audio, long long n, const long long *offsets, int n_trials,
                                   float *out36);
/* The same on device-resident audio and output (offsets stays a host array, read before the call returns), launched on
 * hip_stream; the results are complete when the stream reaches the end of the call's work. */
long long dss_fenc_features_trials_dev(dss_fenc *f, const short *d_audio, long long n, const long long *offsets, int n_trials,
                                       float *d_out36, void *hip_stream);
/* The score scratch of the last call, for tests: (2 * total frames, 256) float64, row s = sub-frame s of the list; columns
 * 0 .. 254 are the damped normalised cross-correlations at lag 256 - column, column 255 (lag 1, which nothing reads) holds the
 * sub-frame's normalised weight.  n must be the number of values; waits for the call's stream.  Returns the number of rows. */
long long dss_fenc_tap_scores(dss_fenc *f, double *out, long long n);
/* Development timing (tools/time_feature_encoder.py): with `on`, every later call records events around its three launches
 * (no host synchronisation); dss_fenc_kernel_ms waits for the last timed call and returns the device time in ms of launch
 * `which`: 0 spectrum / cepstrum / LPC, 1 residual and scores, 2 pitch track.  Negative when there is no timed call. */
int dss_fenc_enable_timing(dss_fenc *f, int on);
double dss_fenc_kernel_ms(dss_fenc *f, int which);

/* ------------------------------------------------------------------------------------------------
 * Part 17 -- the models of a group of trainers (Parts 13 and 15) over one trial list: Part 8's forward calls with a model per
 * trial, so that the validation passes of M models trained side by side are one set of launches and not M.  d_frames, first and
 * len are Part 8's (checked by dss_trials_check; ranges may overlap, so the same trial may be listed once per model: a seed or
 * learning-rate sweep over one corpus); model is a HOST array, model[i] in [0, M), and a model may own no trial.  Outputs are
 * concatenated in LIST order whatever the models are, so Part 8's score functions (dss_vad_score_trials_dev,
 * dss_dec_mse_trials_dev) take them as they are.  Every trial starts from the zero state; there are no dropout masks.
 * The weights are the members' current ones, read in stream order behind any step enqueued on the same stream: nothing is
 * published, no inference handle is involved, and nothing of the members -- gradients, square averages, workspaces, carried
 * state -- is written.  A trial's outputs are bit-identical to Part 8's on an inference handle that holds that member's weights.
 * Refused with a message: a NULL group and, unless the list is empty, NULL frames, outputs or model; a model index out of
 * range; a member named by the list without parameters loaded; a decoder trial starting behind row 2^31 - 1.  An empty list
 * returns DSS_OK and launches nothing.  On one group, trial-list calls are issued on one stream, or one after the other has
 * finished: the group keeps the call's tables.
 * ---------------------------------------------------------------------------------------------- */
/* The detectors (csrc/vad_lstm.hip): one launch, a workgroup per trial, longest first across all models.  d_labels
 * int32[sum len]; d_logits float32[sum len][2] or NULL. */
int dss_vad_group_forward_trials_dev(dss_vad_group *g, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                                     const long long *first, const int *len, const int *model,
                                     int *d_labels, float *d_logits /* or NULL */, void *hip_stream);
/* The decoders (csrc/bilstm_decoder.hip): d_feats float32[sum len][n_outputs].  The layer outputs go to two buffers of
 * min(sum len, max_rows) rows of 2H floats that the group owns and grows on demand; a list of more frames runs as several sets
 * of three launches, cut at trial borders in list order, and a single trial longer than max_rows is refused.  max_rows == 0:
 * 2^19 rows.  A trial's length is not bound by the group's max_frames: the trainers' workspaces are not used. */
int dss_dec_group_forward_trials_dev(dss_dec_group *g, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                                     const long long *first, const int *len, const int *model, long long max_rows /* 0: default */,
                                     float *d_feats, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Part 18 -- the LPC feature encoder of Part 16 on streams: n_streams encoders whose state is carried from push to push, for
 * audio that arrives in packets (a microphone beside 40 ms ECoG packets delivers 4 frames a packet) and for the xiph encoder
 * symbols of Part 1.  The method is causal -- frame i reads samples up to 160 i + 159 -- so ANY chunking of a stream gives,
 * bit for bit, the 36 values Part 16 gives on the whole signal as one trial.  Per stream the handle keeps on the device 480 raw
 * samples, the taps of the two newest frames, the pitch track's state and a frame counter (about 3 KB); a fresh or reset
 * stream is the all-zero state.  A push is ONE launch, a workgroup per stream, whatever the numbers of streams and frames
 * (csrc/feature_encoder_stream.hip); scores never reach global memory, and there is no tap function for this path.
 *   A push takes audio int16 (n_streams, 160 frames_max) and counts, a HOST int[n_streams] or NULL (every stream takes
 * frames_max): stream s encodes its first counts[s] frames, 0 <= counts[s] <= frames_max; a count of 0 lets the stream sit the
 * push out and leaves its state untouched.  out36 is float32 (n_streams, frames_max, 36); rows past a stream's count are written
 * as zeros.  Returns the number of frames encoded.  frames_max == 0, or all counts 0, is a no-op that returns 0 and writes
 * nothing.  Refused with a message before any launch: a NULL handle or NULL buffers, n_streams < 1, frames_max < 0 (or beyond
 * 2^31 / 320), a count out of range, a stream index out of range in a reset.  On one handle, calls are issued on one stream, or
 * one after the other has finished.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dss_fenc_streams dss_fenc_streams;
dss_fenc_streams *dss_fenc_streams_create(int n_streams);
void dss_fenc_streams_destroy(dss_fenc_streams *h);
/* The argument checks of a push on their own (no device needed): the number of frames it would encode, or DSS_EINVAL. */
long long dss_fenc_streams_check(int n_streams, int frames_max, const int *counts /* or NULL */);
/* The listed streams (a HOST int[n]; NULL: all of them) back to the fresh state, in stream order on hip_stream. */
int dss_fenc_streams_reset(dss_fenc_streams *h, const int *streams /* or NULL */, int n, void *hip_stream);
/* Host buffers; complete on return. */
long long dss_fenc_streams_push(dss_fenc_streams *h, const short *audio, int frames_max, const int *counts /* or NULL */,
                                float *out36);
/* The same on device buffers, launched on hip_stream with no host synchronisation; counts is read before the call returns. */
long long dss_fenc_streams_push_dev(dss_fenc_streams *h, const short *d_audio, int frames_max, const int *counts /* or NULL */,
                                    float *d_out36, void *hip_stream);
/* out[s] = frames stream s has encoded since its reset (host bookkeeping: includes pushes still queued). */
int dss_fenc_streams_frames_seen(dss_fenc_streams *h, long long *out);

#ifdef __cplusplus
}
#endif
#endif /* DSS_HIP_H */
