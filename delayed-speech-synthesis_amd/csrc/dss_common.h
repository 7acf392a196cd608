// csrc/dss_common.h -- shared host/device declarations of libdss_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>

#include "../../include/dss_hip.h"
#include "../../include/dss_lpcnet_blob.h"

// ---- fixed architecture constants of the path (checked against the blob at load) ----
#define DSS_NB_FEATURES 20
#define DSS_NB_BANDS 18
#define DSS_LPC_ORDER 16
#define DSS_FRAME_SIZE 160
#define DSS_GRU_A 384
#define DSS_GRU_B 16
#define DSS_FC_OUT 256
#define DSS_COND_STRIDE (3 * DSS_GRU_A + 3 * DSS_GRU_B + DSS_LPC_ORDER)   // 1216 floats per frame
#define DSS_FEATURES_DELAY 2
// Capacities of the CU-resident sample-rate kernel (lpcnet_sample.hip).  Row groups with more z/r blocks than their
// wave has register slots keep the surplus ("tail", in idx order behind the register slots) as LDS records next to the
// h-gate image, and h lists longer than DSS_HCX take the column ids of the further slots from LDS: slower per extra
// block, same results.  A model that exceeds the outer limits (DSS_ZR_TAIL, DSS_HX, or whose LDS image does not fit
// DSS_HBLK_BYTES) runs on the generic kernel instead.
#define DSS_ZRC 12            // register slots per lane for the z-gate and for the r-gate 8x4 blocks
#define DSS_HC 28             // h-gate slots per row group whose column ids sit in VGPRs (7)
#define DSS_ZR_TAIL 16        // max z (and r) blocks per row group beyond its wave's register slots
#define DSS_HCX 32            // ... in the instantiation with the extended paths (8 VGPRs)
#define DSS_HX 32             // max h-gate blocks per row group beyond DSS_HCX (column ids from LDS)
#define DSS_HBLK_BYTES 151552  // dynamic LDS left after the kernel's static 11.9 KB (160 KB per CU)
#define DSS_TANSIG_Y 208       // distance (floats) between the two halves of the activation table pair (lpcnet_device.h)

void dss_set_error(const char *fmt, ...);

#define DSS_HIP_CHECK(expr)                                                                        \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            dss_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return DSS_ENODEV;                                                                     \
        }                                                                                          \
    } while (0)

// ---- device-resident model (built once per loaded blob, per device) ---------------------------------
struct DssSparseGate {
    int slots;            // padded number of 8x4 blocks per unit for this gate
    const int *pos4;      // [slots][384]  byte offset (pos * 4) of the block's first input in the state vector
    const float *w;       // [slots][4][384]
};

struct DssModelDev {
    dss_blob_header h;
    // frame-rate network (input-major dense matrices, as in the blob)
    const float *embed_pitch, *conv1_w, *conv1_b, *conv2_w, *conv2_b, *dense1_w, *dense1_b, *dense2_w, *dense2_b;
    const float *gru_a_dense_w, *gru_a_dense_b, *gru_b_dense_w, *gru_b_dense_b;
    // sample-rate network
    const float *embed_sig, *embed_pred, *embed_exc;        // [256][1152]
    const float *embed_lane[3];   // the same three tables as [256][384 lanes][3 gates] in the fast kernel's lane order: one
                                  // 12-byte load per lane and table, 768 contiguous bytes per wave
    const float *gru_a_rbias, *gru_a_diag;                  // [1152]
    DssSparseGate gate[3];
    const float *gru_b_bias;                                // [2][48]
    const float *gru_b_w_in;                                // [384][48]
    const float *gru_b_w_rec;                               // [16][48]
    const float *fc_bias, *fc_w, *fc_factor;                // [512], [256][2][16], [512]
    // derived tables (host libm, see dss_lpcnet_model.cpp)
    const float *tansig;          // [201] y = tanh(.04 i) as tansig_table.h rounds it; [DSS_TANSIG_Y + i]: 1 - y*y (see lpcnet_device.h)
    const float *logit_table;     // [256]
    const float *ulaw2lin;        // [256]
    const float *dct_table;       // [18*18]
    const float *cos_table;       // [320]
    const float *cos_kl;          // [160][17] cos_table[(bin * lag) mod 320]: the inverse-DFT factor of every (bin, lag)
    const float *interp_a, *interp_b;   // [160] (1-frac), frac of interp_band_gain
    const int *interp_band;       // [160] band index i of each bin
    const double *lag_window;     // [17] 1 - 6e-5*i*i
    // register-resident layout of the sample-rate kernel (lpcnet_sample.hip)
    int fast_ok;                  // 1 when the model fits the capacities above
    int nzr_max;                  // max(z blocks, r blocks) over all row groups, rounded up to even (reporting)
    int zr_cap;                   // register slots per gate of waves 4, 5: 10 or 12 (selects the instantiation)
    int hmax;                     // max h blocks over all row groups (reporting)
    int ext;                      // 1 when the model uses z/r tails or h slots beyond DSS_HC (latency kernel only)
    int ext_tab;                  // float offset inside hblk of the tables the extended paths read (see dss_lpcnet_model.cpp)
    int hblk_floats;              // size of hblk
    const int *unit_of;           // [384] lane of waves 0..5 -> GRU A unit whose z and r chains it runs
    const int *unit_h;            // [384] lane of waves 0..5 -> GRU A unit whose h-gate chain it runs
    const int *wave_nh;           // [8]   per wave: h-gate slots (even), [6],[7] unused
    const int *grp_hoff;          // [48]  per (wave, lane / 8): float offset of that row group's block records inside hblk
    const int *wave_nzr;          // [8]   per wave: z/r register slots actually used (even)
    const int *wave_nzt;          // [8]   per wave: z/r tail slots (LDS records), max over its groups and both gates
    const float *zr_w;            // [2*DSS_ZRC][4][384] z then r block weights per lane slot, zero padded
    const unsigned *zr_col;       // [2*DSS_ZRC/4][384]  four 8-bit block column ids (pos/4) per word
    const unsigned *h_col;        // [DSS_HCX/4][384]    same for the h-gate slots of the lane's row group
    const float *hblk;            // LDS image: one list of [8 rows][4] records per row group, lists back to back (see dss_lpcnet_model.cpp)
    const float *gb_w_lane;       // [384][64] GRU B input weights, input-major, lane = row (rows 48..63 zero)
    const float *fc_w_pair;       // dual-FC weights as [k 8][node 256][4]: (layer 0, layer 1) weights of inputs 2k, 2k+1 (pair kernel)
    const float *gb_w_quad;       // the same weights as [384/4][64 lanes][4 inputs]: one 16-byte load per lane and block of four inputs
};

// ---- per-batch device state ---------------------------------------------------------------------------
struct DssBatchDev {
    int max_utts, max_frames;
    // decoder state, one row per utterance
    float *gru_a_state;   // [B][384]
    float *gru_b_state;   // [B][16]
    float *last_sig;      // [B][16]
    int *last_exc;        // [B]
    float *deemph;        // [B]
    uint32_t *rng;        // [B][4]
    int *frame_count;     // [B]
    float *conv1_mem;     // [B][2][84]
    float *conv2_mem;     // [B][2][128]
    float *old_lpc;       // [B][2][16]   row 0 = older (old_lpc[1]), row 1 = newer (old_lpc[0])
    // per-call scratch of the frame-rate network
    float *in_buf;        // [B][F+2][84]
    float *c1_buf;        // [B][F+2][128]
    float *c2_buf;        // [B][F][128]
    float *d1_buf;        // [B][F][128]
    float *cond_buf;      // [B][F][128]
    float *lpc_buf;       // [B][F+2][16]
    float *frame_out;     // [B][F][DSS_COND_STRIDE]  gru_a_condition | gru_b_condition | lpc
    int *fc0;             // [B] frame_count at the start of the call
    // ragged / slot-indexed calls (NULL = row i continues slot i, every row has n_frames frames)
    const int *slot_of;   // [n] decoder slot continued by row i of the call
    const int *count_of;  // [n] frames of row i (<= n_frames of the call; 0 leaves the slot untouched)
    const int *row_of;    // [n] ragged calls with counts: row handled by the k-th workgroup (slot), longest rows first
    int utt0;             // first row of this launch of the one-utterance sample kernel (a call split over two launches)
    // trace (optional)
    float *trace_exc, *trace_pcm;   // [B][F*160]
    // teacher forcing (tests; honoured by the TRACE instantiations only): sample k of row u takes the excitation
    // force_exc[u*F*160 + k] instead of the sampled one, and the pre-threshold logits of all 255 tree nodes go to
    // trace_logits[(u*F*160 + k)*256 + node]
    const unsigned char *force_exc;
    float *trace_logits;
};

// kernels (defined in the .hip files)
int dss_launch_frame_network(const DssModelDev &m, DssBatchDev &b, const float *d_features, int n_utts, int n_frames,
                             int feat_stride, hipStream_t s);
// pair: 0 = choose (two utterances per workgroup when the call has more utterances than the chip has CUs), -1 = never,
// 2 = always (uniform calls of models that fit, see dss_pair_fits).
// frames_done != NULL: a progressive call (dss_lpcnet_batch_synthesize_ragged_progress_dev): d_pcm is the device view of
// fine-grained host memory, frames_done[row] counts the frames of each row already there; one utterance per workgroup, no trace.
int dss_launch_sample_network(const DssModelDev &m, DssBatchDev &b, int n_utts, int n_frames, short *d_pcm,
                              int trace, int pair, hipStream_t s, int *frames_done = nullptr);
int dss_launch_sample_network_pair(const DssModelDev &m, DssBatchDev &b, int n_utts, int n_frames, short *d_pcm, int trace,
                                   hipStream_t s);
int dss_pair_fits(const DssModelDev &m);
int dss_launch_sample_network_generic(const DssModelDev &m, DssBatchDev &b, int n_utts, int n_frames, short *d_pcm,
                                      int trace, hipStream_t s, int *frames_done = nullptr);
int dss_launch_exp10_selftest(const float *d_x, const float *d_comp, float *d_out, long n, hipStream_t s);
int dss_launch_lin2ulaw_selftest(unsigned start, unsigned stride, long n, unsigned char *d_out, hipStream_t s);
int dss_launch_tansig_selftest(const float *d_tab, int which, unsigned start, unsigned long long n, unsigned long long *d_res, hipStream_t s);
int dss_launch_lpcnet_reset(const DssModelDev &m, DssBatchDev &b, int utt, hipStream_t s);

// ---- speech-segment gate (speech_gate.hip) ---------------------------------------------------------------
#define DSS_GATE_STATE_INTS 8     // sm_write, sm_read, hist_write, speech_count, future_count, mask_lo, mask_hi, frames_seen
struct DssGateDev {
    int S, C;
    int sm_ctx, sm_size;          // smoothing context frames, window = 2*ctx+1 (<= 64)
    int hist_size, hist_ctx;      // segment ring length, context frames kept on both sides of a speech run
    int max_events;               // segments one stream can complete in one push
    double threshold;             // proportion of speech labels in the window that makes a frame speech
    float *sm_buf;                // [S][sm_size][C]
    float *hist;                  // [S][hist_size][C]
    float *seg_out;               // [S][max_events][hist_size][C] completed segments of the last push
    int *state;                   // [S][DSS_GATE_STATE_INTS]
    int *events;                  // [S][2 + max_events]: n_events, n_speech_labels, lengths
};
int dss_launch_gate(const DssGateDev &g, const double *d_frames, const int *d_labels, int W, hipStream_t s);
#define DSS_GATE_COLLECT_MAX 64
struct DssGateCollect { int stream[DSS_GATE_COLLECT_MAX], event[DSS_GATE_COLLECT_MAX], dst_row[DSS_GATE_COLLECT_MAX]; };
int dss_launch_gate_collect(const DssGateDev &g, const DssGateCollect &a, int n, float *d_dst, long dst_row_floats, hipStream_t s);
int dss_launch_gate_reset(const DssGateDev &g, int stream, hipStream_t s);

// ---- neural voice-activity detector (vad_lstm.hip) -----------------------------------------------------------
#define DSS_VAD_MAXH 160          // capacities of the kernels, checked when a handle is created
#define DSS_VAD_MAXC 128
#define DSS_DEC_MAXH 128
#define DSS_DEC_MAXC 256
#define DSS_DEC_MAXO 32
struct DssVadDev {
    int S, C, H;                  // streams, inputs per frame, hidden units (two LSTM layers, two classes)
    const float *wT0;             // [(Cp + Hp) / 4][4H][4]: weight_ih_l0 then weight_hh_l0, four consecutive inputs of a row side by
                                  //   side, input counts padded to multiples of 4 (gate order i, f, g, o)
    const float *b0;              // [4H]  bias_ih_l0 + bias_hh_l0
    const float *wT1;             // [2 Hp / 4][4H][4]: weight_ih_l1 then weight_hh_l1
    const float *b1;              // [4H]
    const float *wc, *bc;         // classifier [2][H], [2]
    float *h, *c;                 // [2 layers][S][H] each
};
int dss_launch_vad(const DssVadDev &v, const void *d_frames, int frames_f64, int W, int *d_labels, float *d_logits, hipStream_t s);
// trial lists (Part 8): one table entry and one workgroup per trial, in table order: rows in_row .. in_row + len of the (N, C)
// frames go to rows out_row .. of the concatenated outputs; v.h / v.c are neither read nor written
// (model: the member that runs the trial in the group form below; the single-model path writes 0)
struct DssVadTrialDesc { long long in_row, out_row; int len, model; };
int dss_launch_vad_trials(const DssVadDev &v, const void *d_frames, int frames_f64, const DssVadTrialDesc *d_desc, int n_trials, int *d_labels,
                          float *d_logits, hipStream_t s);
// up to DSS_TRIAL_CHUNK consecutive trials of a concatenated (sum len, ...) array, handed to a reduction kernel by value: trial
// first_trial + k covers rows base + sum(len[:k]) .. + len[k]
#define DSS_TRIAL_CHUNK 256
struct DssTrialLens { long long base; int first_trial, n; int len[DSS_TRIAL_CHUNK]; };
int dss_launch_vad_score_trials(const DssTrialLens &tl, const float *d_logits, const int *d_labels, const unsigned char *d_targets,
                                double *d_loss, int *d_correct, float *d_prob, hipStream_t s);

// ---- training of the neural detector (vad_train.hip; Part 9) -------------------------------------------------
#define DSS_VAD_TRAIN_MAXT 4096   // largest max_window of a trainer (the workspace takes about 22 H + C floats per frame)
struct DssVadTrainDev {
    DssVadDev v;                  // S = 1.  What the forward half reads: the packed copies below; wc / bc point into p; h / c are the
                                  //   carried state, [2 layers][H] each
    int Tmax;                     // max_window: the rows of the workspace
    float *p, *g, *sq;            // master parameters (torch layout), gradients of the last window, RMSprop square averages: flat, the
                                  //   ten tensors in state_dict order (dss_vad_trainer_read)
    float *wT0, *b0, *wT1, *b1;   // the packed copies (v.wT0 ...), writable: the step kernel refreshes them
    // workspace of one window.  The forward pass leaves: the frames as float32; per layer the gate activations i, f, g, o and
    // c and h with one row in front (row 0 = the window's initial state, row t + 1 = after frame t); layer 0's masked output
    float *xs;                    // [Tmax][C]
    float *act0, *act1;           // [Tmax][4H]
    float *c0, *c1, *h0, *h1;     // [Tmax + 1][H]
    float *h0m;                   // [Tmax][H]
    float *logit, *dl;            // [Tmax][2]: logits; (softmax - onehot) / T
    double *lossf;                // [Tmax]: per-frame cross-entropy
    // ... and the backward pass: the gate gradients, and what layer 1 sends to layer 0's h (through W_ih_l1 and the mask)
    float *dg0, *dg1;             // [Tmax][4H]
    float *dh0m;                  // [Tmax][H]
};
long dss_vad_train_param_count(int C, int H);
// one window: loss, gradients (d.g), the carried state advanced; parameters, square averages and packed copies updated if apply_step
int dss_launch_vad_train_window(const DssVadTrainDev &d, const void *d_frames, int frames_f64, int T, const unsigned char *d_targets,
                                const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss, hipStream_t s);

// ---- several detector trainers of equal sizes stepped by one pair of launches per window (vad_train.hip; Part 15) ----------
#define DSS_VAD_GROUP_MAXM 64     // M serial workgroups of 640 threads in the window launch: a quarter of the 256 CUs
struct DssVadGroupTrial {         // one model's entry of a step's trial table (64 bytes); len == 0: the model sits the step out
    const void *frames;           // (len, C) float32 or float64 (one dtype per step)
    const unsigned char *targets; // [len] 0 / 1
    const float *mask;            // (len, H) or NULL
    double *losses;               // window w's loss goes to losses[w]
    double lr, alpha, eps;
    int len, apply;
};
// A trial step of M trainers on one stream: d_models[M] and d_trials[M] are device tables.  Windows w = 0 .. n_windows - 1 of
// `window` frames each: model m's window w is frames w * window .. of its trial, min(window, len_m - w * window) of them, and a
// model whose trial has run out (or with len == 0) is left alone.  reset != 0: the carried (h, c) of every model with len > 0 is
// zeroed first, by one launch.
int dss_launch_vad_train_group(const DssVadTrainDev *d_models, const DssVadGroupTrial *d_trials, int M, int C, int H, int n_windows,
                               int window, int reset, int frames_f64, hipStream_t s);
// a trial list over the members of a group (Part 17; vad_lstm.hip): as dss_launch_vad_trials, but trial k runs on the packed
// copies of d_models[d_desc[k].model] (the members' current weights: what their trainers' forward halves read); nothing of a
// member is written
int dss_launch_vad_trials_group(const DssVadTrainDev *d_models, int C, int H, const void *d_frames, int frames_f64,
                                const DssVadTrialDesc *d_desc, int n_trials, int *d_labels, float *d_logits, hipStream_t s);

// ---- bidirectional recurrent decoder (bilstm_decoder.hip) ----------------------------------------------------
struct DssDecDev {
    int S_max, T_max, C, H, O;    // capacity (streams x frames per call), inputs per frame, hidden units per direction, outputs (20)
    const float *wT[2][2];        // [layer][direction]: [(Cin_p + Hp) / 4][4H][4]: weight_ih then weight_hh, four consecutive inputs of
                                  //   a row side by side, input counts padded to multiples of 4 (Cin = C, then 2H; gate order i, f, g, o)
    const float *b[2][2];         // [4H]  bias_ih + bias_hh
    const float *wr, *br;         // regressor [O][2H], [O]
    float *mid, *top;             // [S_max][T_max][2H] each: the outputs of layer 0 / layer 1 (forward | backward)
};
// d_counts (frames per stream, <= T), d_in_row (input row of stream s in a buffer of Tin frames per row): device arrays or NULL
int dss_launch_decoder(const DssDecDev &d, const void *d_frames, int frames_f64, int S, int T, float *d_feats,
                       const int *d_counts, const int *d_in_row, int Tin, hipStream_t s);
// trial lists (Part 8): S <= S_max trials whose frames start at rows d_first[s] of one (N, C) array and have d_counts[s] <= T
// frames; features of trial s go to rows d_out_row[s] .. of d_feats, the concatenated (sum len, O) output.  Device arrays.
int dss_launch_decoder_trials(const DssDecDev &d, const void *d_frames, int frames_f64, int S, int T, float *d_feats,
                              const int *d_counts, const int *d_first, const long long *d_out_row, hipStream_t s);
int dss_launch_dec_mse_trials(const DssTrialLens &tl, const float *d_feats, const float *d_targets, int n_outputs, double *d_mse,
                              hipStream_t s);

// ---- training of the decoder (dec_train.hip; Part 10) ---------------------------------------------------------
#define DSS_DEC_TRAIN_MAXT 4096   // largest max_frames of a trainer (the workspace takes about 34 H + C + 3 O floats per frame)
struct DssDecTrainDev {
    int C, H, O, Tmax;            // inputs per frame, hidden units per direction, outputs, max_frames: the rows of the workspace
    float *p, *g, *sq;            // master parameters (torch layout), gradients of the last trial, RMSprop square averages: flat, the
                                  //   eighteen tensors in state_dict order (dss_dec_trainer_read)
    float *wT[2][2], *b[2][2];    // [layer][direction]: the packed copies of DssDecDev, writable: the step kernel refreshes them
    // workspace of one trial.  A direction's stash is in ITS OWN time order: step s is frame s forward, frame T - 1 - s backward.
    // The forward pass leaves: the frames as float32; per (layer, direction) the gate activations i, f, g, o of every step and
    // c and h with one row in front (row 0 = zeros, row s + 1 = after step s); layer 0's masked output, layer 1's output
    float *xs;                    // [Tmax][C]
    float *act[2][2];             // [Tmax][4H]
    float *c[2][2], *h[2][2];     // [Tmax + 1][H]
    float *midm, *top;            // [Tmax][2H], by frame: forward | backward
    float *feat, *dfeat;          // [Tmax][O]: features; 2 (feat - target) / (T O)
    double *lossf;                // [Tmax]: per-frame sum of squared differences
    // ... and the backward pass, by frame: what the head sends to layer 1's h, the gate gradients, what layer 1 sends to layer 0's h
    float *dtop, *dmid;           // [Tmax][2H]
    float *dg[2][2];              // [Tmax][4H]
};
struct DssDecTrainOff { int wih[2][2], whh[2][2], bih[2][2], bhh[2][2], wr, br, total; };
long dss_dec_train_param_count(int C, int H, int O);
// one trial: loss, features (d.feat), gradients (d.g); parameters, square averages and packed copies updated if apply_step
int dss_launch_dec_train_trial(const DssDecTrainDev &d, const void *d_frames, int frames_f64, int T, const float *d_targets,
                               const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss, hipStream_t s);

// ---- several trainers of equal sizes stepped by one set of launches (dec_train.hip; Part 13) -------------------------------
#define DSS_DEC_GROUP_MAXM 64     // 3 x 64 workgroups of 512 threads in the widest serial launch: all resident on 256 CUs
struct DssDecGroupTrial {         // one model's entry of a step's trial table (64 bytes); T == 0: the model sits the step out
    const void *frames;           // (T, C) float32 or float64 (one dtype per step)
    const float *targets, *mask;  // (T, O); (T, 2H) or NULL
    double *loss;                 // where the model's loss goes
    double lr, alpha, eps;
    int T, apply;
};
// one step of M trainers: d_models[M] and d_trials[M] are device tables; max_T is the longest T of the step (>= 1)
int dss_launch_dec_train_group(const DssDecTrainDev *d_models, const DssDecGroupTrial *d_trials, int M, int C, int H, int O, int max_T,
                               int frames_f64, hipStream_t s);
// A trial list over the members of a group (Part 17; bilstm_decoder.hip), one set of three launches.  Stream slot s is one trial:
// frames in_row .. in_row + len of the (N, C) array, layer outputs at rows buf_row .. of the concatenated (rows, 2H) buffers
// mid / top, features at rows out_row .. of d_feats.  A layer workgroup runs the n <= W streams slot0 .. of ONE model (both
// directions: blockIdx.y); a regressor block takes the n <= DEC_RROWS buffer rows row0 .. of one model, whose first row lies in
// stream slot `slot` (the rows of a model's streams follow each other in slot order).  Device tables, read in table order.
#define DSS_DEC_RROWS 8           // rows of `top` per regressor block (bilstm_decoder.hip)
struct DssDecGroupStream { long long in_row, out_row, buf_row; int len, model; };
struct DssDecGroupWg { int model, slot0, n, pad; };
struct DssDecGroupBlock { long long row0; int model, slot, n, pad; };
static_assert(sizeof(DssDecGroupStream) == 32 && sizeof(DssDecGroupWg) == 16 && sizeof(DssDecGroupBlock) == 24,
              "the tables are copied to the device as they stand");
int dss_launch_decoder_trials_group(const DssDecTrainDev *d_models, int C, int H, int O, const void *d_frames, int frames_f64, int W,
                                    const DssDecGroupStream *d_streams, const DssDecGroupWg *d_wgs, int n_wgs,
                                    const DssDecGroupBlock *d_blocks, int n_blocks, float *d_mid, float *d_top, float *d_feats,
                                    hipStream_t s);
// the streams per layer workgroup that both trial-list forms choose for a list of S trials (dss_launch_decoder's rule)
static inline int dss_dec_streams_per_wg(int S) { return 2 * S <= 256 ? 1 : (S <= 256 ? 2 : 4); }

struct DssHgaDev {
    int S, C, fs, nsec;
    float wl, ws;
    int frame_length, overlap, cap_rows;
    double *zi;        // [S][2][8][2][C]
    double *rows;      // [S][cap_rows][C]
    double sos[2][8][6];
    const double *zs_mean, *zs_std;   // optional z-score of the frames, [C] each (device-resident entry points)
    int force_path;    // tests / A-B timing only: 0 choose, 1 hga_fused_kernel, 2 the three-launch form
};
// The LDS ring of hga_fused_kernel / hga_trials_kernel: a frame, one shift and one tile of DSS_HGA_TT steps (+ 2) of rows,
// rounded up to a multiple of 8; 16 columns of float64 per row.  The one-launch forms serve a window shape iff the ring fits
// DSS_HGA_RING_LIMIT bytes beside the kernels' static tiles.  dss_launch_hga, dss_launch_hga_trials and dss_hga_plan (which
// reports the decision without a device) all take it from here.
#define DSS_HGA_TT 64
#define DSS_HGA_RING_LIMIT (40 * 1024)
struct DssHgaRing { int rows; size_t bytes; bool fused; };
static inline DssHgaRing dss_hga_ring(int frame_length, int overlap)
{
    DssHgaRing r;
    r.rows = (frame_length + (frame_length - overlap) + DSS_HGA_TT + 2 + 7) & ~7;
    r.bytes = (size_t)r.rows * 16 * sizeof(double);
    r.fused = r.bytes <= DSS_HGA_RING_LIMIT;
    return r;
}
// d_data is (S, n, C)
int dss_launch_hga(const DssHgaDev &h, const double *d_data, int n, int row0, int zero_rows, int rows, int W, double *d_out,
                   int apply_log, hipStream_t s);
int dss_launch_hga_frontend(const double *d_raw, double *d_pre, int S, int n, int c_raw, int C, const int *src_col,
                            const int *grid_of, int n_grids, const int *comp_cols, const int *comp_off, hipStream_t s);
int dss_launch_hga_wire(const float *d_payload, double *d_rows, int S, int C, int n, hipStream_t s);
int dss_launch_hga_reset(const DssHgaDev &h, const double *d_zi_hg, const double *d_zi_fh, hipStream_t s);
// one launch for n_trials fresh-extractor trials that are row ranges of one (rows, C) device array; d_desc is the device copy of
// the descriptor table: trial i reads rows in_row .. in_row + n - 1, left-padded with zero_rows rows of zeros, and writes frames
// out_row .. out_row + W - 1
struct DssHgaTrialDesc { long long in_row, out_row; int n, W, zero_rows, pad; };
static_assert(sizeof(DssHgaTrialDesc) == 32, "the descriptor table is copied to the device as it stands");
int dss_launch_hga_trials(const DssHgaDev &h, const double *d_data, const DssHgaTrialDesc *d_desc, int n_trials, const double *d_zi_hg,
                          const double *d_zi_fh, double *d_out, int apply_log, int with_zscore, hipStream_t s);
// in place on (N, C) frames: the bad-channel patch (n_patches may be 0; d_single_rows: the frames of trials that emit one
// frame, which numpy sums as a contiguous row), then the z-score when zs_mean is not NULL
int dss_launch_hga_patch(double *d_frames, long N, int C, int n_patches, const int *dst_col, const int *nb_cols, const int *nb_off,
                         const long long *d_single_rows, long n_single, const double *zs_mean, const double *zs_std, hipStream_t s);
int dss_launch_hga_colstats(const double *d_frames, long N, int C, double *d_out, hipStream_t s);
int dss_launch_log_power(const double *d_data, int T, int C, int sr, float wl, float ws, int W, double *d_out,
                         int apply_log, hipStream_t s);
