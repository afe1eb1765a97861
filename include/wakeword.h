/*
 * wakeword.h -- C ABI of the MI355X (gfx950) wake-word inference path.
 *
 * Drop-in boundary for the reference's hot path (Socrates666/esp32-wake-word):
 *   audio window -> MFCC front-end -> xiaoa CNN (LightweightKWS) -> logit.
 * Everything here is plain C: pointers, sizes, status codes; no C++ or torch
 * types cross the boundary.  Device pointers are HIP device memory; `stream`
 * is a hipStream_t passed as void* (NULL = the legacy default stream).
 * Calls that take device pointers are stream-ordered, allocate nothing and
 * never block the host.  Errors are reported as wk_status codes, never aborts.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   - main/esp_mfcc/mfcc.h:10-17   extract_mfcc / free_mfcc / analyze_mfcc_range
 *                                  (identical signatures and ownership below)
 *   - ml_models/src/wakeModel.py:29-34  LightweightKWS.forward (wk_cnn)
 *   - ml_models/src/extract_mfcc.py:137-175  MFCC + CMVN front-end (wk_mfcc)
 *   - main/hello_world_main.cpp:183-267 / esp_wake_word_detector.cpp:154-228
 *     per-window MFCC -> model->run() -> sigmoid (wk_forward)
 */
#ifndef WAKEWORD_H_
#define WAKEWORD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WK_ABI_VERSION 1

typedef enum {
  WK_OK = 0,
  WK_ERR_INVALID_ARG = 1,   /* null pointer, bad size, unsupported parameter combo */
  WK_ERR_HIP = 2,           /* a HIP runtime call failed (see wk_last_error())     */
  WK_ERR_NO_MEMORY = 3,     /* device or host allocation failed                    */
  WK_ERR_UNSUPPORTED = 4,   /* valid request this build does not implement         */
  WK_ERR_DEVICE = 5         /* a kernel reported an internal protocol failure: the */
                            /* results of the launches it covers are invalid       */
} wk_status;

/* Front-end definitions. */
typedef enum {
  WK_MODE_TORCHAUDIO_CMVN = 0, /* mode B: extract_mfcc.py:137-175 (+ CMVN), out [13][63] */
  WK_MODE_ESP_MFCC = 1         /* mode A: esp_mfcc/mfcc.c:431-527, out [n_frames][13]     */
} wk_mode;

typedef enum { WK_DTYPE_F32 = 0, WK_DTYPE_I16 = 1, WK_DTYPE_I8 = 2 } wk_dtype;   /* sample / frame type */
/* CNN arithmetic.  FP32 = fp32 MFMA.  BF16 = bf16 convolutions (SURVEY
 * config 4), fp32 front-end/classifier.  INT8 = the device's esp-dl int8
 * network (power-of-2 per-tensor exponents of ml_models/xiaoa.info,
 * round-half-even requant; reproduces the xiaoa.info known-answer test
 * exactly; wk_set_quant runs it at another model's exponents, wk_calibrate
 * finds them): a device-faithful mode, run unfused after the fp32
 * front-end.  BF16X3 = fp32-grade convolutions on bf16 MFMA: activations and
 * weights split into bf16 hi + lo parts, products hi*hi + hi*lo + lo*hi
 * accumulated in fp32 (relative product error ~2^-16); same logit tolerance
 * as FP32.  Every precision runs in wk_forward and in wk_cnn. */
typedef enum { WK_PREC_FP32 = 0, WK_PREC_BF16 = 1, WK_PREC_INT8 = 2, WK_PREC_BF16X3 = 3 } wk_precision;

typedef struct {
  int32_t mode;            /* wk_mode                                               */
  int32_t precision;       /* wk_precision (front-end is always fp32)               */
  int32_t esp_dsp_packing; /* mode A only: 1 = emulate dsps_cplx2reC_fc32 packing    */
  int32_t device;          /* HIP device ordinal the handle binds to                */
  int32_t cmvn;            /* mode B only: 1 = normalize_mfcc('cmvn') (the training */
                           /* path, extract_mfcc.py:175), 0 = raw MFCC              */
} wk_config;

typedef struct wk_handle wk_handle;

/* Number of floats in the packed weight blob wk_create() expects:
 * conv_layers.0.weight [32][13][3], conv_layers.3.weight [64][32][3],
 * conv_layers.6.weight [128][64][3], classifier.0.weight [64][128],
 * classifier.2.weight [1][64] -- PyTorch state-dict layouts, concatenated. */
#define WK_NUM_WEIGHTS 40224

/* Fixed geometry of the xiaoa model (1 s @ 16 kHz). */
#define WK_WIN_SAMPLES 16000
#define WK_N_MFCC 13
#define WK_N_FRAMES_B 63

/* Create a handle on cfg->device.  `host_weights` (WK_NUM_WEIGHTS floats, host
 * memory) may be NULL for a front-end-only handle.  Replaces the reference's
 * `new dl::Model(...)` + weight load (hello_world_main.cpp:178). */
wk_status wk_create(const wk_config* cfg, const float* host_weights, wk_handle** out);
wk_status wk_destroy(wk_handle* h);

/* The fused kernel's two roles (front-end waves, CNN waves) hand clips over
 * through bounded spins, and the CNN role's waves (also behind wk_cnn)
 * synchronise through bounded spins; a spin that times out (a protocol
 * failure -- never expected) ends the launch with invalid logits instead of a
 * hung GPU, and raises a flag in a host-visible word of the handle.  This call synchronises
 * the handle's device, returns WK_ERR_DEVICE if any launch on the handle since
 * the last check raised it (flags in *flags_out, may be NULL; 0 = clean), and
 * clears it.  A wk_stream has its own word (its pushes' launches report there,
 * not to the handle's): wk_stream_push checks and clears it on every push. */
wk_status wk_check_device_errors(wk_handle* h, uint32_t* flags_out);

/* Front-end only.  d_audio: `batch` clips of `win_len` samples, clip i at
 * d_audio + i*clip_stride elements (dtype WK_DTYPE_F32 or WK_DTYPE_I16; i16 is
 * scaled by 1/32768 like torchaudio.load).  Mode B requires win_len == 16000
 * and writes CMVN'd features [batch][13][63]; mode A accepts win_len >= 320
 * (clip_stride may be smaller than win_len: overlapping sliding windows)
 * and writes [batch][n_frames][13] with n_frames = (win_len-320)/256+1. */
wk_status wk_mfcc(wk_handle* h, const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len,
                  int64_t clip_stride, float* d_feats, void* stream);

/* CNN only: d_feats [batch][13][63] -> d_logits [batch] (LightweightKWS.forward). */
wk_status wk_cnn(wk_handle* h, const float* d_feats, int64_t batch, float* d_logits, void* stream);

/* Fused hot path: audio -> logits [batch]; mode B only (the model's training
 * front-end).  d_feats_or_null, when given, receives the [batch][13][63]
 * features as well.  A handle may be used from several streams and host
 * threads: the INT8 / unfused path stages features in a per-handle workspace
 * (when d_feats_or_null is NULL) and orders its uses across streams with an
 * event; the fused path shares nothing between calls. */
wk_status wk_forward(wk_handle* h, const void* d_audio, int32_t dtype, int64_t batch, int32_t win_len,
                     int64_t clip_stride, float* d_logits, float* d_feats_or_null, void* stream);

/* ---- Dense sliding-window scan of long recordings ---------------------------
 * wk_scan scores every window of `n_rec` recordings of `n_samples` samples each
 * (recording r at d_audio + r*rec_stride elements; f32, or i16 scaled by
 * 1/32768).  Window w covers samples [w*hop, w*hop + 16000) of its recording;
 * W = (n_samples - 16000) / hop + 1 windows per recording (0 if n_samples <
 * 16000; trailing samples that complete no window are ignored; windows never
 * cross recordings).  The result for a window is what wk_forward gives for the
 * clip starting there: d_logits [n_rec][W], and the mode-B CMVN'd features
 * [n_rec][W][13][63] into d_feats_or_null when given.
 *
 * When hop is a multiple of 256 (the front-end's frame hop) frames 1..61 of a
 * window read only samples inside it, so they are frames of the recording
 * (global frame g = hop/256 * w + t) and are computed once; only frame 0 and
 * frame 62 (reflection at the window's own edges) are computed per window.
 * That path needs a caller-owned workspace: the frame store plus the features
 * of one chunk of windows.  wk_scan_workspace_bytes gives its size for
 * `windows_per_chunk` windows per chunk (0 = library default); wk_scan derives
 * the chunk size from workspace_bytes, and a workspace below the size for one
 * window per chunk is WK_ERR_INVALID_ARG.  Any other hop >= 1 (and a multiple
 * of 256 above 15616, where consecutive windows share no frame) is forwarded
 * to the wk_forward path per recording with clip_stride = hop -- bit-identical
 * to wk_forward; the workspace is unused and its size is 0.
 *
 * wk_scan is stream-ordered: it allocates nothing, never blocks the host and
 * issues all its launches to `stream` in order.  The shared-frame path touches
 * no handle state, so concurrent scans on several streams (each with its own
 * workspace) need no ordering.  A forwarded scan is a wk_forward call and
 * shares what wk_forward shares: on an INT8 (or unfused) handle it stages its
 * features in the handle's own workspace, whose uses the library orders across
 * streams with an event, so such scans serialise on the handle.  hop < 1, n_rec < 0, n_samples > 2^30,
 * n_rec > 1 with rec_stride < n_samples, or a null pointer with W > 0 give
 * WK_ERR_INVALID_ARG before any device work; W = 0 is WK_OK with no launches.
 * Handle requirements and the error word are wk_forward's / wk_cnn's. */
wk_status wk_scan_workspace_bytes(int64_t n_rec, int64_t n_samples, int32_t hop,
                                  int64_t windows_per_chunk /* 0 = library default */, size_t* bytes);
wk_status wk_scan(wk_handle* h, const void* d_audio, int32_t dtype, int64_t n_rec, int64_t n_samples,
                  int64_t rec_stride, int32_t hop, float* d_logits /* [n_rec][W] */,
                  float* d_feats_or_null /* [n_rec][W][13][63] */,
                  void* d_workspace, size_t workspace_bytes, void* stream);

/* Device-side synthetic clip generator: fills
 * d_out[count][n] with clips first..first+count-1 of the counter-based
 * generator keyed on `seed` (bit-compatible with oracle.synth_clips up to
 * libm rounding). */
wk_status wk_synth_clips(uint32_t seed, int64_t first, int64_t count, int32_t n, float* d_out, void* stream);

/* normalize_mfcc(mfcc, method) (extract_mfcc.py:47-88) on device:
 * d_in/d_out [batch][n_coef][n_time]; method 0 = 'standardization',
 * 1 = 'minmax', 2 = 'cmvn', 3 = passthrough. In-place allowed. */
wk_status wk_normalize(const float* d_in, float* d_out, int64_t batch, int32_t n_coef, int32_t n_time,
                       int32_t method, void* stream);

/* ---- Streaming -------------------------------------
 * A device ring of `capacity` samples (>= 16000 + hop) fed from host memory,
 * with ring_buffer.c:57-117's overwrite-oldest semantics (write_rinbuffer).
 * Window k covers stream samples [k*hop, k*hop + 16000) -- the device's
 * continuously re-scored 1 s window (esp_wake_word_detector.cpp:52-150 slides
 * it frame by frame).  wk_stream_push() appends n float samples, scores every
 * window the push completes (oldest first; windows whose start was already
 * overwritten are dropped, and when more than max_out complete only the
 * newest max_out are scored) with the fused path on the handle's device, and
 * returns their logits and end positions (samples since create/reset) in host
 * memory.  It blocks until the logits are on the host.  Not thread-safe per
 * stream object.  The ring lives in device memory behind a pinned host
 * staging ring; a push that completes windows is two launches and one wait:
 * a small kernel reads the samples pushed since the last such push across
 * PCIe into the device ring, then the fused kernel scores the windows from
 * HBM and writes the logits to pinned host memory (no copy commands). */
typedef struct wk_stream wk_stream;
wk_status wk_stream_create(wk_handle* h, int32_t hop, int32_t capacity, void* stream, wk_stream** out);
wk_status wk_stream_destroy(wk_stream* s);
wk_status wk_stream_reset(wk_stream* s);   /* forget history (post-detection reset, detector.cpp:249-256) */
wk_status wk_stream_push(wk_stream* s, const float* host_samples, int64_t n, float* out_logits, int64_t* out_end,
                         int32_t max_out, int32_t* n_out);

/* ---- The firmware's detector over an MFCC frame stream --
 * esp_wake_word_detector.cpp keeps the last 63 int8 MFCC frames of 13
 * coefficients (record_task :128-134 quantises each 20 ms frame with lroundf +
 * saturation; write_one_frame_mfcc_to_buffer / read_whole_mfcc_buffer :21-48
 * hand the detector the 63 newest frames, oldest first) and, per window,
 * applies its own CMVN (detect_task :179-211: mean and POPULATION std over the 63
 * frames, (v - mean) / (std + 1e-8), lroundf, saturate) before the int8 model.
 * wk_device_cmvn runs that CMVN for every window of a frame stream: d_frames
 * [n_frames][13] (WK_DTYPE_I8 = the firmware's int8 frames, or WK_DTYPE_F32 =
 * float MFCC frames, quantised first as record_task does); window w = frames
 * w .. w+62, n_frames - 62 windows (none if n_frames < 63).  Outputs (either may
 * be NULL, not both): d_out_i8 [w][63][13] -- the firmware's mfcc_cmvn_buffer --
 * and d_feats_or_null [w][13][63], the same integer values as floats in wk_cnn's
 * layout (feed it to a WK_PREC_INT8 handle for the device's int8 network:
 * dl::TensorBase::assign from exponent 0 to the input exponent -4 is x16 with
 * saturation, which is what WK_PREC_INT8 applies to its float input).
 * Bit-identical to the firmware's C loops (same fp32 summation order). */
wk_status wk_device_cmvn(const void* d_frames, int32_t dtype, int64_t n_frames, int8_t* d_out_i8,
                         float* d_feats_or_null, void* stream);

/* ---- The firmware record task's front (esp_wake_word_detector.cpp:52-150) ---
 * wk_record_front: the sample path of record_task (:102-121), integer-exact.
 * d_tdm holds 3*n_out 48 kHz TDM samples of 4 int16 channels (interleaved
 * CH0 MIC-L, CH1 AEC reference, CH2 MIC-R, CH3 unused; the firmware reads 960
 * of them = 3840 int16 per 20 ms frame); per TDM sample the mono mix
 * m = (int16_t)(((L<<6) + (AEC<<5) + (R<<6)) >> 7) keeps the low 16 bits of the
 * int32 sum as the firmware's cast does; then d_out16[j] =
 * (int16_t)((m[3j] + 2 m[3j+1] + m[3j+2]) >> 2) at 16 kHz (320 per frame).
 * Frames are independent of each other (960 = 3 x 320), so any run of frames
 * is one call.  d_out_f32_or_null receives d_out16 / 32768.  d_out16 can feed
 * wk_forward directly as WK_DTYPE_I16 (clip_stride = hop: sliding windows);
 * the esp-dl MFCC the firmware runs on it (:124-125) is third-party and absent.
 * Alignment: d_tdm 16 bytes, d_out16 4, d_out_f32 8. */
wk_status wk_record_front(const int16_t* d_tdm, int64_t n_out, int16_t* d_out16, float* d_out_f32_or_null,
                          void* stream);
/* record_task's frame quantisation (:128-131): d_out_i8[i] = saturate_int8(lroundf(d_mfcc[i])),
 * n_values = 13 x frames; the result feeds wk_device_cmvn as WK_DTYPE_I8. */
wk_status wk_quantize_frames(const float* d_mfcc, int64_t n_values, int8_t* d_out_i8, void* stream);

/* ---- CTC head (ml_models/ctc.py) -------------------------
 * GRU_CTC_Model (ctc.py:119-152) + its log-mel front-end (ctc.py:82-107) +
 * greedy decode (ctc.py:453-471).  The reference builds V from its corpus at
 * run time (ctc.py:261-278); here V is a parameter.  This build implements the
 * reference Config (ctc.py:21-40): hidden 128, 2 bidirectional GRU layers,
 * 80 mels, n_fft 400, hop 160.  A wk_ctc handle owns its activations
 * workspace: issue one handle's calls on one stream (or order them across
 * streams yourself); use one handle per stream for concurrent batches. */
typedef struct {
  int32_t vocab;    /* V, including <blank> = 0 and <unk> = 1                */
  int32_t hidden;   /* 128 */
  int32_t layers;   /* 2 */
  int32_t n_mels;   /* 80 */
  int32_t device;
  int32_t precision; /* 0: fp32 throughout; 1 (config 5 "fp16"): GEMM and
                        MFMA operands, activations between layers and the gate
                        pre-activations in fp16, fp32 accumulation; the gate
                        arithmetic, state update and front-end stay fp32 */
} wk_ctc_config;
typedef struct wk_ctc wk_ctc;

/* Floats in the weight blob: the GRU_CTC_Model state dict in its own order
 * (audio_encoder.{0,1}.{weight,bias}, gru.{weight_ih,weight_hh,bias_ih,bias_hh}
 * _l{0,1}[_reverse], output_layer.{weight,bias}), concatenated. */
int64_t wk_ctc_num_weights(const wk_ctc_config* cfg);
wk_status wk_ctc_create(const wk_ctc_config* cfg, const float* host_weights, wk_ctc** out);
wk_status wk_ctc_destroy(wk_ctc* c);
/* X1 extract_features: d_audio [batch] rows of float samples (row i at
 * d_audio + i*stride, n_valid samples each) zero-padded / trimmed to
 * n_samples (ctc.py:85-90, max_audio_length) -> d_feats [batch][T][80],
 * T = 1 + n_samples/160, ln(mel+1e-8) z-scored per utterance (ctc.py:95-104). */
wk_status wk_ctc_features(wk_ctc* c, const float* d_audio, int64_t batch, int32_t n_valid, int32_t n_samples,
                          int64_t stride, float* d_feats, void* stream);
/* X2 + X3: d_feats [batch][T][80] -> greedy CTC tokens d_tokens [batch][T]
 * (blank-free, repeats collapsed, padded with -1) and d_lengths [batch];
 * d_log_probs_or_null [batch][T][V] receives log_softmax when given.  The
 * handle's workspace grows on the first call with a larger batch*T. */
wk_status wk_ctc_forward(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T, float* d_log_probs_or_null,
                         int32_t* d_tokens, int32_t* d_lengths, void* stream);

/* X1 + X2 + X3 in one call (audio -> greedy tokens): the same result as
 * wk_ctc_features into a handle-owned buffer followed by wk_ctc_forward
 * without log-probs (ctc.py:82-107 then :148-152, :453-471).  In fp16 mode
 * (precision 1) with T >= 6 the z-score is not applied in place: the log-mel
 * kernel also leaves per-pass sums, a small kernel turns them into each
 * utterance's mean and 1/std, and the encoder applies them as it loads the
 * raw rows -- one read and one write of the [batch][T][80] features fewer.
 * The statistics then differ from wk_ctc_features' by float rounding, so a
 * token may differ only where two logits are within that noise.  An
 * utterance whose log-mel values are all equal (digital silence) is left
 * un-normalised (std = 0 exactly).  Workspace grows on first use. */
wk_status wk_ctc_transcribe(wk_ctc* c, const float* d_audio, int64_t batch, int32_t n_valid, int32_t n_samples,
                            int64_t stride, int32_t* d_tokens, int32_t* d_lengths, void* stream);

/* Stage timing for measurement (bench_ctc.py): while enabled, every stage of
 * wk_ctc_features / wk_ctc_forward is bracketed by a pair of HIP events on the
 * call's stream; wk_ctc_stage_times synchronises on them and returns, per
 * stage, the summed milliseconds and the number of timed launches since the
 * last wk_ctc_profile call (which clears them).  Off by default (no events). */
enum {
  WK_CTC_STAGE_LOGMEL = 0,  /* X1 log-mel (framing, FFT, power, mel, ln)            */
  WK_CTC_STAGE_ZSCORE,      /* X1 global z-score (wk_ctc_transcribe fp16: its statistics only) */
  WK_CTC_STAGE_ENCODER,     /* Linear 80->128 + LayerNorm + ReLU                    */
  WK_CTC_STAGE_PROJ0,       /* GRU layer 0 input projection (x W_ih^T, both dirs)   */
  WK_CTC_STAGE_GRU0,        /* GRU layer 0 recurrence (both directions)             */
  WK_CTC_STAGE_PROJ1,       /* GRU layer 1 input projection                         */
  WK_CTC_STAGE_GRU1,        /* GRU layer 1 recurrence                               */
  WK_CTC_STAGE_OUTPUT,      /* output layer + argmax (+ log_softmax when requested) */
  WK_CTC_STAGE_DECODE,      /* greedy CTC collapse                                  */
  WK_CTC_N_STAGES
};
wk_status wk_ctc_profile(wk_ctc* c, int32_t enable);
wk_status wk_ctc_stage_times(wk_ctc* c, double* ms_sum /* [WK_CTC_N_STAGES] */, int64_t* counts /* [WK_CTC_N_STAGES] */);

/* X3's per-frame argmax -- decode_predictions' `predictions` (ctc.py:454,
 * first maximum per frame), the frame tokens the greedy decode collapsed --
 * of the handle's last wk_ctc_forward: d_pred [batch][T] int32.  batch and T
 * must be that call's (else WK_ERR_INVALID_ARG); stream-ordered after it. */
wk_status wk_ctc_frame_argmax(wk_ctc* c, int64_t batch, int32_t T, int32_t* d_pred, void* stream);

/* What the z-score of the handle's last wk_ctc_transcribe was computed from,
 * when that call took the fused path (fp16 handle, T >= 6): the un-normalised
 * log-mel rows ln(mel + 1e-8) to d_raw_or_null [batch][T][80] and each
 * utterance's {mean, 1/std} ({0, 1} for std 0) to d_zs_or_null [batch][2],
 * copied stream-ordered after it.  batch and T must be that call's and the
 * call fused, else WK_ERR_INVALID_ARG (the message names the last call). */
wk_status wk_ctc_transcribe_stats(wk_ctc* c, int64_t batch, int32_t T, float* d_raw_or_null, float* d_zs_or_null,
                                  void* stream);

/* ---- CTC head: parameter gradients (the backward half of ctc.py:380-407) -----
 * fp32 handles only (precision 0; a precision-1 handle: WK_ERR_UNSUPPORTED
 * before any device work).  The function differentiated is the one the
 * handle's last training forward computed: with wk_ctc_forward_train, the one
 * wk_ctc_forward computes (the eval-mode module, as CTCModel.loss uses it);
 * dropout is off by default and on with wk_ctc_forward_train_dropout (below).
 * No optimiser step and no clipping are done here.
 *
 * wk_ctc_forward_train: d_feats [batch][T][80] -> d_log_probs [batch][T][V],
 * bit for bit wk_ctc_forward's fp32 log-probs (the same kernels), and keeps in
 * a handle-owned training workspace -- apart from wk_ctc_forward's, which it
 * leaves untouched, and grown on the first call with a larger batch*T -- what
 * the backward needs: the features, the encoder output, each GRU layer's gate
 * inputs x W_ih^T and outputs.  No tokens are decoded.
 *
 * wk_ctc_backward: d_dlogits [batch][T][V], the gradient at the logits (what
 * wk_ctc_loss writes to d_grad; frames past an input length carry 0 and are
 * still walked, as the reference runs the GRU over the padded length) ->
 * d_grads [wk_ctc_num_weights], the gradient of every parameter in
 * wk_ctc_create's blob order (a state dict and its gradient share one
 * layout), and d_grad_norm_or_null [1], the 2-norm of that blob accumulated
 * in double (what clip_grad_norm_ needs, ctc.py:401).  batch and T must be
 * those of the handle's last wk_ctc_forward_train (else WK_ERR_INVALID_ARG).
 * A caller whose upstream gradient G is on the log-probs lp converts it first:
 * dlogits = G - exp(lp) * sum_v G.
 *
 * Both are stream-ordered and do not synchronise with the host (but for the
 * workspace growth).  No floating-point atomics are used and every sum has a
 * fixed order: the same handle and inputs give the same bits.  The saved
 * activations belong to the handle: one stream per handle, and nothing else
 * between a forward_train and its backward may call forward_train on it.
 * Null pointers, batch or T <= 0, batch*T > 2^31 - 1: WK_ERR_INVALID_ARG before
 * any launch.  The workspace takes about 4 (7000 + V) bytes per row of batch*T. */
wk_status wk_ctc_forward_train(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T, float* d_log_probs,
                               void* stream);
wk_status wk_ctc_backward(wk_ctc* c, int64_t batch, int32_t T, const float* d_dlogits, float* d_grads,
                          float* d_grad_norm_or_null, void* stream);

/* ---- CTC head: train-mode dropout (ctc.py:131, :140; model.train(), ctc.py:382) ----
 * The reference's two dropouts, as masks that are generated and never stored.
 * Site 0 is the encoder's output after the ReLU, [batch*T][128] (nn.Dropout,
 * ctc.py:131); site 1 is GRU layer 0's output where it is layer 1's input,
 * [batch*T][256] (nn.GRU(dropout=), ctc.py:140; layer 0's own recurrence keeps
 * the undropped output).  An element is kept with probability 1 - p and then
 * multiplied by s = 1.0f / (1.0f - p) (computed in float), else set to 0.
 *
 * The mask is a function of (seed, offset, site, element) alone:
 * Philox4x32-10 (multipliers D2511F53, CD9E8D57; key increments 9E3779B9,
 * BB67AE85) with key = (seed low, seed high) and counter = (q low, q high,
 * offset low, offset high | site << 31), where element e = row * width + unit,
 * row = b * T + t, q = e / 4; element e takes output word e % 4 and is kept
 * iff word >= (uint32) floor((double) p * 2^32).  So offset must be < 2^63.
 * Use one offset per training forward (the step number) under one seed.
 *
 * wk_ctc_forward_train_dropout is wk_ctc_forward_train with the masks applied;
 * p = 0 turns a site off (no kernel runs and no buffer is allocated for it),
 * and with both at 0 it enqueues exactly what wk_ctc_forward_train does.  The
 * handle records *drop as the dropout of its last training forward (a plain
 * wk_ctc_forward_train records "none"), and wk_ctc_backward differentiates
 * that function, making the same masks again.  Site 1 takes a second
 * [batch*T][256] buffer, allocated on the first call with p_gru > 0 (the only
 * other time, besides the workspace growth, that a call may block the host).
 * seed and offset travel by value in the launch arguments: a captured graph
 * replays the same mask every time, so a step captured once does not draw new
 * masks -- re-capture, or leave dropout steps uncaptured.
 *
 * wk_ctc_dropout_masks makes the masks of the handle's last training forward
 * again as bytes (1 = kept), [batch*T][128] and [batch*T][256]; either pointer
 * may be NULL; a site that was off gives all ones.  For tests, and for
 * reproducing a step elsewhere.
 *
 * WK_ERR_INVALID_ARG before any device work: a null drop; a p that is
 * negative, >= 1 or NaN; offset >= 2^63; wk_ctc_forward_train's argument rules;
 * wk_ctc_dropout_masks before any training forward.  WK_ERR_UNSUPPORTED: a
 * precision-1 handle. */
typedef struct { float p_enc, p_gru; uint64_t seed, offset; } wk_ctc_dropout;   /* ctc.py:34: 0.2, 0.2 */
wk_status wk_ctc_forward_train_dropout(wk_ctc* c, const float* d_feats, int64_t batch, int32_t T,
                                       const wk_ctc_dropout* drop, float* d_log_probs, void* stream);
wk_status wk_ctc_dropout_masks(wk_ctc* c, uint8_t* d_mask_enc_or_null /* [batch*T][128] */,
                               uint8_t* d_mask_gru_or_null /* [batch*T][256] */, void* stream);

/* ---- CTC head: the optimiser (clip_grad_norm_ + optim.Adam; ctc.py:368, :401-402) ----
 * fp32 handles only (a precision-1 handle, and a handle created under
 * WAKEWORD_CTC_MIX, whose fp16 output weights would go stale:
 * WK_ERR_UNSUPPORTED from all five calls).  A handle keeps its weights as
 * per-tensor device buffers, some of them derived layouts of W_hh; these calls
 * change them in place, and when one returns every buffer an fp32 entry point
 * reads holds, stream-ordered, exactly what wk_ctc_create would have uploaded
 * for the current blob: wk_ctc_forward, wk_ctc_forward_train and
 * wk_ctc_backward all see the new weights.
 *
 * wk_ctc_adam_step, with g = d_grads [wk_ctc_num_weights] (wk_ctc_backward's
 * layout) and t = the handle's step count + 1, per element and in fp32:
 *   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1
 *   g = coef g + weight_decay p;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * (torch.optim.Adam without amsgrad, L2 weight decay; the bias corrections are
 * computed on the host in double).  norm is read on the device from
 * d_norm_or_null [1] (what wk_ctc_backward wrote), or, when that is NULL and
 * max_norm > 0, computed from d_grads by wk_ctc_backward's own norm kernel into
 * a handle-owned float: the same bits either way.  A non-finite norm propagates
 * as in clip_grad_norm_(error_if_nonfinite=False): inf gives coef 0 (and NaN
 * where a gradient is inf), NaN makes every weight NaN.  The moments and the
 * step count live in the handle, allocated and zeroed by the first
 * wk_ctc_adam_step or wk_ctc_set_optim_state (the only time a call may block
 * the host); nothing is allocated afterwards.  A step is a fixed number of
 * launches (Adam, the W_hh layouts, and the norm when it is not passed),
 * whatever V and the batch.  No atomics: every element is written by one
 * thread, so equal inputs give equal bits.  The step count is host state: a
 * captured graph must not contain wk_ctc_adam_step.  One stream per handle.
 *
 * wk_ctc_weights gathers the current weights into d_out [wk_ctc_num_weights]
 * (blob order); wk_ctc_set_weights scatters d_blob into the handle and rebuilds
 * the derived layouts (the optimiser state is left as it is).
 * wk_ctc_optim_state copies m and v (either may be NULL) and the step count out
 * (zeros and 0 before the first step); wk_ctc_set_optim_state copies them in,
 * NULL meaning zeros: (NULL, NULL, 0) resets the optimiser.
 * WK_ERR_INVALID_ARG before any device work: a null handle, opt, d_grads,
 * d_out or d_blob; lr negative or not finite; a beta outside [0, 1); eps <= 0;
 * weight_decay < 0; a NaN; a negative step. */
typedef struct { float lr, beta1, beta2, eps, weight_decay, max_norm; } wk_ctc_adam;   /* ctc.py:368,401: 1e-3, .9, .999, 1e-8, 0, 5 */
wk_status wk_ctc_weights(wk_ctc* c, float* d_out /* [wk_ctc_num_weights] */, void* stream);
wk_status wk_ctc_set_weights(wk_ctc* c, const float* d_blob, void* stream);
wk_status wk_ctc_adam_step(wk_ctc* c, const wk_ctc_adam* opt, const float* d_grads, const float* d_norm_or_null,
                           void* stream);
wk_status wk_ctc_optim_state(wk_ctc* c, float* d_m, float* d_v, int64_t* step, void* stream);
wk_status wk_ctc_set_optim_state(wk_ctc* c, const float* d_m_or_null, const float* d_v_or_null, int64_t step,
                                 void* stream);

/* ---- CTC loss and its gradient (nn.CTCLoss(blank=0); ctc.py:369, :380-425) ---
 * d_log_probs [batch][T][vocab] fp32 (the layout wk_ctc_forward writes),
 * d_labels [batch][label_stride] int32, d_input_lengths / d_label_lengths
 * [batch] int32 on the device: trusted to lie in [0, T] / [0, max_label_len]
 * and clamped to them.  Outputs: d_nll [batch], each utterance's negative
 * log-likelihood, and d_loss [1], their reduction: the sum (NONE and SUM; with
 * NONE the result proper is d_nll) or mean_b(nll_b / max(S_b, 1)) (MEAN).
 * d_grad_or_null [batch][T][vocab], when given, receives
 *   g[b,t,v] = exp(lp[b,t,v]) - exp(lse_{s: l'_s = v}(alpha_t(s) + beta_t(s)) + nll_b - lp[b,t,v])
 * (torch's native CTC backward: the gradient at the logits under log_softmax,
 * which also passes unchanged through log_softmax's backward), times
 * grad_scale, and with MEAN times 1 / (batch * max(S_b, 1)); exactly 0 at
 * t >= d_input_lengths[b].  An utterance without a valid alignment (T_b < S_b +
 * adjacent repeats, or a label outside [1, vocab), which is never used as an
 * index) has nll = +inf, or 0 with zero_infinity; its gradient rows are 0 and
 * the other utterances are unaffected.  fp32 arithmetic in log space; nothing
 * is accumulated by atomics, so equal inputs give equal bits.
 * Limits: max_label_len <= 255, vocab <= 65536, batch * T <= 2^28; beyond
 * them, and for a null pointer, batch, T or vocab <= 0, label_stride <
 * max_label_len or an unknown reduction: WK_ERR_INVALID_ARG before any device
 * work (wk_ctc_loss_workspace_bytes then returns 0).  Stream-ordered, no host
 * synchronisation; d_workspace (16-byte aligned, wk_ctc_loss_workspace_bytes)
 * is the caller's, so concurrent calls with workspaces of their own are safe. */
enum { WK_CTC_REDUCTION_NONE = 0, WK_CTC_REDUCTION_SUM = 1, WK_CTC_REDUCTION_MEAN = 2 };
int64_t wk_ctc_loss_workspace_bytes(int64_t batch, int32_t T, int32_t max_label_len);
wk_status wk_ctc_loss(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab,
                      const int32_t* d_labels, int32_t label_stride,
                      const int32_t* d_input_lengths, const int32_t* d_label_lengths,
                      int32_t max_label_len, int32_t reduction, int32_t zero_infinity, float grad_scale,
                      void* d_workspace, float* d_nll, float* d_loss, float* d_grad_or_null,
                      int32_t device, void* stream);

/* ---- CTC forced alignment (Viterbi): which frames a known transcript occupies --
 * Inputs as wk_ctc_loss: d_log_probs [batch][T][vocab] fp32, d_labels
 * [batch][label_stride] int32, d_input_lengths / d_label_lengths [batch] int32
 * on the device, clamped to [0, T] / [0, max_label_len].  Blank = 0; l' is the
 * label sequence interleaved with blanks, L = 2S+1 states, Tb the clamped
 * input length:
 *   a_0(0) = lp_0(0),  a_0(1) = lp_0(l'_1),  a_0(s >= 2) = -inf
 *   a_t(s) = lp_t(l'_s) + max(a_{t-1}(s), a_{t-1}(s-1), [a_{t-1}(s-2)])
 * in fp32 with plain IEEE adds, the third term only for a label state whose
 * label differs from the one two states back; score = max(a_{Tb-1}(L-1),
 * a_{Tb-1}(L-2)), and the path follows the back-pointers from that state.
 * Tie rule: among equal predecessors s, then s-1, then s-2 is preferred (a
 * candidate replaces the best so far only if strictly greater); at the exit
 * L-1, the trailing blank, when a(L-1) >= a(L-2).  max is exact and each add
 * rounds once, so every output is defined bit for bit by the recurrence.
 * Outputs:
 *   d_states [batch][T]                 the state index s_t in 0..2S; -1 at t >= Tb
 *   d_frame_tokens_or_null [batch][T]   l'_{s_t} (0 = blank); -1 where the state is
 *   d_frame_lp_or_null [batch][T]       lp_t(l'_{s_t}), the input's bits; 0 where the state is -1
 *   d_spans_or_null [batch][max_label_len][2]   label i occupies frames [start, end): the
 *                                       one contiguous run with s_t = 2i+1; -1, -1 for i >= S
 *   d_score [batch]                     the best path's log-probability
 * No alignment -- a label outside [1, vocab) (never used as an index), Tb < S +
 * the number of adjacent equal labels, Tb = 0, or every path through a -inf --
 * gives score -inf, every state, token and span -1 and every frame_lp 0; the
 * other utterances are unaffected.  S = 0: all blanks, state 0, the score is
 * the sum of the blank column.  On NaN input the outputs are unspecified but
 * every state stays in [0, L).
 * Limits and argument checks are wk_ctc_loss's (max_label_len <= 255, vocab <=
 * 65536, batch * T <= 2^28; null required pointers, non-positive sizes,
 * label_stride < max_label_len, a workspace not 16-byte aligned:
 * WK_ERR_INVALID_ARG before any device work; wk_ctc_align_workspace_bytes
 * returns 0 beyond the limits).  Stream-ordered, no host synchronisation, no
 * atomics; d_workspace is the caller's. */
int64_t wk_ctc_align_workspace_bytes(int64_t batch, int32_t T, int32_t max_label_len);
wk_status wk_ctc_align(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab,
                       const int32_t* d_labels, int32_t label_stride,
                       const int32_t* d_input_lengths, const int32_t* d_label_lengths, int32_t max_label_len,
                       void* d_workspace, int32_t* d_states, int32_t* d_frame_tokens_or_null,
                       float* d_frame_lp_or_null, int32_t* d_spans_or_null, float* d_score,
                       int32_t device, void* stream);

/* ---- CTC prefix beam search: the N best label sequences with their log-probabilities
 * d_log_probs [batch][T][vocab] fp32, blank = 0; beam width W = beam, per-frame
 * candidate count K = top_k; Tb is d_input_lengths_or_null[b] clamped to [0, T]
 * (null: all T).  A hypothesis is a label prefix l with two log-masses, pb for
 * the paths ending in blank and pnb for those ending in its last label e; its
 * total is p = lse(pb, pnb).  Start: the single hypothesis (), pb = 0, pnb =
 * -inf.  For each frame t < Tb, with row lp = log_probs[b, t, :]:
 *   candidates  C_t is the min(K, V-1) non-blank ids with the largest lp, ties to
 *               the lower id; compares only, so C_t is defined bit for bit.
 *   stay        every live (l, pb, pnb) in slot order contributes to l:
 *               pb' (+)= lp[0] + p, and if l is non-empty pnb' (+)= lp[e] + pnb
 *               (lp[e] is read from the row whether or not e is in C_t).
 *   extend      every live hypothesis in slot order, for c in C_t in ascending
 *               id, contributes to l + c: pnb' (+)= lp[c] + (pb if c == e else p).
 *   merge       (+) is log-add-exp; contributions to the same prefix merge.  The
 *               only possible merge is an extension (l_i, c) with the stay of a
 *               live l_j = l_i + c; identity is by prefix, exactly (never by a
 *               hash alone).
 *   prune       candidates whose total is -inf are dropped; the W largest
 *               totals survive, in descending order; equal totals keep
 *               candidate order (stays in slot order, then extensions by parent
 *               slot, then token id): a replacement must be strictly greater.
 * After frame Tb-1 the live hypotheses, in that order, are the result; for
 * i < n_best:
 *   d_tokens [batch][n_best][max_len]   the labels, -1 beyond the length
 *   d_lengths [batch][n_best]           the full length, even beyond max_len (the
 *                                       tokens are then the first max_len); -1 for a
 *                                       slot without a hypothesis
 *   d_scores [batch][n_best]            p, the total; -inf for an empty slot
 *   d_cand_or_null [batch][T][top_k]    C_t in selection order (descending lp);
 *                                       -1 at t >= Tb and beyond V-1 entries
 * Tb = 0 gives the single hypothesis () with score 0.  On NaN input the outputs
 * are unspecified, but nothing is read or written out of bounds and every
 * token stays in [-1, vocab).  Arithmetic is fp32, (+) with the device's exp and
 * log; every sum has one fixed order, so equal inputs give equal bits.
 * Limits: 1 <= beam <= 64, 1 <= top_k <= 32, 1 <= n_best <= beam, 2 <= vocab <=
 * 65536, batch * T <= 2^28, max_len >= 1.  Beyond them, or for a null required
 * pointer, a non-positive size or a workspace not 16-byte aligned:
 * WK_ERR_INVALID_ARG before any device work; wk_ctc_beam_workspace_bytes
 * returns 0.  Stream-ordered, no host synchronisation, no atomics; d_workspace
 * is the caller's. */
int64_t wk_ctc_beam_workspace_bytes(int64_t batch, int32_t T, int32_t beam, int32_t top_k);
wk_status wk_ctc_beam(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab,
                      const int32_t* d_input_lengths_or_null,
                      int32_t beam, int32_t top_k, int32_t n_best, int32_t max_len,
                      void* d_workspace, int32_t* d_tokens, int32_t* d_lengths, float* d_scores,
                      int32_t* d_cand_or_null, int32_t device, void* stream);

/* ---- CTC keyword spotting: is this word somewhere in the utterance, where, how sure
 * d_log_probs [batch][T][vocab] fp32, blank = 0; Tb is d_input_lengths_or_null[b]
 * clamped to [0, T] (null: all T).  Keyword k is d_keywords[k * keyword_stride
 * + 0..S-1] with S = d_keyword_lengths[k] clamped to [0, max_keyword_len]: labels
 * w_0..w_{S-1}, 1 <= S <= 32, each in [1, vocab).  Every (utterance, keyword)
 * pair is scored.  The keyword's lattice has L = 2S-1 states: even state j
 * emits w_{j/2}, odd state j emits blank; there are no outer blanks, so a span
 * is tight.  With g_t = max_v lp_t(v) when normalize != 0 (else g_t is not used):
 *   x_t(j) = lp_t(l_j)                                       normalize == 0 (the input's bits)
 *   x_t(j) = lp_t(l_j) == -inf ? -inf : lp_t(l_j) - g_t      normalize != 0 (one IEEE subtract)
 *   a_{-1}(j) = -inf
 *   a_t(0) = x_t(0) + max(a_{t-1}(0), 0)                     0: the keyword may start at any frame
 *   a_t(j) = x_t(j) + max(a_{t-1}(j), a_{t-1}(j-1), [a_{t-1}(j-2)])
 *                                 third term: j even, j >= 2, w_{j/2} != w_{j/2-1}
 *   e_t    = a_t(L-1)
 *   score  = max_{t < Tb} e_t
 * Every state carries the frame at which its best path entered state 0: an
 * entry at frame t carries t, any other move the chosen predecessor's value, a
 * state whose value is -inf carries -1.  Tie rule: a candidate replaces the
 * best so far only if strictly greater; candidates are tried in the order
 * stay, j-1, j-2 (at state 0: stay, then enter).  Over t the first frame that
 * attains the maximum wins, and span = [start carried by state L-1 at that
 * frame, that frame + 1).  max is exact and every add or subtract rounds once
 * in fp32, so every output is defined bit for bit by the recurrence, whatever
 * the lane layout.  With normalize every x <= 0 and the score is the best
 * log-ratio, over all segments, between the keyword's best path and the greedy
 * path on the same frames: 0 exactly where the greedy path spells the keyword,
 * and exp(score) is a confidence in (0, 1].
 * Outputs:
 *   d_scores [batch][n_keywords]                  the score
 *   d_spans [batch][n_keywords][2]                the span, frames [start, end)
 *   d_frame_scores_or_null [batch][n_keywords][T] e_t, -inf at t >= Tb: the trace a
 *                                                 streaming detector thresholds, and
 *                                                 from which further occurrences are read
 * No occurrence -- Tb < S + the number of adjacent equal labels, Tb = 0, a
 * keyword of length <= 0, a keyword with a label outside [1, vocab) (never used
 * as an index), or every path through a -inf -- gives score -inf and span
 * (-1, -1) (and a trace of -inf for an empty or invalid keyword); the other
 * pairs are unaffected.  On NaN input the outputs are unspecified, but every
 * span value stays in [-1, T].
 * Limits: 1 <= max_keyword_len <= 32, vocab <= 65536, batch * T <= 2^28, 1 <=
 * n_keywords, batch * n_keywords <= 2^24, keyword_stride >= max_keyword_len.
 * Beyond them, or for a null required pointer, a non-positive size, a workspace
 * not 16-byte aligned or device < 0: WK_ERR_INVALID_ARG before any device work;
 * wk_ctc_spot_workspace_bytes returns 0 beyond the limits.  The workspace holds
 * g [batch][T] and nothing per pair.  Stream-ordered, no host synchronisation,
 * no atomics (equal inputs give equal bits); d_workspace is the caller's. */
int64_t wk_ctc_spot_workspace_bytes(int64_t batch, int32_t T, int32_t n_keywords, int32_t max_keyword_len);
wk_status wk_ctc_spot(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab,
                      const int32_t* d_input_lengths_or_null,
                      const int32_t* d_keywords, int32_t keyword_stride, const int32_t* d_keyword_lengths,
                      int32_t n_keywords, int32_t max_keyword_len, int32_t normalize,
                      void* d_workspace, float* d_scores, int32_t* d_spans, float* d_frame_scores_or_null,
                      int32_t device, void* stream);

/* ---- Edit distance and error rates: how well the decoded hypotheses match the references
 * d_hyp [batch][n_hyp][hyp_stride] int32 hypotheses, d_ref [batch][ref_stride]
 * int32 references; pair (b, h) compares hypothesis h of utterance b with
 * reference b.  M is d_ref_lengths[b] clamped to [0, max_ref_len].  The
 * hypothesis and its length N depend on `collapse`:
 *   collapse == 0   the hypothesis is d_hyp[b][h][0..N), N = d_hyp_lengths[b *
 *                   n_hyp + h] clamped to [0, hyp_stride]: a beam slot's -1
 *                   becomes 0, a beam length beyond max_len the stored prefix
 *                   (wk_ctc_forward's d_tokens / d_lengths with n_hyp = 1,
 *                   wk_ctc_beam's with n_hyp = n_best).  d_hyp_lengths is required.
 *   collapse != 0   d_hyp[b][h][0..Tb) are per-frame labels (wk_ctc_frame_argmax's
 *                   output with hyp_stride = T), Tb = d_hyp_lengths[b * n_hyp + h]
 *                   clamped to [0, hyp_stride], all hyp_stride when the pointer is
 *                   null.  The hypothesis is the labels of the frames t with
 *                   label_t != 0 && label_t != label_{t-1} (label_{-1} = 0), the
 *                   greedy CTC collapse; N is their count.
 * Tokens are compared as int32 for equality only, never used as an index, and
 * nothing at or beyond a length is read into a result.
 * An alignment is a monotone path of three moves: match or substitute (h_i with
 * r_j), insertion (h_i alone), deletion (r_j alone).  d is the minimum number
 * of non-match moves, the Levenshtein distance; s the minimum number of
 * substitutions among the alignments that reach d; ins - del = N - M and d = s +
 * del + ins fix del and ins.  So the four numbers are properties of the two
 * sequences, not of a tie rule.  Equivalently d * 2^16 + s is the minimum of one
 * additive cost: match 0, insertion and deletion 2^16, substitution 2^16 + 1.
 * Outputs:
 *   d_stats [batch][n_hyp][4] int32     d, s, del, ins
 *   d_best_or_null [batch] int32        the h with the smallest (d, s, h): the oracle
 *                                       hypothesis of the N-best list
 *   d_totals_or_null [2][8] int64       row 0 over hypothesis 0 of every utterance, row
 *                                       1 over the oracle hypothesis; columns: sum d,
 *                                       sum s, sum del, sum ins, sum M, sum N, the number
 *                                       of utterances with d > 0, batch.  The corpus
 *                                       error rate is column 0 / column 4.
 * Everything is integer arithmetic, so equal inputs give equal bits.
 * Limits: 1 <= hyp_stride <= 32767, 1 <= max_ref_len <= 1024, ref_stride >=
 * max_ref_len, 1 <= n_hyp <= 64, batch * n_hyp <= 2^24, batch * n_hyp *
 * hyp_stride <= 2^30.  Beyond them, or for a null required pointer, a
 * non-positive size, a workspace not 16-byte aligned or device < 0:
 * WK_ERR_INVALID_ARG before any device work; wk_ctc_cer_workspace_bytes returns
 * 0 beyond the limits.  The workspace holds (N, M) per pair and nothing
 * proportional to hyp_stride * max_ref_len: no DP matrix, no back-pointers.
 * Stream-ordered, no host synchronisation, no atomics, no floating point;
 * d_workspace is the caller's. */
int64_t wk_ctc_cer_workspace_bytes(int64_t batch, int32_t n_hyp, int32_t hyp_stride, int32_t max_ref_len);
wk_status wk_ctc_cer(const int32_t* d_hyp, const int32_t* d_hyp_lengths_or_null, int64_t batch, int32_t n_hyp,
                     int32_t hyp_stride, const int32_t* d_ref, int32_t ref_stride, const int32_t* d_ref_lengths,
                     int32_t max_ref_len, int32_t collapse, void* d_workspace, int32_t* d_stats,
                     int32_t* d_best_or_null, int64_t* d_totals_or_null, int32_t device, void* stream);

/* ---- WAV ingest and waveform augmentation (host only) ---
 * No device work: these fill caller (e.g. pinned) host buffers for the H2D copy. */
typedef struct {
  int32_t sample_rate, channels, bits_per_sample;
  int32_t data_samples;   /* frames in the data chunk              */
  int32_t n_samples;      /* frames actually read (<= max_samples) */
} wk_wav_info;
/* esp_wav.cpp:8-139: RIFF/WAVE/"fmt " header, unknown chunks before "data"
 * skipped, PCM 16-bit only (WK_ERR_UNSUPPORTED otherwise); channel 0 of up
 * to max_samples frames into out (the reference truncates to 16000). */
wk_status wk_wav_read(const char* path, int16_t* out, int32_t max_samples, wk_wav_info* info);
/* torchaudio.load scaling (x/32768) + pad_audio (extract_mfcc.py:7-23) for n
 * files on worker threads: out[n][pad_to], right-padded with N(0,
 * noise_level^2) from a counter-hash generator keyed on (seed, file index)
 * (distribution of torch.randn * noise_level, not its bit stream), or zeros
 * when noise_level == 0.  n_read[i] (may be NULL) gets each file's length. */
wk_status wk_wav_load_batch(const char* const* paths, int32_t n, int32_t pad_to, float noise_level, uint32_t seed,
                            float* out, int32_t* n_read);
/* augment_audio_waveform (extract_mfcc.py:90-121): speed change by linear
 * interpolation to int(n*speed) samples (F.interpolate, align_corners=False),
 * padded (noise as above, stream 0) / trimmed to out_len, then x volume with
 * clamp to [-1, 1] when volume != 1. */
wk_status wk_augment(const float* in, int32_t n, float speed, float volume, float noise_level, uint32_t seed, float* out,
                     int32_t out_len);

/* ---- Batched waveform augmentation on the device (extract_mfcc.py:7-45,
 * :90-121, :157-169) -----------------------------------------------------------
 * extract_features' waveform stage for n clips and K variants: pad_audio, the
 * speed / volume variants of augment_audio_waveform and add_random_noise, one
 * workgroup per output row.  d_out[(i*K + v)][out_len], clip-major as the
 * reference appends them; all arithmetic fp32.  Output row r = i*K + v:
 *   1. pad / trim: a[j] = x_i[j] for j < min(len_i, out_len), else pad_noise *
 *      g(0, i, j) (0 when pad_noise == 0).  The stream is keyed by the CLIP, so
 *      all K variants see the same padded clip, as in the reference.
 *   2. speed != 1: m = (int)((double)out_len * speed), scale = (float)out_len /
 *      (float)m; j < m: src = max(scale*(j + 0.5f) - 0.5f, 0), i0 = (int)src, i1 =
 *      i0 + (i0 < out_len-1), l1 = src - i0, l0 = 1 - l1, b[j] = l0*a[i0] + l1*a[i1]
 *      (each product and the sum rounded on its own: with no noise the row is
 *      bit-equal to wk_augment's); j >= m: b[j] = pad_noise * g(1, r, j).
 *      speed == 1: b = a.
 *   3. volume != 1: b = clamp(b * volume, -1, 1) (the pad included, as wk_augment).
 *   4. snr_noise > 0 (add_random_noise as written, its amplitude ratio applied
 *      to powers included): z[j] = snr_noise * g(2, r, j); u = (w >> 8) 2^-24 of
 *      word 0 of block 0 of stream 3, row r; snr = 10^((lo + u (hi - lo)) / 20);
 *      Ps = mean(b^2), Pn = mean(z^2) over out_len; z *= sqrt(Ps / (Pn snr)) when
 *      Pn > 0; out = clamp(b + z, -1, 1).  The two means are reduced in a fixed
 *      order without atomics: the same inputs give the same bits.
 * Noise: g(stream, row, j) is sample j of the Philox4x32-10 stream with key =
 * (seed low, seed high) and counter = (q, row, epoch, stream): block q gives
 * samples 4q..4q+3, words (w0, w1) samples 4q and 4q+1, (w2, w3) samples 4q+2
 * and 4q+3; for a pair (wa, wb): u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8)
 * 2^-24, rho = sqrt(-2 ln u1), the samples are rho cos(2 pi u2) and rho sin(2 pi
 * u2).  Streams 1-3 are keyed by the output ROW, so a variant's noise depends
 * on its position v in the list; a new `epoch` draws all noise afresh.
 *
 * No handle, no allocation, no host synchronisation; stream-ordered on the
 * current device.  Clip i is at d_audio + i*in_stride elements (WK_DTYPE_F32,
 * or WK_DTYPE_I16 scaled by 1/32768).  d_len_or_null[i] is the clip's length
 * (NULL = in_len for all); it lives on the device and cannot be validated
 * without a sync, so the kernel clamps it to [0, in_len] and never reads a
 * clip past in_len.  d_out must not overlap d_audio; n*K must be below 2^32;
 * row and sample offsets are 64-bit.
 * WK_ERR_INVALID_ARG, before any device work: NULL d_audio, d_out, variants or
 * spec; n < 0, in_len < 0, in_stride < in_len; n_variants outside [1,
 * WK_AUG_MAX_VARIANTS]; a non-positive or non-finite speed or volume;
 * (int)(out_len*speed) outside [1, 2^31); negative or non-finite noise levels;
 * snr_lo_db > snr_hi_db or either non-finite; out_len outside [1,
 * WK_AUG_MAX_LEN]; a dtype other than the two above; n*K >= 2^32.  n == 0 is
 * WK_OK and launches nothing. */
#define WK_AUG_MAX_VARIANTS 16
#define WK_AUG_MAX_LEN 16384   /* one workgroup holds a row's b and z in LDS: 2 x 64 KiB */
typedef struct { float speed, volume; } wk_aug_variant;   /* (1, 1) = the clip itself */
typedef struct {
  float    pad_noise;             /* pad_audio's noise_level (0.005); 0 = zero pad        */
  float    snr_noise;             /* add_random_noise's noise_level (0.01); 0 = stage off */
  float    snr_lo_db, snr_hi_db;  /* its snr_range (5, 20)                                */
  uint64_t seed;                  /* Philox key                                           */
  uint32_t epoch;                 /* a new value draws all noise afresh                   */
} wk_aug_spec;
wk_status wk_augment_batch(const void* d_audio, int32_t dtype, const int32_t* d_len_or_null, int64_t n, int32_t in_len,
                           int64_t in_stride, const wk_aug_variant* variants, int32_t n_variants,
                           const wk_aug_spec* spec, int32_t out_len, float* d_out, void* stream);

/* ---- Training step (ml_models/main.py:13-64, train_model) --------------------
 * LightweightKWS(num_classes=1) under BCEWithLogitsLoss and AdamW, fp32.  A
 * wk_trainer owns the weights (blob order of WK_NUM_WEIGHTS), the last
 * gradients, AdamW's moments and step count, and a workspace of per-workgroup
 * gradient sums that grows on the first call with a larger batch (the only
 * time a call blocks the host): issue one trainer's calls on one stream.
 * Gradients are reduced in a fixed order without atomics, so the same inputs
 * give the same bits.  ReLU has gradient 0 at a pre-activation <= 0; a
 * max-pool pair sends its gradient to the larger element, the first on an
 * exact tie (torch's conventions). */
typedef struct wk_trainer wk_trainer;
typedef struct { float lr, beta1, beta2, eps, weight_decay; } wk_adamw;   /* main.py:16-22: 5e-4, .9, .99, 1e-7, 1e-3 */

wk_status wk_trainer_create(int32_t device, const float* host_weights /* WK_NUM_WEIGHTS */, wk_trainer** out);
wk_status wk_trainer_destroy(wk_trainer* t);

/* d_feats [batch][13][63], d_labels [batch] (0/1 floats) -> mean BCE-with-logits loss (*d_loss),
 * logits [batch] and gradients [WK_NUM_WEIGHTS] (either may be NULL); the gradients are also kept in the trainer. */
wk_status wk_trainer_grad(wk_trainer* t, const float* d_feats, const float* d_labels, int64_t batch,
                          float* d_loss, float* d_logits_or_null, float* d_grads_or_null, void* stream);

/* One AdamW step with the trainer's last gradients, or with d_grads_or_null [WK_NUM_WEIGHTS] when given
 * (data-parallel callers average per-rank gradients themselves and pass the result). */
wk_status wk_trainer_step(wk_trainer* t, const wk_adamw* opt, const float* d_grads_or_null, void* stream);

/* Current weights, blob order, device to device, stream-ordered. */
wk_status wk_trainer_weights(wk_trainer* t, float* d_out, void* stream);

/* ---- Post-training int8 quantisation (ml_models/main.py:71-129, quantize_model_esp) ----
 * The int8 network's power-of-2, symmetric, per-tensor exponents: a tensor
 * holds q * 2^e with q in [-128, 127].  e_w follows the state-dict order of
 * WK_NUM_WEIGHTS; e_act is conv1, conv2, conv3 output (a pool output shares its
 * conv's exponent), GAP, classifier.0 output, logit.  A convolution or matmul
 * requantises its int32 sum by s = e_out - e_x - e_w bits (round half to even,
 * then saturate; s = 0 saturates only); GAP computes rne(sum * 2^d / 7) with
 * d = e_act[2] - e_act[3]. */
typedef struct {
  int32_t e_in;
  int32_t e_w[5];
  int32_t e_act[6];
} wk_quant_spec;
#define WK_QUANT_TENSORS 7   /* observed tensors: input, then e_act's six */
#define WK_QUANT_BINS 32     /* exponents -24 .. 7 */

/* ml_models/xiaoa.info:3139-3150: -4; -8 -9 -9 -9 -9; -5 -5 -4 -5 -4 -3. */
wk_status wk_quant_spec_default(wk_quant_spec* out);
/* WK_PREC_INT8 handles only: re-quantise the handle's fp32 weights as
 * sat8(rne(w * 2^-e_w)) and run every later int8 launch of the handle (wk_cnn,
 * wk_forward, wk_scan, wk_stream_push) at `spec`.  Blocks until the handle's
 * device is idle, so it is safe between calls on any stream; launches already
 * queued keep the spec they were issued with.  WK_ERR_INVALID_ARG, before any
 * device work, if the handle is not int8, an exponent is outside [-32, 32], a
 * shift s is outside [0, 24] or d is outside [-4, 4].  A handle that never
 * calls it runs the default spec. */
wk_status wk_set_quant(wk_handle* h, const wk_quant_spec* spec);
wk_status wk_get_quant(wk_handle* h, wk_quant_spec* out);
/* Host only: the int8 export of a WK_NUM_WEIGHTS blob at spec->e_w (only e_w
 * is read, each in [-32, 32]), WK_NUM_WEIGHTS values in the logical layouts
 * conv [k][ci][co], matmul [in][out]. */
wk_status wk_quant_weights(const float* host_weights, const wk_quant_spec* spec, int8_t* out);

/* Calibration: one fp32 forward of the CNN (direct-form convolutions on fp32
 * MFMA, the handle's fp32 weights; any precision) over d_feats [batch][13][63],
 * observing per clip the input (819 values), the conv1 / conv2 / conv3 outputs
 * after ReLU and before the pool (2016, 1984, 1920), GAP (128), classifier.0
 * after ReLU (64) and the logit (1).  |x| is counted in the bin of the smallest
 * exponent that holds it, b = min{e : |x| <= 127 * 2^e}, clamped to [-24, 7]
 * (zeros in the lowest bin).  Per tensor, the exponent is the smallest bin
 * whose cumulative count reaches ceil(percentile / 100 * N); percentile >= 100
 * gives the bin of the maximum.  pin_e_in fixes e_in (the firmware feeds x16:
 * -4) unless it is WK_QUANT_CALIBRATE_INPUT; weight exponents are
 * ceil(log2(max|w| / 127)) per tensor.  Counts are integers summed in a fixed
 * way (no floating-point or global atomics): two calls give the same result.
 * The call allocates nothing and synchronises `stream` once, to read the
 * counters back.  The workspace is device memory of at least
 * wk_calibrate_workspace_bytes(batch) bytes, 256-byte aligned.  The result is
 * not checked against wk_set_quant's shift limits: wk_set_quant does that. */
typedef struct {
  int64_t n_clips;
  int64_t counts[WK_QUANT_TENSORS][WK_QUANT_BINS];
  float max_abs[WK_QUANT_TENSORS];
} wk_calib_stats;
#define WK_QUANT_CALIBRATE_INPUT INT32_MIN
wk_status wk_calibrate_workspace_bytes(int64_t batch, size_t* bytes);
wk_status wk_calibrate(wk_handle* h, const float* d_feats, int64_t batch, double percentile, int32_t pin_e_in,
                       void* d_workspace, size_t workspace_bytes, wk_quant_spec* out, wk_calib_stats* stats_or_null,
                       void* stream);

/* Human-readable text for a status / the last HIP error seen by this thread. */
const char* wk_status_string(wk_status s);
const char* wk_last_error(void);
int32_t wk_abi_version(void);

/* ---- mode A at any parameter set (main/esp_mfcc/mfcc.c:144-234,298-527) ----
 * mfcc.c accepts any sampling rate, frame, hop, n_fft, n_filters and n_mfcc
 * and rebuilds its filterbank, window and DCT tables per call.  A
 * wk_esp_mfcc object holds one parameter set's tables on `device` (built
 * with the reference's float formulas); wk_esp_mfcc_run computes, on the
 * GPU, batch signals of signal_len samples (signal i at d_signal + i*stride)
 * -> d_out[batch][n_frames][n_mfcc], n_frames = (signal_len - frame_size) /
 * hop_size + 1: pre-emphasis `pre_emphasis` (0.97 in extract_mfcc, 0 in the
 * single-frame variant), symmetric Hamming (alpha 0.53836), the frame in the
 * first min(frame_size, n_fft) points of an n_fft-point FFT, power /n_fft +
 * 1e-12 (esp_dsp_packing: dsps_cplx2reC_fc32's packing), mel, ln(max(E,1e-12)),
 * DCT-II; coefficients past n_filters are 0 (mfcc.c's calloc).
 * Domain: n_fft a power of two in [2, 4096] (esp-dsp's FFT refuses other
 * lengths), 1 <= n_filters <= 1024, frame_size, n_mfcc, sampling_rate >= 1;
 * WK_ERR_INVALID_ARG outside it. */
typedef struct wk_esp_mfcc wk_esp_mfcc;
wk_status wk_esp_mfcc_create(int32_t sampling_rate, int32_t frame_size, int32_t n_fft, int32_t n_filters,
                             int32_t n_mfcc, int32_t esp_dsp_packing, int32_t device, wk_esp_mfcc** out);
wk_status wk_esp_mfcc_run(wk_esp_mfcc* m, const float* d_signal, int64_t batch, int32_t signal_len, int64_t stride,
                          int32_t hop_size, float pre_emphasis, float* d_out, void* stream);
wk_status wk_esp_mfcc_destroy(wk_esp_mfcc* m);

/* ---- mfcc.h compatibility shims (main/esp_mfcc/mfcc.h:10-17) --------------
 * Same signatures and ownership as the reference: host signal in, a malloc'd
 * host block of n_frames*n_mfcc floats (frame-major) out, caller frees it with
 * free_mfcc(); NULL on bad arguments.  Computed on device 0 with
 * esp_dsp_packing on: the reference configuration (16000 Hz, 320/256/512, 40
 * filters, 13 coefficients) by the fixed-geometry mode-A kernel, every other
 * parameter set in wk_esp_mfcc's domain by wk_esp_mfcc (tables cached per
 * parameter set); NULL outside that domain (non-power-of-2 n_fft, hop_size
 * < 1, ...). */
float* extract_mfcc(const float* signal, int signal_len, int sampling_rate, int frame_size, int hop_size,
                    int n_fft, int n_filters, int n_mfcc);
void free_mfcc(float* mfcc);
void analyze_mfcc_range(float* mfcc, int size, const char* label);
/* mfcc.c:297-427 (defined there, not declared in mfcc.h): one frame of
 * frame_size <= n_fft samples, no pre-emphasis -> malloc'd n_mfcc floats, NULL
 * on error. */
float* flow_extract_mfcc_single_frame(const float* frame, int frame_size, int sampling_rate, int n_fft, int n_filters,
                                      int n_mfcc);

#ifdef __cplusplus
}
#endif

#endif /* WAKEWORD_H_ */
