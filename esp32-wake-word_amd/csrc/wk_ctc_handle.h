// wk_ctc_handle.h -- the wk_ctc struct, one part per concern, and what the
// units that take one share (internal): wk_ctc.hip (create / destroy, features,
// forward, transcribe, stage timing), wk_ctc_train.hip (the fp32-handle entry
// points) and wk_ctc_bwd.hip (whose launcher reads the training workspace and
// the weights).  No part has a constructor: `new wk_ctc()` starts every scalar
// at zero, and the DevBuf members are the one list of what destroy frees.
#pragma once
#include <initializer_list>
#include <vector>

#include "wk_ctc_dev.h"
#include "wk_devmem.h"

namespace wk {

// Weights as each kernel's unit packs them, and the log-mel tables.
struct CtcWeights {
  DevBuf<float> enc_w, enc_b, ln_g, ln_b;
  DevBuf<float> wih[2];        // per layer: [768][Din] (fwd rows then reverse rows)
  DevBuf<float> bih[2];        // per layer: [768]
  DevBuf<float> bhh[2];        // per layer: [768]
  DevBuf<float> whh_pk[2];     // per layer: [2 dir][24 tiles][32 k-steps][64 lanes]
  DevBuf<float> out_w, out_b;  // [V][256], [V]
  DevBuf<float> zero_b;        // [V] zeros: the log_softmax kernel's bias in fp16 mode (the logits carry theirs)
  DevBuf<__half> wih16[2];     // fp16 copies (precision 1)
  DevBuf<__half> whh16_pk[2];  // per layer: [2 dir][24 tiles][8 k-steps][64 lanes][4]
  DevBuf<__half> whh16x_pk[2]; // per layer: [2 dir][3 gates][8 waves][4 k-steps][64 lanes][8] (W_hh as 16x16x32 fragments, gate-scaled)
  DevBuf<__half> wih16x_pk[2]; // per layer: [2 dir][3 gates][8 waves][din/32 k-steps][64 lanes][8] (fused-projection GRU, gate-scaled)
  DevBuf<__half> out_w16;
  // fp32 handles, for training: W_hh as the backward's GEMM operand ([2 dir][384][128]) and as ctc_gru_bptt_kernel's W_hh^T fragments
  DevBuf<float> whh[2], whht_pk[2];
  DevBuf<float> fft_win;       // [400] periodic Hann
  DevBuf<float> fft_tw;        // [20 k1][20 n2] W400^(n2 k1), complex
  DevBuf<float> melw;          // ctc_logmel_fft2_kernel: per-lane padded mel weights x 1/4, [64][kMelW1] then [64][kMelW2]
  DevBuf<int> melws;           // their window start bins, [64] then [64]
};

// A workspace buffer and its size at the geometry asked for; 0 bytes: not used on this handle's path, stays unallocated.
struct WsEntry {
  DevMem* buf;
  size_t bytes;
};
struct WsCap {
  size_t* cap;
  size_t value;
};

// wk_ctc_forward's workspace (rows = batch x T), and the geometry of its last call (wk_ctc_frame_argmax).
struct CtcInferWs {
  size_t rows;
  DevBuf<float> x0, gi, y0, y1, logits;
  DevBuf<__half> x0h, y0h, y1h, logits16;
  DevBuf<int> best;
  DevBuf<int> best2;           // fp16 mode: the runner-up column of near-tie rows (else -1), for ctc_rescore_kernel
  int64_t last_batch;
  int32_t last_T;
};

// wk_ctc_transcribe's: [rows][80] features (raw in fp16 mode), [slots] per-wave log-mel statistics
// (ctc_logmel_fft2_kernel<true>), [batch] per-utterance z-score; and the geometry and path of its last call
// (wk_ctc_transcribe_stats; T 0: none yet).
struct CtcTranscribeWs {
  DevBuf<float> feats;
  DevBuf<float2> part, zs;
  size_t rows, batch, slots;
  int64_t last_batch;
  int32_t last_T;
  bool last_fused;
};

// The training workspace (fp32 handles), apart from the inference one: what wk_ctc_forward_train saves, then
// wk_ctc_backward's scratch; table() is each buffer's size at `rows` rows.
struct CtcTrainWs {
  size_t rows;
  DevBuf<float> feats, x0, gi[2], y[2], logits;                                // saved: gi = x W_ih^T without bias
  DevBuf<float> hprev, dya, dyb, gh, da_i, da_h, coef, pre, t0, t1, part;     // scratch; part: the split-K partials
  int64_t batch;        // geometry of the last training forward (wk_ctc_backward, wk_ctc_dropout_masks); 0: none
  int32_t T;
  CtcDrop drop;         // its dropout (all off after a plain wk_ctc_forward_train)
  DevBuf<float> y0d;    // site 1's output, the dropped copy of y[0]: `rows` rows, made by the first forward with
                        // p_gru > 0 and dropped again (0 bytes in table) whenever the workspace regrows
  std::vector<WsEntry> table(int V, size_t n) {
    const size_t H = sizeof(float) * kH * n;
    return {{&feats, sizeof(float) * kMels * n}, {&x0, H}, {&gi[0], 6 * H}, {&gi[1], 6 * H}, {&y[0], 2 * H}, {&y[1], 2 * H},
            {&logits, sizeof(float) * V * n}, {&hprev, 2 * H}, {&dya, 2 * H}, {&dyb, 2 * H}, {&gh, 6 * H}, {&da_i, 6 * H},
            {&da_h, 6 * H}, {&coef, 10 * H}, {&pre, H}, {&t0, H}, {&t1, H},
            {&part, sizeof(float) * ctc_bwd_part_floats(V, (int64_t)n)}, {&y0d, 0}};
  }
};

// Adam's moments in blob order and the norm computed when the caller passes none, allocated and zeroed on first
// use (wk_ctc_adam_step); the step count is host state.
struct CtcOptim {
  DevBuf<float> m, v, norm;
  bool ready;
  int64_t step;
};

// Stage timing (wk_ctc_profile): events recorded around each stage of features / forward on the call's stream,
// folded into per-stage sums when read or when the ring fills.
struct CtcStageTimes {
  int on;
  struct { int stage; hipEvent_t a, b; } ev[64];
  int n_ev;
  double ms[WK_CTC_N_STAGES];
  int64_t n[WK_CTC_N_STAGES];
};

}  // namespace wk

struct wk_ctc {
  wk_ctc_config cfg;
  int n_cu;
  bool f16;             // precision 1: GEMM operands in fp16 (fp32 accumulate); recurrence fp32
  bool gru_gemm;        // fp16 mode: input projections as a separate GEMM (WAKEWORD_CTC_GEMM=1; A/B and checks)
  // Decision-parity attribution (WAKEWORD_CTC_MIX): 1 = "out32", the fp16
  // path up to the last GRU layer, then the output layer in fp32 (y1 widened,
  // fp32 W); 2 = "out16", the fp32 path with the fp16 output kernel (y1 and W
  // rounded to fp16).  0 (default) = the precision's own output layer.
  int mix;
  int rescore;          // fp16 output layer: near-tie rows re-decided in fp32 (default; WAKEWORD_CTC_RESCORE=0 off, A/B)
  wk::CtcWeights w;
  wk::CtcInferWs ws;
  wk::CtcTranscribeWs tr;
  wk::CtcTrainWs tn;
  wk::CtcOptim opt;
  wk::CtcStageTimes prof;
};

namespace wk {

// A failed allocation or upload as the entry points report it.
inline wk_status ctc_alloc_failed(hipError_t e, const char* what) {
  return e == hipErrorOutOfMemory ? WK_ERR_NO_MEMORY : hip_fail(e, what);
}

// Grow a workspace: waits for the stream (the buffers may be in use), frees every buffer of the table before it
// allocates any (the peak is the larger set alone), and leaves none allocated after a failure.  The capacities are
// 0 from the first free on and take their new values once every buffer is there.
wk_status ctc_grow(hipStream_t st, const std::vector<WsEntry>& bufs, std::initializer_list<WsCap> caps, const char* what);

// One forward pass as its stages see it (wk_ctc.hip).  Each stage enqueues its kernels on the buffers it is given
// -- the inference workspace's, or the training one's (wk_ctc_train.hip) -- and is bracketed once for
// wk_ctc_profile when `timed`: wk_ctc_stage_times covers features and forward, not the training calls.  Launch
// errors surface in the entry point's closing ctc_launched.
struct Fwd {
  wk_ctc* c;
  hipStream_t st;
  int64_t batch, rows;
  int T;
  bool timed;
};
// features [rows][80] -> x0: fp32, batch-major rows, or (fp16 handle) fp16, time-major rows from here on
wk_status stage_encoder(const Fwd& f, const float* d_feats, const float2* zs, void* x0);
// GRU layer l: in -> y, in the handle's precision; gi [rows][768] holds the projections where they are a GEMM
wk_status stage_gru(const Fwd& f, int l, const void* in, float* gi, void* y);
// fp32 output layer on y [rows][256]: log-probs through logits [rows][V] with best (or null) the argmax; or,
// without d_log_probs, best alone, the argmax inside the GEMM (logits: its keys)
wk_status stage_out32(const Fwd& f, const float* y, float* logits, float* d_log_probs, int* best);

}  // namespace wk
