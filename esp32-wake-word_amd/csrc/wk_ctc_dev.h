// wk_ctc_dev.h -- what the units of the GRU-CTC head share (internal): the
// model's fixed sizes, the fp16 fragment vectors, one wave reduction, and the
// launchers the two ABI units (no kernels: wk_ctc.hip, inference; wk_ctc_train.hip,
// the fp32-handle entry points; their handle: wk_ctc_handle.h) call into the per-stage units:
//
//   wk_ctc_logmel.hip  X1   log-mel front end + z-score, its host tables
//   wk_ctc_dense.hip   X2a  encoder (fp32 / fp16), the block GEMM, fp16 <-> fp32 copy
//   wk_ctc_gru.hip     X2b  the three recurrences and their weight packers
//   wk_ctc_out.hip     X2c / X3  output layer + argmax kernels, re-score, greedy decode
//   wk_ctc_dropout.hip train-mode dropout: Philox masks applied in the forward, made again in the backward
//   wk_ctc_bwd.hip     the fp32 backward pass: parameter gradients from the gradient at the logits
//   wk_ctc_optim.hip   clip + Adam on the handle's weights, the W_hh fragments again, blob <-> buffers
//
// The units that consume the head's [B][T][V] log-probs have their own ABI and
// no launcher here: wk_ctc_loss.hip, wk_ctc_align.hip, wk_ctc_beam.hip,
// wk_ctc_spot.hip, wk_ctc_cer.hip.  What those share is wk_ctc_lattice_dev.h.
//
// Layout constants stay with the kernel that defines the layout: each packer
// and each grid computation sits in the kernel's own unit, so none is needed
// here.  A launcher that only enqueues kernels returns nothing: a launch error
// is picked up by the one hipGetLastError that ends each wk_ctc_* entry point.
// The GEMM entry points check their shapes and report like the ABI does.
#pragma once
#include <hip/hip_fp16.h>

#include <vector>

#include "wk_cnn_dev.h"
#include "wk_kernels.h"

namespace wk {

constexpr int kNfft = 400, kHop = 160, kBins = kNfft / 2 + 1, kMels = 80, kH = 128;

typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// Sum over the four lanes l, l ^ 16, l ^ 32, l ^ 48 (a row's four 16-lane
// groups), in every lane: gfx950's v_permlane16/32_swap exchange rows in the
// VALU (with both operands the same register, the two results are the
// lane's and its partner's values), no LDS round trip as __shfl_xor costs.
__device__ __forceinline__ float sum_rows4(float v) {
  const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(p[0]) + __uint_as_float(p[1]);
  const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}

// ---- wk_ctc_logmel.hip ------------------------------------------------------
// Host tables of ctc_logmel_fft2_kernel: periodic Hann(400), the four-step
// twiddles W400^(n2 k1) [20 k1][20 n2] complex, the per-lane padded mel weights
// x 1/4 ([64][kMelW1] then [64][kMelW2]) and their window start bins ([64] then
// [64]).  False when the filterbank does not fit the kernel's fixed windows.
struct CtcLogmelTables {
  std::vector<float> win, tw, melw;
  std::vector<int> melws;
};
bool ctc_logmel_tables(CtcLogmelTables* t);
// The log-mel kernel's launch: at most one 12-wave workgroup per CU, each wave
// a contiguous range of R passes; MS statistics slots per wave (the most
// utterances 6 R rows can touch), slots = waves x MS.
struct CtcLogmelLayout {
  unsigned grid;
  int64_t R;
  int MS;
  int64_t slots;
};
CtcLogmelLayout ctc_logmel_layout(int n_cu, int64_t rows, int T);
// part != null: the features stay raw and each wave leaves its z-score partials there.
void launch_ctc_logmel(const float* audio, int64_t stride, int n_valid, int n_pad, int T, int64_t rows, const float* win,
                       const float* tw, const float* melw, const int* melws, float* feats, const CtcLogmelLayout& lay,
                       float2* part, hipStream_t st);
// The z-score of [batch][T][80] features in place, or with part (the log-mel launch's) only its {mean, 1/std} to zs.
void launch_ctc_zscore(float* feats, int64_t batch, int T, const CtcLogmelLayout& lay, const float2* part, float2* zs,
                       hipStream_t st);

// ---- wk_ctc_dense.hip -------------------------------------------------------
// feats [B][T][80] -> out: fp32 rows in the same order, or (f16) fp16 time-major rows t B + b, where zs != null
// z-scores the raw feature rows as they load.
void launch_ctc_encoder(bool f16, const float* feats, int B, int T, const float* w, const float* bias, const float* gamma,
                        const float* beta, const float2* zs, void* out, int n_cu, hipStream_t st);
// Row-major C[M][N] (fp32, or fp16 with c16) = A[M][K] * W[N][K]^T with A, W
// fp32 or fp16 (fp32 accumulate), on `st`.
wk_status ctc_gemm_nt(hipStream_t st, int64_t M, int64_t N, int64_t K, const void* A, const void* W, void* C, bool f16,
                      bool c16 = false);
// fp32 best[row] = first argmax of A[M][K] W[N][K]^T + bias (K % 16 == 0),
// with keys [M] as scratch: zero, GEMM + atomic argmax, decode.
wk_status ctc_gemm_argmax(hipStream_t st, int64_t M, int64_t N, int64_t K, const float* A, const float* W,
                          const float* bias, unsigned long long* keys, int* best);
void launch_ctc_convert(const __half* in, float* out, int64_t n, int n_cu, hipStream_t st);
void launch_ctc_convert(const float* in, __half* out, int64_t n, int n_cu, hipStream_t st);

// ---- wk_ctc_gru.hip ---------------------------------------------------------
// One layer, both directions.  W_hh [2 dir][384][128] fp32 -> the fragment
// layouts of ctc_gru_kernel ([2][24 tiles][32 k-steps][64 lanes]) and
// ctc_gru16_kernel ([2][24 tiles][8 k-steps][64 lanes][4]).
std::vector<float> ctc_pack_whh(const float* whh);
std::vector<float> ctc_pack_whh16(const float* whh);
// ctc_gru16x_kernel's 16x16x32 A fragments of src [2 dir][3 gates x 128][K]:
// [dir][gate][wave][K/32 k-steps][lane][8], gate g's rows times scale[g].
constexpr double kCtcGateScale[3] = {-1.4426950408889634, -1.4426950408889634, 2.8853900817779268};
std::vector<float> ctc_pack_frag32(const float* src, int K, const double (&scale)[3]);
// Gate inputs gi [rows][768] from ctc_gemm_nt: fp32 tensors and ctc_pack_whh's weights, or (f16) fp16 time-major
// tensors and ctc_pack_whh16's.
void launch_ctc_gru(bool f16, const void* gi, const void* whh_pk, const float* bih, const float* bhh, int64_t B, int T,
                    void* out, hipStream_t st);
// Input projection fused in: x time-major [T][B][din] fp16, din = 128 or 256.
void launch_ctc_gru16x(int din, const __half* x, const __half* wih16x_pk, const __half* whh16x_pk, const float* bih,
                       const float* bhh, int64_t B, int T, __half* out, hipStream_t st);

// ---- wk_ctc_out.hip ---------------------------------------------------------
// bias + log_softmax + argmax over materialised logits (fp32, or fp16 with
// f16); log_probs and best may be null; tm_B > 0: the logits rows are time-major.
void launch_ctc_argmax(bool f16, const void* logits, const float* bias, int64_t rows, int V, float* log_probs, int* best,
                       int tm_B, int T, hipStream_t st);
// The fused fp16 output layer + argmax.  logits != null also stores the fp16
// logits; fold picks ctc_out_decode16_kernel where it applies (V <= 4096, no logits).
constexpr bool ctc_out_keyed(int V) { return V <= 16 * 256; }   // the tag holds kOutCF tile + cf in 8 bits
void launch_ctc_out16(const __half* y, const __half* w16, const float* bias, int64_t rows, int V, __half* logits, int* best,
                      int* best2, bool fold, hipStream_t st);
void launch_ctc_rescore(const __half* y, const float* w, const float* bias, int64_t rows, int* best, const int* best2,
                        hipStream_t st);
void launch_ctc_greedy(const int* best, int64_t B, int T, int* tokens, int* lengths, int tm, hipStream_t st);
void launch_ctc_pred(const int* best, int64_t B, int T, int tm, int* pred, hipStream_t st);

// ---- wk_ctc_dropout.hip -----------------------------------------------------
// Train-mode dropout as wakeword.h states it.  Site 0: the encoder output
// [rows][128]; site 1: layer 0's output as layer 1's input [rows][256].  on[s]
// false (p = 0): the site is the identity and nothing is launched for it.
constexpr int kCtcDropWidth[2] = {kH, 2 * kH};
struct CtcDrop {
  uint64_t seed, offset;
  uint32_t thr[2];   // kept iff the element's Philox word >= thr
  float scale[2];    // 1.0f / (1.0f - p)
  bool on[2];
};
CtcDrop ctc_drop(const wk_ctc_dropout& d);
// out = scale * mask * in over [rows][width of site]; in == out is allowed.
void launch_ctc_dropout_fwd(const CtcDrop& d, int site, const float* in, float* out, int64_t rows, int n_cu, hipStream_t st);
// dx <- scale * mask * dx, in place: the same mask made again.
void launch_ctc_dropout_bwd(const CtcDrop& d, int site, float* dx, int64_t rows, int n_cu, hipStream_t st);
// mask [rows][width of site] bytes, 1 = kept (all ones for a site that is off).
void launch_ctc_dropout_mask(const CtcDrop& d, int site, uint8_t* mask, int64_t rows, int n_cu, hipStream_t st);

// ---- wk_ctc_bwd.hip ---------------------------------------------------------
// W_hh [2 dir][384][128] fp32 -> ctc_gru_bptt_kernel's fragments of W_hh^T ([2][8 unit tiles][96 k-steps][64 lanes]).
std::vector<float> ctc_pack_whht(const float* whh);
// Floats of the split-K partials workspace (CtcTrainWs::part) for vocabulary V and rows = B T.
size_t ctc_bwd_part_floats(int V, int64_t rows);
// One backward pass (fp32) at geometry B x T <= ws.rows: what the training
// forward saved in ws and its scratch there (sizes: CtcTrainWs::table), the
// weights as wk_ctc_create uploaded them, and the caller's device pointers:
// dlogits [B][T][V]; grads: the parameter blob's layout (ctc_blob); norm (or
// null): its 2-norm.  Dropout (ws.drop.on[s]): ws.x0 is then the dropped
// encoder output (masked in place by the forward), layer 1's input is the
// dropped copy ws.y0d, or ws.y[0] itself with site 1 off, and ws.y[0] stays the
// undropped output, layer 0's h_prev.  The split-K partials ws.part hold
// ctc_bwd_part_floats(V, ws.rows): the workspace's capacity, not this call's rows.
struct CtcTrainWs;   // (wk_ctc_handle.h)
struct CtcWeights;
struct CtcBwd {
  int64_t B;
  int T, V, n_cu;
  const float* dlogits;
  float *grads, *norm;
  const CtcTrainWs& ws;
  const CtcWeights& w;
};
void launch_ctc_backward(const CtcBwd& a, hipStream_t st);
// out[0] = the 2-norm of g [n], accumulated in double in a fixed order (ctc_bwd_norm_kernel, as launch_ctc_backward runs it).
void launch_ctc_bwd_norm(const float* g, int64_t n, float* out, hipStream_t st);

// ---- wk_ctc_optim.hip -------------------------------------------------------
// The weight blob as the handle keeps it: segment k is blob[off, off + len) and
// lives at p (22 segments: 4 encoder, 2 layers x 2 directions x {W_ih, W_hh,
// b_ih, b_hh}, 2 output).  Every off and every len but the last (out_b [V]) is
// a multiple of 4 floats, and every p is 16-byte aligned.  Passed by value.
constexpr int kCtcSegs = 22;
// The blob's layout, stated once for C++ (Python's ctc_state_dict_spec is the independent statement the tests compare
// with): off[k] is segment k's first float, off[kCtcSegs] the total; segment k holds off[k + 1] - off[k] floats.
enum { kSegEncW, kSegEncB, kSegLnG, kSegLnB, kSegGru, kSegOutW = kCtcSegs - 2, kSegOutB };
enum { kGruWih, kGruWhh, kGruBih, kGruBhh };
constexpr int ctc_gru_seg(int l, int d, int which) { return kSegGru + 4 * (2 * l + d) + which; }
struct CtcBlob {
  int64_t off[kCtcSegs + 1];
};
inline CtcBlob ctc_blob(int64_t V, int64_t H = kH) {
  CtcBlob b;
  int k = 0;
  int64_t o = 0;
  auto seg = [&](int64_t len) { b.off[k++] = o, o += len; };
  seg(H * kMels), seg(H), seg(H), seg(H);   // encoder W, b; LayerNorm gamma, beta
  for (int l = 0; l < 2; ++l)               // per layer and direction: W_ih, W_hh, b_ih, b_hh
    for (int d = 0; d < 2; ++d) seg(3 * H * (l == 0 ? H : 2 * H)), seg(3 * H * H), seg(3 * H), seg(3 * H);
  seg(V * 2 * H), seg(V);
  b.off[k] = o;
  return b;
}
struct CtcSeg {
  int64_t off, len;
  float* p;
};
struct CtcSegTable {
  CtcSeg s[kCtcSegs];
};
// Adam's constants for one step, rounded to fp32 from double on the host:
// step_size = lr / (1 - beta1^t), sqrt_bc2 = sqrt(1 - beta2^t).
struct CtcAdamArgs {
  float max_norm, weight_decay, beta1, one_minus_beta1, beta2, one_minus_beta2, step_size, sqrt_bc2, eps;
};
// Clip + Adam in place on the table's buffers; g, m, v [blob].  norm != null:
// the gradient is first scaled by min(1, max_norm / (norm[0] + 1e-6)), read on the device.
void launch_ctc_adam(const CtcSegTable& tab, const float* g, float* m, float* v, const float* norm, const CtcAdamArgs& a,
                     int n_cu, hipStream_t st);
// whh_pk[l] and whht_pk[l] from whh[l] [2 dir][384][128]: what ctc_pack_whh and ctc_pack_whht give, bit for bit.
struct CtcWhhSet {
  const float* whh[2];
  float *whh_pk[2], *whht_pk[2];
};
void launch_ctc_refresh(const CtcWhhSet& w, hipStream_t st);
// The table's buffers -> blob, and blob -> the table's buffers.
void launch_ctc_gather(const CtcSegTable& tab, float* blob, int n_cu, hipStream_t st);
void launch_ctc_scatter(const CtcSegTable& tab, const float* blob, int n_cu, hipStream_t st);

}  // namespace wk
