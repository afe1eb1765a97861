// wk_scan.hip -- dense sliding-window scoring of long recordings with shared
// MFCC frames (wk_scan, mode B).
//
// Window w of a recording covers samples [w*hop, w*hop + 16000).  With the
// mode-B geometry (center=True, reflect pad 256, Hamming 320 centred in 512,
// hop 256) frame t of a window covers window samples [256t - 160, 256t + 160)
// plus the predecessor sample of the pre-emphasis.  For t = 1..61 that range
// lies inside the window, so for hop = 256k the frame is "global frame"
// g = k*w + t of the recording (samples [256g - 160, 256g + 160) and sample
// 256g - 161), whichever window asks for it.  Only frame 0 (reflection at the
// left edge, y[0] = x[0]) and frame 62 (reflection past sample 15999) belong
// to one window alone.
//
// Two kernels, both built from the front-end's device code (wk_fe_dev.h):
//   wk_scan_frames_kernel  raw MFCC (no CMVN) of the global frames
//       g = 1 .. G = k(W-1) + 61 of every recording, in <= 63-frame units like
//       wk_frontend_kernel's mode-A chunks (16 lanes per frame for the FFT,
//       lane per frame for mel and DCT), stored coefficient-major
//       [rec][13][g_pad] at column g.
//   wk_scan_assemble_kernel  per unit of <= 31 windows of one recording: the
//       2 edge frames of each window through the GENERAL (reflecting) loader,
//       then per window one wave gathers frames 1..61 from the frame store,
//       applies CMVN across the 63 lanes and writes the [13][63] features.
// The CNN then runs on each chunk of features (wk_scan below, which plans the
// chunks; wk_scan_workspace_bytes sizes the frame store and the chunk buffer).
#include "wk_handle.h"

using namespace wk;

#include "wk_fe_dev.h"

namespace {

constexpr int kFrameLead = 162;   // a frame unit's resource starts this many samples before sample 256*g0:
                                  // frame fl of the unit is at base 256*fl + 2 (even, like 256t - 160)

// Frame slot of lane group g of wave `wave` in round r (wk_frontend_kernel's).
__device__ __forceinline__ int scan_slot(int wave, int r, int g) { return fe_lds::frame_slot(wave, r, g); }

template <typename T>
__global__ __launch_bounds__(kFeBlock, 4) void wk_scan_frames_kernel(const T* __restrict__ audio, int64_t rec_stride,
                                                                     int64_t n_units, int n_chunks, int G, int g_pad,
                                                                     float* __restrict__ store) {
  __shared__ __attribute__((aligned(16))) float smem[kFeLdsNoWin];
  float* P = smem + kPOff;
  float* L = smem + kLOff;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15;

  fe_init_tables<true, false>(smem, threadIdx.x, kFeBlock);
  const FeTables tb = fe_tables(smem, j, kWinB);
  __syncthreads();

  // Unit u = (recording, chunk): global frames g0 .. g0 + nfc - 1, g0 = 1 + 63*chunk.
  // The resource is rebased to the unit, so byte offsets stay below 64 KiB
  // whatever the recording's length: it spans samples [256*g0 - 162,
  // 256*(g0 + nfc - 1) + 160) of the recording, all inside it (g0 >= 1 and
  // 256*G + 160 <= n_samples - 224).
  auto unit_of = [&](int64_t u, int& nfc, int& g0, int64_t& rec, __amdgpu_buffer_rsrc_t& rs) {
    rec = u / n_chunks;
    const int chunk = (int)(u - rec * n_chunks);
    g0 = 1 + chunk * kNFramesB;
    nfc = min(kNFramesB, G - chunk * kNFramesB);
    const T* xp = audio + rec * rec_stride + ((int64_t)256 * g0 - kFrameLead);
    rs = make_rsrc(xp, (uint32_t)(256 * (nfc - 1) + kFrameLead + 160) * (uint32_t)sizeof(T));
  };
  auto prefetch = [&](int64_t u, int r, Raw<T>& dst) {
    if (u < n_units) {
      int nfc, g0;
      int64_t rec;
      __amdgpu_buffer_rsrc_t rs;
      unit_of(u, nfc, g0, rec, rs);
      const int fl = scan_slot(wave, r, g);
      load_raw<true>(rs, 256 * fl + 2, j, 0, fl < nfc, false, dst);
    }
  };

  Raw<T> pf;
  prefetch(blockIdx.x, 0, pf);

  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    int nfc, g0;
    int64_t rec;
    __amdgpu_buffer_rsrc_t rs;
    unit_of(u, nfc, g0, rec, rs);

#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
      const int fl = scan_slot(wave, r, g);
      f2 a[16];
      if (fl < nfc) fe_stage0<true>(pf, 256 * fl + 2, 0, j, false, tb, a);
      // pf is consumed: prefetch the next wave-round, (u,1) or (u+grid,0), into it.
      prefetch(r == 0 ? u : u + gridDim.x, r ^ 1, pf);
      if (fl < nfc) fe_rest<true>(a, j, P + fl * kPRow, tb, 0, NoPrefetch());
    }
    wg_barrier_lds();

    mel_dispatch<true>(wave, P + min(lane, nfc - 1) * kPRow, L + lane);
    wg_barrier_lds();

    const float* lrow = L + lane;
    const bool valid = lane < nfc;
    const int c0 = wave < 5 ? 2 * wave : wave + 5;
    const int nc = wave < 5 ? 2 : 1;
    for (int ci = 0; ci < nc; ++ci) {
      const int cc = c0 + ci;
      const float v = dct_coef<true>(cc, lrow);
      if (valid) store[(rec * 13 + cc) * g_pad + g0 + lane] = v;
    }
    // (no barrier here, as in wk_frontend_kernel: every wave has passed the mel
    // barrier before any rewrites a power row, and L is rewritten only after
    // the next unit's FFT barrier)
  }
}

// Unit u of the launch = windows [wi0, wi0 + nw) of recording rec, nw <= wpu <= 31.
// Flat window index rec*W + w; features go to feats + (flat - flat0) * 819.
template <typename T>
__global__ __launch_bounds__(kFeBlock, 4) void wk_scan_assemble_kernel(const T* __restrict__ audio, int64_t rec_stride,
                                                                       int hop, int k, int64_t W, int wpu,
                                                                       int64_t units_per_rec, int64_t unit0,
                                                                       int64_t n_units, int64_t flat0, int g_pad,
                                                                       const float* __restrict__ store,
                                                                       float* __restrict__ feats) {
  __shared__ __attribute__((aligned(16))) float smem[kFeLdsNoWin];
  float* P = smem + kPOff;
  float* L = smem + kLOff;
  float* E = P;   // raw MFCC of the unit's edge frames [13][64], over the power rows once mel has read them
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15;

  fe_init_tables<true, false>(smem, threadIdx.x, kFeBlock);
  const FeTables tb = fe_tables(smem, j, kWinB);
  __syncthreads();

  for (int64_t uu = blockIdx.x; uu < n_units; uu += gridDim.x) {
    const int64_t u = unit0 + uu;
    const int64_t rec = u / units_per_rec;
    const int64_t wi0 = (u - rec * units_per_rec) * wpu;
    const int nw = (int)min((int64_t)wpu, W - wi0);
    const int nfe = 2 * nw;   // edge frame e = 2 i + s: window wi0 + i, frame 0 (s = 0) or 62 (s = 1)
    // One resource for the unit: from its first window's start to its last
    // window's end, inside the recording.  Window i starts i*hop samples in
    // (hop <= 15616, i <= 30: far below the 32-bit byte offset range).
    const T* xp = audio + rec * rec_stride + wi0 * hop;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(xp, (uint32_t)((nw - 1) * hop + kWinSamples) * (uint32_t)sizeof(T));

#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
      const int e = scan_slot(wave, r, g);
      if (e < nfe) {
        const int base = (e & 1) ? 256 * (kNFramesB - 1) - 160 : -160;
        Raw<T> raw;
        load_raw<true>(rs, base, j, kWinSamples, true, true, raw, (e >> 1) * hop);
        f2 a[16];
        fe_stage0<true>(raw, base, kWinSamples, j, true, tb, a);
        fe_rest<true>(a, j, P + e * kPRow, tb, 0, NoPrefetch());
      }
    }
    wg_barrier_lds();

    mel_dispatch<true>(wave, P + min(lane, nfe - 1) * kPRow, L + lane);
    wg_barrier_lds();

    {
      const float* lrow = L + lane;
      const int c0 = wave < 5 ? 2 * wave : wave + 5;
      const int nc = wave < 5 ? 2 : 1;
      for (int ci = 0; ci < nc; ++ci) E[(c0 + ci) * 64 + lane] = dct_coef<true>(c0 + ci, lrow);
    }
    wg_barrier_lds();

    // Assembly: wave per window, lane per frame t.
    const int t = lane;
    const bool valid = t < kNFramesB;
    for (int i = wave; i < nw; i += 8) {
      const int64_t w = wi0 + i;
      const float* col = store + rec * 13 * (int64_t)g_pad + (k * w + t);
      float v[13];
#pragma unroll
      for (int cc = 0; cc < 13; ++cc) {
        if (t == 0) v[cc] = E[cc * 64 + 2 * i];
        else if (t == kNFramesB - 1) v[cc] = E[cc * 64 + 2 * i + 1];
        else if (valid) v[cc] = col[(int64_t)cc * g_pad];
        else v[cc] = 0.0f;
      }
      float* out = feats + (rec * W + w - flat0) * (13 * kNFramesB);
#pragma unroll
      for (int cc = 0; cc < 13; ++cc) {
        const float y = cmvn_lane(v[cc], valid, kNFramesB);
        if (valid) out[cc * kNFramesB + t] = y;
      }
    }
    wg_barrier_lds();   // E (= P) and L are rewritten by the next unit
  }
}

// Launchers, mode B, hop = 256k with k <= kScanMaxK.
// launch_scan_frames: raw MFCC of global frames 1..G of each of n_rec
// recordings -> store [n_rec][13][g_pad], frame g at column g (g_pad > G).
// launch_scan_assemble: units [unit0, unit0 + n_units) of <= wpu (<= kScanUnitWindows)
// consecutive windows of one recording each, ceil(W / wpu) units per recording:
// edge frames 0 and 62 of every window + frames 1..61 from the store + CMVN ->
// feats + (flat window index - flat0) * 819, flat index = rec * W + w.
constexpr int kScanMaxK = 61;          // beyond it consecutive windows share no interior frame
constexpr int kScanUnitWindows = 31;   // 62 edge frames per work unit

hipError_t launch_scan_frames(bool i16, const void* audio, int64_t n_rec, int64_t rec_stride, int G, int g_pad,
                              float* store, int grid_cap, hipStream_t stream) {
  const int n_chunks = (G + kNFramesB - 1) / kNFramesB;
  const int64_t n_units = n_rec * n_chunks;
  if (n_units <= 0) return hipSuccess;
  const int grid = (int)(n_units < grid_cap ? n_units : grid_cap);
  if (i16)
    hipLaunchKernelGGL(wk_scan_frames_kernel<int16_t>, dim3(grid), dim3(kFeBlock), 0, stream, (const int16_t*)audio,
                       rec_stride, n_units, n_chunks, G, g_pad, store);
  else
    hipLaunchKernelGGL(wk_scan_frames_kernel<float>, dim3(grid), dim3(kFeBlock), 0, stream, (const float*)audio,
                       rec_stride, n_units, n_chunks, G, g_pad, store);
  return hipGetLastError();
}

hipError_t launch_scan_assemble(bool i16, const void* audio, int64_t rec_stride, int hop, int64_t W, int wpu,
                                int64_t unit0, int64_t n_units, int64_t flat0, int g_pad, const float* store,
                                float* feats, int grid_cap, hipStream_t stream) {
  if (n_units <= 0) return hipSuccess;
  const int64_t units_per_rec = (W + wpu - 1) / wpu;
  const int grid = (int)(n_units < grid_cap ? n_units : grid_cap);
  if (i16)
    hipLaunchKernelGGL(wk_scan_assemble_kernel<int16_t>, dim3(grid), dim3(kFeBlock), 0, stream,
                       (const int16_t*)audio, rec_stride, hop, hop / 256, W, wpu, units_per_rec, unit0, n_units, flat0,
                       g_pad, store, feats);
  else
    hipLaunchKernelGGL(wk_scan_assemble_kernel<float>, dim3(grid), dim3(kFeBlock), 0, stream, (const float*)audio,
                       rec_stride, hop, hop / 256, W, wpu, units_per_rec, unit0, n_units, flat0, g_pad, store, feats);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// wk_scan: every window [w*hop, w*hop + 16000) of long recordings.
// ---------------------------------------------------------------------------
constexpr int64_t kScanMaxSamples = (int64_t)1 << 30;
constexpr int64_t kScanChunkWindows = 65536;                  // default windows per chunk (215 MB of features)
constexpr size_t kScanFeatBytes = sizeof(float) * 13 * 63;    // 3276 B of features per window

struct ScanPlan {
  int64_t W;           // windows per recording
  bool shared;         // hop = 256k, k <= kScanMaxK: interior frames computed once per recording
  int k;
  int G, g_pad;        // global frames 1..G; frame-store pitch (column g, a multiple of 64 above G)
  size_t store_bytes;  // frame store [n_rec][13][g_pad], rounded up to 256 B
};

ScanPlan scan_plan(int64_t n_rec, int64_t n_samples, int32_t hop) {
  ScanPlan p = {};
  p.W = n_samples < WK_WIN_SAMPLES ? 0 : (n_samples - WK_WIN_SAMPLES) / hop + 1;
  p.shared = p.W > 0 && n_rec > 0 && hop % 256 == 0 && hop / 256 <= kScanMaxK;
  if (p.shared) {
    p.k = hop / 256;
    p.G = (int)(p.k * (p.W - 1) + 61);
    p.g_pad = (p.G + 1 + 63) & ~63;
    p.store_bytes = ((size_t)n_rec * 13 * p.g_pad * sizeof(float) + 255) & ~(size_t)255;
  }
  return p;
}

wk_status scan_check_geometry(int64_t n_rec, int64_t n_samples, int32_t hop) {
  if (hop < 1) return invalid("wk_scan: hop < 1");
  if (n_rec < 0) return invalid("wk_scan: n_rec < 0");
  if (n_samples < 0 || n_samples > kScanMaxSamples) return invalid("wk_scan: n_samples outside [0, 2^30]");
  return WK_OK;
}

}  // namespace

extern "C" {

wk_status wk_scan_workspace_bytes(int64_t n_rec, int64_t n_samples, int32_t hop, int64_t windows_per_chunk,
                                  size_t* bytes) {
  if (!bytes) return invalid("wk_scan_workspace_bytes: null bytes");
  *bytes = 0;
  wk_status s = scan_check_geometry(n_rec, n_samples, hop);
  if (s != WK_OK) return s;
  if (windows_per_chunk < 0) return invalid("wk_scan_workspace_bytes: windows_per_chunk < 0");
  const ScanPlan p = scan_plan(n_rec, n_samples, hop);
  if (!p.shared) return WK_OK;   // forwarded to the wk_forward path: no workspace
  const int64_t total = n_rec * p.W;
  int64_t wpc = windows_per_chunk ? windows_per_chunk : kScanChunkWindows;
  if (wpc > total) wpc = total;
  *bytes = p.store_bytes + (size_t)wpc * kScanFeatBytes;
  return WK_OK;
}

wk_status wk_scan(wk_handle* h, const void* d_audio, int32_t dtype, int64_t n_rec, int64_t n_samples,
                  int64_t rec_stride, int32_t hop, float* d_logits, float* d_feats_or_null, void* d_workspace,
                  size_t workspace_bytes, void* stream) {
  if (!h) return invalid("wk_scan: null handle");
  if (h->cfg.mode != WK_MODE_TORCHAUDIO_CMVN) {
    g_last_error = "wk_scan: the xiaoa CNN consumes mode-B (torchaudio+CMVN) features";
    return WK_ERR_UNSUPPORTED;
  }
  if (!h->d_weights) return invalid("wk_scan: handle created without weights");
  wk_status s = scan_check_geometry(n_rec, n_samples, hop);
  if (s != WK_OK) return s;
  if (dtype != WK_DTYPE_F32 && dtype != WK_DTYPE_I16) return invalid("wk_scan: bad dtype");
  if (n_rec > 1 && rec_stride < n_samples) return invalid("wk_scan: rec_stride < n_samples");
  const ScanPlan p = scan_plan(n_rec, n_samples, hop);
  if (p.W == 0 || n_rec == 0) return WK_OK;
  if (!d_audio || !d_logits) return invalid("wk_scan: null audio / logits");
  const bool i16 = dtype == WK_DTYPE_I16;
  const size_t esz = i16 ? 2 : 4;
  if (!p.shared) {
    // No frame of one window is a frame of another: the sliding wk_forward, per recording.
    for (int64_t r = 0; r < n_rec; ++r) {
      s = forward_impl(h, (const char*)d_audio + (size_t)(r * rec_stride) * esz, dtype, p.W, WK_WIN_SAMPLES, hop,
                       d_logits + r * p.W, d_feats_or_null ? d_feats_or_null + r * p.W * 13 * 63 : nullptr, stream,
                       h->err.dev());
      if (s != WK_OK) return s;
    }
    return WK_OK;
  }
  const int64_t total = n_rec * p.W;
  if (!d_workspace || workspace_bytes < p.store_bytes + kScanFeatBytes)
    return invalid("wk_scan: workspace smaller than wk_scan_workspace_bytes(..., 1 window per chunk)");
  int64_t wpc = (int64_t)((workspace_bytes - p.store_bytes) / kScanFeatBytes);
  if (wpc > total) wpc = total;
  // Chunks are whole work units of wpu consecutive windows of one recording
  // (the last unit of a recording may hold fewer), contiguous in the flat
  // [n_rec][W] order, so each chunk is one CNN launch.
  const int wpu = (int)(wpc < kScanUnitWindows ? wpc : kScanUnitWindows);
  const int64_t units_per_rec = (p.W + wpu - 1) / wpu;
  const int64_t n_units = n_rec * units_per_rec;
  const int64_t units_per_chunk = wpc / wpu;
  auto flat_of = [&](int64_t u) { return (u / units_per_rec) * p.W + (u % units_per_rec) * wpu; };
  float* store = (float*)d_workspace;
  float* chunk_feats = (float*)((char*)d_workspace + p.store_bytes);
  const hipStream_t st = (hipStream_t)stream;
  return on_device(h->cfg.device, [&]() -> wk_status {
    hipError_t e = launch_scan_frames(i16, d_audio, n_rec, rec_stride, p.G, p.g_pad, store, 2 * h->n_cu, st);
    if (e != hipSuccess) return hip_fail(e, "scan frames launch");
    for (int64_t u0 = 0; u0 < n_units; u0 += units_per_chunk) {
      const int64_t u1 = u0 + units_per_chunk < n_units ? u0 + units_per_chunk : n_units;
      const int64_t flat0 = flat_of(u0), n = (u1 == n_units ? total : flat_of(u1)) - flat0;
      float* feats = d_feats_or_null ? d_feats_or_null + flat0 * 13 * 63 : chunk_feats;
      e = launch_scan_assemble(i16, d_audio, rec_stride, hop, p.W, wpu, u0, u1 - u0, flat0, p.g_pad, store, feats,
                               2 * h->n_cu, st);
      if (e != hipSuccess) return hip_fail(e, "scan assemble launch");
      if ((e = launch_cnn(h, feats, n, d_logits + flat0, st, h->err.dev())) != hipSuccess)
        return hip_fail(e, "cnn launch");
    }
    return WK_OK;
  });
}

}  // extern "C"
