// wk_fused_lds.h -- what the two roles of the fused kernel share: the LDS
// carve, the control words, the protocol on them (role barriers, the log-mel
// hand-off, bounded spins and the abort report) and the diagnostic stamps.
// Included by the two fused units only (wk_fused.hip, wk_fused_xdl.hip): like
// the rest of the wk_fused_* headers it keeps its names in the unit's unnamed namespace
// at global scope (the kernels' symbol names are looked up by tools and tests).
//
// The roles share no s_barrier: each synchronises its own 8 waves through an
// LDS counter barrier, and the hand-off is two LDS counters (log-mel ready /
// log-mel buffer free).
#pragma once
#include "wk_fe_dev.h"

using namespace wk;

namespace {

#ifdef WK_DIAG
// Diagnostic builds only (-DWK_DIAG, tools/debug): per-wave cycle sums per
// phase, summed into g_wk_stamps (defined in wk_fused.hip, the one unit of
// such a build that instantiates a kernel).
extern __device__ unsigned long long g_wk_stamps[16][16];
#define WK_STAMP_INIT WkStamps _stamps; _stamps.init();
#define WK_STAMP(k) _stamps.hit(k)
#define WK_STAMP_FLUSH(w) do { if (lane == 0) for (int _k = 0; _k < 16; ++_k) atomicAdd(&g_wk_stamps[w][_k], _stamps.st[_k]); } while (0)
#define WK_SP_ARG , &_stamps
#else
#define WK_STAMP_INIT
#define WK_STAMP(k) do {} while (0)
#define WK_STAMP_FLUSH(w) do {} while (0)
#define WK_SP_ARG
#endif

constexpr int NBF = 4;               // clips per CNN batch
constexpr int kFeWaves = 8;          // waves 0-7: the front-end role; 8-15: the CNN role
constexpr int kFusedBlock = 1024;    // 8 front-end + 8 CNN waves
// LDS carve after the front-end's (wk_fe_dev.h): fixed tail, then the CNN
// images [clip][t][ci] -- fp32, or bf16 for bf16 convolutions -- overlaying
// one region.  ci pitch = 8 mod 16 elements: the 16 t-lanes of each lane
// group of a B-fragment read (ds_read_b128 fp32 / ds_read_b64 bf16) and of the
// pooled stores land on distinct banks.
constexpr int kGOff = (kFeLds + 3) & ~3;            // pooled features [128][4] (16-byte aligned carve below)
constexpr int kFcpOff = kGOff + 128 * NBF;          // classifier.0 partials [8 k-slices][4 clips][64 o]
constexpr int kFcpSize = 8 * NBF * 64;
constexpr int kL1Off = kFcpOff + kFcpSize;          // second log-mel buffer [40][64] (first: kLOff)
static_assert(kLOff % 4 == 0 && kL1Off % 4 == 0, "log-mel buffers are read with ds_read_b128");
constexpr int kCtrlOff = kL1Off + kLSize;           // control words
constexpr int kImgOff = (kCtrlOff + 16 + 3) & ~3;   // 16-byte aligned
constexpr int I0_CIP = 24, I1_CIP = 40, I2_CIP = 72;                 // elements (= 8 mod 16)
// t rows: row 0 is the left zero guard, rows 1..L hold the L frames.  No right
// guard: every layer's length L is odd, so maxpool(2) drops the one output
// that would read it; the dropped outputs' reads of rows L+1, L+2 land in the
// next clip's (or the next image's) rows, which only affects their own MFMA
// columns.  conv3 keeps 2 spare rows so its last clip stays inside the carve.
constexpr int I0_TP = 64, I1_TP = 32, I2_TP = 18;
// fp32 images (float units), read by the Winograd convolutions in row pairs:
// pitch = 4 mod 8 floats keeps the stride-2 row reads conflict-free.
constexpr int F0_CIP = 20, F1_CIP = 36, F2_CIP = 68;
constexpr int kF0Off = kImgOff;
constexpr int kF1Off = kF0Off + NBF * I0_TP * F0_CIP;
constexpr int kF2Off = kF1Off + NBF * I1_TP * F1_CIP;
constexpr int kF2End = kF2Off + NBF * I2_TP * F2_CIP;
// bf16 images (the largest user of the carve is the split-bf16 set below)
constexpr int kImgEnd = kImgOff + NBF * (I0_TP * 40 + I1_TP * 72 + I2_TP * 136) / 2 > kF2End
                            ? kImgOff + NBF * (I0_TP * 40 + I1_TP * 72 + I2_TP * 136) / 2
                            : kF2End;
// bf16 images (offsets in float units)
constexpr int kB0Off = kImgOff;
constexpr int kB1Off = kB0Off + NBF * I0_TP * I0_CIP / 2;
constexpr int kB2Off = kB1Off + NBF * I1_TP * I1_CIP / 2;
// split-bf16 images (WK_PREC_BF16X3): xh at ci, xl at ci + 16 CB of the same row
constexpr int X0_CIP = 40, X1_CIP = 72, X2_CIP = 136;                // halfs (= 8 mod 16)
constexpr int kX0Off = kImgOff;
constexpr int kX1Off = kX0Off + NBF * I0_TP * X0_CIP / 2;
constexpr int kX2Off = kX1Off + NBF * I1_TP * X1_CIP / 2;
static_assert(kX2Off + NBF * I2_TP * X2_CIP / 2 <= kImgEnd, "split images fit the fp32 carve");
static_assert(kF1Off % 4 == 0 && kF2Off % 4 == 0 && kB1Off % 2 == 0 && kB2Off % 2 == 0 && kX1Off % 2 == 0 &&
                  kX2Off % 2 == 0, "vector-aligned images");
enum { kConvF32 = 0, kConvBf16 = 1, kConvBf16x3 = 2 };
// Scratch power row for the one frame slot past the clip (frame 63): its lanes
// still run the FFT so that the prefetch loads issued inside fe_rest execute.
constexpr int kDummyRowOff = (kImgEnd + 1) & ~1;          // even: the row is its own 8-byte aligned scratch
constexpr int kFusedLds = kDummyRowOff + kPRow;
static_assert(kFusedLds * 4 <= 163840, "fused LDS budget");
// The CNN role writes only inside [kGOff, kImgEnd) (pooled features,
// classifier partials, the second log-mel buffer it reads, control words,
// conv images); the front-end writes its power rows, the first log-mel
// buffer and (frame 63) the dummy row: the two write sets are disjoint.
static_assert(kPOff + kPSize <= kGOff && kLOff + kLSize <= kPOff && kImgEnd <= kDummyRowOff,
              "CNN carve disjoint from the front-end's power rows, log-mel buffer and dummy row");
// Inside the window, the front-end writes the second log-mel buffer and the
// control words; the CNN role's writes (pooled features, classifier partials,
// every precision's image set) sit in ranges that miss it.
static_assert(kGOff + 128 * NBF <= kFcpOff && kFcpOff + kFcpSize <= kL1Off && kL1Off + kLSize <= kCtrlOff &&
                  kCtrlOff + 16 <= kImgOff,
              "pooled features | partials | log-mel buffer 1 | control words, in that order, disjoint");
static_assert(kF2End <= kImgEnd && kB2Off + NBF * I2_TP * I2_CIP / 2 <= kImgEnd &&
                  kX2Off + NBF * I2_TP * X2_CIP / 2 <= kImgEnd,
              "every precision's conv images end inside [kImgOff, kImgEnd)");

// kCtrlLFree + w (w = CNN wave 0..7): clips whose log-mel buffer CNN wave w
// has finished reading.  Per wave, not one shared count: the CNN waves are not
// lock-stepped inside a batch's DCT loop (and the classifier.2 wave starts the
// next batch late), so a summed count can reach 8 (i - 1) while one wave is
// still reading clip i - 2's buffer -- 7 waves ahead by a clip or more paid
// for the laggard.  That race corrupted the laggard's DCT coefficients in ~1
// clip per 65k (seen with split-bf16 timing).  The other counters are sound as
// sums: their producers pass a barrier between consecutive signals.
enum { kCtrlFeBar = 0, kCtrlCnnBar = 1, kCtrlLReady = 2, kCtrlLFree = 4, kCtrlAbort = 15 };
static_assert(kCtrlOff % 4 == 0 && kCtrlLFree % 4 == 0, "spin_until_all8 reads the eight LFree words as two uint4");
// Every spin is bounded (~4M sleeps, well under a second): a protocol bug
// yields wrong logits and a drained grid, never a hung GPU.
constexpr unsigned kSpinLimit = 1u << 22;

__device__ __forceinline__ unsigned lds_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// The same word as a wave-uniform (SGPR) value: every lane reads the same
// address, and a spin's exit tests on an SGPR compile to a scalar compare and
// branch instead of the exec-mask bookkeeping of a divergent loop exit.
__device__ __forceinline__ unsigned lds_load_u(const unsigned* p) {
  return __builtin_amdgcn_readfirstlane(lds_load(p));
}

constexpr int kPrioFe = 3;     // issue priority of the front-end waves (the critical path; see the kernel)
constexpr int kSpinSleep = 2;  // s_sleep argument (x 64 cycles) between polls (2 measured >= 1; 4, 8 equal)

// Spin until ready() (a wave-uniform test of an LDS word).  On a timeout the
// workgroup's abort word is set and every later spin returns at once.  Every
// poll is issue time taken from the other waves of the SIMD, so a waiting wave
// drops to issue priority 0 (PRIO = the role's priority, restored on exit),
// polls four times per loop trip and checks the bound and the abort word only
// every 32nd poll: per poll a sleep, the read, its wait, one readfirstlane, a
// scalar compare and branch (the former one-poll loop with its two exits
// compiled to ~19 instructions of exec-mask bookkeeping per poll).
template <int PRIO, typename F>
__device__ __forceinline__ void spin_on(unsigned* ctrl, const F& ready) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  if (!ready()) {
    if (PRIO > 0) __builtin_amdgcn_s_setprio(0);
    for (unsigned n = 4;; n += 4) {
      __builtin_amdgcn_s_sleep(kSpinSleep);
      if (ready()) break;
      __builtin_amdgcn_s_sleep(kSpinSleep);
      if (ready()) break;
      __builtin_amdgcn_s_sleep(kSpinSleep);
      if (ready()) break;
      __builtin_amdgcn_s_sleep(kSpinSleep);
      if (ready()) break;
      if ((n & 31) == 0 && (n >= kSpinLimit || lds_load_u(ctrl + kCtrlAbort))) {
        __hip_atomic_store(ctrl + kCtrlAbort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        break;
      }
    }
    if (PRIO > 0) __builtin_amdgcn_s_setprio(PRIO);
  }
  asm volatile("" ::: "memory");
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// Spin until ctrl[idx] >= v.
template <int PRIO>
__device__ __forceinline__ void spin_until(unsigned* ctrl, int idx, unsigned v) {
  spin_on<PRIO>(ctrl, [=] { return lds_load_u(ctrl + idx) >= v; });
}

// Barrier among the 8 waves of one role (LDS counter; s_barrier would also
// stop the other role's waves).  LDS operations of a wave complete in order,
// so a wave's data writes are visible before its arrival is.
template <int PRIO>
__device__ __forceinline__ void role_sync(unsigned* ctrl, int idx, unsigned& gen, int lane) {
  gen += 8;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(ctrl + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  spin_until<PRIO>(ctrl, idx, gen);
}

// Spin until ctrl[idx + w] >= v for all w < 8 (same rules as spin_until).
// The eight words are 16-byte aligned (idx = kCtrlLFree = 4): two 16-byte LDS
// reads per poll instead of eight.
__device__ __forceinline__ unsigned min8(const unsigned* ctrl, int idx) {
  asm volatile("" ::: "memory");
  const uint4* q = reinterpret_cast<const uint4*>(ctrl + idx);
  const uint4 a = q[0], b = q[1];
  return min(min(min(a.x, a.y), min(a.z, a.w)), min(min(b.x, b.y), min(b.z, b.w)));
}
template <int PRIO>
__device__ __forceinline__ void spin_until_all8(unsigned* ctrl, int idx, unsigned v) {
  spin_on<PRIO>(ctrl, [=] { return __builtin_amdgcn_readfirstlane(min8(ctrl, idx)) >= v; });
}

// Publish a per-wave progress value once this wave's LDS ops are complete.
__device__ __forceinline__ void signal_set(unsigned* ctrl, int idx, unsigned v, int lane) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_store(ctrl + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

__device__ __forceinline__ void signal_add(unsigned* ctrl, int idx, int lane) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(ctrl + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// Protocol health: a spin that timed out set its role's abort word, and every
// logit of the launch is then suspect.  Each wave reports what it sees on exit
// to the handle's error word (host-visible; read by wk_check_device_errors /
// wk_stream_push): bit 0 = a spin timed out, bit 1 = the abort word holds a
// value no spin writes (LDS corruption).
__device__ __forceinline__ void report_abort(const unsigned* ctrl, unsigned* err, int lane) {
  if (lane == 0 && err) {
    const unsigned ab = lds_load(ctrl + kCtrlAbort);
    if (ab) __hip_atomic_store(err, ab == 1u ? 1u : 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace
