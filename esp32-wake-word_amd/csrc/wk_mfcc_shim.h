// wk_mfcc_shim.h -- what the mfcc.h drop-ins of both libraries share (internal;
// wk_compat.hip for libwakeword.so, wk_host.cpp for libwakeword_host.so):
// mfcc.c's argument checks with their messages, its frame count, and
// analyze_mfcc_range.  Plain C++, no HIP.
#pragma once
#include <math.h>
#include <stdio.h>

namespace wk {
namespace shim {

// extract_mfcc's arguments; false (message printed) = return NULL.
inline bool check_signal(const float* signal, int signal_len, int frame_size, int hop_size) {
  // mfcc.c:434-437: NULL signal or a signal shorter than one frame -> NULL.
  if (!signal || signal_len < frame_size || frame_size <= 0) {
    fprintf(stderr, "E (MFCC) Invalid signal parameters\n");
    return false;
  }
  if (hop_size < 1) {   // (mfcc.c:447 divides by it)
    fprintf(stderr, "E (MFCC) Invalid hop size\n");
    return false;
  }
  return true;
}

// flow_extract_mfcc_single_frame's (mfcc.c:300-303).
inline bool check_frame(const float* frame, int frame_size, int n_fft) {
  if (!frame || frame_size <= 0 || frame_size > n_fft) {
    fprintf(stderr, "E (MFCC) Invalid frame parameters\n");
    return false;
  }
  return true;
}

inline int frame_count(int signal_len, int frame_size, int hop_size) { return (signal_len - frame_size) / hop_size + 1; }

// mfcc.c:530-553: min/max/avg over the finite entries.
inline void analyze_range(const float* mfcc, int size, const char* label) {
  if (!mfcc || size <= 0) return;
  float mn = INFINITY, mx = -INFINITY, sum = 0.0f;
  int valid = 0;
  for (int i = 0; i < size; i++) {
    if (!isnan(mfcc[i]) && !isinf(mfcc[i])) {
      if (mfcc[i] < mn) mn = mfcc[i];
      if (mfcc[i] > mx) mx = mfcc[i];
      sum += mfcc[i];
      valid++;
    }
  }
  if (valid > 0)
    printf("I (MFCC) %s MFCC Range: min=%.6f, max=%.6f, avg=%.6f, valid=%d/%d\n", label ? label : "", mn, mx,
           sum / valid, valid, size);
  else
    fprintf(stderr, "E (MFCC) %s MFCC: No valid values\n", label ? label : "");
  fflush(stdout);
}

}  // namespace shim
}  // namespace wk
