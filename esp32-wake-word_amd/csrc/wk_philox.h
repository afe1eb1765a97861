// wk_philox.h -- Philox4x32-10 (Salmon et al., "Parallel random numbers: as
// easy as 1, 2, 3", SC'11) as a device function: a stateless, counter-based
// generator.  One call turns a 128-bit counter and a 64-bit key into four
// 32-bit words; nothing is kept between calls, so a value is a function of
// its address alone and can be made again wherever it is needed.
//
// Known answers (counter, key -> words), held by tests/test_ctc_dropout_ref.py
// against the numpy statement of the same rounds and, through the mask export,
// against the kernels:
//   {0, 0, 0, 0}, {0, 0}                                   6627e8d5 e169c58d bc57ac4c 9b00dbd8
//   all ones, all ones                                     408f276d 41c83b0e a20bc7c6 6d5451fd
//   {243f6a88, 85a308d3, 13198a2e, 03707344},
//   {a4093822, 299f31d0}                                   d16cfe09 94fdcceb 5001e420 24126ea1
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wk {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;   // the round's two multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;   // the key's Weyl increments

__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, ctr.x), lo0 = kPhiloxM0 * ctr.x;
    const uint32_t hi1 = __umulhi(kPhiloxM1, ctr.z), lo1 = kPhiloxM1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += kPhiloxW0;   // (the bump after the tenth round is unused)
    key.y += kPhiloxW1;
  }
  return ctr;
}

}  // namespace wk
