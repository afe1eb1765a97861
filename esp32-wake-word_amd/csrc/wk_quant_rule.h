// wk_quant_rule.h -- the power-of-2 quantiser's exponent rule, for the host (weight exponents, wk_calibrate) and
// the device (activation bins), both in wk_quant.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wk {

// b(a) = min{e : |a| <= 127 * 2^e} from the float's bit pattern, clamped to [-24, 7] (zeros lowest).
// 127 * 2^e = 1.984375 * 2^(e + 6), mantissa field 0x7E0000, so with exponent field E it is E - 6 up to that
// mantissa and E - 5 above it: two integer operations on the bits, exact.
__host__ __device__ inline int hold_exp(float a) {
  const uint32_t u = __builtin_bit_cast(uint32_t, a) & 0x7FFFFFFFu;
  const int b = (int)(u >> 23) - 127 - ((u & 0x7FFFFFu) <= 0x7E0000u ? 6 : 5);
  return u == 0 || b < -24 ? -24 : (b > 7 ? 7 : b);
}

}  // namespace wk
