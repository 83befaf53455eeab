// K24: the verdict of one rule of the ls rows (docs/SHIFT.md), exact, shared by the kernels of
// shift.hip and the host (bindings.cpp shift_verdict).
//
//   mB, mR  finite samples of the baseline / of the recent span
//   T2, X2  twice the baseline's / the recent span's percentile q / 1000 (the int64 sum of the one
//           or two ranks K16's rank rule reads; 0 without a finite sample)
//   a, b    recent finite samples v with 2 v > T2 / with 2 v < T2 (a + b <= mR)
// With S = 100000 the rule is judged when mB >= min_baseline and mR >= min_recent; then
//   U  (r_u != 0):  X2 - T2 >= 2 min_delta,  1000 a S >= r_u mR (S - q),  a S >= mR (S - q),
//                   (a S - mR (S - q))^2 * 10^6 >= z^2 mR q (S - q)
//   D  (r_d != 0):  T2 - X2 >= 2 min_delta,  1000 b S >= r_d mR q,        b S >= mR q,
//                   (b S - mR q)^2 * 10^6 >= z^2 mR q (S - q)
// which is the share of recent samples above (below) the baseline's percentile against up (down)
// times the share 1 - p (p) the percentile itself predicts, and against z / 1000 binomial standard
// deviations over that expectation, without a division or a square root.  Both cannot hold:
// min_delta >= 1.
//
// Width.  a, b, mR < 2^31; S, q, S - q < 2^17; r_u, r_d <= 10^6 < 2^20; z <= 10^5 < 2^17.  Then
//   1000 a S                  < 2^10 * 2^31 * 2^17        = 2^58
//   r mR (S - q),  r mR q     < 2^20 * 2^31 * 2^17        = 2^68
//   a S,  mR (S - q),  mR q   < 2^31 * 2^17               = 2^48   (so is their difference)
//   (difference)^2 * 10^6     < 2^96 * 2^20               = 2^116
//   z^2 mR q (S - q)          < 2^34 * 2^31 * 2^17 * 2^17 = 2^99
// so the ratio and the z test do not fit 64 bits and every product is an unsigned __int128 (a
// multiplication only: it compiles inline for the device, no library call).  |T2|, |X2| < 2^32 (two
// int32 samples), so X2 - T2 and 2 min_delta (min_delta < 2^30) are exact in int64.  The callers
// keep their operands inside these bounds (the binding checks them, the kernels' come from int32
// counts and samples and the validated settings).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace apm {

constexpr int LS_N = 0, LS_U = 1, LS_D = 2;  // a rule's verdict
constexpr int LS_SCALE = 100000;             // q of 100 % (winsort.h WP_SCALE)

// one side: c of the mR recent samples beyond the percentile, e = S - q (up) or q (down) the share
// * S it predicts, r the ratio * 1000, z * 1000, var = q (S - q)
__host__ __device__ inline bool shift_side(uint32_t c, uint32_t mR, uint32_t e, uint32_t r, uint32_t z, uint64_t var) {
  typedef unsigned __int128 u128;
  const uint64_t got = (uint64_t)c * LS_SCALE;  // < 2^48
  const uint64_t exp = (uint64_t)mR * e;        // < 2^48
  if ((u128)(got * 1000u) < (u128)((uint64_t)r * mR) * e) return false;  // 2^58 against 2^68
  if (got < exp) return false;
  const uint64_t d = got - exp;                 // < 2^48
  return (u128)d * d * 1000000u >= (u128)((uint64_t)z * z) * mR * var;   // 2^116 against 2^99
}

// q in 1 .. 99999; r_u, r_d 0 or in 1001 .. 1000000 (0: that side is not tested); z in 0 .. 100000;
// min_delta in 1 .. 2^30 - 1; a, b <= mR; min_recent, min_baseline >= 1
__host__ __device__ inline int shift_verdict(int32_t a, int32_t b, int32_t mR, int32_t mB, int64_t T2, int64_t X2, int32_t q,
                                             int32_t r_u, int32_t r_d, int32_t z, int32_t min_delta, int32_t min_recent,
                                             int32_t min_baseline) {
  if (mB < min_baseline || mR < min_recent) return LS_N;
  const uint64_t var = (uint64_t)q * (uint64_t)(LS_SCALE - q);  // < 2^34
  const int64_t floor2 = 2 * (int64_t)min_delta;
  if (r_u != 0 && X2 - T2 >= floor2 &&
      shift_side((uint32_t)a, (uint32_t)mR, (uint32_t)(LS_SCALE - q), (uint32_t)r_u, (uint32_t)z, var))
    return LS_U;
  if (r_d != 0 && T2 - X2 >= floor2 && shift_side((uint32_t)b, (uint32_t)mR, (uint32_t)q, (uint32_t)r_d, (uint32_t)z, var))
    return LS_D;
  return LS_N;
}

}  // namespace apm
