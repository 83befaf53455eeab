// K22: the verdict of one rule of the tf rows (docs/TRAFFIC.md), exact, shared by the kernels of
// traffic.hip and the host (bindings.cpp traffic_verdict).
//
//   R     samples of the newest k' = min(k, n_win) window buckets
//   med2  twice the median, mad4 four times the median absolute deviation of the counts of the
//         other B buckets
// The rule is judged when B >= min_buckets and med2 >= 2 * min_rate; then
//   drop   (r_d != 0):  2000 R <= r_d k' med2   and   4000 R <= k' (2000 med2 - z mad4)
//   surge  (r_s != 0):  2000 R >= r_s k' med2   and   4000 R >= k' (2000 med2 + z mad4)
// which is R / k' against drop (surge) times the median, and against the median minus (plus)
// z / 1000 MADs, without a division.
//
// Width.  A bucket's count is an int32, so c < 2^31; k' <= 64 = 2^6; r_d < 2^10; r_s <= 10^6 < 2^20;
// z <= 10^5 < 2^17.  Then R < 2^37, med2 < 2^32, every |2 c - med2| < 2^32 and so mad4 < 2^33, and
//   4000 R             < 2^12 * 2^37          = 2^49
//   r_s k' med2        < 2^20 * 2^6 * 2^32    = 2^58      (r_d k' med2 < 2^48)
//   2000 med2          < 2^11 * 2^32          = 2^43
//   z mad4             < 2^17 * 2^33          = 2^50
//   k' (2000 med2 + z mad4) < 2^6 * 2^51      = 2^57
// all below 2^63: signed 64-bit arithmetic is exact, and the drop test's right-hand side may be
// negative (z mad4 > 2000 med2), in which case no R >= 0 satisfies it.  The callers keep their
// operands inside these bounds (the binding checks them, the kernels' come from int32 counts and
// the validated rules).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace apm {

constexpr int TF_N = 0, TF_D = 1, TF_S = 2;  // a rule's verdict

// kk = k' in 1 .. 64; r_d in 0 .. 999 (0: no drop test); r_s 0 or in 1001 .. 1000000 (0: no surge
// test); z in 0 .. 100000; B, min_buckets >= 0; min_rate >= 1
__host__ __device__ inline int traffic_verdict(int64_t R, int64_t med2, int64_t mad4, int32_t B, int32_t kk, int32_t r_d,
                                               int32_t r_s, int32_t z, int32_t min_rate, int32_t min_buckets) {
  if (B < min_buckets || med2 < 2 * (int64_t)min_rate) return TF_N;
  const int64_t k = kk;
  const int64_t dev = (int64_t)z * mad4;
  if (r_d != 0 && 2000 * R <= (int64_t)r_d * k * med2 && 4000 * R <= k * (2000 * med2 - dev)) return TF_D;
  if (r_s != 0 && 2000 * R >= (int64_t)r_s * k * med2 && 4000 * R >= k * (2000 * med2 + dev)) return TF_S;
  return TF_N;
}

}  // namespace apm
