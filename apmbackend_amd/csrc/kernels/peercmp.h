// K23: the verdict of one member of the po rows (docs/PEERS.md), exact, shared by the kernels of
// peers.hip and the host (bindings.cpp peer_verdict).
//
//   x   the member's window percentile as K16 stores it: the int64 sum of the one or two ranks read
//       (twice the percentile)
//   X2  x_lo + x_hi of the E eligible members' sorted x (twice their median), D4 = d_lo + d_hi of the
//       sorted d_i = |2 x_i - X2| (four times their median absolute deviation)
// The group is judged when E >= min_peers and X2 >= 4 * min_value; then
//   H  (r_h != 0):  2000 x >= r_h X2   and   4000 x >= 2000 X2 + z D4   and   2 x - X2 >= 4 min_delta
//   L  (r_l != 0):  2000 x <= r_l X2   and   4000 x <= 2000 X2 - z D4   and   X2 - 2 x >= 4 min_delta
// which is x against high (low) times the median, against the median plus (minus) z / 1000 MADs and
// against an absolute distance from the median, without a division.
//
// Width.  A sample is an int32 and may be negative, so |x| < 2^32, |X2| < 2^33, every d < 2^35 and
// D4 < 2^36; r_l < 2^10; r_h <= 10^6 < 2^20; z <= 10^5 < 2^17; min_value, min_delta < 2^31.  Then
//   4000 |x|        < 2^12 * 2^32   = 2^44
//   r_h |X2|        < 2^20 * 2^33   = 2^53
//   2000 |X2|       < 2^11 * 2^33   = 2^44
//   z D4            < 2^17 * 2^36   = 2^53
//   4 min_value, 4 min_delta        < 2^33,   |2 x - X2| < 2^34
// all below 2^63: signed 64-bit arithmetic is exact.  The L test's right-hand side may be negative
// (z D4 > 2000 X2); x may be negative too, so that is an ordinary comparison.  The callers keep their
// operands inside these bounds (the binding checks them, the kernels' come from int32 samples and
// the validated settings).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace apm {

constexpr int PO_N = 0, PO_H = 1, PO_L = 2;  // a member's verdict

// r_h 0 or in 1001 .. 1000000 (0: no H test); r_l in 0 .. 999 (0: no L test); z in 0 .. 100000;
// min_value >= 1; min_delta, min_peers, E >= 0
__host__ __device__ inline int peer_verdict(int64_t x, int64_t X2, int64_t D4, int32_t E, int32_t r_h, int32_t r_l, int32_t z,
                                            int32_t min_value, int32_t min_delta, int32_t min_peers) {
  if (E < min_peers || X2 < 4 * (int64_t)min_value) return PO_N;
  const int64_t dev = (int64_t)z * D4;
  const int64_t floor4 = 4 * (int64_t)min_delta;
  if (r_h != 0 && 2000 * x >= (int64_t)r_h * X2 && 4000 * x >= 2000 * X2 + dev && 2 * x - X2 >= floor4) return PO_H;
  if (r_l != 0 && 2000 * x <= (int64_t)r_l * X2 && 4000 * x <= 2000 * X2 - dev && X2 - 2 * x >= floor4) return PO_L;
  return PO_N;
}

}  // namespace apm
