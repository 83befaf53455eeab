// K21: the burn-rate inequality of the sb rows (docs/BURN.md), exact, shared by the kernels of
// burn.hip and the host (bindings.cpp burn_fires):
//
//   a set of m finite samples, `bad` of them above the threshold, burns at factor f / 1000 when
//   m >= min_samples and bad * 10^8 >= f * m * b        (b = 100000 - q, the error budget)
//
// which is (bad / m) / (b / 100000) >= f / 1000 without a division.  With f <= 10^6, b < 10^5 and
// m < 2^31 the right-hand side needs up to 68 bits, so both sides are built as three 32-bit limbs:
// one 32 x 32 -> 64 multiply and one add per limb, plain C++ on both sides of the compiler (no
// 128-bit type, no builtin).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace apm {

struct BurnU96 {
  uint32_t w0, w1, w2;  // little endian limbs
};

// x * y, x below 2^64 (w2 == 0 on entry is not required: the product must fit 96 bits, which every
// caller's operands guarantee)
__host__ __device__ inline BurnU96 burn_mul32(BurnU96 x, uint32_t y) {
  const uint64_t p0 = (uint64_t)x.w0 * y;
  const uint64_t p1 = (uint64_t)x.w1 * y + (p0 >> 32);
  const uint64_t p2 = (uint64_t)x.w2 * y + (p1 >> 32);
  return BurnU96{(uint32_t)p0, (uint32_t)p1, (uint32_t)p2};
}

__host__ __device__ inline bool burn_ge(BurnU96 a, BurnU96 b) {
  if (a.w2 != b.w2) return a.w2 > b.w2;
  if (a.w1 != b.w1) return a.w1 > b.w1;
  return a.w0 >= b.w0;
}

// bad, m: 0 .. 2^31 - 1; b: 1 .. 99999; f: 1 .. 1000000; min_samples >= 1
__host__ __device__ inline bool burn_fires(uint32_t bad, uint32_t m, uint32_t b, uint32_t f, uint32_t min_samples) {
  if (m < min_samples) return false;
  const BurnU96 lhs = burn_mul32(BurnU96{bad, 0u, 0u}, 100000000u);       // < 2^58
  const BurnU96 rhs = burn_mul32(burn_mul32(BurnU96{f, 0u, 0u}, b), m);   // < 2^68
  return burn_ge(lhs, rhs);
}

}  // namespace apm
