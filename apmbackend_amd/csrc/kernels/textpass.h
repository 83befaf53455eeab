// What the count / scan / write text passes share (format.hip K12, hist.hip K15, winpct.hip K16,
// slo.hip K17, svcwin.hip K19), next to the line writer of textout.h: the exclusive scan of the row
// lengths and its scratch size, the length kernel over a row policy, the block copy-out of an LDS
// stage and the half-value printer.
//
// Every device helper here is __forceinline__ and takes the writer as OutT<W>& only that way: a
// reference to the writer passed into a function that is not inlined puts the whole OutT into
// scratch memory (textout.h).
#pragma once

#include "textout.h"

#include "prim.h"

namespace apm {

// row lengths len[0, n) -> exclusive byte offsets off[0, n); with the sentinel len[n - 1] = 0 the
// last offset is the total
inline int text_scan(PrimScratch& sc, const uint32_t* len, uint32_t* off, size_t n, hipStream_t stream) {
  return prim_exclusive_scan(sc, len, off, 0u, n, rocprim::plus<uint32_t>(), stream);
}

// scratch of text_scan over n_max rows and the sentinel
inline size_t text_scan_tmp_bytes(int32_t n_max) {
  PrimScratch q;
  text_scan(q, nullptr, nullptr, (size_t)n_max + 1, 0);
  return q.need;
}

// The length pass, one lane per emission position.  Row::len(a, i) finds the row position i prints
// and counts its bytes (0: no row); position n stores the scan sentinel (-> total).
template <class Row, int BLOCK, class Args>
__global__ __launch_bounds__(BLOCK) void k_text_len(Args a) {
  const int32_t i = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
  if (i > a.n) return;
  a.len[i] = i < a.n ? Row::len(a, i) : 0u;
}

constexpr uint32_t text_len_blocks(int32_t n, int block) { return (uint32_t)((n + 1 + block - 1) / block); }

// Lengths + scan: afterwards a->off[0..n] hold exclusive offsets, [n] = total bytes.  a->len and
// a->off hold n + 1 entries.  0, or -1 when the scratch is too small (nothing scanned).
template <class Row, int BLOCK, class Args>
inline int text_plan(Args* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  if (a->n <= 0) return 0;
  hipLaunchKernelGGL((k_text_len<Row, BLOCK, Args>), dim3(text_len_blocks(a->n, BLOCK)), dim3(BLOCK), 0, stream, *a);
  PrimScratch sc(tmp, tmp_bytes);
  return text_scan(sc, a->len, a->off, (size_t)a->n + 1, stream);
}

// A block's byte range [g0, g1) of the output from its LDS stage (laid out like the output from
// g0 & ~3 on), by LANES threads: one dword per lane per store (256 B per store instruction of a
// wave); the block's first / last dword is shared with a neighbour: byte stores.
template <int LANES>
__device__ __forceinline__ void block_copy_out(const char* __restrict__ lds, char* __restrict__ out, uint32_t g0,
                                               uint32_t g1) {
  const uint32_t a0 = g0 & ~3u;
  const uint32_t nd = (g1 - a0 + 3) / 4;
  for (uint32_t d = threadIdx.x; d < nd; d += LANES) {
    const uint32_t ga = a0 + 4 * d;
    if (ga >= g0 && ga + 4 <= g1) {
      *reinterpret_cast<uint32_t*>(out + ga) = *reinterpret_cast<const uint32_t*>(lds + 4 * d);
    } else {
      for (uint32_t b = 0; b < 4; ++b)
        if (ga + b >= g0 && ga + b < g1) out[ga + b] = lds[4 * d + b];
    }
  }
}

// v / 2 for the int64 sum v of two ranks, |v| <= 2^32 (the integer half fits 32 bits): the integer
// part, then ".5" when v is odd
template <bool W>
__device__ __forceinline__ void text_half(OutT<W>& o, long long v) {
  const unsigned long long mag = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
  if (v < 0) o.c('-');
  o.u32((uint32_t)(mag >> 1));
  if (mag & 1ull) o.lit(".5");
}

}  // namespace apm
