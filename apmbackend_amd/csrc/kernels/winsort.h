// Window-sample helpers shared by K8 (stats.hip), K16 (winpct.hip), K17 (slo.hip) and K19
// (svcwin.hip): the 32-lane DPP moves and
// register sorting networks of the two-series-per-wave kernels, the block-wide visit of a series'
// window samples, and the exact radix select of R order statistics.  Moved out of stats.hip
// unchanged (as spill.h was for K15); window_select_ranks<R> is K8's four-rank select with the
// rank count a template parameter, window_select_visit<R> the same with the sample visit one as
// well; wp_ranks is the integer rank rule of the wp / sv percentiles.
#pragma once
#include "kernel_api.h"
#include "spill.h"

namespace apm {

// slot of window bucket r (kernel arguments for the first K8_INLINE_SLOTS, then a device array)
__device__ __forceinline__ int win_slot(const WindowArgs& a, int r) {
  return r < K8_INLINE_SLOTS ? a.win_slots[r] : a.win_slots_ext[r];
}

constexpr int HW = 32;                 // lanes per series

// Cross-lane moves inside a 32-lane half without the LDS crossbar (ds_bpermute): DPP where the
// pattern stays inside a 16-lane row (quad permutes for xor 1 / 2, a quad reversal then
// row_half_mirror for xor 4, row_ror:8 for xor 8, row shifts and row_bcast:15 for scans), and
// ds_swizzle (no LDS bank access, no address VGPR) only for xor 16, the one move between rows.
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ int dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xF, false); }
template <int J>
__device__ __forceinline__ int32_t half_xor(int32_t v) {
  if constexpr (J == 1) return dpp<0xB1>(v);          // quad_perm [1,0,3,2]
  else if constexpr (J == 2) return dpp<0x4E>(v);     // quad_perm [2,3,0,1]
  else if constexpr (J == 8) return dpp<0x128>(v);    // row_ror:8 == xor 8 inside a row
  else if constexpr (J == 4) return dpp<0x141>(dpp<0x1B>(v));  // quad_perm [3,2,1,0], row_half_mirror: i^3^7
  else return __builtin_amdgcn_ds_swizzle(v, 0x401F);         // BitMode xor 16
}
// inclusive prefix sum over each 32-lane half
__device__ __forceinline__ int half_scan(int x) {
  x += dpp<0x111>(x);        // row_shr:1
  x += dpp<0x112>(x);        // row_shr:2
  x += dpp<0x114>(x);        // row_shr:4
  x += dpp<0x118>(x);        // row_shr:8
  x += dpp<0x142, 0xA>(x);   // row_bcast:15 -> rows 1, 3
  return x;
}
// the same for doubles (exact sums of integers below 2^53): the two words move together
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ double dpp_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = dpp<CTRL, ROWS>((int)(b & 0xffffffffll));
  const int hi = dpp<CTRL, ROWS>((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double half_scan_f64(double x) {
  x += dpp_f64<0x111>(x);
  x += dpp_f64<0x112>(x);
  x += dpp_f64<0x114>(x);
  x += dpp_f64<0x118>(x);
  x += dpp_f64<0x142, 0xA>(x);
  return x;
}
// lane 31 of this half (a half's total after half_scan): two readlanes, no crossbar
__device__ __forceinline__ int half_last(int x, int half) {
  const int a = __builtin_amdgcn_readlane(x, 31), b = __builtin_amdgcn_readlane(x, 63);
  return half ? b : a;
}
__device__ __forceinline__ double half_last_f64(double x, int half) {
  const long long v = __double_as_longlong(x);
  const int lo = half_last((int)(v & 0xffffffffll), half), hi = half_last((int)(v >> 32), half);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int K, int J>
__device__ __forceinline__ int32_t bitonic_step(int32_t v, int hl) {
  const int32_t o = half_xor<J>(v);
  const bool keep_min = ((hl & J) == 0) == ((hl & K) == 0);
  return keep_min ? min(v, o) : max(v, o);
}
template <int K>
__device__ __forceinline__ int32_t bitonic_merge(int32_t v, int hl) {
  if constexpr (K >= 32) v = bitonic_step<K, 16>(v, hl);
  if constexpr (K >= 16) v = bitonic_step<K, 8>(v, hl);
  if constexpr (K >= 8) v = bitonic_step<K, 4>(v, hl);
  if constexpr (K >= 4) v = bitonic_step<K, 2>(v, hl);
  return bitonic_step<K, 1>(v, hl);
}

// Register bitonic sort of a 32-lane half's N = 32 E samples, E per lane.  Index bits 0-3 are the
// lane's position in its 16-lane row (DPP moves), bits 4 .. 3 + log2 E the element (moves inside
// the lane), and the top bit the row (ds_swizzle xor 16): the top bit is compared in one stage
// only, so the network makes E swizzles in all and no LDS access (the LDS form below made ~20
// loads / stores per stage for a 256-sample window).
template <int E>
__device__ __forceinline__ void reg_bitonic(int32_t (&v)[E], int hl) {
  constexpr int N = 32 * E;
  const int base = (hl >> 4) * (16 * E) + (hl & 15);
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= 16 && j < 16 * E) {
        const int je = j >> 4;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (e & je) continue;
          const bool up = ((base + e * 16) & k) == 0;
          const int32_t x = v[e], y = v[e | je];
          v[e] = up ? min(x, y) : max(x, y);
          v[e | je] = up ? max(x, y) : min(x, y);
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int i = base + e * 16;
          int32_t o;
          if (j == 1) o = half_xor<1>(v[e]);
          else if (j == 2) o = half_xor<2>(v[e]);
          else if (j == 4) o = half_xor<4>(v[e]);
          else if (j == 8) o = half_xor<8>(v[e]);
          else o = half_xor<16>(v[e]);
          const bool keep_min = ((i & j) == 0) == ((i & k) == 0);
          v[e] = keep_min ? min(v[e], o) : max(v[e], o);
        }
      }
    }
  }
}

// Sorts the half's n (<= 32 E) samples in t[0, n) in place (t holds at least 32 E entries).
template <int E>
__device__ __forceinline__ void half_sort_regs(int32_t* t, int n, int hl) {
  const int base = (hl >> 4) * (16 * E) + (hl & 15);
  int32_t v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = base + e * 16 < n ? t[base + e * 16] : 0x7fffffff;
  reg_bitonic<E>(v, hl);
#pragma unroll
  for (int e = 0; e < E; ++e) t[base + e * 16] = v[e];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

// Every sample of series s in the window (inline cells + spill lists), visited by the block.
template <class F>
__device__ __forceinline__ void for_each_window_sample(const WindowArgs& a, int s, F&& f) {
  for (int r = 0; r < a.n_win; ++r) {
    const int sl = win_slot(a, r);
    if (sl < 0) continue;
    const int cnt = a.st.counts[(size_t)sl * a.st.S + s];
    const int inl = min(cnt, a.st.cap);
    const int32_t* cell = a.st.cells + ((size_t)sl * a.st.S + s) * a.st.cap;
    for (int k = threadIdx.x; k < inl; k += blockDim.x) f(cell[k]);
    if (cnt > inl) {
      const int32_t* run = spill_run(a.st, sl, s);
      for (int k = threadIdx.x; k < cnt - inl; k += blockDim.x) f(run[k]);
    }
  }
}

// Exact k-th smallest of the samples `visit` enumerates, R ranks (ascending order of all samples,
// ELAPSED_NAN = INT32_MIN first) selected together by the whole block: K8's radix select
// (stats.hip window_select), 8 bits per pass, four passes over the window's samples, with the
// rank count a template parameter.  Ranks whose keys agree in the bits fixed so far would count
// the same samples into equal histograms (all of them in the first pass, neighbouring ranks such
// as a percentile's pair in most later ones): only the first rank of such a group counts, the
// others read its row, so a sample costs one LDS atomic per distinct prefix instead of R.
// `hist` holds R x 256 LDS bins.  Returns the R keys in LDS: after the call (it ends in a
// __syncthreads) key[r] ^ 0x80000000 is the sample of rank ranks[r].  Every thread of the block
// calls it with the same arguments.  `visit(f)` calls f(sample) for every sample once, the samples
// shared out over the block's threads, and is called four times (one series' window:
// window_select_ranks below; the windows of a service's series: svcwin.hip).
template <int R, class V>
__device__ __forceinline__ const uint32_t* window_select_visit(V&& visit, const int (&ranks)[R], uint32_t* hist) {
  __shared__ uint32_t prefix[R];
  __shared__ int32_t want[R];
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (threadIdx.x == r) { prefix[r] = 0; want[r] = ranks[r]; }
  __syncthreads();
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t hi_mask = pass == 0 ? 0u : ~((1u << (shift + 8)) - 1u);
    for (int i = threadIdx.x; i < R * 256; i += blockDim.x) hist[i] = 0;
    uint32_t pf[R];
#pragma unroll
    for (int r = 0; r < R; ++r) pf[r] = prefix[r] & hi_mask;
    // row[r]: the first rank with r's prefix; lead: the ranks that are their own row
    uint32_t lead = 0;
    int my_row = 0;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
      int row = r;
#pragma unroll
      for (int o = r - 1; o >= 0; --o)
        if (pf[o] == pf[r]) row = o;
      if (row == r) lead |= 1u << r;
      if ((int)threadIdx.x == r) my_row = row;
    }
    __syncthreads();
    visit([&](int32_t v) {
      const uint32_t u = (uint32_t)v ^ 0x80000000u;  // order-preserving unsigned key
      const uint32_t bin = (u >> shift) & 255u;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (((lead >> r) & 1u) && (u & hi_mask) == pf[r]) atomicAdd(&hist[r * 256 + bin], 1u);
    });
    __syncthreads();
    if (threadIdx.x < R) {
      const int r = threadIdx.x;
      int k = want[r];
      uint32_t b = 0;
      for (; b < 256; ++b) {
        const int c = (int)hist[my_row * 256 + b];
        if (k < c) break;
        k -= c;
      }
      want[r] = k;
      prefix[r] |= (b & 255u) << shift;
    }
    __syncthreads();
  }
  return prefix;
}

// the ranks of series s's window
template <int R>
__device__ __forceinline__ const uint32_t* window_select_ranks(const WindowArgs& a, int s, const int (&ranks)[R],
                                                               uint32_t* hist) {
  return window_select_visit<R>([&](auto&& f) { for_each_window_sample(a, s, f); }, ranks, hist);
}

constexpr int WP_SCALE = 100000;       // q of 100 %

// The (lo, hi) ranks among m >= 1 ascending samples for percentile q / 1000: t = q m; a multiple
// of 100000 reads rank t / 100000 - 1; else i = ceil(t / 100000) - 1 = floor(t / 100000) and
// (i, i + 1), or (i, i) at the last sample.  m == 1: rank 0.
__device__ __forceinline__ void wp_ranks(int m, int q, int& lo, int& hi) {
  if (m == 1) { lo = hi = 0; return; }
  const long long t = (long long)q * (long long)m;
  const int i = (int)(t / WP_SCALE);
  if (t % WP_SCALE == 0) { lo = hi = i - 1; return; }
  lo = i;
  hi = i == m - 1 ? i : i + 1;
}

}  // namespace apm
