// K20: rw rows -- exact stats of the newest buckets of the K8 window (docs/RECENT.md).
//
// A span of k buckets is the window entries r >= n_win - min(k, n_win) (r = n_win - 1 is the
// newest).  Value pass, on the window K8 just read (same slots, same samples, spill lists still
// sorted), one record per (series, span) for every series with an st row whose window holds a sample:
//   group  32 lanes per series, two series a wave (as K16): lane r owns window entry r, and only the
//          entries of the largest span are gathered into the half's LDS tile -- newest entry first,
//          a bucket's start the sample count of all newer buckets (a suffix sum over the half), so
//          span j is the prefix [0, n_j) of the tile and the tile is filled once.  A lane counts the
//          NaN samples and sums the finite ones of its own bucket; a span's nan and sum are those
//          reduced over the span's lanes.  The spans are taken in ascending order: the prefix is
//          sorted by K8's register networks (winsort.h reg_bitonic) and the ranks read at nan + rank.
//          The write-back is guarded (rw_sort_prefix): half_sort_regs stores its padding beyond n,
//          which here is the next span's samples.  A sorted prefix stays a valid part of the next.
//          Windows of more than RW_GROUP_WIN buckets, and series whose largest span holds more than
//          RW_GROUP_MAX samples, are deferred (big_list) -- the span's own count decides, not
//          WinStat.n: old load outside every span costs nothing here.
//   block  one block per deferred series: per span one pass counts n, nan and the sum, then all 2Q
//          ranks are radix-selected together over the same entries (window_select_visit).
// Only integers: the rank rule is K16's wp_ranks on q = p * 1000, a value the int64 sum of the two
// ranks (one rank: twice the sample).
// Text pass: K12's count / scan / write shape, one lane per (emission position, span) -- index
// i * nspan + j, as K12 lays out its fs lines -- through textout.h; the length kernel, the scan and
// the half-value printer are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "spill.h"
#include "winsort.h"

namespace apm {

namespace {

constexpr int RW_WAVES = 4;            // waves per block (group pass): eight series
constexpr int RW_GROUP_MAX = 512;      // samples a 32-lane group sorts itself (its LDS tile)
constexpr int RW_GROUP_WIN = HW;       // window buckets a group covers (one per lane)
constexpr int RW_BLOCK = 512;          // threads per series (block pass)
constexpr int RW_BIG_GRID = 512;       // blocks of the block pass (they loop over big_list)
constexpr int RW_TEXT_BLOCK = 256;

__device__ __forceinline__ int half_sum(int x, int half) { return half_last(half_scan(x), half); }

// the int64 total of a 32-lane half, in every lane of it: the two words move together (DPP)
template <int J>
__device__ __forceinline__ long long half_xor_i64(long long v) {
  const int lo = half_xor<J>((int)(v & 0xffffffffll)), hi = half_xor<J>((int)(v >> 32));
  return ((long long)hi << 32) | (unsigned int)lo;
}
__device__ __forceinline__ long long half_total_i64(long long v) {
  v += half_xor_i64<1>(v);
  v += half_xor_i64<2>(v);
  v += half_xor_i64<4>(v);
  v += half_xor_i64<8>(v);
  v += half_xor_i64<16>(v);
  return v;
}
__device__ __forceinline__ int half_total(int v) {
  v += half_xor<1>(v);
  v += half_xor<2>(v);
  v += half_xor<4>(v);
  v += half_xor<8>(v);
  v += half_xor<16>(v);
  return v;
}

// Sorts the half's n (<= 32 E) samples in t[0, n) in place and leaves t[n, 32 E) as it is: those
// entries are the samples of the next larger span (half_sort_regs would store its padding there).
template <int E>
__device__ __forceinline__ void rw_sort_prefix(int32_t* t, int n, int hl) {
  const int base = (hl >> 4) * (16 * E) + (hl & 15);
  int32_t v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = base + e * 16 < n ? t[base + e * 16] : 0x7fffffff;
  reg_bitonic<E>(v, hl);
  // (ascending: the padding, INT32_MAX, ends at or beyond n, so [0, n) holds the n samples)
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (base + e * 16 < n) t[base + e * 16] = v[e];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

// first window entry of span j
__device__ __forceinline__ int rw_span_lo(const RecentArgs& a, int j) {
  return a.w.n_win - min(a.span[j], a.w.n_win);
}

__global__ __launch_bounds__(RW_WAVES * APM_WAVE) void k_recent_group(RecentArgs a) {
  __shared__ int32_t tile[RW_WAVES * 2][RW_GROUP_MAX];
  const WindowArgs& w = a.w;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (HW - 1);
  const int wv = threadIdx.x >> 6;
  const int s = (blockIdx.x * RW_WAVES + wv) * 2 + half;
  // no early return per half: the moves below are 32 lanes wide, and both halves run them
  const bool valid = s < w.n_series;
  bool row = false;
  if (valid) { const WinStat ws = w.out[s]; row = ws.active && ws.n >= 1; }  // an st row, and a sample in the window
  const bool wide = w.n_win > RW_GROUP_WIN;  // (uniform) every series with a row goes to the block pass
  const int r_lo = rw_span_lo(a, a.nspan - 1);  // the largest span
  int cnt = 0, slot = -1;
  if (row && !wide && hl >= r_lo && hl < w.n_win) {
    slot = w.win_slots[hl];
    if (slot >= 0) cnt = max(w.st.counts[(size_t)slot * w.st.S + s], 0);
  }
  const int inl = min(cnt, w.st.cap);
  const int spill = cnt - inl;
  const int incl = half_scan(cnt);
  const int total = half_last(incl, half);
  const int total_spill = half_sum(spill, half);
  const bool big = row && (wide || total > RW_GROUP_MAX);
  if (big && hl == 0) { const int j = atomicAdd(a.big_n, 1); a.big_list[j] = s; }
  const bool go = row && !big;
  int32_t* t = tile[wv * 2 + half];
  // newest entry first: this bucket starts where all newer buckets end (start + cnt <= total <= the tile)
  const int start = total - incl;
  int nan = 0;        // of this lane's bucket
  long long sum = 0;  // of its finite samples
  if (go && inl > 0) {
    const int32_t* cell = w.st.cells + ((size_t)slot * w.st.S + s) * w.st.cap;
    for (int k = 0; k < inl; ++k) {
      const int32_t v = cell[k];
      t[start + k] = v;
      if (v == ELAPSED_NAN) ++nan; else sum += v;
    }
  }
  // spilled samples: each bucket's run found by its lane, copied by the half behind the bucket's
  // inline cells; what the copying lanes counted goes back to the bucket's lane
  const unsigned long long any_spill = __ballot(go && total_spill > 0);
  if (any_spill) {
    const int32_t* run = go && spill > 0 ? spill_run(w.st, slot, s) : nullptr;
    const unsigned long long all = __ballot(go && spill > 0);
    unsigned int todo = (unsigned int)(half ? (all >> 32) : (all & 0xffffffffull));
    __builtin_amdgcn_wave_barrier();
    // (both halves run the loop the larger number of times; a half with nothing left idles)
    const unsigned int other = (unsigned int)(half ? (all & 0xffffffffull) : (all >> 32));
    const int iters = max(__popc(todo), __popc(other));
    for (int it = 0; it < iters; ++it) {
      const int r = todo ? __ffs((int)todo) - 1 : 0;
      const bool mine = todo != 0;
      todo &= todo - 1;
      const int mm = __shfl(spill, r, HW);
      const int off = __shfl(start + inl, r, HW);
      const uintptr_t rp = (uintptr_t)__shfl((long long)(uintptr_t)run, r, HW);
      int rnan = 0;
      long long rsum = 0;
      if (mine) {
        const int32_t* src = (const int32_t*)rp;
        for (int k = hl; k < mm; k += HW) {  // (off + k < start + cnt of bucket r)
          const int32_t v = src[k];
          t[off + k] = v;
          if (v == ELAPSED_NAN) ++rnan; else rsum += v;
        }
      }
      rnan = half_total(rnan);
      rsum = half_total_i64(rsum);
      if (mine && hl == r) { nan += rnan; sum += rsum; }
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  // the spans, ascending: each a longer prefix of the tile
  int sorted_n = 0;
  for (int sj = 0; sj < a.nspan; ++sj) {
    const bool in = hl >= rw_span_lo(a, sj);
    const int n = half_sum(in ? cnt : 0, half);
    const int nn = half_sum(in ? nan : 0, half);
    const long long tsum = half_total_i64(in ? sum : 0);
    if (!go) continue;
    if (n > sorted_n) {  // (a span clipped to the window repeats the one before it)
      if (n <= HW) rw_sort_prefix<1>(t, n, hl);
      else if (n <= 2 * HW) rw_sort_prefix<2>(t, n, hl);
      else if (n <= 4 * HW) rw_sort_prefix<4>(t, n, hl);
      else if (n <= 8 * HW) rw_sort_prefix<8>(t, n, hl);
      else rw_sort_prefix<16>(t, n, hl);
      sorted_n = n;
    }
    // lanes 2 j, 2 j + 1 read the lower / upper rank of percentile j (nan + rank < n <= tile)
    const int m = n - nn;
    const int j = hl >> 1;
    int32_t x = 0;
    if (m > 0 && j < a.nq) {
      int lo, hi;
      wp_ranks(m, a.q[j], lo, hi);
      x = t[nn + ((hl & 1) ? hi : lo)];
    }
    const int32_t y = half_xor<1>(x);
    RecentRec& rc = a.rec[(size_t)s * a.nspan + sj];
    if (m > 0 && j < a.nq && !(hl & 1)) rc.sum2[j] = (long long)x + (long long)y;
    if (hl == 0) { rc.m = m; rc.nan = nn; rc.sum = tsum; }
  }
}

// every sample of series s in the window entries r >= r_lo, visited by the block
// (for_each_window_sample restricted to a span)
template <class F>
__device__ __forceinline__ void for_each_span_sample(const WindowArgs& a, int s, int r_lo, F&& f) {
  for (int r = r_lo; r < a.n_win; ++r) {
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

// R = 2 Q ranks (padded to the next of 4 / 8 / 16 by repeating the last one)
template <int R, class V>
__device__ __forceinline__ void recent_select(const RecentArgs& a, V&& visit, RecentRec& rc, int m, int nan,
                                              uint32_t* hist) {
  int ranks[R];
#pragma unroll
  for (int j = 0; j < R / 2; ++j) {
    int lo, hi;
    wp_ranks(m, a.q[j < a.nq ? j : a.nq - 1], lo, hi);
    ranks[2 * j] = nan + lo;
    ranks[2 * j + 1] = nan + hi;
  }
  const uint32_t* key = window_select_visit<R>(visit, ranks, hist);
  const int j = threadIdx.x;
  if (j < a.nq)
    rc.sum2[j] = (long long)(int32_t)(key[2 * j] ^ 0x80000000u) + (long long)(int32_t)(key[2 * j + 1] ^ 0x80000000u);
}

__global__ __launch_bounds__(RW_BLOCK) void k_recent_big(RecentArgs a) {
  __shared__ uint32_t hist[2 * WP_MAX_Q * 256];
  __shared__ int tot[2];                  // n, nan
  __shared__ unsigned long long tsum;     // (two's complement: the int64 sum)
  const int nb = min(*a.big_n, a.w.n_series);
  for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const int s = a.big_list[bi];
    for (int sj = 0; sj < a.nspan; ++sj) {
      const int r_lo = rw_span_lo(a, sj);
      auto visit = [&](auto&& f) { for_each_span_sample(a.w, s, r_lo, f); };
      if (threadIdx.x < 2) tot[threadIdx.x] = 0;
      if (threadIdx.x == 2) tsum = 0;
      __syncthreads();
      int n = 0, nan = 0;
      long long sum = 0;
      visit([&](int32_t v) { ++n; if (v == ELAPSED_NAN) ++nan; else sum += v; });
      for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_xor(n, o, 64);
        nan += __shfl_xor(nan, o, 64);
        sum += __shfl_xor(sum, o, 64);
      }
      if ((threadIdx.x & 63) == 0) {
        atomicAdd(&tot[0], n);
        if (nan) atomicAdd(&tot[1], nan);
        atomicAdd(&tsum, (unsigned long long)sum);
      }
      __syncthreads();
      n = tot[0];
      nan = tot[1];
      const int m = n - nan;
      RecentRec& rc = a.rec[(size_t)s * a.nspan + sj];
      if (threadIdx.x == 0) { rc.m = m; rc.nan = nan; rc.sum = (long long)tsum; }
      if (m > 0) {  // (uniform)
        if (a.nq <= 2) recent_select<4>(a, visit, rc, m, nan, hist);
        else if (a.nq <= 4) recent_select<8>(a, visit, rc, m, nan, hist);
        else recent_select<16>(a, visit, rc, m, nan, hist);
      }
      __syncthreads();
    }
  }
}

// The int64 sum in decimal, |v| < 10^19, as the sv rows print theirs: at most three 32-bit pieces
// by 64-bit constant divisions, in registers (OutT::u's general path fills a local buffer, which is
// scratch memory).
template <bool W>
__device__ __forceinline__ void rw_i64(OutT<W>& o, long long v) {
  unsigned long long mag = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
  if (v < 0) o.c('-');
  if (mag <= 0xffffffffull) { o.u32((uint32_t)mag); return; }
  const unsigned long long hi = mag / 10000000000000000ull;  // < 1000
  mag -= hi * 10000000000000000ull;
  const uint32_t mid = (uint32_t)(mag / 100000000ull), lo = (uint32_t)(mag % 100000000ull);
  if (hi) { o.u32((uint32_t)hi); o.u32_fixed8(mid); } else o.u32(mid);
  o.u32_fixed8(lo);
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t rw_row(const RecentTextArgs& a, int32_t s, int32_t sj, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const RecentRec& r = a.rec[(size_t)s * a.nspan + sj];
  const int32_t m = r.m;
  o.lit("rw|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)a.span[sj]); o.c('|');  // (the configured value, not the clipped one)
  o.u32((uint32_t)m); o.c('|');
  o.u32((uint32_t)r.nan); o.c('|');
  rw_i64(o, r.sum); o.c('|');
#pragma unroll
  for (int j = 0; j < WP_MAX_Q; ++j) {
    if (m > 0 && j < a.nq) {  // (m == 0: an empty last field, and no sum2 was written)
      if (j) o.c(',');
      o.sb(a.ptxt[j], a.plen[j]);
      text_half(o, r.sum2[j]);
    }
  }
  o.c('\n');
  o.finish();
  return o.n;
}

// lane i = (emission position, span): the series whose row it prints (-1: none) and the span
__device__ __forceinline__ int32_t rw_row_series(const RecentTextArgs& a, int32_t i, int32_t& sj) {
  const int32_t p = i / a.nspan;
  sj = i - p * a.nspan;
  const int32_t s = a.perm[p];
  if (s < 0 || s >= a.n_series) return -1;
  const WinStat w = a.win[s];
  return w.active && w.n >= 1 ? s : -1;  // (exactly the series the value pass wrote records for)
}

// the length pass' row policy (k_text_len)
struct RwRow {
  static __device__ __forceinline__ uint32_t len(const RecentTextArgs& a, int32_t i) {
    int32_t sj;
    const int32_t s = rw_row_series(a, i, sj);
    return s >= 0 ? rw_row<false>(a, s, sj, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(RW_TEXT_BLOCK) void k_recent_write(RecentTextArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * RW_TEXT_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  int32_t sj;
  const int32_t s = rw_row_series(a, i, sj);
  if (s >= 0) rw_row<true>(a, s, sj, a.out + a.off[i]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_recent_group_max() { return RW_GROUP_MAX; }
int32_t apm_recent_group_win() { return RW_GROUP_WIN; }

size_t apm_recent_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "rw|" + ts (<= 23) + names + 2 separators + k| + m| + nan| (11 each) + sum| (a sign, 19 digits) +
// nq pairs of at most 7 label bytes, a sign, 10 digits, ".5" and a comma + newline
size_t apm_recent_row_bound(size_t name_bytes, int32_t nq) {
  return 3 + 23 + name_bytes + 2 + 33 + 21 + (size_t)nq * 21 + 1;
}

void apm_recent_values(RecentArgs* a, hipStream_t stream) {
  const int32_t n = a->w.n_series;
  if (n <= 0 || a->nspan <= 0) return;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  const int per_block = RW_WAVES * 2;
  hipLaunchKernelGGL(k_recent_group, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(RW_WAVES * APM_WAVE), 0,
                     stream, *a);
  hipLaunchKernelGGL(k_recent_big, dim3(RW_BIG_GRID), dim3(RW_BLOCK), 0, stream, *a);
}

int apm_recent_plan(RecentTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<RwRow, RW_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_recent_write(RecentTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  // (the length pass' grid: n + 1 lanes)
  hipLaunchKernelGGL(k_recent_write, dim3(text_len_blocks(a->n, RW_TEXT_BLOCK)), dim3(RW_TEXT_BLOCK), 0, stream, *a);
}

}  // extern "C"
