// K24: ls rows -- latency shifts of a series' newest buckets against the rest of its own K8 window
// (docs/SHIFT.md).
//
// Rule j splits the window entries into the recent span r >= n_win - min(span[j], n_win) (r =
// n_win - 1 is the newest; rw's span) and the baseline, the other entries.  T2 is twice the
// percentile q[j] of the baseline's finite samples (K16's rank rule, wp_ranks), X2 the same of the
// span's, a / b the span's finite samples strictly above / below the baseline's percentile; the
// verdict is shift_verdict's (shiftcmp.h).  Value pass, on the window K8 just read (same slots, same
// samples, spill lists still sorted), one record per series with an st row and a class:
//   group  32 lanes per series, two series a wave (as K16 and K20): lane r owns window entry r, the
//          whole window is gathered newest entry first into the half's pristine LDS tile (rw's
//          layout: a bucket starts at the sample count of all newer buckets), so a span is the
//          prefix [0, nR) and its baseline the suffix [nR, n).  Per distinct span, ascending: the
//          prefix is sorted in place with a guarded write-back (it stays a valid part of the next,
//          longer prefix, and the suffix keeps its bucket order), the suffix is sorted out of
//          place into the half's work tile (winsort.h reg_bitonic both times).  The four ranks are
//          read at nan + rank by lanes 0 .. 3; a and b are counted over the prefix, 32 samples a
//          step.  A lane counts the NaN samples of its own bucket; a side's nan is that reduced over
//          the side's lanes.  Windows of more than LS_GROUP_WIN buckets or LS_GROUP_MAX samples are
//          deferred (big_list).
//   block  one block per deferred series: per rule one pass counts both sides, the two ranks of
//          each side are radix-selected (window_select_visit<2>) over that side's entries, and one
//          more pass over the span's entries counts a and b.
// Only integers.  A class-0 or inactive series reads no sample.
// Text pass: K12's count / scan / write shape over the emission permutation; a position whose
// series has no rule with a verdict has length 0, which is the compaction.  Rows are rare, so the
// write pass stores each row directly through textout.h (no LDS stage).  The length kernel and the
// scan are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "shiftcmp.h"
#include "spill.h"
#include "winsort.h"

namespace apm {

namespace {

constexpr int LS_WAVES = 4;            // waves per block (group pass): eight series
constexpr int LS_GROUP_MAX = 512;      // samples a 32-lane group sorts itself (each of its two LDS tiles)
constexpr int LS_GROUP_WIN = HW;       // window buckets a group covers (one per lane)
constexpr int LS_BLOCK = 512;          // threads per series (block pass)
constexpr int LS_BIG_GRID = 512;       // blocks of the block pass (they loop over big_list)
constexpr int LS_TEXT_BLOCK = 256;

static_assert(LS_SCALE == WP_SCALE, "shiftcmp.h and wp_ranks share the percentile scale");

__device__ __forceinline__ int half_sum(int x, int half) { return half_last(half_scan(x), half); }
__device__ __forceinline__ int half_total(int v) {
  v += half_xor<1>(v);
  v += half_xor<2>(v);
  v += half_xor<4>(v);
  v += half_xor<8>(v);
  v += half_xor<16>(v);
  return v;
}

// class of series s: [0, n_classes), anything else is "no row"
__device__ __forceinline__ int shift_class(const int32_t* cls, int n_classes, int s) {
  const int c = cls[s];
  return c > 0 && c < n_classes ? c : 0;
}

// first window entry of rule j's span
__device__ __forceinline__ int ls_span_lo(const ShiftArgs& a, int j) { return a.w.n_win - min(a.span[j], a.w.n_win); }

// Sorts the half's n (<= 32 E) samples src[0, n) into dst[0, n) and leaves dst[n, 32 E) as it is
// (rw's guarded write-back: with dst == src the entries beyond n are the baseline in bucket order).
// Every load comes before the first store, so dst may be src.
template <int E>
__device__ __forceinline__ void ls_sort(const int32_t* src, int32_t* dst, int n, int hl) {
  const int base = (hl >> 4) * (16 * E) + (hl & 15);
  int32_t v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = base + e * 16 < n ? src[base + e * 16] : 0x7fffffff;
  reg_bitonic<E>(v, hl);
  // (ascending: the padding, INT32_MAX, ends at or beyond n, so [0, n) holds the n samples)
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (base + e * 16 < n) dst[base + e * 16] = v[e];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

__device__ __forceinline__ void ls_sort_n(const int32_t* src, int32_t* dst, int n, int hl) {
  if (n <= HW) ls_sort<1>(src, dst, n, hl);
  else if (n <= 2 * HW) ls_sort<2>(src, dst, n, hl);
  else if (n <= 4 * HW) ls_sort<4>(src, dst, n, hl);
  else if (n <= 8 * HW) ls_sort<8>(src, dst, n, hl);
  else ls_sort<16>(src, dst, n, hl);
}

// rule j of series s into its record, and the verdict's two bits
__device__ __forceinline__ int ls_store(const ShiftArgs& a, ShiftRec& rc, int j, int min_delta, int mB, int nanB, int mR,
                                        int nanR, int na, int nb, long long T2, long long X2) {
  rc.mB[j] = mB; rc.nanB[j] = nanB; rc.mR[j] = mR; rc.nanR[j] = nanR;
  rc.a[j] = na; rc.b[j] = nb; rc.T2[j] = T2; rc.X2[j] = X2;
  return shift_verdict(na, nb, mR, mB, T2, X2, a.q[j], a.up[j], a.down[j], a.z[j], min_delta, a.min_recent, a.min_baseline)
         << (2 * j);
}

__global__ __launch_bounds__(LS_WAVES * APM_WAVE) void k_shift_group(ShiftArgs a) {
  __shared__ int32_t tile[LS_WAVES * 2][2][LS_GROUP_MAX];
  const WindowArgs& w = a.w;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (HW - 1);
  const int wv = threadIdx.x >> 6;
  const int s = (blockIdx.x * LS_WAVES + wv) * 2 + half;
  // no early return per half: the moves below are 32 lanes wide, and both halves run them
  const bool valid = s < w.n_series;
  int cls = 0, n_stat = 0;
  if (valid) {
    const WinStat ws = w.out[s];
    if (ws.active) { cls = shift_class(a.cls, a.n_classes, s); n_stat = ws.n; }  // an st row, and a class
  }
  const bool row = cls > 0;
  const bool wide = w.n_win > LS_GROUP_WIN;  // (uniform) every series with a class goes to the block pass
  int cnt = 0, slot = -1;
  if (row && !wide && hl < w.n_win) {
    slot = w.win_slots[hl];
    if (slot >= 0) cnt = max(w.st.counts[(size_t)slot * w.st.S + s], 0);
  }
  const int inl = min(cnt, w.st.cap);
  const int spill = cnt - inl;
  const int incl = half_scan(cnt);
  const int total = half_last(incl, half);
  const int total_spill = half_sum(spill, half);
  const bool big = row && (wide || total > LS_GROUP_MAX);
  if (big && hl == 0) { const int j = atomicAdd(a.big_n, 1); a.big_list[j] = s; }
  const bool go = row && !big;
  // (the text pass reads the verdict of every series with a class, an inactive one included)
  if (valid && !go && !big && hl == 0) { a.rec[s].n = 0; a.rec[s].verdict = 0; }
  if (!__ballot(go)) return;  // (the wave leaves when neither half sorts)
  int32_t* p = tile[wv * 2 + half][0];  // pristine: newest bucket first
  int32_t* t = tile[wv * 2 + half][1];  // work: the sorted baseline
  // newest entry first: this bucket starts where all newer buckets end (start + cnt <= total <= the tile)
  const int start = total - incl;
  int nan = 0;  // of this lane's bucket
  if (go && inl > 0) {
    const int32_t* cell = w.st.cells + ((size_t)slot * w.st.S + s) * w.st.cap;
    for (int k = 0; k < inl; ++k) {
      const int32_t v = cell[k];
      p[start + k] = v;
      nan += v == ELAPSED_NAN;
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
      if (mine) {
        const int32_t* src = (const int32_t*)rp;
        for (int k = hl; k < mm; k += HW) {  // (off + k < start + cnt of bucket r)
          const int32_t v = src[k];
          p[off + k] = v;
          rnan += v == ELAPSED_NAN;
        }
      }
      rnan = half_total(rnan);
      if (mine && hl == r) nan += rnan;
    }
  }
  const int total_nan = half_sum(nan, half);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  const int min_delta = a.delta[cls];  // (cls 0: entry 0 of the table, read and never used)
  int verdict = 0;
  int sorted_lo = -1;  // the span whose prefix / baseline sorts stand in the tiles
  for (int j = 0; j < a.nrule; ++j) {
    const int r_lo = ls_span_lo(a, j);
    const bool in = hl >= r_lo;
    const int nR = half_sum(in ? cnt : 0, half);
    const int nanR = half_sum(in ? nan : 0, half);
    if (!go) continue;
    const int nB = total - nR, nanB = total_nan - nanR;
    if (r_lo != sorted_lo) {  // (rules of one span, or spans clipped to the window, share the sorts)
      if (nR > 0) ls_sort_n(p, p, nR, hl);
      if (nB > 0) ls_sort_n(p + nR, t, nB, hl);
      sorted_lo = r_lo;
    }
    const int mB = nB - nanB, mR = nR - nanR;
    // lanes 0, 1 read the lower / upper rank of the baseline, lanes 2, 3 those of the span
    // (nan + rank < the side's samples)
    int32_t x = 0;
    if (hl < 2 && mB > 0) {
      int lo, hi;
      wp_ranks(mB, a.q[j], lo, hi);
      x = t[nanB + ((hl & 1) ? hi : lo)];
    } else if (hl >= 2 && hl < 4 && mR > 0) {
      int lo, hi;
      wp_ranks(mR, a.q[j], lo, hi);
      x = p[nanR + ((hl & 1) ? hi : lo)];
    }
    const long long sum2 = (long long)x + (long long)half_xor<1>(x);
    const long long T2 = __shfl(sum2, 0, HW), X2 = __shfl(sum2, 2, HW);
    int na = 0, nb = 0;
    if (mB > 0) {
      for (int i = hl; i < nR; i += HW) {
        const int32_t v = p[i];
        if (v != ELAPSED_NAN) { na += 2ll * v > T2; nb += 2ll * v < T2; }
      }
    }
    na = half_total(na);
    nb = half_total(nb);
    if (hl == 0) verdict |= ls_store(a, a.rec[s], j, min_delta, mB, nanB, mR, nanR, na, nb, T2, X2);
  }
  if (go && hl == 0) { a.rec[s].n = n_stat; a.rec[s].verdict = verdict; }
}

// every sample of series s in the window entries [r0, r1), visited by the block
// (for_each_window_sample restricted to an entry range)
template <class F>
__device__ __forceinline__ void for_each_range_sample(const WindowArgs& a, int s, int r0, int r1, F&& f) {
  for (int r = r0; r < r1; ++r) {
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

// twice the percentile q of the m finite samples `visit` enumerates behind their nan NaN ones
template <class V>
__device__ __forceinline__ long long ls_select(V&& visit, int m, int nan, int q, uint32_t* hist) {
  int lo, hi;
  wp_ranks(m, q, lo, hi);
  const int ranks[2] = {nan + lo, nan + hi};
  const uint32_t* key = window_select_visit<2>(visit, ranks, hist);
  const long long v = (long long)(int32_t)(key[0] ^ 0x80000000u) + (long long)(int32_t)(key[1] ^ 0x80000000u);
  __syncthreads();  // (the keys are read before the next select rewrites them)
  return v;
}

__global__ __launch_bounds__(LS_BLOCK) void k_shift_big(ShiftArgs a) {
  __shared__ uint32_t hist[2 * 256];
  __shared__ int tot[4];  // the span's n, nan, the baseline's; then a, b
  const WindowArgs& w = a.w;
  const int nb_list = min(*a.big_n, w.n_series);
  for (int bi = blockIdx.x; bi < nb_list; bi += gridDim.x) {
    const int s = a.big_list[bi];
    const int cls = shift_class(a.cls, a.n_classes, s);
    const int min_delta = a.delta[cls];
    int verdict = 0;
    for (int j = 0; j < a.nrule; ++j) {
      const int r_lo = ls_span_lo(a, j);
      auto visit_r = [&](auto&& f) { for_each_range_sample(w, s, r_lo, w.n_win, f); };
      auto visit_b = [&](auto&& f) { for_each_range_sample(w, s, 0, r_lo, f); };
      if (threadIdx.x < 4) tot[threadIdx.x] = 0;
      __syncthreads();
      int c[4] = {0, 0, 0, 0};
      visit_r([&](int32_t v) { ++c[0]; c[1] += v == ELAPSED_NAN; });
      visit_b([&](int32_t v) { ++c[2]; c[3] += v == ELAPSED_NAN; });
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        for (int o = 32; o > 0; o >>= 1) c[i] += __shfl_xor(c[i], o, 64);
        if ((threadIdx.x & 63) == 0 && c[i]) atomicAdd(&tot[i], c[i]);
      }
      __syncthreads();
      const int nanR = tot[1], mR = tot[0] - nanR, nanB = tot[3], mB = tot[2] - nanB;
      __syncthreads();
      if (threadIdx.x < 2) tot[threadIdx.x] = 0;  // a, b
      // (mB, mR: uniform)
      const long long T2 = mB > 0 ? ls_select(visit_b, mB, nanB, a.q[j], hist) : 0;
      const long long X2 = mR > 0 ? ls_select(visit_r, mR, nanR, a.q[j], hist) : 0;
      __syncthreads();
      int na = 0, nb = 0;
      if (mB > 0) {
        visit_r([&](int32_t v) {
          if (v != ELAPSED_NAN) { na += 2ll * v > T2; nb += 2ll * v < T2; }
        });
      }
      for (int o = 32; o > 0; o >>= 1) { na += __shfl_xor(na, o, 64); nb += __shfl_xor(nb, o, 64); }
      if ((threadIdx.x & 63) == 0) {
        if (na) atomicAdd(&tot[0], na);
        if (nb) atomicAdd(&tot[1], nb);
      }
      __syncthreads();
      if (threadIdx.x == 0) verdict |= ls_store(a, a.rec[s], j, min_delta, mB, nanB, mR, nanR, tot[0], tot[1], T2, X2);
      __syncthreads();
    }
    if (threadIdx.x == 0) { a.rec[s].n = w.out[s].n; a.rec[s].verdict = verdict; }
  }
}

// twice a percentile, |v| < 2^32, as a plain signed decimal
template <bool W>
__device__ __forceinline__ void ls_i64(OutT<W>& o, long long v) {
  const unsigned long long mag = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
  if (v < 0) o.c('-');
  o.u32((uint32_t)mag);
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t ls_row(const ShiftTextArgs& a, int32_t s, int cls, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const ShiftRec& r = a.rec[s];
  o.lit("ls|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)r.n); o.c('|');
  o.u32((uint32_t)a.delta[cls]); o.c('|');
  const int verdict = r.verdict;
#pragma unroll
  for (int j = 0; j < LS_MAX_RULES; ++j) {
    if (j < a.nrule) {
      if (j) o.c(',');
      o.u32((uint32_t)a.span[j]); o.c(':');  // (the configured value, not the clipped one)
      o.sb(a.ptxt[j], a.plen[j]);
      o.u32((uint32_t)r.mB[j]); o.c(':');
      ls_i64(o, r.T2[j]); o.c(':');
      o.u32((uint32_t)r.mR[j]); o.c(':');
      ls_i64(o, r.X2[j]); o.c(':');
      o.u32((uint32_t)r.a[j]); o.c(':');
      o.u32((uint32_t)r.b[j]); o.c(':');
      const int v = (verdict >> (2 * j)) & 3;
      o.c(v == LS_U ? 'U' : v == LS_D ? 'D' : 'N');
    }
  }
  o.c('\n');
  o.finish();
  return o.n;
}

// series of emission position i that prints a row (-1: none) and its class: a rule has a verdict
// (the value pass wrote verdict 0 for every series without an st row)
__device__ __forceinline__ int32_t ls_row_series(const ShiftTextArgs& a, int32_t i, int& cls) {
  const int32_t s = a.perm[i];
  if (s < 0 || s >= a.n_series) return -1;
  cls = shift_class(a.cls, a.n_classes, s);
  return cls > 0 && a.rec[s].verdict != 0 ? s : -1;
}

// the length pass' row policy (k_text_len)
struct LsRow {
  static __device__ __forceinline__ uint32_t len(const ShiftTextArgs& a, int32_t i) {
    int cls = 0;
    const int32_t s = ls_row_series(a, i, cls);
    return s >= 0 ? ls_row<false>(a, s, cls, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(LS_TEXT_BLOCK) void k_shift_write(ShiftTextArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * LS_TEXT_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  int cls = 0;
  const int32_t s = ls_row_series(a, i, cls);
  if (s >= 0) ls_row<true>(a, s, cls, a.out + a.off[i]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_shift_group_max() { return LS_GROUP_MAX; }
int32_t apm_shift_group_win() { return LS_GROUP_WIN; }

size_t apm_shift_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "ls|" + ts (<= 23) + names + 2 separators + n| + minDelta| (11 each) + 4 groups of k (<= 2
// digits), a label of at most 7 bytes with its colon, four counts of at most 10 digits, two signed
// values of at most 11 bytes, their colons, the verdict and a comma + newline
size_t apm_shift_row_bound(size_t name_bytes) { return 3 + 23 + name_bytes + 2 + 22 + (size_t)LS_MAX_RULES * 84 + 1; }

void apm_shift_values(ShiftArgs* a, hipStream_t stream) {
  const int32_t n = a->w.n_series;
  if (n <= 0 || a->nrule <= 0) return;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  const int per_block = LS_WAVES * 2;
  hipLaunchKernelGGL(k_shift_group, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(LS_WAVES * APM_WAVE), 0,
                     stream, *a);
  // the list length is on the device: a fixed grid whose blocks loop over the list
  hipLaunchKernelGGL(k_shift_big, dim3(LS_BIG_GRID), dim3(LS_BLOCK), 0, stream, *a);
}

int apm_shift_plan(ShiftTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<LsRow, LS_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_shift_write(ShiftTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  hipLaunchKernelGGL(k_shift_write, dim3((uint32_t)((a->n + LS_TEXT_BLOCK - 1) / LS_TEXT_BLOCK)), dim3(LS_TEXT_BLOCK), 0,
                     stream, *a);
}

}  // extern "C"
