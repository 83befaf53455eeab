// K16: wp rows -- exact, configurable percentiles of the K8 window (docs/PERCENTILES.md).
//
// Value pass, on the window K8 just read (same slots, same samples, spill lists still sorted):
//   group  32 lanes per series, two series a wave (as k_window_stats_h2 and K15): lane r owns
//          window bucket r, the inline cells and the spill runs are gathered into the half's LDS
//          tile and sorted by K8's register networks (winsort.h).  NaN samples (INT32_MIN) sort
//          first, so rank r of the finite samples is rank nan + r of the tile; lanes 0 .. 2Q - 1
//          read the two ranks of each percentile.  Windows of more than WP_GROUP_WIN buckets or
//          WP_GROUP_MAX samples are deferred (big_list).
//   block  one block per deferred series: the samples are counted, then all 2Q ranks are radix-
//          selected together (window_select_ranks, 8 bits per pass) -- exact at every n, without a
//          tile whose size would be one more boundary.
// Only integers: the rank rule is calcPercentile in exact rational arithmetic on q = p * 1000
// (wp_ranks), the value the int64 sum of the two ranks (one rank: twice the sample).
// Text pass: K12's count / scan / write shape, one lane per emission position, through textout.h;
// the length kernel, the scan and the half-value printer are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "spill.h"
#include "winsort.h"

namespace apm {

namespace {

constexpr int WP_WAVES = 4;            // waves per block (group pass): eight series
constexpr int WP_GROUP_MAX = 512;      // samples a 32-lane group sorts itself (its LDS tile)
constexpr int WP_GROUP_WIN = HW;       // window buckets a group covers (one per lane)
constexpr int WP_BLOCK = 512;          // threads per series (block pass)
constexpr int WP_BIG_GRID = 512;       // blocks of the block pass (they loop over big_list)
constexpr int WP_TEXT_BLOCK = 256;
// (the integer rank rule, wp_ranks, lives in winsort.h: K19 reads the same ranks)

__global__ __launch_bounds__(WP_WAVES * APM_WAVE) void k_winpct_group(WinPctArgs a) {
  __shared__ int32_t tile[WP_WAVES * 2][WP_GROUP_MAX];
  const WindowArgs& w = a.w;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (HW - 1);
  const int wv = threadIdx.x >> 6;
  const int s = (blockIdx.x * WP_WAVES + wv) * 2 + half;
  // no early return per half: the shuffles below are 32 lanes wide, and both halves run them
  const bool valid = s < w.n_series;
  const bool active = valid && w.st.active[s];
  const bool wide = w.n_win > WP_GROUP_WIN;  // (uniform) every series with a sample goes to the block pass
  int cnt = 0, slot = -1;
  if (active && !wide && hl < w.n_win) {
    slot = w.win_slots[hl];
    if (slot >= 0) cnt = max(w.st.counts[(size_t)slot * w.st.S + s], 0);
  }
  const int inl = min(cnt, w.st.cap);
  const int spill = cnt - inl;
  int pre = half_scan(inl);
  const int total_inl = half_last(pre, half);
  const int total_spill = half_last(half_scan(spill), half);
  const int n = total_inl + total_spill;
  const bool big = active && (wide ? w.out[s].n > 0 : n > WP_GROUP_MAX);
  if (big && hl == 0) { const int j = atomicAdd(a.big_n, 1); a.big_list[j] = s; }
  const bool go = active && !big && n > 0;
  if (valid && !go && !big && hl == 0) { a.m[s] = 0; a.nan[s] = 0; }  // no sample: no row
  int32_t* t = tile[wv * 2 + half];
  pre -= inl;
  int nan = 0;
  if (go && inl > 0) {
    const int32_t* cell = w.st.cells + ((size_t)slot * w.st.S + s) * w.st.cap;
    for (int k = 0; k < inl; ++k) { const int32_t v = cell[k]; t[pre + k] = v; nan += v == ELAPSED_NAN; }
  }
  // spilled samples: each window bucket's run found by its lane, copied by the half
  const unsigned long long any_spill = __ballot(go && total_spill > 0);
  if (any_spill) {
    const int32_t* run = go && spill > 0 ? spill_run(w.st, slot, s) : nullptr;
    int spre = half_scan(go ? spill : 0);
    spre -= go ? spill : 0;
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
      const int off = total_inl + __shfl(spre, r, HW);
      const uintptr_t rp = (uintptr_t)__shfl((long long)(uintptr_t)run, r, HW);
      if (mine) {
        const int32_t* src = (const int32_t*)rp;
        for (int k = hl; k < mm; k += HW) {
          const int32_t v = src[k];
          t[off + k] = v;
          nan += v == ELAPSED_NAN;
        }
      }
    }
  }
  nan = half_last(half_scan(nan), half);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  // register network for n <= 32 (every lane runs it: the shuffles need both halves)
  const bool small = go && n <= HW;
  int32_t v = small && hl < n ? t[hl] : 0x7fffffff;
  v = bitonic_merge<2>(v, hl);
  v = bitonic_merge<4>(v, hl);
  v = bitonic_merge<8>(v, hl);
  v = bitonic_merge<16>(v, hl);
  v = bitonic_merge<32>(v, hl);
  if (!go) return;
  if (small) {
    if (hl < n) t[hl] = v;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  } else if (n <= 2 * HW) {  // 32 < n <= 512: this half sorts its tile in registers
    half_sort_regs<2>(t, n, hl);
  } else if (n <= 4 * HW) {
    half_sort_regs<4>(t, n, hl);
  } else if (n <= 8 * HW) {
    half_sort_regs<8>(t, n, hl);
  } else {
    half_sort_regs<16>(t, n, hl);
  }
  // lanes 2 j, 2 j + 1 read the lower / upper rank of percentile j (nan + rank < n <= tile)
  const int m = n - nan;
  const int j = hl >> 1;
  int32_t x = 0;
  if (m > 0 && j < a.nq) {
    int lo, hi;
    wp_ranks(m, a.q[j], lo, hi);
    x = t[nan + ((hl & 1) ? hi : lo)];
  }
  const int32_t y = half_xor<1>(x);
  if (j < a.nq && !(hl & 1)) a.sum2[(size_t)s * a.nq + j] = (long long)x + (long long)y;
  if (hl == 0) { a.m[s] = m; a.nan[s] = nan; }
}

// R = 2 Q ranks (padded to the next of 4 / 8 / 16 by repeating the last one)
template <int R>
__device__ __forceinline__ void winpct_select(const WinPctArgs& a, int s, int m, int nan, uint32_t* hist) {
  int ranks[R];
#pragma unroll
  for (int j = 0; j < R / 2; ++j) {
    int lo, hi;
    wp_ranks(m, a.q[j < a.nq ? j : a.nq - 1], lo, hi);
    ranks[2 * j] = nan + lo;
    ranks[2 * j + 1] = nan + hi;
  }
  const uint32_t* key = window_select_ranks<R>(a.w, s, ranks, hist);
  const int j = threadIdx.x;
  if (j < a.nq)
    a.sum2[(size_t)s * a.nq + j] = (long long)(int32_t)(key[2 * j] ^ 0x80000000u) + (long long)(int32_t)(key[2 * j + 1] ^ 0x80000000u);
}

__global__ __launch_bounds__(WP_BLOCK) void k_winpct_big(WinPctArgs a) {
  __shared__ uint32_t hist[2 * WP_MAX_Q * 256];
  __shared__ int tot[2];
  const int nb = min(*a.big_n, a.w.n_series);
  for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const int s = a.big_list[bi];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    int n = 0, nan = 0;
    for_each_window_sample(a.w, s, [&](int32_t v) { ++n; nan += v == ELAPSED_NAN; });
    for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o, 64); nan += __shfl_xor(nan, o, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&tot[0], n); if (nan) atomicAdd(&tot[1], nan); }
    __syncthreads();
    n = tot[0];
    nan = tot[1];
    const int m = n - nan;
    if (threadIdx.x == 0) { a.m[s] = m; a.nan[s] = nan; }
    if (m > 0) {  // (uniform)
      if (a.nq <= 2) winpct_select<4>(a, s, m, nan, hist);
      else if (a.nq <= 4) winpct_select<8>(a, s, m, nan, hist);
      else winpct_select<16>(a, s, m, nan, hist);
    }
    __syncthreads();
  }
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t wp_row(const WinPctTextArgs& a, int32_t s, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  o.lit("wp|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)a.m[s]); o.c('|');
  o.u32((uint32_t)a.nan[s]); o.c('|');
#pragma unroll
  for (int j = 0; j < WP_MAX_Q; ++j) {
    if (j < a.nq) {
      if (j) o.c(',');
      o.sb(a.ptxt[j], a.plen[j]);
      text_half(o, a.sum2[(size_t)s * a.nq + j]);
    }
  }
  o.c('\n');
  o.finish();
  return o.n;
}

// series of emission position i that prints a row (-1: none)
__device__ __forceinline__ int32_t wp_row_series(const WinPctTextArgs& a, int32_t i) {
  const int32_t s = a.perm[i];
  if (s < 0 || s >= a.n_series) return -1;
  return a.m[s] >= 1 ? s : -1;
}

// the length pass' row policy (k_text_len)
struct WpRow {
  static __device__ __forceinline__ uint32_t len(const WinPctTextArgs& a, int32_t i) {
    const int32_t s = wp_row_series(a, i);
    return s >= 0 ? wp_row<false>(a, s, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(WP_TEXT_BLOCK) void k_winpct_write(WinPctTextArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * WP_TEXT_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  const int32_t s = wp_row_series(a, i);
  if (s >= 0) wp_row<true>(a, s, a.out + a.off[i]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_winpct_group_max() { return WP_GROUP_MAX; }
int32_t apm_winpct_group_win() { return WP_GROUP_WIN; }

size_t apm_winpct_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "wp|" + ts (<= 23) + names + 2 separators + m| + nan| (11 each) + nq pairs of at most 7 label
// bytes, a sign, 10 digits, ".5" and a comma + newline
size_t apm_winpct_row_bound(size_t name_bytes, int32_t nq) {
  return 3 + 23 + name_bytes + 2 + 22 + (size_t)nq * 21 + 1;
}

void apm_winpct_values(WinPctArgs* a, hipStream_t stream) {
  const int32_t n = a->w.n_series;
  if (n <= 0) return;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  const int per_block = WP_WAVES * 2;
  hipLaunchKernelGGL(k_winpct_group, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(WP_WAVES * APM_WAVE), 0,
                     stream, *a);
  hipLaunchKernelGGL(k_winpct_big, dim3(WP_BIG_GRID), dim3(WP_BLOCK), 0, stream, *a);
}

int apm_winpct_plan(WinPctTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<WpRow, WP_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_winpct_write(WinPctTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  // (the length pass' grid: n + 1 positions)
  hipLaunchKernelGGL(k_winpct_write, dim3(text_len_blocks(a->n, WP_TEXT_BLOCK)), dim3(WP_TEXT_BLOCK), 0, stream, *a);
}

}  // extern "C"
