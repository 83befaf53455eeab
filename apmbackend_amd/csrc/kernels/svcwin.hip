// K19: sv rows -- exact window stats per service across its servers (docs/SERVICEWINDOW.md).
//
// The unit of work is a group: the series of one service on this engine (a CSR the host keeps,
// members in emission order).  Value pass, on the window K8 just read (same slots, same samples,
// spill lists still sorted), over the union of the windows of a group's active members:
//   group  32 lanes per service, two services a wave: the members are visited one after the other,
//          each with K16's gather (lane r owns window bucket r, the spill runs are copied by the
//          half) appended to the half's LDS tile at a running offset; NaN samples and the int64 sum
//          are counted on the way.  The tile is sorted by K8's register networks (winsort.h), NaN
//          samples (INT32_MIN) sort first, and lanes 0 .. 2Q - 1 read the ranks at nan + rank.
//          Windows of more than SV_GROUP_WIN buckets, and services whose members' WinStat.n total
//          more than SV_GROUP_MAX, are deferred (big_list).
//   block  one block per deferred service: one pass over all members' samples counts n, nan and
//          the sum, then all 2Q ranks are radix-selected together over the union
//          (window_select_visit, 8 bits per pass).
// Only integers: the rank rule is K16's wp_ranks on q = p * 1000, a value the int64 sum of the two
// ranks (one rank: twice the sample).
// Text pass: K12's count / scan / write shape, one lane per emission position, through textout.h:
// a position prints the row of its series' service when it is the first active member's.  The
// length kernel, the scan and the half-value printer are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "spill.h"
#include "winsort.h"

namespace apm {

namespace {

constexpr int SV_WAVES = 4;            // waves per block (group pass): eight services
constexpr int SV_GROUP_MAX = 512;      // samples a 32-lane group sorts itself (its LDS tile)
constexpr int SV_GROUP_WIN = HW;       // window buckets a group covers (one per lane)
constexpr int SV_BLOCK = 512;          // threads per service (block pass)
constexpr int SV_BIG_GRID = 512;       // blocks of the block pass (they loop over big_list)
constexpr int SV_TEXT_BLOCK = 256;
constexpr int SV_TOT_CLAMP = 1 << 24;  // a lane's WinStat.n total saturates here (32 lanes: no int overflow)

__device__ __forceinline__ int half_sum(int x, int half) { return half_last(half_scan(x), half); }

__global__ __launch_bounds__(SV_WAVES * APM_WAVE) void k_svcwin_group(SvcWinArgs a) {
  __shared__ int32_t tile[SV_WAVES * 2][SV_GROUP_MAX];
  const WindowArgs& w = a.w;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (HW - 1);
  const int wv = threadIdx.x >> 6;
  const int g = (blockIdx.x * SV_WAVES + wv) * 2 + half;
  // no early return per half: the moves below are 32 lanes wide, and both halves run them
  const bool valid = g < a.n_groups;
  const int m0 = valid ? a.grp_off[g] : 0;
  const int nmem = valid ? a.grp_off[g + 1] - m0 : 0;
  const bool wide = w.n_win > SV_GROUP_WIN;  // (uniform) every service with a sample goes to the block pass
  // the active members, the first of them and K8's sample total: the lanes stride over the members
  int servers = 0, first = 0x7fffffff, tot = 0;
  for (int k = hl; k < nmem; k += HW) {
    const int s = a.grp_mem[m0 + k];
    if (w.st.active[s]) {
      ++servers;
      first = min(first, k);
      tot = min(tot + max(w.out[s].n, 0), SV_TOT_CLAMP);
    }
  }
  servers = half_sum(servers, half);
  tot = half_sum(tot, half);
  for (int o = 16; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, HW));
  const int first_pos = servers > 0 ? a.grp_pos[m0 + first] : -1;
  const bool pre_big = servers > 0 && (wide ? tot > 0 : tot > SV_GROUP_MAX);
  const bool go = servers > 0 && !pre_big && !wide && tot > 0;
  int32_t* t = tile[wv * 2 + half];
  // Members one after the other; both halves run the loop the larger number of times (a half with
  // fewer members, or nothing to do, idles through the 32-lane moves).
  const int mine_n = go ? nmem : 0;
  const int iters = max(mine_n, __shfl_xor(mine_n, 32));
  int fill = 0, nan = 0;
  long long sum = 0;
  bool ovf = false;  // (never, while WinStat.n is the window's sample count: the tile's bound all the same)
  for (int it = 0; it < iters; ++it) {
    const bool have = it < mine_n;
    const int s = have ? a.grp_mem[m0 + it] : 0;
    const bool act = have && !ovf && w.st.active[s];
    int cnt = 0, slot = -1;
    if (act && hl < w.n_win) {
      slot = w.win_slots[hl];
      if (slot >= 0) cnt = max(w.st.counts[(size_t)slot * w.st.S + s], 0);
    }
    const int inl = min(cnt, w.st.cap);
    const int spill = cnt - inl;
    int pre = half_scan(inl);
    const int total_inl = half_last(pre, half);
    const int total_spill = half_sum(spill, half);
    const int n = total_inl + total_spill;
    const bool fit = fill + n <= SV_GROUP_MAX;
    if (act && !fit) ovf = true;
    const bool put = act && fit && n > 0;
    int32_t* tm = t + fill;
    pre -= inl;
    if (put && inl > 0) {
      const int32_t* cell = w.st.cells + ((size_t)slot * w.st.S + s) * w.st.cap;
      for (int k = 0; k < inl; ++k) {
        const int32_t v = cell[k];
        tm[pre + k] = v;
        if (v == ELAPSED_NAN) ++nan; else sum += v;
      }
    }
    // spilled samples: each window bucket's run found by its lane, copied by the half
    const unsigned long long any_spill = __ballot(put && total_spill > 0);
    if (any_spill) {
      const int32_t* run = put && spill > 0 ? spill_run(w.st, slot, s) : nullptr;
      int spre = half_scan(put ? spill : 0);
      spre -= put ? spill : 0;
      const unsigned long long all = __ballot(put && spill > 0);
      unsigned int todo = (unsigned int)(half ? (all >> 32) : (all & 0xffffffffull));
      __builtin_amdgcn_wave_barrier();
      const unsigned int other = (unsigned int)(half ? (all & 0xffffffffull) : (all >> 32));
      const int runs = max(__popc(todo), __popc(other));
      for (int ri = 0; ri < runs; ++ri) {
        const int r = todo ? __ffs((int)todo) - 1 : 0;
        const bool mine = todo != 0;
        todo &= todo - 1;
        const int mm = __shfl(spill, r, HW);
        const int off = total_inl + __shfl(spre, r, HW);
        const uintptr_t rp = (uintptr_t)__shfl((long long)(uintptr_t)run, r, HW);
        if (mine) {
          const int32_t* src = (const int32_t*)rp;
          for (int k = hl; k < mm; k += HW) {  // (off + k < n, and fill + n <= the tile)
            const int32_t v = src[k];
            tm[off + k] = v;
            if (v == ELAPSED_NAN) ++nan; else sum += v;
          }
        }
      }
    }
    if (put) fill += n;
  }
  nan = half_sum(nan, half);
  for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, HW);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  const bool big = pre_big || ovf;
  const bool sorts = go && !ovf && fill > 0;
  const int n = fill;
  // register network for n <= 32 (every lane runs it: the shuffles need both halves)
  const bool small = sorts && n <= HW;
  int32_t v = small && hl < n ? t[hl] : 0x7fffffff;
  v = bitonic_merge<2>(v, hl);
  v = bitonic_merge<4>(v, hl);
  v = bitonic_merge<8>(v, hl);
  v = bitonic_merge<16>(v, hl);
  v = bitonic_merge<32>(v, hl);
  if (big && hl == 0) { const int j = atomicAdd(a.big_n, 1); a.big_list[j] = g; }
  if (valid && !big && !sorts && hl == 0) {  // no active member, or no sample: no row
    SvcRec& r = a.rec[g];
    r.servers = servers; r.m = 0; r.nan = 0; r.first_pos = first_pos; r.sum = 0;
  }
  if (!sorts) return;
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
  SvcRec& r = a.rec[g];
  if (j < a.nq && !(hl & 1)) r.sum2[j] = (long long)x + (long long)y;
  if (hl == 0) { r.servers = servers; r.m = m; r.nan = nan; r.first_pos = first_pos; r.sum = sum; }
}

// R = 2 Q ranks (padded to the next of 4 / 8 / 16 by repeating the last one)
template <int R, class V>
__device__ __forceinline__ void svcwin_select(const SvcWinArgs& a, V&& visit, int g, int m, int nan, uint32_t* hist) {
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
    a.rec[g].sum2[j] = (long long)(int32_t)(key[2 * j] ^ 0x80000000u) + (long long)(int32_t)(key[2 * j + 1] ^ 0x80000000u);
}

__global__ __launch_bounds__(SV_BLOCK) void k_svcwin_big(SvcWinArgs a) {
  __shared__ uint32_t hist[2 * WP_MAX_Q * 256];
  __shared__ int tot[4];                  // n, nan, active members, first active member
  __shared__ unsigned long long tsum;     // (two's complement: the int64 sum)
  const int nb = min(*a.big_n, a.n_groups);
  for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const int g = a.big_list[bi];
    const int m0 = a.grp_off[g];
    const int nmem = a.grp_off[g + 1] - m0;
    // every sample of the service: its active members' windows, one after the other
    auto visit = [&](auto&& f) {
      for (int k = 0; k < nmem; ++k) {
        const int s = a.grp_mem[m0 + k];
        if (a.w.st.active[s]) for_each_window_sample(a.w, s, f);
      }
    };
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    if (threadIdx.x == 3) { tot[3] = 0x7fffffff; tsum = 0; }
    __syncthreads();
    int act = 0, first = 0x7fffffff;
    for (int k = threadIdx.x; k < nmem; k += blockDim.x)
      if (a.w.st.active[a.grp_mem[m0 + k]]) { ++act; first = min(first, k); }
    if (act) { atomicAdd(&tot[2], act); atomicMin(&tot[3], first); }
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
    if (threadIdx.x == 0) {
      SvcRec& r = a.rec[g];
      r.servers = tot[2]; r.m = m; r.nan = nan;
      r.first_pos = tot[2] > 0 ? a.grp_pos[m0 + tot[3]] : -1;
      r.sum = (long long)tsum;
    }
    if (m > 0) {  // (uniform)
      if (a.nq <= 2) svcwin_select<4>(a, visit, g, m, nan, hist);
      else if (a.nq <= 4) svcwin_select<8>(a, visit, g, m, nan, hist);
      else svcwin_select<16>(a, visit, g, m, nan, hist);
    }
    __syncthreads();
  }
}

// The int64 sum in decimal, |v| < 10^19 (it is below 2^31 times a sample count): at most three
// 32-bit pieces by 64-bit constant divisions, in registers (OutT::u's general path fills a local
// buffer, which is scratch memory).
template <bool W>
__device__ __forceinline__ void sv_i64(OutT<W>& o, long long v) {
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
__device__ __forceinline__ uint32_t sv_row(const SvcWinTextArgs& a, int32_t g, int32_t s, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const SvcRec& r = a.rec[g];
  o.lit("sv|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)r.servers); o.c('|');
  o.u32((uint32_t)r.m); o.c('|');
  o.u32((uint32_t)r.nan); o.c('|');
  sv_i64(o, r.sum); o.c('|');
#pragma unroll
  for (int j = 0; j < WP_MAX_Q; ++j) {
    if (j < a.nq) {
      if (j) o.c(',');
      o.sb(a.ptxt[j], a.plen[j]);
      text_half(o, r.sum2[j]);
    }
  }
  o.c('\n');
  o.finish();
  return o.n;
}

// the service whose row emission position i prints (-1: none), and the series at i
__device__ __forceinline__ int32_t sv_row_group(const SvcWinTextArgs& a, int32_t i, int32_t& s) {
  s = a.perm[i];
  if (s < 0 || s >= a.n_series) return -1;
  const int32_t g = a.series_grp[s];
  if (g < 0 || g >= a.n_groups) return -1;
  return a.rec[g].m >= 1 && a.rec[g].first_pos == i ? g : -1;
}

// the length pass' row policy (k_text_len)
struct SvRow {
  static __device__ __forceinline__ uint32_t len(const SvcWinTextArgs& a, int32_t i) {
    int32_t s;
    const int32_t g = sv_row_group(a, i, s);
    return g >= 0 ? sv_row<false>(a, g, s, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(SV_TEXT_BLOCK) void k_svcwin_write(SvcWinTextArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * SV_TEXT_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  int32_t s;
  const int32_t g = sv_row_group(a, i, s);
  if (g >= 0) sv_row<true>(a, g, s, a.out + a.off[i]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_svcwin_group_max() { return SV_GROUP_MAX; }
int32_t apm_svcwin_group_win() { return SV_GROUP_WIN; }

size_t apm_svcwin_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "sv|" + ts (<= 23) + name + separator + servers| + m| + nan| (11 each) + sum| (a sign, 19
// digits) + nq pairs of at most 7 label bytes, a sign, 10 digits, ".5" and a comma + newline
size_t apm_svcwin_row_bound(size_t name_bytes, int32_t nq) {
  return 3 + 23 + name_bytes + 1 + 33 + 21 + (size_t)nq * 21 + 1;
}

void apm_svcwin_values(SvcWinArgs* a, hipStream_t stream) {
  const int32_t n = a->n_groups;
  if (n <= 0) return;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  const int per_block = SV_WAVES * 2;
  hipLaunchKernelGGL(k_svcwin_group, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(SV_WAVES * APM_WAVE), 0,
                     stream, *a);
  hipLaunchKernelGGL(k_svcwin_big, dim3(SV_BIG_GRID), dim3(SV_BLOCK), 0, stream, *a);
}

int apm_svcwin_plan(SvcWinTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<SvRow, SV_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_svcwin_write(SvcWinTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  // (the length pass' grid: n + 1 positions)
  hipLaunchKernelGGL(k_svcwin_write, dim3(text_len_blocks(a->n, SV_TEXT_BLOCK)), dim3(SV_TEXT_BLOCK), 0, stream, *a);
}

}  // extern "C"
