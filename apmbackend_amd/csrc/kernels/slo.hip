// K17: sl rows -- exact window threshold counts per service objective (docs/OBJECTIVES.md).
//
// Value pass, on the window K8 just read (same slots, same samples, spill lists still sorted):
//   group  32 lanes per series, two series a wave (as k_window_stats_h2, K15 and K16).  No sort and
//          no LDS tile: lane r owns window buckets r, r + 32, ... and reads their inline cells, the
//          spill runs are walked by the half with a stride of 32, and every sample is compared
//          with the series' thresholds held in registers.  The per-lane counters are summed over
//          the 32 lanes with the DPP row moves of winsort.h.  A window of any length stays here;
//          only a series K8 counted more than SL_GROUP_MAX samples for is deferred (big_list).
//   block  one block per deferred series, the same counters over for_each_window_sample.
// A class-0 series (no threshold: no row) reads no sample.  One SloRec per series: m, nan, counts.
// Only integers: c_j = #{v != ELAPSED_NAN : v <= T_j}, cumulative by construction.
// Text pass: K12's count / scan / write shape; k_slo_write stages a 64-row block in LDS and stores
// the block's contiguous byte range one dword per lane (k_format_write's way); a block over the
// stage stores its rows directly through textout.h.  The length kernel, the scan and the stage's
// copy-out are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "spill.h"
#include "winsort.h"

namespace apm {

namespace {

constexpr int SL_WAVES = 4;            // waves per block (group pass): eight series
constexpr int SL_GROUP_MAX = 4096;     // samples a 32-lane group counts itself (128 per lane)
constexpr int SL_BLOCK = 256;          // threads per series (block pass)
constexpr int SL_BIG_GRID = 32;        // blocks of the block pass (they loop over big_list)
constexpr int SL_LEN_BLOCK = 256;
constexpr int SL_ROWS = 64;            // rows per block of the write pass (one wave)
constexpr uint32_t SL_STAGE = 8192;    // its LDS stage

// The counters of one lane: cumulative by threshold, the NaN samples apart.  Thresholds past the
// class' k are INT32_MAX (their counters are never stored).
struct SloCount {
  int32_t t[SL_MAX_T];
  int32_t c[SL_MAX_T];
  int32_t m = 0, nan = 0;
  __device__ __forceinline__ void load(const SloArgs& a, int cls, int k) {
#pragma unroll
    for (int j = 0; j < SL_MAX_T; ++j) {
      t[j] = j < k ? a.thr[(size_t)cls * SL_MAX_T + j] : 0x7fffffff;
      c[j] = 0;
    }
  }
  __device__ __forceinline__ void add(int32_t v) {
    const bool fin = v != ELAPSED_NAN;
    nan += !fin;
    m += fin;
#pragma unroll
    for (int j = 0; j < SL_MAX_T; ++j) c[j] += (fin && v <= t[j]) ? 1 : 0;
  }
};

// class of series s: [0, n_classes), anything else is "no row"
__device__ __forceinline__ int slo_class(const int32_t* cls, int n_classes, int s) {
  const int c = cls[s];
  return c > 0 && c < n_classes ? c : 0;
}

__global__ __launch_bounds__(SL_WAVES * APM_WAVE) void k_slo_group(SloArgs a) {
  const WindowArgs& w = a.w;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (HW - 1);
  const int wv = threadIdx.x >> 6;
  const int s = (blockIdx.x * SL_WAVES + wv) * 2 + half;
  const bool valid = s < w.n_series;
  int cls = 0, k = 0;
  bool big = false;
  if (valid && w.st.active[s]) {
    cls = slo_class(a.cls, a.n_classes, s);
    k = min(max(a.nthr[cls], 0), SL_MAX_T);
    big = k > 0 && w.out[s].n > SL_GROUP_MAX;
  }
  if (big && hl == 0) { const int j = atomicAdd(a.big_n, 1); a.big_list[j] = s; }
  const bool go = k > 0 && !big;
  // no threshold, inactive or deferred: nothing is read; the wave leaves when neither half counts
  // (the moves below are 32 lanes wide and need both halves, so one half alone does not return)
  if (valid && !go && !big && hl == HW - 1) { SloRec z{}; a.rec[s] = z; }
  if (!__ballot(go)) return;
  SloCount ct;
  ct.load(a, cls, k);
  // inline cells: lane hl owns buckets hl, hl + 32, ... and reads their cells itself
  for (int r0 = 0; r0 < w.n_win; r0 += HW) {  // (uniform)
    const int r = r0 + hl;
    int cnt = 0, slot = -1;
    if (go && r < w.n_win) {
      slot = win_slot(w, r);
      if (slot >= 0) cnt = max(w.st.counts[(size_t)slot * w.st.S + s], 0);
    }
    const int inl = min(cnt, w.st.cap);
    const int spill = cnt - inl;
    if (inl > 0) {
      const int32_t* cell = w.st.cells + ((size_t)slot * w.st.S + s) * w.st.cap;
      for (int i = 0; i < inl; ++i) ct.add(cell[i]);
    }
    // spill runs: each bucket's run found by its lane, walked by the half with a stride of 32
    const unsigned long long all = __ballot(spill > 0);
    if (all) {  // (uniform)
      const int32_t* run = spill > 0 ? spill_run(w.st, slot, s) : nullptr;
      unsigned int todo = (unsigned int)(half ? (all >> 32) : (all & 0xffffffffull));
      const unsigned int other = (unsigned int)(half ? (all & 0xffffffffull) : (all >> 32));
      // (both halves run the loop the larger number of times; a half with nothing left idles)
      const int iters = max(__popc(todo), __popc(other));
      for (int it = 0; it < iters; ++it) {
        const int b = todo ? __ffs((int)todo) - 1 : 0;
        const bool mine = todo != 0;
        todo &= todo - 1;
        const int mm = __shfl(spill, b, HW);
        const uintptr_t rp = (uintptr_t)__shfl((long long)(uintptr_t)run, b, HW);
        if (mine) {
          const int32_t* src = (const int32_t*)rp;
          for (int i = hl; i < mm; i += HW) ct.add(src[i]);
        }
      }
    }
  }
  // totals of the half in its lane 31 (inclusive scans); the wave-uniform bound keeps all 64 lanes
  // in every DPP move
  const int k0 = __builtin_amdgcn_readlane(k, 0), k1 = __builtin_amdgcn_readlane(k, 32);
  const int kmax = max(k0, k1);
  ct.m = half_scan(ct.m);
  ct.nan = half_scan(ct.nan);
#pragma unroll
  for (int j = 0; j < SL_MAX_T; ++j)
    if (j < kmax) ct.c[j] = half_scan(ct.c[j]);
  if (go && hl == HW - 1) {
    SloRec o;
    o.m = ct.m;
    o.nan = ct.nan;
#pragma unroll
    for (int j = 0; j < SL_MAX_T; ++j) o.c[j] = j < k ? ct.c[j] : 0;
    a.rec[s] = o;
  }
}

__global__ __launch_bounds__(SL_BLOCK) void k_slo_big(SloArgs a) {
  __shared__ int32_t tot[2 + SL_MAX_T];
  const int nb = min(*a.big_n, a.w.n_series);
  for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const int s = a.big_list[bi];
    if (threadIdx.x < 2 + SL_MAX_T) tot[threadIdx.x] = 0;
    __syncthreads();
    const int cls = slo_class(a.cls, a.n_classes, s);
    const int k = min(max(a.nthr[cls], 0), SL_MAX_T);
    SloCount ct;
    ct.load(a, cls, k);
    for_each_window_sample(a.w, s, [&](int32_t v) { ct.add(v); });
    for (int o = 32; o > 0; o >>= 1) {
      ct.m += __shfl_xor(ct.m, o, 64);
      ct.nan += __shfl_xor(ct.nan, o, 64);
#pragma unroll
      for (int j = 0; j < SL_MAX_T; ++j) ct.c[j] += __shfl_xor(ct.c[j], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&tot[0], ct.m);
      if (ct.nan) atomicAdd(&tot[1], ct.nan);
#pragma unroll
      for (int j = 0; j < SL_MAX_T; ++j)
        if (j < k && ct.c[j]) atomicAdd(&tot[2 + j], ct.c[j]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      SloRec o;
      o.m = tot[0];
      o.nan = tot[1];
#pragma unroll
      for (int j = 0; j < SL_MAX_T; ++j) o.c[j] = j < k ? tot[2 + j] : 0;
      a.rec[s] = o;
    }
    __syncthreads();
  }
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t sl_row(const SloTextArgs& a, int32_t s, int cls, int k, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const SloRec r = a.rec[s];
  o.lit("sl|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)r.m); o.c('|');
  o.u32((uint32_t)r.nan); o.c('|');
#pragma unroll
  for (int j = 0; j < SL_MAX_T; ++j) {
    if (j < k) {
      if (j) o.c(',');
      o.u32((uint32_t)a.thr[(size_t)cls * SL_MAX_T + j]);
      o.c(':');
      o.u32((uint32_t)r.c[j]);
    }
  }
  o.c('\n');
  o.finish();
  return o.n;
}

// series of emission position i that prints a row (-1: none), its class and threshold count
__device__ __forceinline__ int32_t sl_row_series(const SloTextArgs& a, int32_t i, int& cls, int& k) {
  const int32_t s = a.perm[i];
  if (s < 0 || s >= a.n_series) return -1;
  cls = slo_class(a.cls, a.n_classes, s);
  k = min(max(a.nthr[cls], 0), SL_MAX_T);
  return k >= 1 && a.rec[s].m >= 1 ? s : -1;
}

// the length pass' row policy (k_text_len)
struct SlRow {
  static __device__ __forceinline__ uint32_t len(const SloTextArgs& a, int32_t i) {
    int cls = 0, k = 0;
    const int32_t s = sl_row_series(a, i, cls, k);
    return s >= 0 ? sl_row<false>(a, s, cls, k, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(SL_ROWS) void k_slo_write(SloTextArgs a) {
  __shared__ __align__(16) char stage[SL_STAGE];
  const int32_t j0 = (int32_t)blockIdx.x * SL_ROWS;
  const int32_t j1 = min(a.n, j0 + SL_ROWS);
  const int32_t i = j0 + (int32_t)threadIdx.x;
  const uint32_t g0 = a.off[j0], g1 = a.off[j1];
  if (g1 == g0) return;                                  // (uniform) no row in this block
  const bool lds = (g1 - (g0 & ~3u)) <= SL_STAGE;        // (uniform)
  if (i < j1) {
    int cls = 0, k = 0;
    const int32_t s = sl_row_series(a, i, cls, k);
    if (s >= 0) {
      const uint32_t at = a.off[i];
      sl_row<true>(a, s, cls, k, lds ? stage + (at - (g0 & ~3u)) : a.out + at);
    }
  }
  __syncthreads();
  if (lds) block_copy_out<SL_ROWS>(stage, a.out, g0, g1);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_slo_group_max() { return SL_GROUP_MAX; }
int32_t apm_slo_stage_bytes() { return (int32_t)SL_STAGE; }

size_t apm_slo_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "sl|" + ts (<= 23) + names + 2 separators + m| + nan| (11 each) + 8 pairs of at most 10 + 10
// digits, a colon and a comma + newline
size_t apm_slo_row_bound(size_t name_bytes) { return 3 + 23 + name_bytes + 2 + 22 + (size_t)SL_MAX_T * 22 + 1; }

void apm_slo_values(SloArgs* a, hipStream_t stream) {
  const int32_t n = a->w.n_series;
  if (n <= 0) return;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  const int per_block = SL_WAVES * 2;
  hipLaunchKernelGGL(k_slo_group, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(SL_WAVES * APM_WAVE), 0,
                     stream, *a);
  // the list length is on the device: a fixed, small grid whose blocks loop over the list
  hipLaunchKernelGGL(k_slo_big, dim3(SL_BIG_GRID), dim3(SL_BLOCK), 0, stream, *a);
}

int apm_slo_plan(SloTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<SlRow, SL_LEN_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_slo_write(SloTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  hipLaunchKernelGGL(k_slo_write, dim3((uint32_t)((a->n + SL_ROWS - 1) / SL_ROWS)), dim3(SL_ROWS), 0, stream, *a);
}

}  // extern "C"
