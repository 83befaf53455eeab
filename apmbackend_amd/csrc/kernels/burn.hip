// K21: sb rows -- SLO burn-rate breaches decided on the device (docs/BURN.md).
//
// A series' objective is its class' {T, q}: a sample is bad when it is finite and above T, and the
// error budget is b = 100000 - q.  A set of m finite samples burns at factor f when m >= minSamples
// and bad * 10^8 >= f * m * b (burncmp.h, exact on 32-bit limbs).  Rule j fires when the whole K8
// window and its newest span[j] buckets both burn at factor[j]; a span of k buckets is rw's: the
// window entries r >= n_win - min(k, n_win) (r = n_win - 1 is the newest).
// Value pass, on the window K8 just read (same slots, same samples, spill lists still sorted):
//   group  32 lanes per series, two series a wave, k_slo_group's shape.  No sort and no LDS: lane r
//          owns window entries r, r + 32, ... and reads their inline cells, the spill runs are
//          walked by the half with a stride of 32.  T and the spans' first entries sit in
//          registers; a sample adds to the window's (m, bad, nan) and, per rule, to (m_k, bad_k)
//          when its entry lies in the rule's span.  The counters are summed over the 32 lanes with
//          the DPP scans of winsort.h and lane 31 decides the rules.  A window of any length stays
//          here; only a series K8 counted more than SB_GROUP_MAX samples for is deferred.
//   block  one block per deferred series, the same counters over the window's entries.
// A class-0 or inactive series reads no sample.  One BurnRec per series.  Only integers.
// Text pass: K12's count / scan / write shape over the emission permutation; a position whose
// series has no rule that fired has length 0, which is the compaction.  Rows are rare, so the write
// pass stores each row directly through textout.h (no LDS stage).  The length kernel and the scan
// are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "burncmp.h"
#include "spill.h"
#include "winsort.h"

namespace apm {

namespace {

constexpr int SB_WAVES = 4;            // waves per block (group pass): eight series
constexpr int SB_GROUP_MAX = 4096;     // samples a 32-lane group counts itself (slo.hip SL_GROUP_MAX)
constexpr int SB_BLOCK = 256;          // threads per series (block pass)
constexpr int SB_BIG_GRID = 32;        // blocks of the block pass (they loop over big_list)
constexpr int SB_TEXT_BLOCK = 256;

// The counters of one lane.  A rule past nrule starts at INT32_MAX: no entry is in its span.
struct BurnCount {
  int32_t T;
  int32_t r_lo[SB_MAX_RULES];
  int32_t mk[SB_MAX_RULES], badk[SB_MAX_RULES];
  int32_t m = 0, bad = 0, nan = 0;
  __device__ __forceinline__ void load(const BurnArgs& a, int cls) {
    T = a.obj[(size_t)cls * 2];
#pragma unroll
    for (int j = 0; j < SB_MAX_RULES; ++j) {
      r_lo[j] = j < a.nrule ? a.w.n_win - min(a.span[j], a.w.n_win) : 0x7fffffff;
      mk[j] = 0;
      badk[j] = 0;
    }
  }
  // bit j: window entry r lies in rule j's span
  __device__ __forceinline__ int spans_of(int r) const {
    int in = 0;
#pragma unroll
    for (int j = 0; j < SB_MAX_RULES; ++j) in |= (r >= r_lo[j] ? 1 : 0) << j;
    return in;
  }
  __device__ __forceinline__ void add(int32_t v, int in) {
    const int fin = v != ELAPSED_NAN ? 1 : 0;
    const int b = (fin && v > T) ? 1 : 0;
    nan += 1 - fin;
    m += fin;
    bad += b;
#pragma unroll
    for (int j = 0; j < SB_MAX_RULES; ++j) {
      const int inj = (in >> j) & 1;
      mk[j] += fin & inj;
      badk[j] += b & inj;
    }
  }
};

// class of series s: [0, n_classes), anything else is "no row"
__device__ __forceinline__ int burn_class(const int32_t* cls, int n_classes, int s) {
  const int c = cls[s];
  return c > 0 && c < n_classes ? c : 0;
}

// the record of a series from its totals: every rule decided by the shared routine
__device__ __forceinline__ BurnRec burn_decide(const BurnArgs& a, int cls, int32_t m, int32_t bad, int32_t nan,
                                               const int32_t (&mk)[SB_MAX_RULES], const int32_t (&badk)[SB_MAX_RULES]) {
  BurnRec o;
  o.m = m;
  o.bad = bad;
  o.nan = nan;
  const uint32_t b = (uint32_t)(100000 - a.obj[(size_t)cls * 2 + 1]);
  const uint32_t ms = (uint32_t)a.min_samples;
  int fired = 0;
#pragma unroll
  for (int j = 0; j < SB_MAX_RULES; ++j) {
    const bool on = j < a.nrule;
    o.mk[j] = on ? mk[j] : 0;
    o.badk[j] = on ? badk[j] : 0;
    if (on) {
      const uint32_t f = (uint32_t)a.factor[j];
      if (burn_fires((uint32_t)bad, (uint32_t)m, b, f, ms) && burn_fires((uint32_t)badk[j], (uint32_t)mk[j], b, f, ms))
        fired |= 1 << j;
    }
  }
  o.fired = fired;
  return o;
}

__global__ __launch_bounds__(SB_WAVES * APM_WAVE) void k_burn_group(BurnArgs a) {
  const WindowArgs& w = a.w;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (HW - 1);
  const int wv = threadIdx.x >> 6;
  const int s = (blockIdx.x * SB_WAVES + wv) * 2 + half;
  const bool valid = s < w.n_series;
  int cls = 0;
  bool big = false;
  if (valid && w.st.active[s]) {
    cls = burn_class(a.cls, a.n_classes, s);
    big = cls > 0 && w.out[s].n > SB_GROUP_MAX;
  }
  if (big && hl == 0) { const int j = atomicAdd(a.big_n, 1); a.big_list[j] = s; }
  const bool go = cls > 0 && !big;
  // no objective, inactive or deferred: nothing is read; the wave leaves when neither half counts
  // (the moves below are 32 lanes wide and need both halves, so one half alone does not return)
  if (valid && !go && !big && hl == HW - 1) { BurnRec z{}; a.rec[s] = z; }
  if (!__ballot(go)) return;
  BurnCount ct;
  ct.load(a, cls);  // (cls 0: row 0 of the table, read and never used)
  // inline cells: lane hl owns entries hl, hl + 32, ... and reads their cells itself
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
      const int in = ct.spans_of(r);
      const int32_t* cell = w.st.cells + ((size_t)slot * w.st.S + s) * w.st.cap;
      for (int i = 0; i < inl; ++i) ct.add(cell[i], in);
    }
    // spill runs: each entry's run found by its lane, walked by the half with a stride of 32
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
          const int in = ct.spans_of(r0 + b);  // the run's entry, not this lane's
          const int32_t* src = (const int32_t*)rp;
          for (int i = hl; i < mm; i += HW) ct.add(src[i], in);
        }
      }
    }
  }
  // totals of the half in its lane 31 (inclusive scans); every lane of the wave takes part
  ct.m = half_scan(ct.m);
  ct.bad = half_scan(ct.bad);
  ct.nan = half_scan(ct.nan);
#pragma unroll
  for (int j = 0; j < SB_MAX_RULES; ++j) {
    if (j < a.nrule) {  // (uniform)
      ct.mk[j] = half_scan(ct.mk[j]);
      ct.badk[j] = half_scan(ct.badk[j]);
    }
  }
  if (go && hl == HW - 1) a.rec[s] = burn_decide(a, cls, ct.m, ct.bad, ct.nan, ct.mk, ct.badk);
}

__global__ __launch_bounds__(SB_BLOCK) void k_burn_big(BurnArgs a) {
  __shared__ int32_t tot[3 + 2 * SB_MAX_RULES];
  const WindowArgs& w = a.w;
  const int nb = min(*a.big_n, w.n_series);
  for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const int s = a.big_list[bi];
    if (threadIdx.x < 3 + 2 * SB_MAX_RULES) tot[threadIdx.x] = 0;
    __syncthreads();
    const int cls = burn_class(a.cls, a.n_classes, s);
    BurnCount ct;
    ct.load(a, cls);
    for (int r = 0; r < w.n_win; ++r) {
      const int sl = win_slot(w, r);
      if (sl < 0) continue;
      const int cnt = max(w.st.counts[(size_t)sl * w.st.S + s], 0);
      const int inl = min(cnt, w.st.cap);
      const int in = ct.spans_of(r);
      const int32_t* cell = w.st.cells + ((size_t)sl * w.st.S + s) * w.st.cap;
      for (int k = threadIdx.x; k < inl; k += blockDim.x) ct.add(cell[k], in);
      if (cnt > inl) {
        const int32_t* run = spill_run(w.st, sl, s);
        for (int k = threadIdx.x; k < cnt - inl; k += blockDim.x) ct.add(run[k], in);
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      ct.m += __shfl_xor(ct.m, o, 64);
      ct.bad += __shfl_xor(ct.bad, o, 64);
      ct.nan += __shfl_xor(ct.nan, o, 64);
#pragma unroll
      for (int j = 0; j < SB_MAX_RULES; ++j) {
        ct.mk[j] += __shfl_xor(ct.mk[j], o, 64);
        ct.badk[j] += __shfl_xor(ct.badk[j], o, 64);
      }
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&tot[0], ct.m);
      if (ct.bad) atomicAdd(&tot[1], ct.bad);
      if (ct.nan) atomicAdd(&tot[2], ct.nan);
#pragma unroll
      for (int j = 0; j < SB_MAX_RULES; ++j) {
        if (ct.mk[j]) atomicAdd(&tot[3 + j], ct.mk[j]);
        if (ct.badk[j]) atomicAdd(&tot[3 + SB_MAX_RULES + j], ct.badk[j]);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int32_t mk[SB_MAX_RULES], badk[SB_MAX_RULES];
#pragma unroll
      for (int j = 0; j < SB_MAX_RULES; ++j) { mk[j] = tot[3 + j]; badk[j] = tot[3 + SB_MAX_RULES + j]; }
      a.rec[s] = burn_decide(a, cls, tot[0], tot[1], tot[2], mk, badk);
    }
    __syncthreads();
  }
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t sb_row(const BurnTextArgs& a, int32_t s, int cls, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const BurnRec r = a.rec[s];
  o.lit("sb|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)a.obj[(size_t)cls * 2]); o.c('|');
  o.u32((uint32_t)a.obj[(size_t)cls * 2 + 1]); o.c('|');
  o.u32((uint32_t)r.m); o.c('|');
  o.u32((uint32_t)r.bad); o.c('|');
  o.u32((uint32_t)r.nan); o.c('|');
#pragma unroll
  for (int j = 0; j < SB_MAX_RULES; ++j) {
    if (j < a.nrule) {
      if (j) o.c(',');
      o.u32((uint32_t)a.span[j]); o.c(':');  // (the configured value, not the clipped one)
      o.u32((uint32_t)a.factor[j]); o.c(':');
      o.u32((uint32_t)r.mk[j]); o.c(':');
      o.u32((uint32_t)r.badk[j]); o.c(':');
      o.c((r.fired >> j) & 1 ? '1' : '0');
    }
  }
  o.c('\n');
  o.finish();
  return o.n;
}

// series of emission position i that prints a row (-1: none) and its class: a rule fired (the
// value pass wrote a zero record for every series without an objective or an st row)
__device__ __forceinline__ int32_t sb_row_series(const BurnTextArgs& a, int32_t i, int& cls) {
  const int32_t s = a.perm[i];
  if (s < 0 || s >= a.n_series) return -1;
  cls = burn_class(a.cls, a.n_classes, s);
  return cls > 0 && a.rec[s].fired != 0 ? s : -1;
}

// the length pass' row policy (k_text_len)
struct SbRow {
  static __device__ __forceinline__ uint32_t len(const BurnTextArgs& a, int32_t i) {
    int cls = 0;
    const int32_t s = sb_row_series(a, i, cls);
    return s >= 0 ? sb_row<false>(a, s, cls, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(SB_TEXT_BLOCK) void k_burn_write(BurnTextArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * SB_TEXT_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  int cls = 0;
  const int32_t s = sb_row_series(a, i, cls);
  if (s >= 0) sb_row<true>(a, s, cls, a.out + a.off[i]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_burn_group_max() { return SB_GROUP_MAX; }

size_t apm_burn_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "sb|" + ts (<= 23) + names + 2 separators + T| + q| + m| + bad| + nan| (11 each) + 4 groups of
// four numbers of at most 10 digits with their colons, the flag and a comma + newline
size_t apm_burn_row_bound(size_t name_bytes) { return 3 + 23 + name_bytes + 2 + 55 + (size_t)SB_MAX_RULES * 46 + 1; }

void apm_burn_values(BurnArgs* a, hipStream_t stream) {
  const int32_t n = a->w.n_series;
  if (n <= 0 || a->nrule <= 0) return;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  const int per_block = SB_WAVES * 2;
  hipLaunchKernelGGL(k_burn_group, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(SB_WAVES * APM_WAVE), 0,
                     stream, *a);
  // the list length is on the device: a fixed, small grid whose blocks loop over the list
  hipLaunchKernelGGL(k_burn_big, dim3(SB_BIG_GRID), dim3(SB_BLOCK), 0, stream, *a);
}

int apm_burn_plan(BurnTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<SbRow, SB_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_burn_write(BurnTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  hipLaunchKernelGGL(k_burn_write, dim3((uint32_t)((a->n + SB_TEXT_BLOCK - 1) / SB_TEXT_BLOCK)), dim3(SB_TEXT_BLOCK), 0,
                     stream, *a);
}

}  // extern "C"
