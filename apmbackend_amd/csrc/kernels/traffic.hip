// K22: tf rows -- traffic drops and surges decided on the device (docs/TRAFFIC.md).
//
// Per series and rule j the newest k' = min(span[j], n_win) window buckets hold R samples; the other
// B = n_win - k' buckets are the baseline: med2 is twice the median of their counts, mad4 four
// times the median absolute deviation.  trafficcmp.h decides D / S / N from those integers.
// Value pass, on the window K8 just read.  It reads counts[slot][s] only -- no cell, no spill list:
//   group  a block takes 64 consecutive series.  Its four waves read one slot row each at a time,
//          64 consecutive counts (256 B) per wave, and store them transposed into an LDS tile of
//          odd pitch: the column store of a 32-lane group and the row read of a half (lane l reads
//          entries l, l + 32, ...: 32 consecutive dwords a load) both touch 32 different banks.
//          Each 32-lane half then takes eight of the tile's series in turn: the
//          row sits in registers (E entries a lane, n_win <= 32 E), per rule the entries outside
//          the baseline are replaced by INT32_MAX and winsort.h's register network sorts the rest;
//          the two middle entries come back by lane moves, the deviations are sorted the same
//          way.  No scratch, no device state.
//   wide   windows of more than 128 buckets: a block takes eight series, one per half, the rows in
//          dynamic LDS; the order statistics are found by counting (every lane ranks its entries
//          against the whole row).  Quadratic in n_win: routing decides cost only.
// A class-0 or inactive series reads no count and gets a zero record.  Only integers.
// Text pass: K12's count / scan / write shape over the emission permutation; a position whose
// series has no rule with a verdict has length 0, which is the compaction.  Rows are rare, so the
// write pass stores each row directly through textout.h (no LDS stage).  The length kernel and the
// scan are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "trafficcmp.h"
#include "winsort.h"

namespace apm {

namespace {

constexpr int TF_TILE = 64;            // series per block (group pass): one wave reads a slot row of the tile
constexpr int TF_BLOCK = 256;
constexpr int TF_ROWS = TF_BLOCK / TF_TILE;  // slot rows in flight per block
constexpr int TF_HALVES = TF_BLOCK / HW;     // series sorted at a time
constexpr int TF_GROUP_WIN = 128;      // window buckets the group pass takes (E = 4)
constexpr int TF_WIDE = TF_HALVES;     // series per block (wide pass)
constexpr int TF_WIDE_WIN = 2047;      // (8 rows of n_win | 1 dwords in 64 KiB of LDS)
constexpr int TF_TEXT_BLOCK = 256;

// class of series s: [0, n_classes), anything else is "no row"
__device__ __forceinline__ int traffic_class(const int32_t* cls, int n_classes, int s) {
  const int c = cls[s];
  return c > 0 && c < n_classes ? c : 0;
}

// entry i of the half's sorted 32 E entries (reg_bitonic's layout); i is the same in every lane
template <int E>
__device__ __forceinline__ int32_t sorted_at(const int32_t (&v)[E], int i) {
  const int rem = i % (16 * E);
  const int src = (i / (16 * E)) * 16 + (rem & 15), e = rem >> 4;
  int32_t out = 0;
#pragma unroll
  for (int q = 0; q < E; ++q) {
    const int32_t t = __shfl(v[q], src, HW);
    if (q == e) out = t;
  }
  return out;
}

// the rules of one series from its per-rule totals: every verdict by the shared routine
struct TrafficOut {
  TrafficRec o;
  __device__ __forceinline__ void begin(int32_t n) {
    o.n = n;
    o.verdict = 0;
#pragma unroll
    for (int j = 0; j < TF_MAX_RULES; ++j) { o.R[j] = 0; o.med2[j] = 0; o.B[j] = 0; o.mad4[j] = 0; }
  }
  __device__ __forceinline__ void rule(const TrafficArgs& a, int j, int cls, int kk, int B, uint32_t R, int64_t med2,
                                       int64_t mad4) {
    o.R[j] = R;
    o.med2[j] = (uint32_t)med2;
    o.B[j] = B;
    o.mad4[j] = (uint64_t)mad4;
    o.verdict |= traffic_verdict((int64_t)R, med2, mad4, B, kk, a.drop[j], a.surge[j], a.z[j], a.rate[cls],
                                 a.min_buckets) << (2 * j);
  }
};

template <int E>
__global__ __launch_bounds__(TF_BLOCK) void k_traffic_group(TrafficArgs a) {
  constexpr int P = 32 * E + 1;  // odd: column s of row r and entry r of series s both spread over the banks
  __shared__ int32_t tile[TF_TILE * P];
  __shared__ int32_t cls_of[TF_TILE];
  const WindowArgs& w = a.w;
  const int s0 = blockIdx.x * TF_TILE;
  {
    // the tile: wave rsub reads slot rows rsub, rsub + 4, ..., lane sl the count of series s0 + sl
    const int sl = threadIdx.x & (TF_TILE - 1), rsub = threadIdx.x / TF_TILE;
    const int s = s0 + sl;
    int cls = 0;
    if (s < w.n_series && w.st.active[s]) cls = traffic_class(a.cls, a.n_classes, s);
    if (rsub == 0) cls_of[sl] = cls;
    for (int r = rsub; r < w.n_win; r += TF_ROWS) {  // (n_win <= 32 E: the launch routes by it)
      const int slot = win_slot(w, r);
      int c = 0;
      if (slot >= 0 && cls > 0) c = max(w.st.counts[(size_t)slot * w.st.S + s], 0);
      tile[sl * P + r] = c;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (HW - 1);
  const int g = (threadIdx.x >> 6) * 2 + half;
  const int base = (hl >> 4) * (16 * E) + (hl & 15);
  for (int it = 0; it < TF_TILE / TF_HALVES; ++it) {
    const int sl = it * TF_HALVES + g;
    const int s = s0 + sl;
    const int cls = cls_of[sl];
    if (s < w.n_series && cls == 0 && hl == 0) { TrafficOut z; z.begin(0); a.rec[s] = z.o; }
    // the moves below are a wave wide: a wave leaves a round only when neither half has a series
    if (!__ballot(cls > 0)) continue;
    // raw[e] is window entry hl + 32 e: a load reads 32 consecutive dwords per half.  (Which lane
    // holds which entry does not matter to the sort; only the sorted positions below are the
    // network's base + 16 e.)
    int32_t raw[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int r = hl + HW * e;
      raw[e] = r < w.n_win ? tile[sl * P + r] : 0;
    }
    TrafficOut out;
    out.begin(cls > 0 ? w.out[s].n : 0);
#pragma unroll
    for (int j = 0; j < TF_MAX_RULES; ++j) {
      if (j >= a.nrule) continue;  // (uniform)
      const int kk = min(a.span[j], w.n_win), B = w.n_win - kk;
      int32_t v[E];
      // R in 32 bits: the counts of a series' window sum to WinStat.n, an int32, so no partial sum
      // passes 2^31 - 1 here.  (trafficcmp.h's bound R < 2^37 is what the routine itself is exact
      // for -- 64 buckets of 2^31 - 1 -- not what a kernel carries.)
      int rs = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const bool in = hl + HW * e < B;
        v[e] = in ? raw[e] : 0x7fffffff;
        rs += in ? 0 : raw[e];
      }
      const uint32_t R = (uint32_t)half_last(half_scan(rs), half);
      int64_t med2 = 0, mad4 = 0;
      if (B > 0) {  // (uniform)
        const int lo = (B - 1) >> 1, hi = B >> 1;
        reg_bitonic<E>(v, hl);
        med2 = (int64_t)sorted_at<E>(v, lo) + (int64_t)sorted_at<E>(v, hi);
        // |2 b - med2| has med2's parity for every b: half of it (at most 2^31 - 1) keeps the order
        int32_t d[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int64_t x = 2 * (int64_t)v[e] - med2;
          d[e] = base + e * 16 < B ? (int32_t)((x < 0 ? -x : x) >> 1) : 0x7fffffff;
        }
        reg_bitonic<E>(d, hl);
        mad4 = 2 * ((int64_t)sorted_at<E>(d, lo) + (int64_t)sorted_at<E>(d, hi)) + 2 * (med2 & 1);
      }
      out.rule(a, j, cls, kk, B, R, med2, mad4);
    }
    if (cls > 0 && hl == 0) a.rec[s] = out.o;
  }
}

__device__ __forceinline__ int32_t half_max(int32_t x) {
#pragma unroll
  for (int o = HW / 2; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, HW));
  return x;
}
__device__ __forceinline__ uint32_t half_sum(uint32_t x) {
#pragma unroll
  for (int o = HW / 2; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o, HW);
  return x;
}

// entries t_lo and t_hi of the ascending keys of row[0, B), found by counting: entry i is the t-th
// when (keys below it) <= t < (keys at or below it).  DEV: the key is |2 c - med2| / 2, else c.
template <bool DEV>
__device__ __forceinline__ void wide_select(const int32_t* row, int B, int64_t med2, int t_lo, int t_hi, int hl,
                                            int64_t& k_lo, int64_t& k_hi) {
  const auto key = [&](int i) -> int32_t {
    const int32_t c = row[i];
    if (!DEV) return c;
    const int64_t x = 2 * (int64_t)c - med2;
    return (int32_t)((x < 0 ? -x : x) >> 1);
  };
  int32_t f_lo = -1, f_hi = -1;
  for (int i0 = 0; i0 < B; i0 += HW) {
    const int i = i0 + hl;
    const int32_t x = i < B ? key(i) : 0;
    int lt = 0, le = 0;
    for (int q = 0; q < B; ++q) {
      const int32_t y = key(q);
      lt += y < x ? 1 : 0;
      le += y <= x ? 1 : 0;
    }
    if (i < B && lt <= t_lo && t_lo < le) f_lo = x;
    if (i < B && lt <= t_hi && t_hi < le) f_hi = x;
  }
  k_lo = half_max(f_lo);  // (keys are >= 0; every lane that found the entry found the same key)
  k_hi = half_max(f_hi);
}

__global__ __launch_bounds__(TF_BLOCK) void k_traffic_wide(TrafficArgs a) {
  extern __shared__ int32_t wide_rows[];  // [TF_WIDE][n_win | 1]
  const WindowArgs& w = a.w;
  const int P = w.n_win | 1;
  const int s0 = blockIdx.x * TF_WIDE;
  {
    const int sl = threadIdx.x & (TF_WIDE - 1), rsub = threadIdx.x / TF_WIDE;
    const int s = s0 + sl;
    int cls = 0;
    if (s < w.n_series && w.st.active[s]) cls = traffic_class(a.cls, a.n_classes, s);
    for (int r = rsub; r < w.n_win; r += TF_BLOCK / TF_WIDE) {
      const int slot = win_slot(w, r);
      int c = 0;
      if (slot >= 0 && cls > 0) c = max(w.st.counts[(size_t)slot * w.st.S + s], 0);
      wide_rows[sl * P + r] = c;
    }
  }
  __syncthreads();
  const int hl = threadIdx.x & (HW - 1);
  const int g = threadIdx.x / HW;
  const int s = s0 + g;
  if (s >= w.n_series) return;  // (a whole half; nothing below crosses halves)
  int cls = 0;
  if (w.st.active[s]) cls = traffic_class(a.cls, a.n_classes, s);
  TrafficOut out;
  if (cls == 0) {
    if (hl == 0) { out.begin(0); a.rec[s] = out.o; }
    return;
  }
  const int32_t* row = wide_rows + g * P;
  out.begin(w.out[s].n);
#pragma unroll
  for (int j = 0; j < TF_MAX_RULES; ++j) {
    if (j >= a.nrule) continue;
    const int kk = min(a.span[j], w.n_win), B = w.n_win - kk;
    uint32_t rs = 0;
    for (int r = B + hl; r < w.n_win; r += HW) rs += (uint32_t)row[r];
    const uint32_t R = half_sum(rs);
    int64_t med2 = 0, mad4 = 0;
    if (B > 0) {
      const int lo = (B - 1) >> 1, hi = B >> 1;
      int64_t x_lo, x_hi;
      wide_select<false>(row, B, 0, lo, hi, hl, x_lo, x_hi);
      med2 = x_lo + x_hi;
      wide_select<true>(row, B, med2, lo, hi, hl, x_lo, x_hi);
      mad4 = 2 * (x_lo + x_hi) + 2 * (med2 & 1);
    }
    out.rule(a, j, cls, kk, B, R, med2, mad4);
  }
  if (hl == 0) a.rec[s] = out.o;
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t tf_row(const TrafficTextArgs& a, int32_t s, int cls, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const TrafficRec& r = a.rec[s];  // (read field by field: a local copy indexed by the rule is scratch memory)
  o.lit("tf|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)r.n); o.c('|');
  o.u32((uint32_t)a.rate[cls]); o.c('|');
#pragma unroll
  for (int j = 0; j < TF_MAX_RULES; ++j) {
    if (j < a.nrule) {
      if (j) o.c(',');
      o.u32((uint32_t)a.span[j]); o.c(':');  // (the configured value, not the clipped one)
      o.u32((uint32_t)r.B[j]); o.c(':');
      o.u32(r.R[j]); o.c(':');
      o.u32(r.med2[j]); o.c(':');
      // mad4 < 2^34: above 2^32 the quotient by 10^8 has two digits
      const uint64_t m4 = r.mad4[j];
      if (m4 <= 0xffffffffull) {
        o.u32((uint32_t)m4);
      } else {
        const uint64_t q = m4 / 100000000ull;
        o.u32((uint32_t)q);
        o.u32_fixed8((uint32_t)(m4 - q * 100000000ull));
      }
      o.c(':');
      const int v = (r.verdict >> (2 * j)) & 3;
      o.c(v == TF_D ? 'D' : v == TF_S ? 'S' : 'N');
    }
  }
  o.c('\n');
  o.finish();
  return o.n;
}

// series of emission position i that prints a row (-1: none) and its class: a rule has a verdict
// (the value pass wrote a zero record for every series without a class or an st row)
__device__ __forceinline__ int32_t tf_row_series(const TrafficTextArgs& a, int32_t i, int& cls) {
  const int32_t s = a.perm[i];
  if (s < 0 || s >= a.n_series) return -1;
  cls = traffic_class(a.cls, a.n_classes, s);
  return cls > 0 && a.rec[s].verdict != 0 ? s : -1;
}

// the length pass' row policy (k_text_len)
struct TfRow {
  static __device__ __forceinline__ uint32_t len(const TrafficTextArgs& a, int32_t i) {
    int cls = 0;
    const int32_t s = tf_row_series(a, i, cls);
    return s >= 0 ? tf_row<false>(a, s, cls, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(TF_TEXT_BLOCK) void k_traffic_write(TrafficTextArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * TF_TEXT_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  int cls = 0;
  const int32_t s = tf_row_series(a, i, cls);
  if (s >= 0) tf_row<true>(a, s, cls, a.out + a.off[i]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_traffic_group_win() { return TF_GROUP_WIN; }
int32_t apm_traffic_max_win() { return TF_WIDE_WIN; }
int32_t apm_traffic_tile() { return TF_TILE; }

size_t apm_traffic_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "tf|" + ts (<= 23) + names + 2 separators + n| + minRate| (11 each) + 4 groups of five numbers of
// at most 10 digits with their colons, the verdict and a comma + newline
size_t apm_traffic_row_bound(size_t name_bytes) { return 3 + 23 + name_bytes + 2 + 22 + (size_t)TF_MAX_RULES * 57 + 1; }

int apm_traffic_values(TrafficArgs* a, hipStream_t stream) {
  const int32_t n = a->w.n_series;
  if (n <= 0 || a->nrule <= 0) return 0;
  const int32_t nw = a->w.n_win;
  if (nw < 1 || nw > TF_WIDE_WIN) return -1;
  const dim3 grid((uint32_t)((n + TF_TILE - 1) / TF_TILE)), block(TF_BLOCK);
  if (nw <= 32) {
    hipLaunchKernelGGL(k_traffic_group<1>, grid, block, 0, stream, *a);
  } else if (nw <= 64) {
    hipLaunchKernelGGL(k_traffic_group<2>, grid, block, 0, stream, *a);
  } else if (nw <= TF_GROUP_WIN) {
    hipLaunchKernelGGL(k_traffic_group<4>, grid, block, 0, stream, *a);
  } else {
    const size_t lds = (size_t)TF_WIDE * (size_t)(nw | 1) * 4;
    hipLaunchKernelGGL(k_traffic_wide, dim3((uint32_t)((n + TF_WIDE - 1) / TF_WIDE)), block, lds, stream, *a);
  }
  return 0;
}

int apm_traffic_plan(TrafficTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<TfRow, TF_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_traffic_write(TrafficTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  hipLaunchKernelGGL(k_traffic_write, dim3((uint32_t)((a->n + TF_TEXT_BLOCK - 1) / TF_TEXT_BLOCK)), dim3(TF_TEXT_BLOCK),
                     0, stream, *a);
}

}  // extern "C"
