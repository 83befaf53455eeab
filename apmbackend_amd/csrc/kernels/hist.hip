// K15: lh rows -- the samples of one ten-second bucket per series as a sparse log-linear
// histogram (docs/HISTOGRAM.md), encoded on the GPU like the st / fs rows (format.hip):
//   count  per emission position: 120-counter LDS histogram of the bucket's samples (inline cell +
//          the series' run in the slot's sorted spill list), row length from the non-zero bins
//   scan   exclusive prefix sums (textpass.h) -> byte offsets
//   write  the same histogram again, each lane prints its bins at its offset inside the row
// A bucket reads 1 / window of what K8 reads, so rebuilding the histogram in the write pass is
// cheaper than keeping 120 counters per series between the passes.
//
// Two paths, as in K8.  Group pass: 32 lanes per series (two series a wave, eight a block), for
// up to HIST_GROUP_MAX samples -- nearly every bucket fits its inline cell.  Larger buckets are
// deferred (big_list) to the block pass: 256 threads per series, any size up to the spill capacity.
// Both passes end in hist_emit: lane 0 of the 32 prints the row's head, lanes 1..30 four bins
// each, lane 31 the newline; a lane's offset inside the row is the scan of the lanes' byte counts.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "spill.h"

namespace apm {

namespace {

constexpr int HIST_LANES = 32;        // lanes per series (group pass), and of hist_emit
constexpr int HIST_GROUPS = 8;        // series per block (group pass)
constexpr int HIST_GROUP_MAX = 256;   // samples a group counts itself (8 per lane); more: block pass
constexpr int HIST_BLOCK = 256;       // threads per series (block pass)
constexpr int HIST_BIG_GRID = 256;    // blocks of the block pass (they loop over big_list)
constexpr int HIST_WORDS = 128;       // LDS words per series: bins [0, 120), [120] NaN samples

// samples [first, cnt) step `step` of series s in the bucket's slot -> h (LDS atomics)
__device__ __forceinline__ void hist_count(const HistArgs& a, int32_t s, int cnt, int first, int step, uint32_t* h) {
  const StatsState& st = a.st;
  const int32_t* cell = st.cells + ((size_t)a.slot * st.S + s) * st.cap;
  const int32_t* run = cnt > st.cap ? spill_run(st, a.slot, s) : nullptr;
  for (int k = first; k < cnt; k += step) {
    const int32_t v = k < st.cap ? cell[k] : run[k - st.cap];
    atomicAdd(&h[v == ELAPSED_NAN ? HIST_BINS : hist_bin(v)], 1u);
  }
}

// The row of emission position i from its finished histogram h, by 32 lanes (hl = 0..31; every
// lane of the wave runs this, `live` lanes store).  Returns the row's bytes.
template <bool W>
__device__ __forceinline__ uint32_t hist_emit(const HistArgs& a, int32_t i, int32_t s, uint32_t cnt, const uint32_t* h,
                                              int hl, bool live) {
  uint32_t c[4] = {0, 0, 0, 0};
  uint32_t nz = 0;
  if (hl >= 1 && hl <= 30) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = h[4 * (hl - 1) + j]; nz += c[j] != 0; }
  }
  // pairs before this lane's (the row's first pair takes no comma)
  uint32_t before = nz;
#pragma unroll
  for (int d = 1; d < HIST_LANES; d <<= 1) {
    const uint32_t y = __shfl_up(before, d, HIST_LANES);
    if (hl >= d) before += y;
  }
  before -= nz;
  // length of this lane's piece
  OutT<false> q(nullptr);
  if (hl == 0) {
    const int4 nm = a.series_names[s];
    q.n = 3 + (uint32_t)a.ts_len + (uint32_t)nm.y + 1 + (uint32_t)nm.w + 1;
    q.u32(cnt); q.c('|'); q.u32(h[HIST_BINS]); q.c('|');
  } else if (hl == 31) {
    q.c('\n');
  } else {
    uint32_t k = before;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c[j]) { if (k++) q.c(','); q.u32(hist_lower(4 * (hl - 1) + j)); q.c(':'); q.u32(c[j]); }
  }
  uint32_t inc = q.n;
#pragma unroll
  for (int d = 1; d < HIST_LANES; d <<= 1) {
    const uint32_t y = __shfl_up(inc, d, HIST_LANES);
    if (hl >= d) inc += y;
  }
  const uint32_t total = __shfl(inc, HIST_LANES - 1, HIST_LANES);
  if (W && live && q.n) {
    OutT<true> o(a.out + a.off[i] + (inc - q.n));
    if (hl == 0) {
      const int4 nm = a.series_names[s];
      o.lit("lh|");
      o.sb(a.ts, a.ts_len);
      o.s(a.names + nm.x, nm.y); o.c('|');
      o.s(a.names + nm.z, nm.w); o.c('|');
      o.u32(cnt); o.c('|'); o.u32(h[HIST_BINS]); o.c('|');
    } else if (hl == 31) {
      o.c('\n');
    } else {
      uint32_t k = before;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c[j]) { if (k++) o.c(','); o.u32(hist_lower(4 * (hl - 1) + j)); o.c(':'); o.u32(c[j]); }
    }
    o.finish();
  }
  return total;
}

// samples of emission position i's series in the bucket (0: no row)
__device__ __forceinline__ int hist_samples(const HistArgs& a, int32_t i, int32_t& s) {
  s = -1;
  if (i >= a.n) return 0;
  s = a.perm[i];
  if (s < 0 || s >= a.st.S || !a.st.active[s]) return 0;
  return max(a.st.counts[(size_t)a.slot * a.st.S + s], 0);
}

template <bool W>
__global__ __launch_bounds__(HIST_GROUPS * HIST_LANES) void k_hist_group(HistArgs a) {
  __shared__ uint32_t hist[HIST_GROUPS][HIST_WORDS];
  const int g = threadIdx.x / HIST_LANES, hl = threadIdx.x % HIST_LANES;
  const int32_t i = (int32_t)blockIdx.x * HIST_GROUPS + g;
  uint32_t* h = hist[g];
  int32_t s;
  const int cnt = hist_samples(a, i, s);
  const bool big = cnt > HIST_GROUP_MAX;
  const bool go = cnt > 0 && !big;
#pragma unroll
  for (int k = hl; k < HIST_WORDS; k += HIST_LANES) h[k] = 0;
  __syncthreads();
  if (go) hist_count(a, s, cnt, hl, HIST_LANES, h);
  __syncthreads();
  if (!W) {
    if (big && hl == 0) a.big_list[atomicAdd(a.big_n, 1)] = i;
    if (i == a.n && hl == 0) a.len[i] = 0;  // scan sentinel (-> total)
  }
  // (uniform per group; the shuffles inside stay within the group's 32 lanes)
  const uint32_t total = go ? hist_emit<W>(a, i, s, (uint32_t)cnt, h, hl, true) : 0u;
  if (!W && hl == 0 && i < a.n && !big) a.len[i] = total;
}

template <bool W>
__global__ __launch_bounds__(HIST_BLOCK) void k_hist_big(HistArgs a) {
  __shared__ uint32_t h[HIST_WORDS];
  const int nb = min(*a.big_n, a.n);
  for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const int32_t i = a.big_list[bi];
    int32_t s;
    const int cnt = hist_samples(a, i, s);
    if (cnt <= 0) continue;  // (uniform: never listed)
    if (threadIdx.x < HIST_WORDS) h[threadIdx.x] = 0;
    __syncthreads();
    hist_count(a, s, cnt, (int)threadIdx.x, HIST_BLOCK, h);
    __syncthreads();
    if (threadIdx.x < APM_WAVE) {  // the first wave; its lower 32 lanes store
      const int hl = (int)threadIdx.x % HIST_LANES;
      const uint32_t total = hist_emit<W>(a, i, s, (uint32_t)cnt, h, hl, threadIdx.x < HIST_LANES);
      if (!W && threadIdx.x == 0) a.len[i] = total;
    }
    __syncthreads();
  }
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_hist_group_max() { return HIST_GROUP_MAX; }

size_t apm_hist_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "lh|" + ts (<= 23) + names + 2 separators + count| + nan| (11 each) + 120 pairs of at most
// 10 + 1 + 10 digits and a comma + newline
size_t apm_hist_row_bound(size_t name_bytes) { return 3 + 23 + name_bytes + 2 + 22 + (size_t)HIST_BINS * 22 + 1; }

static uint32_t hist_group_blocks(int32_t n) { return (uint32_t)((n + 1 + HIST_GROUPS - 1) / HIST_GROUPS); }

int apm_hist_plan(HistArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  if (a->n <= 0) return 0;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  // (n + 1 positions: the group of position n stores the scan sentinel)
  hipLaunchKernelGGL(k_hist_group<false>, dim3(hist_group_blocks(a->n)), dim3(HIST_GROUPS * HIST_LANES), 0, stream, *a);
  hipLaunchKernelGGL(k_hist_big<false>, dim3(HIST_BIG_GRID), dim3(HIST_BLOCK), 0, stream, *a);
  PrimScratch sc(tmp, tmp_bytes);
  return text_scan(sc, a->len, a->off, (size_t)a->n + 1, stream);
}

void apm_hist_write(HistArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  hipLaunchKernelGGL(k_hist_group<true>, dim3(hist_group_blocks(a->n)), dim3(HIST_GROUPS * HIST_LANES), 0, stream, *a);
  hipLaunchKernelGGL(k_hist_big<true>, dim3(HIST_BIG_GRID), dim3(HIST_BLOCK), 0, stream, *a);
}

}  // extern "C"
