// K23: po rows -- peer-outlier servers per service, decided on the device (docs/PEERS.md).
//
// The unit of work is K19's group: the series of one service on this engine (the CSR the host
// keeps, members in emission order).  Stage A is K16's value pass with one percentile: per series
// the finite sample count m and x = sum2, twice the window percentile.  A member is eligible when
// it is active, has a class other than 0 and m >= min_samples.  Over the E eligible members
//   X2 = x_lo + x_hi            of the ascending x,            lo = (E - 1) / 2, hi = E / 2
//   D4 = d_lo + d_hi            of the ascending d_i = |2 x_i - X2|
// and peercmp.h decides H / L / N per eligible member from those integers.
// Value pass (stage B):
//   group  32 lanes per group, two groups a wave; lane l holds members l, l + 32, ... (PEER_E of
//          them) in registers.  |x| < 2^32 and d < 2^35 do not fit winsort.h's int32 networks, so
//          the order statistics are found by counting: member i's rank is the number of eligible
//          members j with (key_j, j) < (key_i, i), a permutation of 0 .. E - 1, from lane reads of
//          the other lanes' 64-bit keys; the lanes holding ranks lo and hi publish their keys by a
//          32-lane sum in which every other lane adds 0.  The same routine runs over d.  Both
//          halves of a wave run every loop the larger number of times (the lane reads are a wave
//          wide).  Every lane stores the records of its own members.  No LDS, no scratch.
//   block  groups of more than 32 PEER_E members: one block per deferred group, looping over the
//          list.  The members' (m, x) are staged in their own records, then each thread ranks its
//          members against all of the group's keys read back from global memory.  Quadratic, and
//          without a bound on the group's size: routing decides cost only.
// An inactive, class-0 or ineligible series gets a zero record.  Only integers.
// Text pass: K12's count / scan / write shape over the emission permutation; a position whose
// series has no verdict has length 0, which is the compaction.  Rows are rare, so the write pass
// stores each row directly through textout.h (no LDS stage).  The length kernel and the scan are
// textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "peercmp.h"

namespace apm {

namespace {

constexpr int PO_HW = 32;              // lanes per group
constexpr int PEER_E = 4;              // members a lane holds (group pass)
constexpr int PO_GROUP_MAX = PO_HW * PEER_E;
constexpr int PO_WAVES = 4;            // waves per block (group pass): eight groups
constexpr int PO_BLOCK = 256;          // threads per group (block pass)
constexpr int PO_BIG_GRID = 256;       // blocks of the block pass (they loop over big_list)
constexpr int PO_TEXT_BLOCK = 256;

// class of series s: [0, n_classes), anything else is "no row"
__device__ __forceinline__ int peer_class(const int32_t* cls, int n_classes, int s) {
  const int c = cls[s];
  return c > 0 && c < n_classes ? c : 0;
}

__device__ __forceinline__ int po_half_sum(int x) {
#pragma unroll
  for (int o = PO_HW / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, PO_HW);
  return x;
}
__device__ __forceinline__ int po_half_min(int x) {
#pragma unroll
  for (int o = PO_HW / 2; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, PO_HW));
  return x;
}
__device__ __forceinline__ long long po_half_sum64(long long x) {
#pragma unroll
  for (int o = PO_HW / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, PO_HW);
  return x;
}

// rank[e]: the eligible members of this half whose (key, index) is below that of this lane's member
// e (index = lane + 32 e).  cnt: members of the larger of the wave's two groups, so both halves run
// the same loops; a half with fewer members reads keys of ineligible lanes and counts none.
template <int E>
__device__ __forceinline__ void half_ranks(const long long (&k)[E], const bool (&el)[E], int hl, int half, int cnt,
                                           int (&rank)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) rank[e] = 0;
#pragma unroll
  for (int f = 0; f < E; ++f) {
    if (f * PO_HW < cnt) {  // (uniform)
      const unsigned long long b = __ballot(el[f]);
      const unsigned int mask = (unsigned int)(half ? (b >> 32) : (b & 0xffffffffull));
      const int jn = min(PO_HW, cnt - f * PO_HW);
      for (int j = 0; j < jn; ++j) {
        const long long y = __shfl(k[f], j, PO_HW);
        const bool ye = (mask >> j) & 1u;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const bool before = y < k[e] || (y == k[e] && (f < e || (f == e && j < hl)));
          rank[e] += ye && before ? 1 : 0;
        }
      }
    }
  }
}

// the key of rank t among the half's eligible members (the ranks are a permutation: one lane adds
// its key, every other one 0; 0 when no member has the rank)
template <int E>
__device__ __forceinline__ long long half_pick(const long long (&k)[E], const bool (&el)[E], const int (&rank)[E], int t) {
  long long v = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) v += el[e] && rank[e] == t ? k[e] : 0;
  return po_half_sum64(v);
}

__device__ __forceinline__ long long po_dev(long long x, long long X2) {
  const long long d = 2 * x - X2;  // |.| < 2^35
  return d < 0 ? -d : d;
}

__global__ __launch_bounds__(PO_WAVES * APM_WAVE) void k_peer_group(PeerArgs a) {
  constexpr int E = PEER_E;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, hl = lane & (PO_HW - 1);
  const int wv = threadIdx.x >> 6;
  const int g = (blockIdx.x * PO_WAVES + wv) * 2 + half;
  // no early return per half: the lane reads below are a wave wide, and both halves run them
  const bool valid = g < a.n_groups;
  const int m0 = valid ? a.grp_off[g] : 0;
  const int nmem = valid ? a.grp_off[g + 1] - m0 : 0;
  const bool big = nmem > PO_GROUP_MAX;
  if (big && hl == 0) { const int j = atomicAdd(a.big_n, 1); a.big_list[j] = g; }
  const int mine_n = big ? 0 : nmem;
  const int cnt = max(mine_n, __shfl_xor(mine_n, 32));
  if (cnt == 0) return;  // (the whole wave)
  int32_t ser[E], mm[E];
  long long x[E];
  bool el[E];
  int n_el = 0, first = 0x7fffffff, first_cls = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int idx = hl + PO_HW * e;
    int s = idx < mine_n ? a.grp_mem[m0 + idx] : -1;
    if (s >= a.n_series) s = -1;
    ser[e] = s;
    mm[e] = 0;
    x[e] = 0;
    el[e] = false;
    if (s >= 0 && a.active[s]) {
      const int c = peer_class(a.cls, a.n_classes, s);
      const int m = a.m[s];
      if (c > 0 && m >= a.min_samples) {
        el[e] = true;
        mm[e] = m;
        x[e] = a.sum2[s];
        ++n_el;
        if (idx < first) { first = idx; first_cls = c; }
      }
    }
  }
  const int n_elig = po_half_sum(n_el);
  // the group's class is its first eligible member's (a service's members share one)
  const int gfirst = po_half_min(first);
  const int gcls = po_half_sum(first == gfirst && n_el > 0 ? first_cls : 0);
  long long X2 = 0, D4 = 0;
  if (__ballot(n_elig > 0)) {  // (uniform: a wave without an eligible member ranks nothing)
    const int lo = (n_elig - 1) >> 1, hi = n_elig >> 1;  // (n_elig == 0: no member has rank -1 or 0)
    int rank[E];
    half_ranks<E>(x, el, hl, half, cnt, rank);
    X2 = half_pick<E>(x, el, rank, lo) + half_pick<E>(x, el, rank, hi);
    long long d[E];
#pragma unroll
    for (int e = 0; e < E; ++e) d[e] = po_dev(x[e], X2);
    half_ranks<E>(d, el, hl, half, cnt, rank);
    D4 = half_pick<E>(d, el, rank, lo) + half_pick<E>(d, el, rank, hi);
  }
  const int32_t min_value = a.val[gcls];  // (gcls < n_classes; class 0 when nothing is eligible)
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (ser[e] < 0) continue;
    PeerRec r;
    r.m = mm[e];
    r.verdict = el[e] ? peer_verdict(x[e], X2, D4, n_elig, a.r_h, a.r_l, a.z, min_value, a.min_delta, a.min_peers) : PO_N;
    r.E = el[e] ? n_elig : 0;
    r.pad = 0;
    r.x = x[e];
    r.X2 = el[e] ? X2 : 0;
    r.D4 = el[e] ? D4 : 0;
    a.rec[ser[e]] = r;
  }
}

// the staged member j of a deferred group (m == 0: not eligible)
__device__ __forceinline__ const PeerRec* big_member(const PeerArgs& a, int m0, int j) {
  const int s = a.grp_mem[m0 + j];
  return a.rec + s;
}

// the keys of ranks lo and hi among the staged eligible members into sel[0], sel[1].  DEV: the key
// is |2 x - X2|, else x.
template <bool DEV>
__device__ __forceinline__ void big_select(const PeerArgs& a, int m0, int nmem, long long X2, int lo, int hi,
                                           long long* sel) {
  for (int k = threadIdx.x; k < nmem; k += PO_BLOCK) {
    const PeerRec* me = big_member(a, m0, k);
    if (me->m == 0) continue;
    const long long xk = DEV ? po_dev(me->x, X2) : me->x;
    int rank = 0;
    for (int j = 0; j < nmem; ++j) {
      const PeerRec* o = big_member(a, m0, j);
      const long long y = DEV ? po_dev(o->x, X2) : o->x;
      rank += o->m != 0 && (y < xk || (y == xk && j < k)) ? 1 : 0;
    }
    if (rank == lo) sel[0] = xk;
    if (rank == hi) sel[1] = xk;
  }
}

__global__ __launch_bounds__(PO_BLOCK) void k_peer_big(PeerArgs a) {
  __shared__ int sh_cnt, sh_first;
  __shared__ long long sel[4];
  const int nb = min(*a.big_n, a.n_groups);
  for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const int g = a.big_list[bi];
    const int m0 = a.grp_off[g];
    const int nmem = a.grp_off[g + 1] - m0;
    if (threadIdx.x == 0) { sh_cnt = 0; sh_first = 0x7fffffff; sel[0] = sel[1] = sel[2] = sel[3] = 0; }
    __syncthreads();
    // stage: every member's record holds (m, x) of an eligible member, zeros otherwise
    int cnt = 0, first = 0x7fffffff;
    for (int k = threadIdx.x; k < nmem; k += PO_BLOCK) {
      const int s = a.grp_mem[m0 + k];
      if (s < 0 || s >= a.n_series) continue;
      PeerRec r;
      r.m = 0; r.verdict = PO_N; r.E = 0; r.pad = 0; r.x = 0; r.X2 = 0; r.D4 = 0;
      if (a.active[s] && peer_class(a.cls, a.n_classes, s) > 0 && a.m[s] >= a.min_samples) {
        r.m = a.m[s];
        r.x = a.sum2[s];
        ++cnt;
        first = min(first, k);
      }
      a.rec[s] = r;
    }
    if (cnt) { atomicAdd(&sh_cnt, cnt); atomicMin(&sh_first, first); }
    __syncthreads();  // (the staged records are visible to the block)
    const int n_elig = sh_cnt;
    if (n_elig > 0) {  // (uniform)
      const int lo = (n_elig - 1) >> 1, hi = n_elig >> 1;
      big_select<false>(a, m0, nmem, 0, lo, hi, sel);
      __syncthreads();
      const long long X2 = sel[0] + sel[1];
      big_select<true>(a, m0, nmem, X2, lo, hi, sel + 2);
      __syncthreads();
      const long long D4 = sel[2] + sel[3];
      const int32_t min_value = a.val[peer_class(a.cls, a.n_classes, a.grp_mem[m0 + sh_first])];
      for (int k = threadIdx.x; k < nmem; k += PO_BLOCK) {
        const int s = a.grp_mem[m0 + k];
        if (s < 0 || s >= a.n_series) continue;
        PeerRec* r = a.rec + s;
        if (r->m == 0) continue;
        r->verdict = peer_verdict(r->x, X2, D4, n_elig, a.r_h, a.r_l, a.z, min_value, a.min_delta, a.min_peers);
        r->E = n_elig;
        r->X2 = X2;
        r->D4 = D4;
      }
    }
    __syncthreads();  // (the next group resets the shared cells)
  }
}

// A signed value of magnitude below 2^37 in decimal: at most two 32-bit pieces by one 64-bit
// constant division, in registers (OutT::u's general path fills a local buffer, which is scratch
// memory; docs/SERVICEWINDOW.md)
template <bool W>
__device__ __forceinline__ void po_i64(OutT<W>& o, long long v) {
  const unsigned long long mag = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
  if (v < 0) o.c('-');
  if (mag <= 0xffffffffull) { o.u32((uint32_t)mag); return; }
  const unsigned long long q = mag / 100000000ull;  // < 1375
  o.u32((uint32_t)q);
  o.u32_fixed8((uint32_t)(mag - q * 100000000ull));
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t po_row(const PeerTextArgs& a, int32_t s, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const PeerRec& r = a.rec[s];
  o.lit("po|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  o.u32((uint32_t)r.m); o.c('|');
  o.sb(a.ptxt, a.plen);
  po_i64(o, r.x); o.c('|');
  o.u32((uint32_t)r.E); o.c('|');
  po_i64(o, r.X2); o.c('|');
  po_i64(o, r.D4); o.c('|');
  o.c(r.verdict == PO_H ? 'H' : 'L');
  o.c('\n');
  o.finish();
  return o.n;
}

// series of emission position i that prints a row (-1: none): it has a verdict (the value pass
// wrote a zero record for every inactive, class-0 or ineligible series)
__device__ __forceinline__ int32_t po_row_series(const PeerTextArgs& a, int32_t i) {
  const int32_t s = a.perm[i];
  if (s < 0 || s >= a.n_series) return -1;
  const int v = a.rec[s].verdict;
  return v == PO_H || v == PO_L ? s : -1;
}

// the length pass' row policy (k_text_len)
struct PoRow {
  static __device__ __forceinline__ uint32_t len(const PeerTextArgs& a, int32_t i) {
    const int32_t s = po_row_series(a, i);
    return s >= 0 ? po_row<false>(a, s, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(PO_TEXT_BLOCK) void k_peer_write(PeerTextArgs a) {
  const int32_t i = (int32_t)(blockIdx.x * PO_TEXT_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  const int32_t s = po_row_series(a, i);
  if (s >= 0) po_row<true>(a, s, a.out + a.off[i]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

int32_t apm_peer_group_max() { return PO_GROUP_MAX; }

size_t apm_peer_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max); }

// "po|" + ts (<= 23) + names + 2 separators + m| (11) + label (<= 7) + x| (a sign, 10 digits) + E|
// (11) + X2| (a sign, 11 digits) + D4| (11 digits) + the verdict + newline
size_t apm_peer_row_bound(size_t name_bytes) { return 3 + 23 + name_bytes + 2 + 11 + 7 + 12 + 11 + 13 + 12 + 2; }

void apm_peer_values(PeerArgs* a, hipStream_t stream) {
  const int32_t n = a->n_groups;
  if (n <= 0) return;
  HIP_OK(hipMemsetAsync(a->big_n, 0, 4, stream));
  const int per_block = PO_WAVES * 2;
  hipLaunchKernelGGL(k_peer_group, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(PO_WAVES * APM_WAVE), 0, stream,
                     *a);
  hipLaunchKernelGGL(k_peer_big, dim3(PO_BIG_GRID), dim3(PO_BLOCK), 0, stream, *a);
}

int apm_peer_plan(PeerTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<PoRow, PO_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_peer_write(PeerTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  hipLaunchKernelGGL(k_peer_write, dim3((uint32_t)((a->n + PO_TEXT_BLOCK - 1) / PO_TEXT_BLOCK)), dim3(PO_TEXT_BLOCK), 0,
                     stream, *a);
}

}  // extern "C"
