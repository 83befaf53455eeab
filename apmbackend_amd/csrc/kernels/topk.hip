// K18: tk rows -- per-rollover top-K series leaderboards (docs/LEADERBOARD.md).
//
// A selection across series over K8's result (WinStat[S]) at a rollover: for each board (a key out
// of tpm / average / per75 / per95) the k candidates with the largest key value, ordered by value
// descending (compared as doubles, -0.0 == +0.0), ties by emission position ascending.  A candidate
// is a series with an st row (WinStat.active), a key value that is not NaN and tpm >= min_tpm.
//
// The order is carried by bit patterns: a double maps to a uint64 whose unsigned order is the
// doubles' order (-0.0 canonicalised to +0.0 first).  No candidate maps to 0 (0 would be a NaN
// with the sign bit set), so 0 marks "no candidate" and sorts below every candidate.
//
//   k_topk_tile   one 256-thread block per tile of TK_TILE emission positions, 8 consecutive
//                 positions per thread.  Each position's WinStat is read once through perm and
//                 turned into one key per board (registers).  Per board: a block-wide radix select
//                 of the min(k, candidates)-th largest key, 8 digits of 8 bits over LDS histograms
//                 (all boards share a pass: three barriers per digit), then an ordered compaction
//                 -- a block scan of (greater, equal) counts -- that keeps everything above the
//                 pivot and the pivot-equal entries in position order until k is reached.  The
//                 survivors (position, key) go to scratch [board][tile][k]; unused slots get key 0.
//   k_topk_final  one block per board over the tiles' survivors, read from scratch in sweeps of 256
//                 (one per thread; it loops when tiles * k is larger).  It selects on the 96-bit
//                 composite (key, ~position), whose values are distinct: 12 digits, no tie rule,
//                 exactly min(k, candidates) entries at or above the pivot.  Those <= 128 entries
//                 are ranked in LDS (each counts the entries above it) and entry of rank r stores
//                 record r {series, position, WinStat} and the count straight into host-mapped
//                 pinned memory.
// Plain C++, vector stores only.  No device state outlives the two launches.
#include "kernel_api.h"

namespace apm {

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_IPT = 8;                        // positions per thread
constexpr int TK_TILE = TK_THREADS * TK_IPT;     // positions per block of k_topk_tile
constexpr int TK_WAVES = TK_THREADS / 64;

template <int NB>
struct SelShared {
  int hist[NB][256];
  int wtot[NB][TK_WAVES];
  int digit[NB];
  int krem[NB];
  int cnt[NB];
};

// the unsigned order of the result is the order of the doubles (v is not NaN)
__device__ __forceinline__ uint64_t order_key(double v) {
  if (v == 0.0) v = 0.0;  // -0.0 -> +0.0
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double key_value(const WinStat& w, int32_t by) {
  return by == TK_TPM ? w.tpm : by == TK_AVG ? w.avg : by == TK_P75 ? w.p75 : w.p95;
}

// One digit of the select for every board with krem[b] >= 1: sh.hist[b] holds, per digit value,
// the number of entries that match the prefix so far.  Afterwards digit[b] is the digit of the
// krem[b]-th largest of them and krem[b] its rank among the entries with that digit; the
// histograms are zero again.  Called by all threads; nb and krem are uniform.
template <int NB>
__device__ __forceinline__ void pick_digits(SelShared<NB>& sh, int nb, int (&krem)[NB], int (&digit)[NB]) {
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  int c[NB], incl[NB];
  __syncthreads();  // the histograms are complete
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    c[b] = 0;
    incl[b] = 0;
    if (b < nb && krem[b] > 0) {
      c[b] = sh.hist[b][t];
      sh.hist[b][t] = 0;
      int v = c[b];  // entries with a digit >= this one, inside the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d, 64);
        if (lane + d < 64) v += o;
      }
      incl[b] = v;
      if (lane == 0) sh.wtot[b][w] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b < nb && krem[b] > 0) {
      int in = incl[b];
#pragma unroll
      for (int ww = 1; ww < TK_WAVES; ++ww)
        if (ww > w) in += sh.wtot[b][ww];
      const int ex = in - c[b];
      if (ex < krem[b] && krem[b] <= in) {  // exactly one digit
        sh.digit[b] = t;
        sh.krem[b] = krem[b] - ex;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    digit[b] = 0;
    if (b < nb && krem[b] > 0) {
      digit[b] = sh.digit[b];
      krem[b] = sh.krem[b];
    }
  }
}

__global__ __launch_bounds__(TK_THREADS) void k_topk_tile(TopKArgs a) {
  constexpr int NB = TK_MAX_BOARDS;
  __shared__ SelShared<NB> sh;
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const int nb = a.nb;
  const int32_t base = (int32_t)blockIdx.x * TK_TILE + t * TK_IPT;
#pragma unroll
  for (int b = 0; b < NB; ++b) sh.hist[b][t] = 0;
  if (t < NB) sh.cnt[t] = 0;
  __syncthreads();

  // ---- each position's WinStat once, one key per board
  uint64_t key[NB][TK_IPT];
  int lc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) lc[b] = 0;
  int32_t ser[TK_IPT];
  if (base + TK_IPT <= a.n) {  // (perm is 16-byte aligned and base a multiple of 8)
    const int4 p0 = reinterpret_cast<const int4*>(a.perm + base)[0];
    const int4 p1 = reinterpret_cast<const int4*>(a.perm + base)[1];
    ser[0] = p0.x; ser[1] = p0.y; ser[2] = p0.z; ser[3] = p0.w;
    ser[4] = p1.x; ser[5] = p1.y; ser[6] = p1.z; ser[7] = p1.w;
  } else {
#pragma unroll
    for (int j = 0; j < TK_IPT; ++j) ser[j] = base + j < a.n ? a.perm[base + j] : -1;
  }
#pragma unroll
  for (int j = 0; j < TK_IPT; ++j) {
#pragma unroll
    for (int b = 0; b < NB; ++b) key[b][j] = 0;
    const int32_t s = ser[j];
    if ((uint32_t)s < (uint32_t)a.n_series) {
      const WinStat ws = a.win[s];
      const bool ok = ws.active != 0 && ws.tpm >= a.min_tpm;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < nb) {
          const double v = key_value(ws, a.by[b]);
          if (ok && v == v) {
            key[b][j] = order_key(v);
            ++lc[b];
          }
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
    if (b < nb && lc[b]) atomicAdd(&sh.cnt[b], lc[b]);
  __syncthreads();

  // ---- the min(k, candidates)-th largest key per board
  int kk[NB], krem[NB], digit[NB];
  uint64_t pivot[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    kk[b] = b < nb ? min(a.k, sh.cnt[b]) : 0;
    krem[b] = kk[b];
    pivot[b] = 0;
  }
  for (int s = 56; s >= 0; s -= 8) {
    const uint64_t mask = s == 56 ? 0ull : ~0ull << (s + 8);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < nb && krem[b] > 0) {
#pragma unroll
        for (int j = 0; j < TK_IPT; ++j)
          if ((key[b][j] & mask) == pivot[b]) atomicAdd(&sh.hist[b][(int)((key[b][j] >> s) & 255u)], 1);
      }
    }
    pick_digits<NB>(sh, nb, krem, digit);
#pragma unroll
    for (int b = 0; b < NB; ++b) pivot[b] |= (uint64_t)digit[b] << s;
  }
  // krem[b]: how many pivot-equal entries belong to the tile's best kk[b]

  // ---- ordered compaction: block scan of the packed (greater | equal << 16) counts
  uint32_t pk[NB], incl[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    pk[b] = 0;
    incl[b] = 0;
    if (b < nb && kk[b] > 0) {
      uint32_t g = 0, e = 0;
#pragma unroll
      for (int j = 0; j < TK_IPT; ++j) {
        g += key[b][j] > pivot[b];
        e += key[b][j] == pivot[b];
      }
      pk[b] = g | (e << 16);  // (both at most 2048)
      uint32_t v = pk[b];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
      }
      incl[b] = v;
      if (lane == 63) sh.wtot[b][w] = (int)v;
    }
  }
  __syncthreads();
  const int32_t tile = (int32_t)blockIdx.x;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b < nb) {
      const size_t row = ((size_t)b * a.tiles + tile) * (size_t)a.k;
      if (kk[b] > 0) {
        uint32_t ex = incl[b] - pk[b];
#pragma unroll
        for (int ww = 0; ww < TK_WAVES - 1; ++ww)
          if (ww < w) ex += (uint32_t)sh.wtot[b][ww];
        int32_t g = (int32_t)(ex & 0xffffu), e = (int32_t)(ex >> 16);
        const int32_t above = kk[b] - krem[b];
#pragma unroll
        for (int j = 0; j < TK_IPT; ++j) {
          int32_t slot = -1;
          if (key[b][j] > pivot[b]) slot = g++;
          else if (key[b][j] == pivot[b]) {
            if (e < krem[b]) slot = above + e;
            ++e;
          }
          if (slot >= 0 && slot < a.k) {
            a.sc_key[row + slot] = key[b][j];
            a.sc_pos[row + slot] = base + j;
          }
        }
      }
      if (t >= kk[b] && t < a.k) {  // unused slots: no candidate
        a.sc_key[row + t] = 0;
        a.sc_pos[row + t] = 0;
      }
    }
  }
}

__global__ __launch_bounds__(TK_THREADS) void k_topk_final(TopKArgs a) {
  __shared__ SelShared<1> sh;
  __shared__ uint64_t s_key[TK_MAX_K];
  __shared__ uint32_t s_np[TK_MAX_K];
  __shared__ int s_n;
  const int t = (int)threadIdx.x;
  const int b = (int)blockIdx.x;
  const int32_t M = a.tiles * a.k;  // slots of this board (at most n_max / TK_TILE * 128)
  const uint64_t* keys = a.sc_key + (size_t)b * M;
  const int32_t* pos = a.sc_pos + (size_t)b * M;
  sh.hist[0][t] = 0;
  if (t == 0) { sh.cnt[0] = 0; s_n = 0; }
  if (t < TK_MAX_K) { s_key[t] = 0; s_np[t] = 0; }
  __syncthreads();
  int lc = 0;
  for (int32_t i = t; i < M; i += TK_THREADS) lc += keys[i] != 0;
  if (lc) atomicAdd(&sh.cnt[0], lc);
  __syncthreads();
  const int kk = min(a.k, sh.cnt[0]);
  if (kk == 0) {  // (uniform)
    if (t == 0) a.out_n[b] = 0;
    return;
  }
  // ---- the kk-th largest composite (key, ~position): 8 digits of the key, 4 of ~position
  int krem[1] = {kk}, digit[1];
  uint64_t pkey = 0;
  for (int s = 56; s >= 0; s -= 8) {
    const uint64_t mask = s == 56 ? 0ull : ~0ull << (s + 8);
    for (int32_t i = t; i < M; i += TK_THREADS) {
      const uint64_t k = keys[i];
      if ((k & mask) == pkey) atomicAdd(&sh.hist[0][(int)((k >> s) & 255u)], 1);
    }
    pick_digits<1>(sh, 1, krem, digit);
    pkey |= (uint64_t)digit[0] << s;
  }
  uint32_t pnp = 0;
  for (int s = 24; s >= 0; s -= 8) {
    const uint32_t mask = s == 24 ? 0u : ~0u << (s + 8);
    for (int32_t i = t; i < M; i += TK_THREADS) {
      const uint32_t np = ~(uint32_t)pos[i];
      if (keys[i] == pkey && (np & mask) == pnp) atomicAdd(&sh.hist[0][(int)((np >> s) & 255u)], 1);
    }
    pick_digits<1>(sh, 1, krem, digit);
    pnp |= (uint32_t)digit[0] << s;
  }
  // ---- the entries at or above the pivot (exactly kk: composites are distinct), then their ranks
  for (int32_t i = t; i < M; i += TK_THREADS) {
    const uint64_t k = keys[i];
    const uint32_t np = ~(uint32_t)pos[i];
    if (k > pkey || (k == pkey && np >= pnp)) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < TK_MAX_K) { s_key[slot] = k; s_np[slot] = np; }
    }
  }
  __syncthreads();
  if (t < kk) {
    const uint64_t mk = s_key[t];
    const uint32_t mn = s_np[t];
    int r = 0;
    for (int j = 0; j < kk; ++j) r += s_key[j] > mk || (s_key[j] == mk && s_np[j] > mn);
    const int32_t p = (int32_t)~mn;
    const int32_t s = a.perm[p];
    TopKRec rec;
    rec.series = s;
    rec.pos = p;
    rec.w = a.win[s];
    a.out[(size_t)b * a.k + r] = rec;
  }
  if (t == 0) a.out_n[b] = kk;
}

}  // namespace

}  // namespace apm

using namespace apm;

int32_t apm_topk_tile() { return TK_TILE; }
int32_t apm_topk_final_span() { return TK_THREADS; }

static size_t topk_slots(int32_t n_max, int32_t k, int32_t nb) {
  const size_t tiles = ((size_t)std::max(n_max, 0) + TK_TILE - 1) / TK_TILE;
  return tiles * (size_t)k * (size_t)nb;
}

size_t apm_topk_scratch_bytes(int32_t n_max, int32_t k, int32_t nb) {
  return topk_slots(n_max, k, nb) * 12 + 256;
}

void apm_topk(TopKArgs* a, void* scratch, hipStream_t stream) {
  if (a->nb < 1 || a->nb > TK_MAX_BOARDS || a->k < 1 || a->k > TK_MAX_K || a->n < 0)
    throw std::invalid_argument("apm_topk: 1..4 boards, k in 1..128");
  for (int b = 0; b < a->nb; ++b)
    if (a->by[b] < 0 || a->by[b] > TK_P95) throw std::invalid_argument("apm_topk: unknown key");
  a->tiles = (a->n + TK_TILE - 1) / TK_TILE;
  // keys first (8-byte aligned), then the positions
  a->sc_key = (uint64_t*)scratch;
  a->sc_pos = (int32_t*)(a->sc_key + topk_slots(a->n, a->k, a->nb));
  if (a->tiles > 0) hipLaunchKernelGGL(k_topk_tile, dim3((uint32_t)a->tiles), dim3(TK_THREADS), 0, stream, *a);
  hipLaunchKernelGGL(k_topk_final, dim3((uint32_t)a->nb), dim3(TK_THREADS), 0, stream, *a);
}
