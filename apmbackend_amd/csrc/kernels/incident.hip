// K25: ic rows -- incidents opened and closed on the device (docs/INCIDENTS.md).
//
// The sb, tf, po and ls streams are level-triggered: a breaching series prints a row at every
// rollover.  This pass keeps, per (series, source), the 16-byte state of incidentcmp.h across
// rollovers and prints a row only when something changes: an incident opened (O), is still open at
// a reminder step (S), or closed (C).
// Step pass (k_incident_step): one lane per series id below n_series.  A source is a strided view
// of its records' verdict words; a series without an st row at this rollover (active[s] == 0) is
// clear for every source and its records are not read.  Per configured source the lane decodes hot
// and code (incident_code), steps the state (incident_step), and keeps the event byte and the two
// letters the row prints; the four event bytes and the eight letters of a series leave as one dword
// and one pair of dwords.  The open incidents per source are counted with a ballot per wave and one
// atomic per wave and source.  Only integers; no LDS; plain C++ with vector stores.
// Text pass: K12's count / scan / write shape over n * 4 positions (emission position x source); a
// position whose event byte is 0 has length 0, which is the compaction.  Rows are rare, so the
// write pass stores each row directly through textout.h (no LDS stage).  The length kernel and the
// scan are textpass.h's.
#include "kernel_api.h"  // (common.h pulls <cstring> in before rocprim)
#include "devjoin_dev.h"
#include "textpass.h"

#include "incidentcmp.h"

namespace apm {

namespace {

constexpr int IC_BLOCK = 256;
constexpr int IC_TEXT_BLOCK = 256;

static_assert(IC_MAX_SOURCES == IC_SOURCES, "four sources");

__global__ __launch_bounds__(IC_BLOCK) void k_incident_step(IncidentArgs a) {
  const int32_t s = (int32_t)(blockIdx.x * IC_BLOCK + threadIdx.x);
  const bool in = s < a.n_series;  // (a lane past n_series only takes part in the ballots)
  const bool act = in && a.active[s] != 0;
  uint32_t ev4 = 0, c0 = 0, c1 = 0;  // ev[s][0..3]; codes[s][0..1][2], codes[s][2..3][2]
#pragma unroll
  for (int k = 0; k < IC_MAX_SOURCES; ++k) {
    if (a.src[k].word == nullptr) continue;  // (uniform: a kernel argument)
    bool open = false;
    if (in) {
      // bounds: s < n_series <= the records' and the state's capacity S
      const int32_t w = act ? *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(a.src[k].word) +
                                                                 (size_t)s * (size_t)a.src[k].stride_bytes)
                            : 0;
      const uint8_t code = incident_code(a.src[k].kind, w);
      IncidentState st = a.state[(size_t)s * IC_MAX_SOURCES + k];
      const IncidentOut o = incident_step(st, code != 0, code, a.edge_ts, (uint32_t)a.open_after[k],
                                          (uint32_t)a.close_after[k], (uint32_t)a.remind_every);
      a.state[(size_t)s * IC_MAX_SOURCES + k] = st;
      open = st.code0 != 0;
      ev4 |= (uint32_t)o.event << (8 * k);
      const uint32_t pair = (uint32_t)(o.code0 ? o.code0 : (uint8_t)'-') | (uint32_t)(code ? code : (uint8_t)'-') << 8;
      if (k < 2) c0 |= pair << (16 * k);
      else c1 |= pair << (16 * (k - 2));
    }
    const unsigned long long m = __ballot(open ? 1 : 0);
    if ((threadIdx.x & (APM_WAVE - 1)) == 0 && m != 0) atomicAdd(&a.open_n[k], (int32_t)__popcll(m));
  }
  if (in) {
    reinterpret_cast<uint32_t*>(a.ev)[s] = ev4;
    reinterpret_cast<uint2*>(a.codes)[s] = make_uint2(c0, c1);
  }
}

// a signed 64-bit decimal in registers: at most three 32-bit parts split by 10^8 (OutT::u's path
// above 10^8 * 2^32 fills a local buffer, which is scratch memory)
template <bool W>
__device__ __forceinline__ void ic_i64(OutT<W>& o, long long x) {
  unsigned long long v = (unsigned long long)x;
  if (x < 0) { o.c('-'); v = 0ull - v; }
  if (v <= 0xffffffffull) { o.u32((uint32_t)v); return; }
  const unsigned long long q = v / 100000000ull;
  const uint32_t r = (uint32_t)(v - q * 100000000ull);
  if (q <= 0xffffffffull) {
    o.u32((uint32_t)q);
  } else {
    const unsigned long long q2 = q / 100000000ull;  // (at most 1844)
    o.u32((uint32_t)q2);
    o.u32_fixed8((uint32_t)(q - q2 * 100000000ull));
  }
  o.u32_fixed8(r);
}

// one row: W = false counts its bytes
template <bool W>
__device__ __forceinline__ uint32_t ic_row(const IncidentTextArgs& a, int32_t s, int k, uint8_t ev, char* dst) {
  OutT<W> o(dst);
  const int4 nm = a.series_names[s];
  const IncidentState st = a.state[(size_t)s * IC_MAX_SOURCES + k];
  const uint8_t code0 = a.codes[((size_t)s * IC_MAX_SOURCES + k) * 2];
  const uint8_t code = a.codes[((size_t)s * IC_MAX_SOURCES + k) * 2 + 1];
  o.lit("ic|");
  o.sb(a.ts, a.ts_len);
  o.s(a.names + nm.x, nm.y); o.c('|');
  o.s(a.names + nm.z, nm.w); o.c('|');
  if (k == IC_SB) o.lit("sb|");
  else if (k == IC_TF) o.lit("tf|");
  else if (k == IC_PO) o.lit("po|");
  else o.lit("ls|");
  o.c((char)ev); o.c('|');
  o.c((char)code0); o.c('|');
  o.c((char)code); o.c('|');
  ic_i64(o, st.since_ts); o.c('|');
  o.u32(st.age); o.c('|');
  // a hot step leaves clear_run 0 and a clear one hot_run 0: the run of this rollover's side
  o.u32((uint32_t)(st.hot_run ? st.hot_run : st.clear_run));
  o.c('\n');
  o.finish();
  return o.n;
}

// series of text position p that prints a row (-1: none), its source and its event
__device__ __forceinline__ int32_t ic_row_series(const IncidentTextArgs& a, int32_t p, int& k, uint8_t& ev) {
  const int32_t s = a.perm[p / IC_MAX_SOURCES];
  k = p % IC_MAX_SOURCES;
  if (s < 0 || s >= a.n_series) return -1;
  ev = a.ev[(size_t)s * IC_MAX_SOURCES + k];
  return ev != 0 ? s : -1;
}

// the length pass' row policy (k_text_len)
struct IcRow {
  static __device__ __forceinline__ uint32_t len(const IncidentTextArgs& a, int32_t p) {
    int k = 0;
    uint8_t ev = 0;
    const int32_t s = ic_row_series(a, p, k, ev);
    return s >= 0 ? ic_row<false>(a, s, k, ev, nullptr) : 0u;
  }
};

__global__ __launch_bounds__(IC_TEXT_BLOCK) void k_incident_write(IncidentTextArgs a) {
  const int32_t p = (int32_t)(blockIdx.x * IC_TEXT_BLOCK + threadIdx.x);
  if (p >= a.n) return;
  int k = 0;
  uint8_t ev = 0;
  const int32_t s = ic_row_series(a, p, k, ev);
  if (s >= 0) ic_row<true>(a, s, k, ev, a.out + a.off[p]);
}

}  // namespace

}  // namespace apm

extern "C" {
using namespace apm;

size_t apm_incident_tmp_bytes(int32_t n_max) { return text_scan_tmp_bytes(n_max * IC_MAX_SOURCES); }

// "ic|" + ts (<= 23) + names + 2 separators + "sb|" + "O|" + "B|" + "B|" + since (<= 20 and a sign)
// + '|' + age (<= 10) + '|' + run (<= 3) + newline
size_t apm_incident_row_bound(size_t name_bytes) { return 3 + 23 + name_bytes + 2 + 3 + 2 + 2 + 2 + 22 + 11 + 3 + 1; }

void apm_incident_step(IncidentArgs* a, hipStream_t stream) {
  if (a->n_series <= 0) return;
  hipLaunchKernelGGL(k_incident_step, dim3((uint32_t)((a->n_series + IC_BLOCK - 1) / IC_BLOCK)), dim3(IC_BLOCK), 0, stream,
                     *a);
}

int apm_incident_plan(IncidentTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  return text_plan<IcRow, IC_TEXT_BLOCK>(a, tmp, tmp_bytes, stream);
}

void apm_incident_write(IncidentTextArgs* a, hipStream_t stream) {
  if (a->n <= 0) return;
  hipLaunchKernelGGL(k_incident_write, dim3((uint32_t)((a->n + IC_TEXT_BLOCK - 1) / IC_TEXT_BLOCK)), dim3(IC_TEXT_BLOCK), 0,
                     stream, *a);
}

}  // extern "C"
