// Launch-side API of the CDNA4 kernels: argument structs + host entry points.
// Included by the .hip translation units and by the host runtime (engine.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../apm_types.h"
#include "common.h"

namespace apm {

struct StatsState {
  int32_t* counts;        // [nslot][S]
  int32_t* cells;         // [nslot][S][cap]
  int32_t* spill_n;       // [nslot]
  int32_t* spill_series;  // [nslot][spill_cap]  (sorted by series, stably, before every K8)
  int32_t* spill_val;     // [nslot][spill_cap]
  uint8_t* active;        // [S]
  int32_t cap;
  int32_t spill_cap;
  int32_t S;
  int32_t nslot = NSLOT_MIN;  // bucket ring slots (bucket b lives in slot b % nslot)
  unsigned long long* spill_drop = nullptr;  // [0] samples lost to a full spill list, [1] NaN windows clipped
  // NaN elapsed samples (stream_calc_stats.js:131 pushes parseInt -> NaN): once a series holds one,
  // the JS binaryInsert order of every later sample in its windows matters, so the series' samples
  // are appended in arrival order (not atomic order) while a NaN is live in its window.
  int32_t* nan_until = nullptr;  // [S] last bucket whose window can still see a NaN sample (INT32_MIN = none)
  int32_t* ord_list = nullptr;   // [max_tx] tx indices deferred to the ordered append
  int32_t* ord_n = nullptr;
  uint32_t* ord_done = nullptr;  // blocks of the ordered append finished (the last one resets ord_n)
  int32_t keep = 0;              // windowSz + intervalBufferSz
  // host-mapped pinned [nslot]: spill_n after each append (the host's exact fill level, read once
  // the append's event completed; it sizes the spill area so no sample is ever dropped)
  int32_t* spill_snap = nullptr;
};

struct WindowArgs {
  StatsState st;
  int32_t win_slots[K8_INLINE_SLOTS];  // slot index per window bucket (-1 = bucket absent), n_win <= 64
  const int32_t* win_slots_ext;        // device [n_win] when n_win > K8_INLINE_SLOTS (else null)
  int32_t n_win;          // window buckets: windowSizeInIntervals + 1 (31 in the shipped config)
  double tpm_div;         // windowSz * intervalLen / 60
  WinStat* out;           // [S]
  int32_t* big_list;      // series deferred to the block pass
  int32_t* big_n;
  int32_t* nan_list;      // series whose window holds a NaN sample (JS insertion emulation)
  int32_t* nan_n;
  int32_t* js_scratch;    // [JS_BLOCKS][js_cap] ordered window samples of a NaN series
  int32_t js_cap;
  int32_t n_series;       // ids < n_series may be active
};
constexpr int JS_BLOCKS = 8;

struct ZArgs {
  void* ring;              // [NSTAT][LAG][S] of T for this lag
  int32_t* len;            // [S]
  double* sum;             // [NSTAT][S]
  double* comp;            // [NSTAT][S]
  int32_t* cnt;            // [NSTAT][S]
  double* sumsq;           // [NSTAT][S]
  double* sqcomp;          // [NSTAT][S]
  const double* thr;       // [S]
  const double* infl;      // [S]
  const WinStat* win;      // [S]
  ZOut* out;               // [S]
  int32_t S;
  int32_t n_series;
  int32_t lag;
  int32_t head;            // write position this rollover
  int32_t exact;           // 1 = sequential mean every time
  int32_t sigma_stddev;    // 0 = sqrt(mean) quirk, 1 = population sigma
  int32_t resync_k;        // rolling mode: exact resync period (0 = never)
  int64_t rollover_idx;
  // rolling-mode resync range of this rollover (host computes it; rs_n = 0 -> none)
  int32_t rs_lo, rs_n, rs_parts;
  int32_t rs_mfma;         // 1: window re-sum as MFMA tile reductions (k_zscore_resync_mfma)
  double* rs_part;         // [NSTAT][rs_parts][rs_n][4] partial (sum, comp, sumsq, sqcomp)
  int32_t* rs_cnt;         // [NSTAT][rs_parts][rs_n]
};

// K14 per-JVM rollup fused with exogenous gauges (context.hip)
constexpr int ROLLUP_ACC = 6;    // live series, window tx, window elapsed sum, max p95 bits, #avg sig, #p75 sig
constexpr int ROLLUP_OUT = 15;   // see k_server_fuse
constexpr int CTX_FIELDS = 18;   // [0] gauge ts (ms), [1..16] JmxEntry gauges, [17] VM load
struct RollupArgs {
  const WinStat* win;
  const int32_t* series_server;
  const ZOut* z[MAX_LAGS];
  int32_t n_lags;
  int32_t n_series;
  int32_t n_servers;
  int64_t edge_ts;
  double tpm_div;
  const double* ctx;              // [n_servers][CTX_FIELDS]
  unsigned long long* acc;        // [n_servers][ROLLUP_ACC]
  double* out;                    // [n_servers][ROLLUP_OUT]
};

// apm_copy_segs: up to 8 device -> device / host-mapped copies in one launch (stats.hip); a
// segment without a source is a zero fill of its destination
struct CopySeg {
  void* dst;
  const void* src;
  size_t bytes;
};
struct CopySegs {
  CopySeg seg[8];
  int32_t n = 0;
  void add(void* d, const void* s, size_t b) {
    if (b) seg[n++] = CopySeg{d, s, b};
  }
  void zero(void* d, size_t b) {
    if (b) seg[n++] = CopySeg{d, nullptr, b};
  }
};

// apm_export: device scalars -> pinned host memory (stats.hip)
struct ExportArgs {
  static constexpr int kMax = 8;
  void* src[kMax];  // device scalars
  void* dst[kMax];  // device views of pinned host memory
  uint64_t reset_val[kMax];
  uint8_t bytes[kMax];  // 4 or 8
  uint8_t reset[kMax];
  int32_t n;
  void add(void* s, void* d, int nb, bool rst = false, uint64_t rv = 0) {
    src[n] = s; dst[n] = d; bytes[n] = (uint8_t)nb; reset[n] = rst ? 1 : 0; reset_val[n] = rv; ++n;
  }
};

// K12 st/fs encoding (format.hip)
struct FormatArgs {
  const int32_t* perm;          // [n] series in emission order
  const WinStat* win;           // [S]
  const ZOut* z[MAX_LAGS];      // [S] per lag
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int64_t edge_ts;
  int32_t n;
  int32_t n_lags;
  int32_t lag_order[MAX_LAGS];  // ascending LAG value
  int32_t lag_value[MAX_LAGS];
  int32_t want_st, want_fs;
  // fs as Postgres COPY rows (the DB sink's K13 encoding fused into K12): the fs stream then
  // carries `timestamp \t server \t service \t tpm \t lag \t stats-json` rows (copyenc.cpp)
  int32_t fs_copy;
  uint32_t stage_hint;  // bytes of an average 64-line block of the longer stream (previous batch); 0 = unknown
  int32_t ts_copy_len;
  char ts_copy[32];        // edge_ts as 'YYYY-MM-DD HH:MM:SS.mmm+00'
  int32_t ts_wire_len;
  char ts_wire[24];        // "<edge_ts>|" as the wire lines' second field (printed once, on the host)
  uint32_t *st_len, *fs_len, *st_off, *fs_off;  // st [n + 1], fs per (series, LAG) line [n * n_lags + 1]
  char *st_out, *fs_out;
  int32_t* fallback;
};

// fb rows: the fleet-merged per-service baseline (all ranks' series of a service), one row per
// (service slot, LAG) with a baseline, after the moments all-reduce (format.hip).  Every rank
// formats the rows of its own slice of the slots [slot_lo, slot_lo + n_slots).
struct FleetFormatArgs {
  const double* moments;   // [cap][n_lags][NSTAT][3] {n, sum of means, sum of squared means}
  const int2* names;       // [all slots] {offset, length} into chars
  const char* chars;
  int32_t slot_lo, n_slots, n_lags;
  int32_t lag_order[MAX_LAGS], lag_value[MAX_LAGS];
  int64_t edge_ts;
  int32_t copy;            // 1: Postgres COPY rows (apm_fleet_stats), 0: fb wire lines
  int32_t ts_len;
  char ts[32];
  unsigned long long* status;  // [blocks] each 64-row wave's byte total (k_fleet_len)
  uint32_t* total;         // bytes written (device)
  char* out;
  int32_t* fallback;
};
// K15 lh rows: one bucket's samples per series as a sparse histogram (hist.hip).  One row per
// emission position whose series holds a sample in ring slot `slot`:
//   lh|<bucket start ms>|server|service|<count>|<nan>|<lo>:<c>,<lo>:<c>,...
struct HistArgs {
  StatsState st;                // spill lists sorted (apm_spill_sort) before the call
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t slot;                 // ring slot of the reported bucket
  int32_t ts_len;
  char ts[24];                  // "<bucket * 10000>|"
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  int32_t* big_list;            // [n] emission positions deferred to the block pass
  int32_t* big_n;
  char* out;                    // at least apm_hist_row_bound(max name bytes) * n bytes
};
// K16 wp rows: exact window percentiles (winpct.hip, docs/PERCENTILES.md).  The value pass reads
// the window K8 just read (the same WindowArgs) and writes, per series, the non-NaN sample count m,
// the NaN count and for each configured percentile the sum of the one or two ranks the integer
// rank rule reads (one rank: twice the sample).  The text pass prints, per emission position whose
// series has m >= 1:   wp|<edge ts>|server|service|<m>|<nan>|<p>:<v>,<p>:<v>,...
constexpr int WP_MAX_Q = 8;
struct WinPctArgs {
  WindowArgs w;                 // K8's arguments of this rollover (spill lists sorted; w.out = K8's result)
  int32_t nq;                   // 1 .. WP_MAX_Q
  int32_t q[WP_MAX_Q];          // percentile * 1000, strictly ascending, 1 .. 100000
  long long* sum2;              // [S][nq]
  int32_t *m, *nan;             // [S]
  int32_t* big_list;            // [S] series deferred to the block pass
  int32_t* big_n;
};
struct WinPctTextArgs {
  const long long* sum2;        // [S][nq]
  const int32_t *m, *nan;       // [S]
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t n_series;
  int32_t nq;
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  char ptxt[WP_MAX_Q][8];       // "<p>:" per percentile (at most "99.999:")
  int32_t plen[WP_MAX_Q];
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_winpct_row_bound(max name bytes, nq) * n bytes
};
// K17 sl rows: exact window threshold counts per service objective (slo.hip, docs/OBJECTIVES.md).
// The value pass reads the window K8 just read and writes one record per series: the non-NaN sample
// count m, the NaN count and, for the thresholds T_1 < ... < T_k of the series' class, the number
// of non-NaN samples v <= T_j (cumulative).  Class 0 has no threshold (no row).  The text pass
// prints, per emission position whose series has m >= 1 and k >= 1:
//   sl|<edge ts>|server|service|<m>|<nan>|<T>:<c>,<T>:<c>,...
constexpr int SL_MAX_T = 8;
struct SloRec {
  int32_t m, nan;
  int32_t c[SL_MAX_T];
};
struct SloArgs {
  WindowArgs w;                 // K8's arguments of this rollover (spill lists sorted; w.out = K8's result)
  const int32_t* cls;           // [S] class per series (values outside [0, n_classes) count as 0)
  const int32_t* nthr;          // [n_classes] thresholds per class, 0 .. SL_MAX_T (class 0: 0)
  const int32_t* thr;           // [n_classes][SL_MAX_T] strictly ascending, 0 .. INT32_MAX
  int32_t n_classes;
  SloRec* rec;                  // [S]
  int32_t* big_list;            // [S] series deferred to the block pass
  int32_t* big_n;
};
struct SloTextArgs {
  const SloRec* rec;            // [S]
  const int32_t* cls;           // [S]
  const int32_t* nthr;
  const int32_t* thr;
  int32_t n_classes;
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t n_series;
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_slo_row_bound(max name bytes) * n bytes
};
// K18 tk rows: per-rollover top-K series leaderboards (topk.hip, docs/LEADERBOARD.md).  For each
// board (key) the k candidates with the largest key value -- value descending as doubles, ties by
// emission position ascending; a candidate is active, has a non-NaN key value and tpm >= min_tpm.
constexpr int TK_MAX_BOARDS = 4;
constexpr int TK_MAX_K = 128;
enum TopKKey { TK_TPM = 0, TK_AVG, TK_P75, TK_P95 };
struct TopKRec {
  int32_t series, pos;          // series id and emission position
  WinStat w;                    // the series' K8 result of this rollover
};
struct TopKArgs {
  const WinStat* win;           // [n_series]
  const int32_t* perm;          // [n] series in emission order (16-byte aligned)
  int32_t n;
  int32_t n_series;
  int32_t k;                    // 1 .. TK_MAX_K
  int32_t nb;                   // boards, 1 .. TK_MAX_BOARDS
  int32_t by[TK_MAX_BOARDS];    // TopKKey per board
  double min_tpm;
  TopKRec* out;                 // [nb][k] rank order (host-mapped pinned memory or device memory)
  int32_t* out_n;               // [nb] rows of each board
  // set by apm_topk
  int32_t tiles;
  uint64_t* sc_key;             // [nb][tiles][k] tile survivors: order key (0: unused slot)
  int32_t* sc_pos;              // [nb][tiles][k] their emission positions
};
// K19 sv rows: exact per-service window stats across servers (svcwin.hip, docs/SERVICEWINDOW.md).
// The unit of work is a group: the series of one service (CSR grp_off / grp_mem, members in
// emission order, grp_pos their emission positions).  The value pass reads the window K8 just read
// of every active member and writes one record per group over the union of their samples; the text
// pass prints, at the emission position of a group's first active member when m >= 1:
//   sv|<edge ts>|service|<servers>|<m>|<nan>|<sum>|<p>:<v>,<p>:<v>,...
struct SvcRec {
  int32_t servers;              // active members
  int32_t m, nan;               // samples that are not / are ELAPSED_NAN
  int32_t first_pos;            // emission position of the first active member (-1: none)
  long long sum;                // of the m finite samples
  long long sum2[WP_MAX_Q];     // per percentile: sum of the one or two ranks read (one rank: twice it)
};
struct SvcWinArgs {
  WindowArgs w;                 // K8's arguments of this rollover (spill lists sorted; w.out = K8's result)
  int32_t nq;                   // 1 .. WP_MAX_Q
  int32_t q[WP_MAX_Q];          // percentile * 1000, strictly ascending, 1 .. 100000
  int32_t n_groups;
  const int32_t* grp_off;       // [n_groups + 1]
  const int32_t* grp_mem;       // [n_series] member series, group by group, each in emission order
  const int32_t* grp_pos;       // [n_series] their emission positions
  SvcRec* rec;                  // [n_groups]
  int32_t* big_list;            // [n_groups] groups deferred to the block pass
  int32_t* big_n;
};
struct SvcWinTextArgs {
  const SvcRec* rec;            // [n_groups]
  const int32_t* series_grp;    // [n_series] group of a series
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t n_series;
  int32_t n_groups;
  int32_t nq;
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  char ptxt[WP_MAX_Q][8];       // "<p>:" per percentile (at most "99.999:")
  int32_t plen[WP_MAX_Q];
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_svcwin_row_bound(max name bytes, nq) * n_groups bytes
};
// K20 rw rows: exact stats of the newest window buckets (recent.hip, docs/RECENT.md).  A span of k
// buckets is the window entries r >= n_win - min(k, n_win) of the window K8 just read (the same
// WindowArgs).  The value pass writes one record per (series, span) for every series with
// WinStat.active and WinStat.n >= 1, and none for any other; the text pass prints, per emission
// position of such a series and per span, ascending:
//   rw|<edge ts>|server|service|<k>|<m>|<nan>|<sum>|<p>:<v>,<p>:<v>,...
constexpr int RW_MAX_SPAN = 4;
struct RecentRec {
  int32_t m, nan;               // samples of the span that are not / are ELAPSED_NAN
  long long sum;                // of the m finite samples
  long long sum2[WP_MAX_Q];     // per percentile: sum of the one or two ranks read (m >= 1 only)
};
struct RecentArgs {
  WindowArgs w;                 // K8's arguments of this rollover (spill lists sorted; w.out = K8's result)
  int32_t nspan;                // 1 .. RW_MAX_SPAN
  int32_t span[RW_MAX_SPAN];    // buckets per span, strictly ascending, >= 1
  int32_t nq;                   // 1 .. WP_MAX_Q
  int32_t q[WP_MAX_Q];          // percentile * 1000, strictly ascending, 1 .. 100000
  RecentRec* rec;               // [S][nspan]
  int32_t* big_list;            // [S] series deferred to the block pass
  int32_t* big_n;
};
struct RecentTextArgs {
  const RecentRec* rec;         // [S][nspan]
  const WinStat* win;           // [S] K8's result: which series have records
  const int32_t* perm;          // [n / nspan] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;                    // lanes: emission positions * nspan
  int32_t n_series;
  int32_t nspan;
  int32_t span[RW_MAX_SPAN];
  int32_t nq;
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  char ptxt[WP_MAX_Q][8];       // "<p>:" per percentile (at most "99.999:")
  int32_t plen[WP_MAX_Q];
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_recent_row_bound(max name bytes, nq) * n bytes
};
// K21 sb rows: SLO burn-rate breaches decided on the device (burn.hip, docs/BURN.md).  A class is
// one objective {T, q}: T the latency threshold, q = target * 1000, b = 100000 - q the error budget;
// class 0 is "no row".  Over the window K8 just read (the same WindowArgs) and, per rule j, over
// its newest span[j] buckets (rw's span: the entries r >= n_win - min(span[j], n_win)) the value
// pass counts the finite samples and those above T, decides every rule with burn_fires (burncmp.h)
// and writes one record per series; the text pass prints, per emission position of a series with a
// rule that fired:
//   sb|<edge ts>|server|service|<T>|<q>|<m>|<bad>|<nan>|<k>:<f>:<m_k>:<bad_k>:<0|1>,...
constexpr int SB_MAX_RULES = 4;
struct BurnRec {
  int32_t m, bad, nan;          // window samples that are finite / finite and above T / ELAPSED_NAN
  int32_t mk[SB_MAX_RULES];     // per rule: the finite samples of its span
  int32_t badk[SB_MAX_RULES];   // ... and those of them above T
  int32_t fired;                // bit j: rule j fired (window and span both burn at factor[j])
};
struct BurnArgs {
  WindowArgs w;                 // K8's arguments of this rollover (w.out = K8's result)
  const int32_t* cls;           // [S] class per series (0 or out of range: no row)
  const int32_t* obj;           // [n_classes][2] {T, q} (class 0: unused)
  int32_t n_classes;
  int32_t nrule;                // 1 .. SB_MAX_RULES
  int32_t span[SB_MAX_RULES];   // buckets per rule, strictly ascending, >= 1
  int32_t factor[SB_MAX_RULES]; // f = factor * 1000, 1 .. 1000000
  int32_t min_samples;          // >= 1
  BurnRec* rec;                 // [S]
  int32_t* big_list;            // [S] series deferred to the block pass
  int32_t* big_n;
};
struct BurnTextArgs {
  const BurnRec* rec;           // [S]
  const int32_t* cls;           // [S]
  const int32_t* obj;           // [n_classes][2]
  int32_t n_classes;
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t n_series;
  int32_t nrule;
  int32_t span[SB_MAX_RULES];
  int32_t factor[SB_MAX_RULES];
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_burn_row_bound(max name bytes) * n bytes
};
// K22 tf rows: traffic drops and surges decided on the device (traffic.hip, docs/TRAFFIC.md).  A
// class is one gate minRate (samples per bucket); class 0 is "no row".  Over the per-bucket counts
// of the window K8 just read (the same WindowArgs; counts[slot][s] only, an absent bucket counts 0)
// the value pass finds, per rule j, the samples R of the newest k' = min(span[j], n_win) buckets and
// twice the median / four times the MAD of the other B = n_win - k' buckets' counts, decides the
// rule with traffic_verdict (trafficcmp.h) and writes one record per series; the text pass prints,
// per emission position of a series with a verdict other than N:
//   tf|<edge ts>|server|service|<n>|<minRate>|<k>:<B>:<R>:<med2>:<mad4>:<D|S|N>,...
constexpr int TF_MAX_RULES = 4;
struct TrafficRec {
  int32_t n;                    // WinStat.n of the series (= the sum of its window's counts)
  uint32_t R[TF_MAX_RULES];     // per rule: samples of the recent span (at most n, so 32 bits hold it)
  uint32_t med2[TF_MAX_RULES];  // ... twice the median of the baseline buckets' counts
  int32_t B[TF_MAX_RULES];      // ... the baseline buckets
  int32_t verdict;              // bits 2j, 2j + 1: rule j's verdict (TF_N / TF_D / TF_S)
  uint64_t mad4[TF_MAX_RULES];  // ... four times the median absolute deviation (below 2^34)
};
struct TrafficArgs {
  WindowArgs w;                 // K8's arguments of this rollover (w.out = K8's result)
  const int32_t* cls;           // [S] class per series (0 or out of range: no row)
  const int32_t* rate;          // [n_classes] minRate (class 0: unused)
  int32_t n_classes;
  int32_t nrule;                // 1 .. TF_MAX_RULES
  int32_t span[TF_MAX_RULES];   // buckets per rule, strictly ascending, 1 .. 64
  int32_t drop[TF_MAX_RULES];   // r_d = drop * 1000, 1 .. 999 (0: no drop test)
  int32_t surge[TF_MAX_RULES];  // r_s = surge * 1000, 1001 .. 1000000 (0: no surge test)
  int32_t z[TF_MAX_RULES];      // z * 1000, 0 .. 100000
  int32_t min_buckets;          // >= 3
  TrafficRec* rec;              // [S]
};
struct TrafficTextArgs {
  const TrafficRec* rec;        // [S]
  const int32_t* cls;           // [S]
  const int32_t* rate;          // [n_classes]
  int32_t n_classes;
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t n_series;
  int32_t nrule;
  int32_t span[TF_MAX_RULES];
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_traffic_row_bound(max name bytes) * n bytes
};
// K23 po rows: peer-outlier servers per service, decided on the device (peers.hip, docs/PEERS.md).
// The unit of work is K19's group: the series of one service (the same CSR).  A class is one gate
// minValue (ms); class 0 is "no row".  Stage A is K16's value pass with one percentile into po's own
// buffers (sum2 = x, m).  A member is eligible when it is active, has a class and m >= min_samples;
// over the E eligible members' x the value pass finds X2 = x_lo + x_hi and D4 = d_lo + d_hi of
// d_i = |2 x_i - X2| by counting ranks, decides every eligible member with peer_verdict
// (peercmp.h) and writes one record per series; the text pass prints, per emission position of a
// series with a verdict other than N:
//   po|<edge ts>|server|service|<m>|<p>:<x>|<E>|<X2>|<D4>|<H|L>
struct PeerRec {
  int32_t m;                    // finite samples of the series' window (0: no record)
  int32_t verdict;              // PO_N / PO_H / PO_L
  int32_t E;                    // eligible members of the series' group
  int32_t pad;
  long long x;                  // |x| < 2^32
  long long X2;                 // |X2| < 2^33
  long long D4;                 // 0 <= D4 < 2^36
};
struct PeerArgs {
  const uint8_t* active;        // [S] the series has an st row at this rollover
  const long long* sum2;        // [S] stage A: x per series (defined where m >= 1)
  const int32_t* m;             // [S] stage A: finite samples
  const int32_t* cls;           // [S] class per series (0 or out of range: no row)
  const int32_t* val;           // [n_classes] minValue (class 0: unused)
  int32_t n_classes;
  int32_t n_series;
  int32_t n_groups;
  const int32_t* grp_off;       // [n_groups + 1]
  const int32_t* grp_mem;       // [n_series] member series, group by group, each in emission order
  int32_t r_h;                  // high * 1000, 1001 .. 1000000 (0: no H test)
  int32_t r_l;                  // low * 1000, 1 .. 999 (0: no L test)
  int32_t z;                    // z * 1000, 0 .. 100000
  int32_t min_delta;            // ms, >= 0
  int32_t min_peers;            // >= 3
  int32_t min_samples;          // >= 1
  PeerRec* rec;                 // [S]
  int32_t* big_list;            // [n_groups] groups deferred to the block pass
  int32_t* big_n;
};
struct PeerTextArgs {
  const PeerRec* rec;           // [S]
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t n_series;
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  char ptxt[8];                 // "<p>:" (at most "99.999:")
  int32_t plen;
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_peer_row_bound(max name bytes) * n bytes
};
// K24 ls rows: latency shifts of a series' newest buckets against the rest of its own window,
// decided on the device (shift.hip, docs/SHIFT.md).  A class is one gate minDelta (ms); class 0 is
// "no row".  Over the window K8 just read (the same WindowArgs) the value pass splits the entries,
// per rule j, into the recent span (rw's span: the entries r >= n_win - min(span[j], n_win)) and the
// baseline (the others), finds twice the percentile q[j] of each side's finite samples (K16's rank
// rule) and the recent finite samples strictly above / below the baseline's, decides the rule with
// shift_verdict (shiftcmp.h) and writes one record per series; the text pass prints, per emission
// position of a series with a verdict other than N:
//   ls|<edge ts>|server|service|<n>|<minDelta>|<k>:<p>:<mB>:<T2>:<mR>:<X2>:<a>:<b>:<U|D|N>,...
constexpr int LS_MAX_RULES = 4;
struct ShiftRec {
  int32_t n;                    // WinStat.n of the series
  int32_t verdict;              // bits 2j, 2j + 1: rule j's verdict (LS_N / LS_U / LS_D)
  int32_t mB[LS_MAX_RULES], nanB[LS_MAX_RULES];  // per rule: finite / ELAPSED_NAN samples of the baseline
  int32_t mR[LS_MAX_RULES], nanR[LS_MAX_RULES];  // ... of the recent span
  int32_t a[LS_MAX_RULES], b[LS_MAX_RULES];      // ... recent finite samples v with 2 v > T2 / 2 v < T2
  long long T2[LS_MAX_RULES];   // ... twice the baseline's percentile (0: no finite sample), |T2| < 2^32
  long long X2[LS_MAX_RULES];   // ... twice the recent span's
};
struct ShiftArgs {
  WindowArgs w;                 // K8's arguments of this rollover (w.out = K8's result)
  const int32_t* cls;           // [S] class per series (0 or out of range: no row)
  const int32_t* delta;         // [n_classes] minDelta (class 0: unused)
  int32_t n_classes;
  int32_t nrule;                // 1 .. LS_MAX_RULES
  int32_t span[LS_MAX_RULES];   // buckets per rule, ascending (not strictly), 1 .. 64
  int32_t q[LS_MAX_RULES];      // percentile * 1000, 1 .. 99999
  int32_t up[LS_MAX_RULES];     // r_u = up * 1000, 1001 .. 1000000 (0: no up test)
  int32_t down[LS_MAX_RULES];   // r_d = down * 1000, 1001 .. 1000000 (0: no down test)
  int32_t z[LS_MAX_RULES];      // z * 1000, 0 .. 100000
  int32_t min_recent;           // >= 1
  int32_t min_baseline;         // >= 2
  ShiftRec* rec;                // [S]
  int32_t* big_list;            // [S] series deferred to the block pass
  int32_t* big_n;
};
struct ShiftTextArgs {
  const ShiftRec* rec;          // [S]
  const int32_t* cls;           // [S]
  const int32_t* delta;         // [n_classes]
  int32_t n_classes;
  const int32_t* perm;          // [n] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;
  int32_t n_series;
  int32_t nrule;
  int32_t span[LS_MAX_RULES];
  char ptxt[LS_MAX_RULES][8];   // "<p>:" per rule (at most "99.999:")
  int32_t plen[LS_MAX_RULES];
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_shift_row_bound(max name bytes) * n bytes
};
// K25 ic rows: incidents opened and closed on the device (incident.hip, docs/INCIDENTS.md).  The
// four verdict streams (sb, tf, po, ls) are level-triggered; per (series, source) a 16-byte state
// (incidentcmp.h) is stepped once a rollover from the source's verdict word and the series' st flag,
// and a row is printed only when the step has an event (opened, still open, closed):
//   ic|<edge ts>|server|service|<sb|tf|po|ls>|<O|S|C>|<code0>|<code>|<since ts>|<age>|<run>
// A source is handed over as a strided view of its records' verdict words, so the kernel depends on
// none of the four record layouts (a test hands it plain int32 arrays with stride 4).
constexpr int IC_MAX_SOURCES = 4;     // sb, tf, po, ls in this order (incidentcmp.h IC_SB ..)
struct IncidentSource {
  const int32_t* word;          // the verdict word of record 0 (null: the source is off)
  int32_t stride_bytes;         // sizeof of the record
  int32_t kind;                 // IC_SB / IC_TF / IC_PO / IC_LS
};
struct IncidentState;
struct IncidentArgs {
  IncidentSource src[IC_MAX_SOURCES];  // slot k belongs to source kind k
  const uint8_t* active;        // [S] the series has an st row at this rollover (PeerArgs::active)
  int32_t n_series;             // series ids at or above it are not touched
  int32_t open_after[IC_MAX_SOURCES];   // 1 .. 255
  int32_t close_after[IC_MAX_SOURCES];  // 1 .. 255
  int32_t remind_every;         // 0 (never) or 1 .. 65535
  long long edge_ts;
  IncidentState* state;         // [S][4]
  uint8_t* ev;                  // [S][4] this rollover's event: 0, 'O', 'S', 'C'
  uint8_t* codes;               // [S][4][2] what the row prints: {code0, code} ('-': not hot)
  int32_t* open_n;              // [4] += open incidents per source (the caller zeroes them)
};
struct IncidentTextArgs {
  const IncidentState* state;   // [S][4]
  const uint8_t* ev;            // [S][4]
  const uint8_t* codes;         // [S][4][2]
  const int32_t* perm;          // [n / 4] series in emission order
  const int4* series_names;     // [S] {server off, len, service off, len} into `names`
  const char* names;
  int32_t n;                    // text positions: emission positions * 4 (position p: series perm[p / 4], source p % 4)
  int32_t n_series;
  int32_t ts_len;
  char ts[24];                  // "<edge ts>|"
  uint32_t *len, *off;          // [n + 1] row bytes / exclusive offsets (off[n] = total)
  char* out;                    // at least apm_incident_row_bound(max name bytes) * n bytes
};
struct AlertArgs {
  const WinStat* win;         // [S]
  const ZOut* z;              // [S] for this lag
  int32_t* counter;           // [S] leaky counter for this lag
  const double* hard_max;     // [S] per-series effective hardMaxMsAlertThreshold
  const uint8_t* suppressed;  // [S] service in suppressedServices
  const uint64_t* emit_key;   // [S]
  AlertRec* out;
  int32_t* n_out;
  int32_t n_series;
  int32_t lag_idx;
  int32_t n_lags;
  int32_t lag_suppressed;
  int32_t window;             // rollingAlertWindowSizeInIntervals
  int32_t threshold;          // requiredNumberBadIntervalsInAlertWindowToTrigger
  double hard_min_ms;
  double hard_min_tpm;
  int32_t both_only;
  int32_t max_out;
  // Device-side cooldown pre-filter: time of the latest alert of the series' cooldown key (NaN:
  // none).  A candidate the host's cooldown would certainly suppress -- same expression, same
  // `now` -- is not emitted (cooldown times only grow, so a stale value can only let through a
  // candidate the host then suppresses).  An alert storm otherwise ships ~20k candidates per
  // rollover to the host decision.
  const double* cool_t;       // [S] or nullptr
  double now;
  double cool_s;              // cooldown in seconds (perServiceAlertCooldownInMinutes * 60)
};

}  // namespace apm

extern "C" {
// parse.hip
size_t apm_parse_workspace_bytes(uint64_t max_bytes, uint32_t max_lines, uint32_t max_chunks);
int apm_parse_batch(const uint8_t* d_bytes, uint64_t n_bytes, const uint32_t* d_chunk_begin,
                    const uint8_t* d_chunk_kind, const uint32_t* d_chunk_file, uint32_t n_chunks,
                    void* d_ws, uint32_t max_lines, apm::Event* d_events, uint32_t* d_n_events,
                    uint32_t* d_n_lines, unsigned long long* d_watermark, uint8_t* d_file_open,
                    const apm::TzTable* tz, hipStream_t stream);
// stats.hip
// checkpoint: occupied cells of k bucket slots packed on the device (entry i * n + s = slot
// d_slots[i], series s); offs[k * n] = total cells.  lens / offs: k * n + 1 entries.
size_t apm_ck_pack_tmp_bytes(uint64_t n_entries);
int apm_ck_pack_cells(const int32_t* counts, const int32_t* cells, const int32_t* d_slots, int k, int32_t n, int32_t S,
                      int32_t cap, uint32_t* lens, uint32_t* offs, void* tmp, size_t tmp_bytes, int32_t* packed,
                      hipStream_t s);
void apm_stats_clear_slot(apm::StatsState* st, int slot, hipStream_t stream);
void apm_bucket_append(const apm::TxRec* d_tx, uint32_t lo, uint32_t hi, apm::StatsState* st,
                       int64_t min_live_bucket, hipStream_t stream);
// marks series with a NaN elapsed sample in tx[0, n) (before any of the batch is appended)
void apm_nan_mark(const apm::TxRec* d_tx, uint32_t n, apm::StatsState* st, hipStream_t stream);
void apm_window_stats(apm::WindowArgs* a, hipStream_t stream);
// before K8: every slot's spill list [slot * cap, + spill_n[slot]) sorted by series, stably (a
// series' samples keep their arrival order), into (series_out, val_out); the caller swaps buffers
size_t apm_spill_sort_tmp_bytes(int32_t spill_cap, int32_t S, int32_t nslot);
int apm_spill_sort(const apm::StatsState* st, int32_t* series_out, int32_t* val_out, void* tmp, size_t tmp_bytes,
                   hipStream_t stream);
void apm_pool_append(const apm::TxRec* d_tx, uint32_t lo, uint32_t hi, const int64_t* d_gid, int64_t* tail_end,
                     int64_t* tail_gid, int64_t base, hipStream_t stream);
size_t apm_release_tmp_bytes(int64_t cap);
int apm_release_merge(const int64_t* pool_end, const int64_t* pool_gid, int64_t n_pool, const int64_t* tail_end,
                      const int64_t* tail_gid, int64_t n_tail, int64_t* sort_end, int64_t* sort_gid,
                      int64_t* out_end, int64_t* out_gid, void* tmp, size_t tmp_bytes, hipStream_t stream);
// device scalars (4 or 8 bytes) -> host-mapped pinned memory, optional device reset afterwards
void apm_export(const apm::ExportArgs* a, hipStream_t stream);
// copy by a kernel (src / dst may be device views of pinned host memory): ordered on `stream`,
// never blocks the calling thread
void apm_copy(void* dst, const void* src, size_t bytes, hipStream_t stream);
// the same on at most `max_blocks` workgroups of 256 (a host-link copy that leaves the CUs to
// the kernels running beside it)
void apm_copy_capped(void* dst, const void* src, size_t bytes, uint32_t max_blocks, hipStream_t stream);
void apm_copy_segs(const apm::CopySegs* c, hipStream_t stream);
// up to 8 doubles -> device memory, passed as kernel arguments (nothing read over the host link)
void apm_set_f64(double* dst, const double* vals, int n, hipStream_t stream);
// zscore.hip
void apm_zscore(apm::ZArgs* a, int dtype_bytes, hipStream_t stream);
void apm_zscore_warm(apm::ZArgs* a, int dtype_bytes, int fill, uint64_t seed, const apm::WinStat* base,
                     hipStream_t stream);
void apm_server_rollup(apm::RollupArgs* a, hipStream_t stream);
size_t apm_format_tmp_bytes(int32_t n_max);
void apm_format_fixed_batch(const double* d_x, int n, int f, int mode, char* d_out, hipStream_t stream);
int apm_format_plan(apm::FormatArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_format_write(apm::FormatArgs* a, hipStream_t stream);
void apm_alert_eval(apm::AlertArgs* a, hipStream_t stream);
// dst[idx[i]] = val[i]; idx / val may be device views of pinned host memory
void apm_scatter_f64(double* dst, const int32_t* idx, const double* val, int32_t n, hipStream_t stream);
// blocks of the one-pass fb formatter for `n_rows` rows (the status array's length)
uint32_t apm_fleet_format_blocks(int32_t n_rows);
// capacity of FleetFormatArgs::out for `rows` rows and names of at most `longest` bytes
size_t apm_fleet_out_bound(int32_t rows, size_t longest);
void apm_fleet_format(apm::FleetFormatArgs* a, hipStream_t stream);
// after K11: the candidate count (clamped to max_n), the candidates and -- rows != 0 -- their window
// stats and candidate-LAG z-score rows, written into host-mapped pinned buffers (device pointers
// of hipHostMalloc memory) in candidate order
void apm_alert_gather(const apm::AlertRec* alerts, const int32_t* n_dev, int32_t max_n, const apm::WinStat* win,
                      const apm::ZOut* const* z_by_lag, int32_t n_lags, int32_t rows, apm::AlertRec* alerts_out,
                      apm::WinStat* win_out, apm::ZOut* z_out, int32_t* n_out, hipStream_t stream);
// hist.hip
// sample counts of the count pass' two paths (tests bracket them): a series with more samples in
// the bucket than apm_hist_group_max() is counted by a whole block instead of 32 lanes
int32_t apm_hist_group_max();
size_t apm_hist_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes
size_t apm_hist_row_bound(size_t name_bytes);
// count pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_hist_plan(apm::HistArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_hist_write(apm::HistArgs* a, hipStream_t stream);
// winpct.hip
// the value pass' two paths (tests bracket them): a series stays in its 32-lane group while the
// window has at most apm_winpct_group_win() buckets and at most apm_winpct_group_max() samples;
// every other series is selected by a whole block
int32_t apm_winpct_group_max();
int32_t apm_winpct_group_win();
size_t apm_winpct_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes and nq percentiles
size_t apm_winpct_row_bound(size_t name_bytes, int32_t nq);
void apm_winpct_values(apm::WinPctArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_winpct_plan(apm::WinPctTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_winpct_write(apm::WinPctTextArgs* a, hipStream_t stream);
// slo.hip
// the value pass' two paths (tests bracket the boundary): a series whose window K8 counted at most
// apm_slo_group_max() samples stays in its 32-lane group, every other one is counted by a block
int32_t apm_slo_group_max();
int32_t apm_slo_stage_bytes();   // the write pass' LDS stage (a 64-row block over it stores directly)
size_t apm_slo_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes
size_t apm_slo_row_bound(size_t name_bytes);
void apm_slo_values(apm::SloArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_slo_plan(apm::SloTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_slo_write(apm::SloTextArgs* a, hipStream_t stream);
// topk.hip
int32_t apm_topk_tile();         // emission positions per block of the tile pass (tests bracket it)
int32_t apm_topk_final_span();   // survivors the final block reads per sweep (it loops beyond)
size_t apm_topk_scratch_bytes(int32_t n_max, int32_t k, int32_t nb);
// both launches for all boards; `scratch` holds apm_topk_scratch_bytes(a->n, a->k, a->nb) bytes
void apm_topk(apm::TopKArgs* a, void* scratch, hipStream_t stream);
// svcwin.hip
// the value pass' two paths (tests bracket them): a service stays in its 32-lane group while the
// window has at most apm_svcwin_group_win() buckets and its active members' windows hold at most
// apm_svcwin_group_max() samples together; every other service is selected by a whole block
int32_t apm_svcwin_group_max();
int32_t apm_svcwin_group_win();
size_t apm_svcwin_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for a service name of `name_bytes` bytes and nq percentiles
size_t apm_svcwin_row_bound(size_t name_bytes, int32_t nq);
void apm_svcwin_values(apm::SvcWinArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_svcwin_plan(apm::SvcWinTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_svcwin_write(apm::SvcWinTextArgs* a, hipStream_t stream);
// recent.hip
// the value pass' two paths (tests bracket them): a series stays in its 32-lane group while the
// window has at most apm_recent_group_win() buckets and its largest span holds at most
// apm_recent_group_max() samples; every other series with a row is selected by a whole block
int32_t apm_recent_group_max();
int32_t apm_recent_group_win();
size_t apm_recent_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes and nq percentiles
size_t apm_recent_row_bound(size_t name_bytes, int32_t nq);
void apm_recent_values(apm::RecentArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_recent_plan(apm::RecentTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_recent_write(apm::RecentTextArgs* a, hipStream_t stream);
// burn.hip
// the value pass' two paths (tests bracket them): a series K8 counted at most apm_burn_group_max()
// samples for stays in its 32-lane group, every other one is counted by a block
int32_t apm_burn_group_max();
size_t apm_burn_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes
size_t apm_burn_row_bound(size_t name_bytes);
void apm_burn_values(apm::BurnArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_burn_plan(apm::BurnTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_burn_write(apm::BurnTextArgs* a, hipStream_t stream);
// traffic.hip
// the value pass' two paths (tests bracket them): a window of at most apm_traffic_group_win()
// buckets is sorted in registers, 64 series (apm_traffic_tile()) a block; a longer one, up to
// apm_traffic_max_win() buckets, is ranked by counting
int32_t apm_traffic_group_win();
int32_t apm_traffic_max_win();
int32_t apm_traffic_tile();
size_t apm_traffic_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes
size_t apm_traffic_row_bound(size_t name_bytes);
// 0, or -1 when the window is longer than apm_traffic_max_win() (nothing launched)
int apm_traffic_values(apm::TrafficArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_traffic_plan(apm::TrafficTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_traffic_write(apm::TrafficTextArgs* a, hipStream_t stream);
// peers.hip
// the value pass' two paths (tests bracket them): a group of at most apm_peer_group_max() members
// is ranked by 32 lanes in registers; a larger one by a whole block, without a bound
int32_t apm_peer_group_max();
size_t apm_peer_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes
size_t apm_peer_row_bound(size_t name_bytes);
void apm_peer_values(apm::PeerArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_peer_plan(apm::PeerTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_peer_write(apm::PeerTextArgs* a, hipStream_t stream);
// shift.hip
// the value pass' two paths (tests bracket them): a series whose window has at most
// apm_shift_group_win() buckets and holds at most apm_shift_group_max() samples stays in its
// 32-lane group, every other one is selected by a block
int32_t apm_shift_group_max();
int32_t apm_shift_group_win();
size_t apm_shift_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes
size_t apm_shift_row_bound(size_t name_bytes);
void apm_shift_values(apm::ShiftArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_shift_plan(apm::ShiftTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_shift_write(apm::ShiftTextArgs* a, hipStream_t stream);
// incident.hip
// scan scratch for n_max series (4 text positions each)
size_t apm_incident_tmp_bytes(int32_t n_max);
// upper bound of a row's bytes for names of `name_bytes` (server + service) bytes
size_t apm_incident_row_bound(size_t name_bytes);
// one step of every (series, source) state below n_series; a->open_n must be zero before it
void apm_incident_step(apm::IncidentArgs* a, hipStream_t stream);
// length pass + scan: afterwards a->off[0..n] hold the rows' offsets, off[n] the total bytes
int apm_incident_plan(apm::IncidentTextArgs* a, void* tmp, size_t tmp_bytes, hipStream_t stream);
void apm_incident_write(apm::IncidentTextArgs* a, hipStream_t stream);
// fleet.hip
void apm_service_moments(const int32_t* series_service, const uint8_t* active, int32_t n_series, int32_t S,
                         int32_t n_lags, int32_t n_services_cap, const double* const* sums, const double* const* comps,
                         const int32_t* const* cnts, double* dst, hipStream_t stream);
void apm_service_moments_tail(const int32_t* series_service, const uint8_t* active, int32_t s_lo, int32_t n_series,
                              int32_t S, int32_t n_lags, int32_t n_services_cap, const double* const* sums,
                              const double* const* comps, const int32_t* const* cnts, double* dst,
                              hipStream_t stream);
int apm_service_gram(const int32_t* svc_off, const int32_t* svc_ids, const uint8_t* active, int32_t n_services,
                     int32_t S, int32_t n_lags, const double* const* sums, const double* const* comps,
                     const int32_t* const* cnts, double* dst, hipStream_t stream, const int32_t* svc_map = nullptr,
                     int32_t accumulate = 0);
}
