// Python bindings for the native runtime (pybind11, no torch headers).
//
//   _apm_native.Engine        -- the GPU pipeline (engine.h)
//   _apm_native.JoinHarness   -- the host join workers alone, fed with Python-built events
//                                (CPU-testable; used by tests/test_join_native.py)
//   _apm_native.js_*          -- JS-exact number formatting helpers (parity tests)
//   _apm_native.Tailer / proc_* / synth_* are registered from their own translation units.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <memory>

#include "kernels/burncmp.h"
#include "kernels/incidentcmp.h"
#include "kernels/kernel_api.h"
#include "kernels/peercmp.h"
#include "kernels/shiftcmp.h"
#include "kernels/trafficcmp.h"
#include "runtime/engine.h"
#include "runtime/format.h"
#include "runtime/jsutil.h"
#include "runtime/merge.h"

namespace apm {
namespace copyenc {
void encode_blob(std::string_view blob, std::string* out, int64_t* counts);
}
int apm_txcopy_lines(const char* d_text, const uint64_t* h_line_off, int64_t n, std::string& out_rows);  // txcopy.hip
std::vector<double> apm_release_bench(int64_t n, int iters, uint64_t seed);                               // txcopy.hip
}  // namespace apm

namespace py = pybind11;
using namespace apm;

void register_tailer(py::module_& m);
void register_synth(py::module_& m);
void register_procstat(py::module_& m);
void register_dbsink(py::module_& m);

namespace {

// device memory of a test hook: freed on every way out, a throwing HIP_OK included
struct DevMem {
  void* p = nullptr;
  explicit DevMem(size_t bytes) { HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 8))); }
  ~DevMem() { if (p) (void)hipFree(p); }
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  template <class T> T* as() const { return static_cast<T*>(p); }
};

template <class T>
T get(const py::dict& d, const char* k, T dflt) {
  if (d.contains(k)) return d[k].cast<T>();
  return dflt;
}

TzTable tz_from(const py::dict& d) {
  TzTable tz{};
  tz.n = 1;
  tz.local_start[0] = INT64_MIN / 2;
  tz.offset_ms[0] = 0;
  if (d.contains("tz_table")) {
    auto rows = d["tz_table"].cast<std::vector<std::pair<int64_t, int64_t>>>();
    // ops/parse_ref.py tz_table picks the rows around a centre time; cutting here would keep the
    // oldest instead
    if (rows.size() > 64) throw std::invalid_argument("tz_table: more than 64 rows");
    tz.n = (int)rows.size();
    for (int i = 0; i < tz.n; ++i) { tz.local_start[i] = rows[i].first; tz.offset_ms[i] = rows[i].second; }
    if (tz.n == 0) { tz.n = 1; tz.local_start[0] = INT64_MIN / 2; tz.offset_ms[0] = 0; }
  }
  return tz;
}

EngineConfig config_from(const py::dict& d) {
  EngineConfig c;
  c.device = get<int>(d, "device", 0);
  c.max_series = get<int32_t>(d, "max_series", c.max_series);
  c.cell_cap = get<int32_t>(d, "cell_cap", c.cell_cap);
  c.spill_cap = get<int32_t>(d, "spill_cap", c.spill_cap);
  c.max_batch_bytes = get<uint64_t>(d, "max_batch_bytes", c.max_batch_bytes);
  c.max_lines = get<uint32_t>(d, "max_lines", c.max_lines);
  c.max_chunks = get<uint32_t>(d, "max_chunks", c.max_chunks);
  c.pool_cap = get<int64_t>(d, "pool_cap", c.pool_cap);
  c.max_tx_per_batch = get<int32_t>(d, "max_tx_per_batch", c.max_tx_per_batch);
  c.max_alerts = get<int32_t>(d, "max_alerts", c.max_alerts);
  c.ring_bytes = get<int>(d, "ring_bytes", c.ring_bytes);
  c.exact_mean = get<int>(d, "exact_mean", c.exact_mean);
  c.sigma_stddev = get<int>(d, "sigma_stddev", c.sigma_stddev);
  c.resync_k = get<int>(d, "resync_k", c.resync_k);
  c.resync_mfma = get<bool>(d, "resync_mfma", c.resync_mfma);
  c.emulate_aliasing = get<int>(d, "emulate_aliasing", c.emulate_aliasing);
  if (d.contains("lags")) {
    auto lags = d["lags"].cast<std::vector<std::tuple<int, double, double>>>();
    c.n_lags = (int)std::min<size_t>(lags.size(), MAX_LAGS);
    for (int i = 0; i < c.n_lags; ++i) {
      c.lags[i] = std::get<0>(lags[i]);
      c.thr[i] = std::get<1>(lags[i]);
      c.infl[i] = std::get<2>(lags[i]);
    }
  }
  if (d.contains("lag_suppressed")) {
    auto v = d["lag_suppressed"].cast<std::vector<int>>();
    for (size_t i = 0; i < v.size() && i < MAX_LAGS; ++i) c.lag_suppressed[i] = v[i];
  }
  c.alert_window = get<int>(d, "alert_window", c.alert_window);
  c.alert_threshold = get<int>(d, "alert_threshold", c.alert_threshold);
  c.hard_min_ms = get<double>(d, "hard_min_ms", c.hard_min_ms);
  c.hard_min_tpm = get<double>(d, "hard_min_tpm", c.hard_min_tpm);
  c.hard_max_ms = get<double>(d, "hard_max_ms", c.hard_max_ms);
  c.both_only = get<int>(d, "both_only", c.both_only);
  c.cooldown_ms = get<double>(d, "cooldown_ms", c.cooldown_ms);
  c.cooldown_by_service = get<int>(d, "cooldown_by_service", c.cooldown_by_service);
  c.alert_clock_entry = get<int>(d, "alert_clock_entry", c.alert_clock_entry);
  c.interval_len = get<int>(d, "interval_len", c.interval_len);
  c.window = get<int>(d, "window", c.window);
  c.buffer = get<int>(d, "buffer", c.buffer);
  c.nslot = get<int>(d, "nslot", c.nslot);
  c.ck_stage_bytes = get<int64_t>(d, "ck_stage_bytes", c.ck_stage_bytes);
  c.record_ttl_ms = get<double>(d, "record_ttl_ms", c.record_ttl_ms);
  c.acct_ttl_ms = get<double>(d, "acct_ttl_ms", c.acct_ttl_ms);
  c.need_ttl_ms = get<double>(d, "need_ttl_ms", c.need_ttl_ms);
  c.tz = tz_from(d);
  c.join_threads = get<int>(d, "join_threads", c.join_threads);
  c.pin_threads = get<bool>(d, "pin_threads", c.pin_threads);
  c.coll_timeout_ms = get<double>(d, "coll_timeout_ms", c.coll_timeout_ms);
  c.coll_init_timeout_ms = get<double>(d, "coll_init_timeout_ms", c.coll_init_timeout_ms);
  c.node_cooldown = get<int>(d, "node_cooldown", c.node_cooldown);
  c.outputs = get<uint32_t>(d, "outputs", c.outputs);
  if (d.contains("win_pcts")) {
    auto v = d["win_pcts"].cast<std::vector<int64_t>>();
    if (v.size() > 8) throw std::invalid_argument("win_pcts: at most 8 percentiles");
    c.n_win_pcts = (int32_t)v.size();
    for (size_t i = 0; i < v.size(); ++i) {
      if (v[i] < 1 || v[i] > 100000 || (i && v[i] <= v[i - 1]))
        throw std::invalid_argument("win_pcts: strictly ascending integers in 1 .. 100000 (percentile * 1000)");
      c.win_pcts[i] = (int32_t)v[i];
    }
  }
  if (d.contains("slo_classes")) {  // (the constructor checks the tables when the sl stream is on)
    c.slo_classes = d["slo_classes"].cast<std::vector<std::vector<int64_t>>>();
    if (d.contains("slo_services")) c.slo_services = d["slo_services"].cast<std::map<std::string, int32_t>>();
    c.slo_default = get<int32_t>(d, "slo_default", 0);
  }
  if (d.contains("svc_pcts")) {
    auto v = d["svc_pcts"].cast<std::vector<int64_t>>();
    if (v.size() > 8) throw std::invalid_argument("svc_pcts: at most 8 percentiles");
    c.n_svc_pcts = (int32_t)v.size();
    for (size_t i = 0; i < v.size(); ++i) {
      if (v[i] < 1 || v[i] > 100000 || (i && v[i] <= v[i - 1]))
        throw std::invalid_argument("svc_pcts: strictly ascending integers in 1 .. 100000 (percentile * 1000)");
      c.svc_pcts[i] = (int32_t)v[i];
    }
  }
  if (d.contains("rw_buckets")) {  // K20 (the constructor checks the bound against the window)
    auto v = d["rw_buckets"].cast<std::vector<int64_t>>();
    if (v.size() > 4) throw std::invalid_argument("rw_buckets: at most 4 spans");
    c.n_rw_buckets = (int32_t)v.size();
    for (size_t i = 0; i < v.size(); ++i) {
      if (v[i] < 1 || v[i] > 0x7fffffff || (i && v[i] <= v[i - 1]))
        throw std::invalid_argument("rw_buckets: strictly ascending integers >= 1");
      c.rw_buckets[i] = (int32_t)v[i];
    }
  }
  if (d.contains("rw_pcts")) {
    auto v = d["rw_pcts"].cast<std::vector<int64_t>>();
    if (v.size() > 8) throw std::invalid_argument("rw_pcts: at most 8 percentiles");
    c.n_rw_pcts = (int32_t)v.size();
    for (size_t i = 0; i < v.size(); ++i) {
      if (v[i] < 1 || v[i] > 100000 || (i && v[i] <= v[i - 1]))
        throw std::invalid_argument("rw_pcts: strictly ascending integers in 1 .. 100000 (percentile * 1000)");
      c.rw_pcts[i] = (int32_t)v[i];
    }
  }
  if (d.contains("sb_classes")) {  // K21 (the constructor checks the tables and rules when the sb stream is on)
    c.sb_classes = d["sb_classes"].cast<std::vector<std::vector<int64_t>>>();
    if (d.contains("sb_services")) c.sb_services = d["sb_services"].cast<std::map<std::string, int32_t>>();
    c.sb_default = get<int32_t>(d, "sb_default", 0);
  }
  if (d.contains("sb_short")) {
    auto k = d["sb_short"].cast<std::vector<int64_t>>();
    auto f = d.contains("sb_factor") ? d["sb_factor"].cast<std::vector<int64_t>>() : std::vector<int64_t>();
    if (k.size() > 4 || f.size() != k.size()) throw std::invalid_argument("sb_short / sb_factor: at most 4 rules, one factor per span");
    c.n_sb_rules = (int32_t)k.size();
    for (size_t i = 0; i < k.size(); ++i) {
      if (k[i] < 1 || k[i] > 0x7fffffff || (i && k[i] <= k[i - 1]))
        throw std::invalid_argument("sb_short: strictly ascending integers >= 1");
      if (f[i] < 1 || f[i] > 1000000) throw std::invalid_argument("sb_factor: integers in 1 .. 1000000 (factor * 1000)");
      c.sb_short[i] = (int32_t)k[i];
      c.sb_factor[i] = (int32_t)f[i];
    }
  }
  if (d.contains("sb_min_samples")) {
    const int64_t ms = d["sb_min_samples"].cast<int64_t>();
    if (ms < 1 || ms > 0x7fffffff) throw std::invalid_argument("sb_min_samples: an integer >= 1");
    c.sb_min_samples = (int32_t)ms;
  }
  if (d.contains("tf_classes")) {  // K22 (the constructor checks the tables and rules when the tf stream is on)
    c.tf_classes = d["tf_classes"].cast<std::vector<std::vector<int64_t>>>();
    if (d.contains("tf_services")) c.tf_services = d["tf_services"].cast<std::map<std::string, int32_t>>();
    c.tf_default = get<int32_t>(d, "tf_default", 0);
  }
  if (d.contains("tf_short")) {
    const auto list = [&](const char* key) {
      return d.contains(key) ? d[key].cast<std::vector<int64_t>>() : std::vector<int64_t>();
    };
    const auto k = list("tf_short"), dr = list("tf_drop"), su = list("tf_surge"), z = list("tf_z");
    if (k.size() > 4 || dr.size() != k.size() || su.size() != k.size() || z.size() != k.size())
      throw std::invalid_argument("tf_short / tf_drop / tf_surge / tf_z: at most 4 rules, one value of each per span");
    c.n_tf_rules = (int32_t)k.size();
    for (size_t i = 0; i < k.size(); ++i) {
      if (k[i] < 1 || k[i] > 64 || (i && k[i] <= k[i - 1]))
        throw std::invalid_argument("tf_short: strictly ascending integers in 1 .. 64");
      if (dr[i] < 0 || dr[i] > 999) throw std::invalid_argument("tf_drop: integers in 1 .. 999 (drop * 1000), 0 for none");
      if (su[i] != 0 && (su[i] < 1001 || su[i] > 1000000))
        throw std::invalid_argument("tf_surge: integers in 1001 .. 1000000 (surge * 1000), 0 for none");
      if (dr[i] == 0 && su[i] == 0) throw std::invalid_argument("tf_drop / tf_surge: a rule needs at least one of them");
      if (z[i] < 0 || z[i] > 100000) throw std::invalid_argument("tf_z: integers in 0 .. 100000 (z * 1000)");
      c.tf_short[i] = (int32_t)k[i];
      c.tf_drop[i] = (int32_t)dr[i];
      c.tf_surge[i] = (int32_t)su[i];
      c.tf_z[i] = (int32_t)z[i];
    }
  }
  if (d.contains("tf_min_buckets")) {
    const int64_t mb = d["tf_min_buckets"].cast<int64_t>();
    if (mb < 3 || mb > 0x7fffffff) throw std::invalid_argument("tf_min_buckets: an integer >= 3");
    c.tf_min_buckets = (int32_t)mb;
  }
  if (d.contains("po_classes")) {  // K23 (the constructor checks the tables and settings when the po stream is on)
    c.po_classes = d["po_classes"].cast<std::vector<std::vector<int64_t>>>();
    if (d.contains("po_services")) c.po_services = d["po_services"].cast<std::map<std::string, int32_t>>();
    c.po_default = get<int32_t>(d, "po_default", 0);
  }
  {
    const auto num = [&](const char* key, int64_t lo, int64_t hi, int64_t also, int32_t& dst, const char* what) {
      if (!d.contains(key)) return;
      const int64_t v = d[key].cast<int64_t>();
      if (v != also && (v < lo || v > hi)) throw std::invalid_argument(std::string(key) + ": " + what);
      dst = (int32_t)v;
    };
    num("po_pct", 1, 100000, 0, c.po_pct, "a percentile * 1000 in 1 .. 100000");
    num("po_high", 1001, 1000000, 0, c.po_high, "an integer in 1001 .. 1000000 (high * 1000), 0 for none");
    num("po_low", 1, 999, 0, c.po_low, "an integer in 1 .. 999 (low * 1000), 0 for none");
    num("po_z", 0, 100000, 0, c.po_z, "an integer in 0 .. 100000 (z * 1000)");
    num("po_min_delta", 0, 0x7fffffff, 0, c.po_min_delta, "an integer in 0 .. 2147483647");
    num("po_min_peers", 3, 0x7fffffff, 3, c.po_min_peers, "an integer >= 3");
    num("po_min_samples", 1, 0x7fffffff, 1, c.po_min_samples, "an integer in 1 .. 2147483647");
  }
  if (d.contains("ls_classes")) {  // K24 (the constructor checks the tables and rules when the ls stream is on)
    c.ls_classes = d["ls_classes"].cast<std::vector<std::vector<int64_t>>>();
    if (d.contains("ls_services")) c.ls_services = d["ls_services"].cast<std::map<std::string, int32_t>>();
    c.ls_default = get<int32_t>(d, "ls_default", 0);
  }
  if (d.contains("ls_short")) {
    const auto list = [&](const char* key) {
      return d.contains(key) ? d[key].cast<std::vector<int64_t>>() : std::vector<int64_t>();
    };
    const auto k = list("ls_short"), q = list("ls_pct"), up = list("ls_up"), dn = list("ls_down"), z = list("ls_z");
    if (k.size() > 4 || q.size() != k.size() || up.size() != k.size() || dn.size() != k.size() || z.size() != k.size())
      throw std::invalid_argument("ls_short / ls_pct / ls_up / ls_down / ls_z: at most 4 rules, one value of each per rule");
    c.n_ls_rules = (int32_t)k.size();
    for (size_t i = 0; i < k.size(); ++i) {
      if (k[i] < 1 || k[i] > 64) throw std::invalid_argument("ls_short: integers in 1 .. 64");
      if (q[i] < 1 || q[i] > 99999) throw std::invalid_argument("ls_pct: integers in 1 .. 99999 (percentile * 1000)");
      if (i && k[i] < k[i - 1]) throw std::invalid_argument("ls_short: ascending");
      for (size_t o = 0; o < i; ++o)
        if (k[o] == k[i] && q[o] == q[i]) throw std::invalid_argument("ls_short / ls_pct: a (short, percentile) pair stands twice");
      if (up[i] != 0 && (up[i] < 1001 || up[i] > 1000000))
        throw std::invalid_argument("ls_up: integers in 1001 .. 1000000 (up * 1000), 0 for none");
      if (dn[i] != 0 && (dn[i] < 1001 || dn[i] > 1000000))
        throw std::invalid_argument("ls_down: integers in 1001 .. 1000000 (down * 1000), 0 for none");
      if (up[i] == 0 && dn[i] == 0) throw std::invalid_argument("ls_up / ls_down: a rule needs at least one of them");
      if (z[i] < 0 || z[i] > 100000) throw std::invalid_argument("ls_z: integers in 0 .. 100000 (z * 1000)");
      c.ls_short[i] = (int32_t)k[i];
      c.ls_pct[i] = (int32_t)q[i];
      c.ls_up[i] = (int32_t)up[i];
      c.ls_down[i] = (int32_t)dn[i];
      c.ls_z[i] = (int32_t)z[i];
    }
  }
  if (d.contains("ls_min_recent")) {
    const int64_t v = d["ls_min_recent"].cast<int64_t>();
    if (v < 1 || v > 0x7fffffff) throw std::invalid_argument("ls_min_recent: an integer >= 1");
    c.ls_min_recent = (int32_t)v;
  }
  if (d.contains("ls_min_baseline")) {
    const int64_t v = d["ls_min_baseline"].cast<int64_t>();
    if (v < 2 || v > 0x7fffffff) throw std::invalid_argument("ls_min_baseline: an integer >= 2");
    c.ls_min_baseline = (int32_t)v;
  }
  if (d.contains("ic_open_after")) {  // K25 (the constructor checks them again when the ic stream is on)
    const auto list = [&](const char* key) {
      return d.contains(key) ? d[key].cast<std::vector<int64_t>>() : std::vector<int64_t>();
    };
    const auto o = list("ic_open_after"), cl = list("ic_close_after");
    if (o.size() != 4 || cl.size() != 4)
      throw std::invalid_argument("ic_open_after / ic_close_after: one value per source (sb, tf, po, ls), 0 for a source that is off");
    for (size_t k = 0; k < 4; ++k) {
      if ((o[k] == 0) != (cl[k] == 0) || o[k] < 0 || o[k] > 255 || cl[k] < 0 || cl[k] > 255)
        throw std::invalid_argument("ic_open_after / ic_close_after: integers in 1 .. 255 (both 0: the source is off)");
      c.ic_open_after[k] = (int32_t)o[k];
      c.ic_close_after[k] = (int32_t)cl[k];
    }
  }
  if (d.contains("ic_remind_every")) {
    const int64_t v = d["ic_remind_every"].cast<int64_t>();
    if (v < 0 || v > 65535) throw std::invalid_argument("ic_remind_every: 0 or an integer in 1 .. 65535");
    c.ic_remind_every = (int32_t)v;
  }
  if (d.contains("tk_k") && !d["tk_k"].is_none()) {  // (the constructor checks them when the tk stream is on)
    c.tk_k = d["tk_k"].cast<int32_t>();
    if (d.contains("tk_by")) c.tk_by = d["tk_by"].cast<std::vector<int32_t>>();
    c.tk_min_tpm = get<double>(d, "tk_min_tpm", 0.0);
  }
  c.async_stats = get<int>(d, "async_stats", c.async_stats);
  c.device_join = get<int>(d, "device_join", c.device_join);
  c.join_table_bits = get<int>(d, "join_table_bits", c.join_table_bits);
  c.need_arena = get<uint32_t>(d, "need_arena", c.need_arena);
  c.join_chain_blocks = get<uint32_t>(d, "join_chain_blocks", c.join_chain_blocks);
  c.tx_ring_bytes = get<uint64_t>(d, "tx_ring_bytes", c.tx_ring_bytes);
  c.max_raw_services = get<uint32_t>(d, "max_raw_services", c.max_raw_services);
  return c;
}

ServiceOverride override_from(const py::dict& d) {
  ServiceOverride o;
  if (d.contains("thr")) {
    auto v = d["thr"].cast<std::vector<py::object>>();
    for (size_t i = 0; i < v.size() && i < MAX_LAGS; ++i)
      if (!v[i].is_none()) { o.has_thr[i] = true; o.thr[i] = v[i].cast<double>(); }
  }
  if (d.contains("infl")) {
    auto v = d["infl"].cast<std::vector<py::object>>();
    for (size_t i = 0; i < v.size() && i < MAX_LAGS; ++i)
      if (!v[i].is_none()) { o.has_infl[i] = true; o.infl[i] = v[i].cast<double>(); }
  }
  o.hard_max = get<double>(d, "hard_max", 0.0);
  o.suppressed = get<bool>(d, "suppressed", false);
  return o;
}

std::vector<Chunk> chunks_from(const std::vector<std::tuple<int32_t, uint64_t, uint64_t>>& v) {
  std::vector<Chunk> out;
  out.reserve(v.size());
  for (auto& t : v) out.push_back(Chunk{std::get<0>(t), std::get<1>(t), std::get<2>(t)});
  return out;
}

py::dict metrics_dict(const EngineMetrics& m) {
  py::dict d;
  d["batches"] = m.batches; d["bytes"] = m.bytes; d["lines"] = m.lines; d["events"] = m.events;
  d["tx"] = m.tx; d["tx_db"] = m.tx_db; d["tx_dropped"] = m.tx_dropped; d["rollovers"] = m.rollovers;
  d["alerts"] = m.alerts; d["alert_candidates"] = m.alert_candidates;
  d["alert_candidates_dropped"] = m.alert_candidates_dropped; d["released"] = m.released;
  d["staged_batches"] = m.staged_batches;
  d["t_join_shards_ms"] = m.t_join_shards_ms; d["t_merge_ms"] = m.t_merge_ms;
  d["t_shard_busy_ms"] = m.t_shard_busy_ms; d["t_shard_max_ms"] = m.t_shard_max_ms;
  d["t_out_ms"] = m.t_out_ms;
  d["t_lockstep_ms"] = m.t_lockstep_ms; d["t_lockstep_max_ms"] = m.t_lockstep_max_ms;
  d["t_lockstep_stats_ms"] = m.t_lockstep_stats_ms;
  d["db_copy_rows"] = m.db_copy_rows; d["db_copy_fallbacks"] = m.db_copy_fallbacks;
  d["t_stats_tx_ms"] = m.t_stats_tx_ms; d["t_rollover_ms"] = m.t_rollover_ms;
  d["t_format_ms"] = m.t_format_ms; d["t_release_ms"] = m.t_release_ms;
  d["sb_rows"] = m.sb_rows;
  d["tf_rows"] = m.tf_rows;
  d["po_rows"] = m.po_rows;
  d["ls_rows"] = m.ls_rows;
  d["ic_rows"] = m.ic_rows;
  d["ic_open_sb"] = m.ic_open[0]; d["ic_open_tf"] = m.ic_open[1]; d["ic_open_po"] = m.ic_open[2]; d["ic_open_ls"] = m.ic_open[3];
  d["formatted_bytes"] = m.formatted_bytes; d["lockstep_rollovers"] = m.lockstep_rollovers; d["format_fallbacks"] = m.format_fallbacks;
  d["t_parse_ms"] = m.t_parse_ms; d["t_join_ms"] = m.t_join_ms; d["t_stats_ms"] = m.t_stats_ms;
  d["t_total_ms"] = m.t_total_ms;
  d["series_overflow_tx"] = m.series_overflow_tx;
  d["spill_dropped"] = m.spill_dropped;
  d["nan_windows_clipped"] = m.nan_windows_clipped;
  d["tx_capacity_grows"] = m.tx_capacity_grows;
  d["spill_grows"] = m.spill_grows;
  d["spill_capacity"] = m.spill_capacity;
  d["rollover_latency_ms"] = m.rollover_latency_ms;
  return d;
}

py::dict counters_dict(const JoinCounters& c) {
  py::dict d;
  d["events"] = c.events; d["tx"] = c.tx; d["tx_db"] = c.tx_db; d["expired_partials"] = c.expired_partials;
  d["need_expired"] = c.need_expired; d["ejb_exit_unmatched"] = c.ejb_exit_unmatched;
  d["invalid_acct"] = c.invalid_acct; d["audit_errors"] = c.audit_errors; d["host_fallback"] = c.host_fallback;
  d["partial_overflow"] = c.partial_overflow; d["need_overflow"] = c.need_overflow; d["table_full"] = c.table_full;
  d["pool_exhausted"] = c.pool_exhausted; d["chain_partial_blocks"] = c.chain_partial_blocks;
  d["chain_need_blocks"] = c.chain_need_blocks; d["chain_logid_blocks"] = c.chain_logid_blocks;
  d["table_slots"] = c.table_slots; d["table_grows"] = c.table_grows; d["table_rebuilds"] = c.table_rebuilds; d["trims"] = c.trims;
  d["need_arena_entries"] = c.need_arena_entries; d["arena_grows"] = c.arena_grows;
  d["chain_pool_blocks"] = c.chain_pool_blocks; d["pool_grows"] = c.pool_grows;
  d["host_events"] = c.host_events;
  return d;
}

// Host join alone (CPU): events built by Python (apmbackend_amd.ops.parse_ref) are fed to the
// shards exactly as Engine::process_batch does after the GPU parse.
class JoinHarness {
 public:
  explicit JoinHarness(const py::dict& d) {
    cfg_.record_ttl_ms = get<double>(d, "record_ttl_ms", 120000);
    cfg_.acct_ttl_ms = get<double>(d, "acct_ttl_ms", 120000);
    cfg_.need_ttl_ms = get<double>(d, "need_ttl_ms", 30000);
    cfg_.tz = tz_from(d);
  }
  int32_t add_file(const std::string& path, int kind, const std::string& server) {
    int32_t sid;
    auto it = server_ids_.find(server);
    if (it == server_ids_.end()) {
      sid = (int32_t)servers_.size();
      servers_.push_back(server);
      server_ids_[server] = sid;
      shards_.emplace_back(new JoinShard(cfg_, &dict_, &files_, &servers_));
    } else {
      sid = it->second;
    }
    files_.push_back(FileInfo{path, sid, (uint8_t)kind});
    return (int32_t)files_.size() - 1;
  }
  // events: bytes of packed apm::Event; batch: the batch bytes; chunk_file: chunk -> file id
  std::vector<std::pair<std::string, std::string>> process(py::bytes events, py::bytes batch,
                                                           std::vector<int32_t> chunk_file, double now) {
    std::string ev = events;
    std::string by = batch;
    const Event* e = reinterpret_cast<const Event*>(ev.data());
    const size_t n = ev.size() / sizeof(Event);
    std::vector<std::pair<uint32_t, uint32_t>> range(shards_.size(), {0, 0});
    uint32_t i = 0;
    while (i < n) {
      const int32_t srv = files_[chunk_file[e[i].chunk]].server;
      uint32_t j = i;
      while (j < n && files_[chunk_file[e[j].chunk]].server == srv) ++j;
      range[srv] = {i, j};
      i = j;
    }
    std::vector<std::pair<std::string, std::string>> out;
    std::vector<TxOut> all;
    for (size_t s = 0; s < shards_.size(); ++s) {
      shards_[s]->out().clear();
      shards_[s]->begin_batch(now, batch_no_);
      if (range[s].second > range[s].first)
        shards_[s]->process(e + range[s].first, range[s].second - range[s].first, (const uint8_t*)by.data(),
                            chunk_file);
      for (auto& t : shards_[s]->out()) all.push_back(t);
    }
    std::stable_sort(all.begin(), all.end(), [](const TxOut& a, const TxOut& b) { return a.seq < b.seq; });
    for (auto& t : all)
      out.push_back({t.to_db ? "db_insert" : "transactions", shards_[t.server]->text().substr(t.line_off, t.line_len)});
    ++batch_no_;
    return out;
  }
  py::dict counters() {
    JoinCounters t;
    for (auto& s : shards_) {
      t.events += s->counters.events; t.tx += s->counters.tx; t.need_expired += s->counters.need_expired;
      t.expired_partials += s->counters.expired_partials; t.ejb_exit_unmatched += s->counters.ejb_exit_unmatched;
      t.invalid_acct += s->counters.invalid_acct; t.audit_errors += s->counters.audit_errors;
      t.host_fallback += s->counters.host_fallback; t.tx_db += s->counters.tx_db;
    }
    return counters_dict(t);
  }

 private:
  JoinConfig cfg_;
  Dictionary dict_;
  std::vector<FileInfo> files_;
  std::vector<std::string> servers_;
  std::unordered_map<std::string, int32_t> server_ids_;
  std::vector<std::unique_ptr<JoinShard>> shards_;
  uint64_t batch_no_ = 0;
};

}  // namespace

extern "C" const char* apm_csrc_hash();  // build/native/provenance.cpp (generated at build time)

PYBIND11_MODULE(_apm_native, m) {
  m.doc() = "apm-mi355x native runtime (HIP kernels for gfx950 + host runtime)";
  m.def("csrc_hash", []() { return std::string(apm_csrc_hash()); });
  // process-wide live GPU resources over every owner (runtime/hipres.h): leak checks in the tests
  m.def("live_resources", []() {
    const LiveResources& L = live_resources();
    py::dict d;
    d["device_blocks"] = L.device_blocks.load();
    d["device_bytes"] = L.device_bytes.load();
    d["pinned_blocks"] = L.pinned_blocks.load();
    d["pinned_bytes"] = L.pinned_bytes.load();
    d["events"] = L.events.load();
    d["streams"] = L.streams.load();
    return d;
  });
  m.attr("EVENT_SIZE") = (int)sizeof(Event);
  m.def("hash_bytes", [](py::bytes b, uint64_t seed) {
    const std::string s = b;
    return hash_bytes(s.data(), s.size(), seed);
  }, py::arg("data"), py::arg("seed") = kHashSeed);
  m.attr("NSLOT_MIN") = NSLOT_MIN;
  m.attr("MAX_LAGS") = MAX_LAGS;

  // TCP host transport on host buffers (CPU tests of the multi-process collective path)
  py::class_<Collective>(m, "HostCollective")
      .def(py::init([](const std::string& addr, int port, int n, int rank, double timeout_ms) {
             py::gil_scoped_release rel;
             return make_host_collective(addr, port, n, rank, timeout_ms).release();
           }),
           py::arg("addr"), py::arg("port"), py::arg("nranks"), py::arg("rank"), py::arg("timeout_ms") = 30000.0)
      .def("all_reduce", [](Collective& c, std::vector<double> v, bool max) {
        py::gil_scoped_release rel;
        return c.all_reduce_host(v, max);
      }, py::arg("values"), py::arg("max") = false)
      .def("all_gather", [](Collective& c, py::bytes b) {
        std::string s = b;
        std::vector<uint8_t> v(s.begin(), s.end()), out;
        { py::gil_scoped_release rel; out = c.all_gather_host(v); }
        return py::bytes((const char*)out.data(), out.size());
      })
      .def("abort", &Collective::abort)
      .def("aborted", &Collective::aborted)
      .def_property_readonly("rank", &Collective::rank)
      .def_property_readonly("nranks", &Collective::nranks);
  py::class_<LocalGroup, std::shared_ptr<LocalGroup>>(m, "LocalCollGroup")
      .def(py::init([](int n, double timeout_ms) { return make_local_group(n, timeout_ms); }), py::arg("n"),
           py::arg("timeout_ms") = 120000.0);

  py::class_<Engine>(m, "Engine")
      .def(py::init([](const py::dict& d) { return new Engine(config_from(d)); }))
      .def("add_file", &Engine::add_file)
      .def("add_server", &Engine::add_server)
      .def("set_override", [](Engine& e, const std::string& svc, const py::dict& d) { e.set_override(svc, override_from(d)); })
      .def("clear_overrides", &Engine::clear_overrides)
      .def("refresh_series_settings", &Engine::refresh_series_settings)
      .def("stage_reconfig", [](Engine& e, const py::dict& ecfg, const py::dict& overrides, uint64_t gen) {
        const EngineConfig c = config_from(ecfg);
        ReconfigSpec r;
        r.gen = gen;
        r.n_lags = c.n_lags;
        for (int l = 0; l < MAX_LAGS; ++l) {
          r.lags[l] = c.lags[l]; r.thr[l] = c.thr[l]; r.infl[l] = c.infl[l]; r.lag_suppressed[l] = c.lag_suppressed[l];
        }
        r.alert_window = c.alert_window; r.alert_threshold = c.alert_threshold; r.both_only = c.both_only;
        r.hard_min_ms = c.hard_min_ms; r.hard_min_tpm = c.hard_min_tpm; r.hard_max_ms = c.hard_max_ms;
        r.cooldown_ms = c.cooldown_ms;
        r.interval_len = c.interval_len; r.window = c.window; r.buffer = c.buffer;
        for (auto kv : overrides) r.overrides[kv.first.cast<std::string>()] = override_from(kv.second.cast<py::dict>());
        e.stage_reconfig(r);
      }, py::arg("ecfg"), py::arg("overrides"), py::arg("gen"))
      .def("reconfig_info", [](Engine& e) {
        py::dict d;
        d["applied_gen"] = e.reconfig_applied_gen(); d["applied"] = e.reconfigs_applied();
        d["lag_set_changes"] = e.lag_set_changes();
        d["window_changes"] = e.window_changes();
        d["ring_slots"] = e.ring_slots();
        d["ring_grows"] = e.ring_grows();
        return d;
      })
      .def("lag_values", &Engine::lag_values)
      .def("cache_stats", [](Engine& e, bool drain) {
        std::vector<uint64_t> v;
        { py::gil_scoped_release rel; v = e.cache_stats(drain); }
        py::dict d;
        if (v.size() == 6) {
          d["slots"] = v[0]; d["occupied"] = v[1]; d["acct"] = v[2]; d["record"] = v[3]; d["partials"] = v[4];
          d["need"] = v[5];
        }
        return d;
      }, py::arg("drain") = true)
      .def("process_batch",
           [](Engine& e, py::buffer buf, const std::vector<std::tuple<int32_t, uint64_t, uint64_t>>& chunks,
              double now) {
             py::buffer_info bi = buf.request();
             const uint8_t* p = (const uint8_t*)bi.ptr;
             const uint64_t n = (uint64_t)(bi.size * bi.itemsize);
             auto ch = chunks_from(chunks);
             py::gil_scoped_release rel;
             e.process_batch(p, n, ch, now);
           },
           py::arg("buf"), py::arg("chunks"), py::arg("now") = -1.0)
      .def("process_batch_ptr",
           [](Engine& e, uintptr_t ptr, uint64_t n, const std::vector<std::tuple<int32_t, uint64_t, uint64_t>>& chunks,
              double now, uintptr_t next_ptr, uint64_t next_n,
              const std::vector<std::tuple<int32_t, uint64_t, uint64_t>>& next_chunks) {
             auto ch = chunks_from(chunks);
             auto nch = chunks_from(next_chunks);
             py::gil_scoped_release rel;
             e.process_batch((const uint8_t*)ptr, n, ch, now, next_ptr ? (const uint8_t*)next_ptr : nullptr, next_n,
                             next_ptr ? &nch : nullptr);
           },
           py::arg("ptr"), py::arg("n"), py::arg("chunks"), py::arg("now") = -1.0, py::arg("next_ptr") = 0,
           py::arg("next_n") = 0,
           py::arg("next_chunks") = std::vector<std::tuple<int32_t, uint64_t, uint64_t>>())
      .def("stage_batch_ptr",
           [](Engine& e, uintptr_t ptr, uint64_t n) {
             py::gil_scoped_release rel;
             e.stage_batch((const uint8_t*)ptr, n);
           },
           py::arg("ptr"), py::arg("n"))
      .def("process_tx_lines", [](Engine& e, py::bytes b, double now) {
             std::string v = b;
             py::gil_scoped_release rel;
             e.process_tx_lines(v, now);
           }, py::arg("blob"), py::arg("now") = -1.0)
      .def("take", &Engine::take, py::call_guard<py::gil_scoped_release>())
      .def("flush", &Engine::flush, py::call_guard<py::gil_scoped_release>())
      .def("dump_state", [](Engine& e, const std::string& path, const std::string& reason) {
        py::gil_scoped_release rel;
        return e.dump_state(path, reason);
      })
      .def("save_state", [](Engine& e, const std::string& path, py::bytes extra) {
             std::string x = extra;
             py::gil_scoped_release rel;
             return e.save_state(path, x);
           }, py::arg("path"), py::arg("extra") = py::bytes(""))
      .def("checkpoint_async", [](Engine& e, const std::string& prefix, py::bytes extra, bool force_base) {
             std::string x = extra;
             py::gil_scoped_release rel;
             return e.checkpoint_async(prefix, x, force_base);
           }, py::arg("prefix"), py::arg("extra") = py::bytes(""), py::arg("force_base") = false)
      .def("checkpoint_wait", &Engine::checkpoint_wait, py::call_guard<py::gil_scoped_release>())
      .def("checkpoint_info", [](Engine& e) {
        const CheckpointInfo c = e.checkpoint_info();
        py::dict d;
        d["busy"] = c.busy; d["done"] = c.done; d["skipped"] = c.skipped; d["sync_fallbacks"] = c.sync_fallbacks;
        d["chain_len"] = c.chain_len; d["last_base"] = c.last_base; d["last_stall_ms"] = c.last_stall_ms;
        d["last_write_ms"] = c.last_write_ms; d["last_bytes"] = c.last_bytes; d["stage_bytes"] = c.stage_bytes;
        d["last_deferred_bytes"] = c.last_deferred_bytes;
        d["streamed"] = c.streamed; d["streamed_live_rows"] = c.streamed_live_rows;
        d["side_rows"] = c.side_rows; d["guard_stalls"] = c.guard_stalls; d["stage_cap"] = c.stage_cap;
        d["last_ring_rows"] = c.last_ring_rows;
        return d;
      })
      .def("export_series", &Engine::export_series, py::call_guard<py::gil_scoped_release>())
      .def("import_series", &Engine::import_series, py::call_guard<py::gil_scoped_release>())
      .def("export_buckets", [](Engine& e) {
        BucketDump d;
        { py::gil_scoped_release rel; d = e.export_buckets(); }
        return py::make_tuple(d.latest, d.series, d.bucket, d.count, d.values);
      })
      .def("import_buckets", &Engine::import_buckets, py::call_guard<py::gil_scoped_release>())
      .def("export_history", [](Engine& e, int lag_idx, int32_t lo, int32_t hi) {
        std::vector<int32_t> len;
        std::vector<double> vals;
        { py::gil_scoped_release rel; e.export_history(lag_idx, lo, hi, len, vals); }
        return py::make_tuple(len, py::bytes((const char*)vals.data(), vals.size() * 8));
      })
      .def("import_history", [](Engine& e, int lag_idx, const std::vector<int32_t>& series,
                                const std::vector<int32_t>& len, py::bytes vals) {
        std::string b = vals;
        std::vector<double> v(b.size() / 8);
        std::memcpy(v.data(), b.data(), v.size() * 8);
        py::gil_scoped_release rel;
        e.import_history(lag_idx, series, len, v);
      })
      .def("export_lag_settings", &Engine::export_lag_settings)
      .def("export_pending", &Engine::export_pending, py::call_guard<py::gil_scoped_release>())
      .def("import_pending", &Engine::import_pending, py::call_guard<py::gil_scoped_release>())
      .def("export_cooldowns", &Engine::export_cooldowns)
      .def("import_cooldowns", &Engine::import_cooldowns)
      .def("export_alert_counters", &Engine::export_alert_counters)
      .def("import_alert_counters", &Engine::import_alert_counters)
      .def("cooldown_by_service", &Engine::cooldown_by_service)
      .def("set_trace", &Engine::set_trace)
      .def("take_trace", [](Engine& e) {
        std::vector<TraceEvent> t;
        { py::gil_scoped_release rel; t = e.take_trace(); }
        py::list out;
        for (auto& x : t) out.append(py::make_tuple(std::string(x.name), x.t0_ms, x.t1_ms, x.tid, x.batch));
        return out;
      })
      .def("set_server_context", &Engine::set_server_context, py::arg("server"), py::arg("ts_ms"),
           py::arg("gauges"), py::arg("host_load") = 0.0)
      .def("load_state", [](Engine& e, const std::string& path) {
             std::string x;
             { py::gil_scoped_release rel; x = e.load_state(path); }
             return py::bytes(x);
           })
      .def("take_bytes", [](Engine& e, const std::string& k) {
        std::string b;
        { py::gil_scoped_release rel; b = e.take_bytes(k); }
        return py::bytes(b);
      })
      .def("set_sink_fd", &Engine::set_sink_fd, py::call_guard<py::gil_scoped_release>())
      .def("set_fs_copy", &Engine::set_fs_copy, py::call_guard<py::gil_scoped_release>())
      .def("set_db_copy", &Engine::set_db_copy, py::call_guard<py::gil_scoped_release>())
      .def("sink_bytes", &Engine::sink_bytes)
      .def("lane_cpus", &Engine::lane_cpus)
      .def("last_events", [](Engine& e) { return py::bytes(e.last_events()); })
      .def("warm_history", &Engine::warm_history)
      .def("metrics", [](Engine& e, bool drain) {
        // drain=False: the counters as they stand (a batch or two behind), without draining the
        // pipeline -- the periodic stat lines must not stall ingest
        EngineMetrics m;
        { py::gil_scoped_release rel; m = drain ? e.metrics() : e.metrics_nowait(); }
        return metrics_dict(m);
      }, py::arg("drain") = true)
      .def("join_counters", [](Engine& e) { return counters_dict(e.join_counters()); })
      .def("n_series", &Engine::n_series)
      .def("n_services", &Engine::n_services)
      .def("services", &Engine::services)
      .def("files", [](Engine& e) {
        std::vector<std::tuple<std::string, int, std::string>> r;
        for (auto& f : e.files()) r.emplace_back(f.path, (int)f.kind, e.servers()[f.server]);
        return r;
      })
      .def("servers", &Engine::servers)
      .def("watermark", &Engine::watermark)
      .def("batch_no", &Engine::batch_no)
      .def("device_bytes", &Engine::device_bytes)
      .def("trim_device_memory", &Engine::trim_device_memory, py::call_guard<py::gil_scoped_release>())
      .def("stream_handle", [](Engine& e) { return (uintptr_t)e.stream(); })
      .def("comm_stream_handle", [](Engine& e) { return (uintptr_t)e.comm_stream(); })
      .def_static("fleet_unique_id", []() {
        auto v = Engine::fleet_unique_id();
        return py::bytes((const char*)v.data(), v.size());
      })
      .def("fleet_init", [](Engine& e, py::bytes uid, int nranks, int rank, int32_t cap, py::bytes clock_uid) {
        std::string s = uid, c = clock_uid;
        std::vector<uint8_t> v(s.begin(), s.end()), cv(c.begin(), c.end());
        py::gil_scoped_release rel;
        e.fleet_init(v, cv, nranks, rank, cap);
      }, py::arg("uid"), py::arg("nranks"), py::arg("rank"), py::arg("cap"), py::arg("clock_uid") = py::bytes(""))
      .def("fleet_merged", [](Engine& e) {
        std::vector<double> v;
        { py::gil_scoped_release rel; v = e.fleet_merged(); }
        return py::bytes((const char*)v.data(), v.size() * 8);
      })
      .def("fleet_rounds", &Engine::fleet_rounds)
      .def("gram_tail_series", [](Engine& e) { return e.last_gram_tail_; })
      .def("node_metrics", &Engine::node_metrics)
      .def("fleet_slot_names", [](Engine& e) { return e.fleet_slot_names(); })
      .def("fleet_info", [](Engine& e) {
        py::dict d;
        const auto i = e.fleet_info();
        d["slots"] = i[0]; d["registry_rounds"] = i[1]; d["registry_overflow"] = i[2]; d["fb_rows"] = i[3]; d["nranks"] = i[4];
        return d;
      })
      .def("fleet_init_local", [](Engine& e, std::shared_ptr<LocalGroup> g, int rank, int32_t cap, bool lockstep) {
        py::gil_scoped_release rel;
        e.fleet_init_local(std::move(g), rank, cap, lockstep);
      }, py::arg("group"), py::arg("rank"), py::arg("cap"), py::arg("lockstep") = true)
      .def("fleet_init_host", [](Engine& e, const std::string& addr, int port, int nranks, int rank, int32_t cap,
                                 bool lockstep) {
        py::gil_scoped_release rel;
        e.fleet_init_host(addr, port, nranks, rank, cap, lockstep);
      }, py::arg("addr"), py::arg("port"), py::arg("nranks"), py::arg("rank"), py::arg("cap"), py::arg("lockstep") = true)
      .def("set_server_index", &Engine::set_server_index)
      .def("node_drain", [](Engine& e) { py::gil_scoped_release rel; e.node_drain(); })
      .def("pack_service_moments", [](Engine& e, uintptr_t dst, int32_t cap, bool atomic_path) {
        e.pack_service_moments((double*)dst, cap, e.comm_stream(), atomic_path);
      }, py::arg("dst"), py::arg("cap"), py::arg("atomic_path") = false)
      .def("winpcts", [](Engine& e) {
        // per series (m, nan, [sum2 per configured percentile]) of the last rollover's K16 value pass
        std::vector<int32_t> m, nan;
        std::vector<long long> sum2;
        e.download_winpcts(m, nan, sum2);
        const size_t nq = m.empty() ? 0 : sum2.size() / m.size();
        py::list out;
        for (size_t i = 0; i < m.size(); ++i) {
          py::list v;
          for (size_t j = 0; j < nq; ++j) v.append(py::int_(sum2[i * nq + j]));
          out.append(py::make_tuple(m[i], nan[i], v));
        }
        return out;
      })
      .def("slo_counts", [](Engine& e) {
        // per series (m, nan, [c_j per threshold of its class]) of the last rollover's K17 value pass
        std::vector<SloRec> rec;
        std::vector<int32_t> nthr;
        e.download_slo(rec, nthr);
        py::list out;
        for (size_t i = 0; i < rec.size(); ++i) {
          py::list v;
          for (int32_t j = 0; j < nthr[i]; ++j) v.append(py::int_(rec[i].c[j]));
          out.append(py::make_tuple(rec[i].m, rec[i].nan, v));
        }
        return out;
      })
      .def("svcwins", [](Engine& e) {
        // per service (name, servers, m, nan, sum, [sum2 per configured percentile]) of the last
        // rollover's K19 value pass, in the order of each service's first series in emission order
        std::vector<std::string> names;
        std::vector<SvcRec> rec;
        e.download_svcwins(names, rec);
        const int nq = e.svc_nq();
        py::list out;
        for (size_t i = 0; i < rec.size(); ++i) {
          py::list v;
          for (int j = 0; j < nq && rec[i].m > 0; ++j) v.append(py::int_(rec[i].sum2[j]));
          out.append(py::make_tuple(names[i], rec[i].servers, rec[i].m, rec[i].nan, py::int_(rec[i].sum), v));
        }
        return out;
      })
      .def("recents", [](Engine& e) {
        // per series id of the last rollover's K20 value pass: None for a series without rows, else a
        // list over the configured spans of (m, nan, sum, [sum2 per configured percentile])
        std::vector<RecentRec> rec;
        std::vector<uint8_t> has;
        e.download_recents(rec, has);
        const int ns = e.rw_nspan(), nq = e.rw_nq();
        py::list out;
        for (size_t s = 0; s < has.size(); ++s) {
          if (!has[s]) { out.append(py::none()); continue; }
          py::list spans;
          for (int k = 0; k < ns; ++k) {
            const RecentRec& r = rec[s * (size_t)ns + (size_t)k];
            py::list v;
            for (int j = 0; j < nq && r.m > 0; ++j) v.append(py::int_(r.sum2[j]));
            spans.append(py::make_tuple(r.m, r.nan, py::int_(r.sum), v));
          }
          out.append(spans);
        }
        return out;
      })
      .def("burns", [](Engine& e) {
        // per series id of the last rollover's K21 value pass: None for a series without an st row or
        // an objective, else (m, bad, nan, [(m_k, bad_k) per configured rule], fired mask)
        std::vector<BurnRec> rec;
        std::vector<uint8_t> has;
        e.download_burns(rec, has);
        const int nr = e.sb_nrule();
        py::list out;
        for (size_t s = 0; s < has.size(); ++s) {
          if (!has[s]) { out.append(py::none()); continue; }
          const BurnRec& r = rec[s];
          py::list rules;
          for (int j = 0; j < nr; ++j) rules.append(py::make_tuple(r.mk[j], r.badk[j]));
          out.append(py::make_tuple(r.m, r.bad, r.nan, rules, r.fired));
        }
        return out;
      })
      .def("traffic", [](Engine& e) {
        // per series id of the last rollover's K22 value pass: None for a series without an st row or
        // a class, else (n, [(B, R, med2, mad4, verdict "D" / "S" / "N") per configured rule])
        std::vector<TrafficRec> rec;
        std::vector<uint8_t> has;
        e.download_traffic(rec, has);
        const int nr = e.tf_nrule();
        py::list out;
        for (size_t s = 0; s < has.size(); ++s) {
          if (!has[s]) { out.append(py::none()); continue; }
          const TrafficRec& r = rec[s];
          py::list rules;
          for (int j = 0; j < nr; ++j) {
            const int v = (r.verdict >> (2 * j)) & 3;
            rules.append(py::make_tuple(r.B[j], r.R[j], r.med2[j], r.mad4[j], v == TF_D ? "D" : v == TF_S ? "S" : "N"));
          }
          out.append(py::make_tuple(r.n, rules));
        }
        return out;
      })
      .def("peers", [](Engine& e) {
        // per series id of the last rollover's K23 value pass: None for a series without an st row,
        // with class 0 or below minSamples, else (m, x, E, X2, D4, verdict "H" / "L" / "N")
        std::vector<PeerRec> rec;
        e.download_peers(rec);
        py::list out;
        for (const PeerRec& r : rec) {
          if (r.m == 0) { out.append(py::none()); continue; }
          out.append(py::make_tuple(r.m, (int64_t)r.x, r.E, (int64_t)r.X2, (int64_t)r.D4,
                                    r.verdict == PO_H ? "H" : r.verdict == PO_L ? "L" : "N"));
        }
        return out;
      })
      .def("shifts", [](Engine& e) {
        // per series id of the last rollover's K24 value pass: None for a series without an st row or
        // a class, else (n, [(mB, nanB, mR, nanR, a, b, T2, X2, verdict "U" / "D" / "N") per configured rule])
        std::vector<ShiftRec> rec;
        std::vector<uint8_t> has;
        e.download_shifts(rec, has);
        const int nr = e.ls_nrule();
        py::list out;
        for (size_t s = 0; s < has.size(); ++s) {
          if (!has[s]) { out.append(py::none()); continue; }
          const ShiftRec& r = rec[s];
          py::list rules;
          for (int j = 0; j < nr; ++j) {
            const int v = (r.verdict >> (2 * j)) & 3;
            rules.append(py::make_tuple(r.mB[j], r.nanB[j], r.mR[j], r.nanR[j], r.a[j], r.b[j], (int64_t)r.T2[j],
                                        (int64_t)r.X2[j], v == LS_U ? "U" : v == LS_D ? "D" : "N"));
          }
          out.append(py::make_tuple(r.n, rules));
        }
        return out;
      })
      .def("incidents", [](Engine& e) {
        // per series id the K25 state: None for a series with every configured source closed and
        // every run 0, else per source (sb, tf, po, ls) None when it is not configured or
        // (code0 -- "" when closed, since_ts, age, hot_run, clear_run)
        std::vector<IncidentState> st;
        e.download_incidents(st);
        py::list out;
        for (size_t s = 0; s * 4 < st.size(); ++s) {
          bool any = false;
          py::list per;
          for (int k = 0; k < 4; ++k) {
            const IncidentState& x = st[s * 4 + k];
            if (!e.ic_source(k)) { per.append(py::none()); continue; }
            any = any || x.code0 != 0 || x.hot_run != 0 || x.clear_run != 0;
            per.append(py::make_tuple(x.code0 ? std::string(1, (char)x.code0) : std::string(), (int64_t)x.since_ts,
                                      (uint64_t)x.age, (int)x.hot_run, (int)x.clear_run));
          }
          if (any) out.append(py::tuple(per)); else out.append(py::none());
        }
        return out;
      })
      .def("leaderboard", [](Engine& e) {
        // the last rollover's K18 records: (board, rank, series id, tpm, avg, p75, p95), raw doubles
        std::vector<std::tuple<int32_t, int32_t, int32_t, WinStat>> rows;
        {
          py::gil_scoped_release rel;
          rows = e.leaderboard();
        }
        static const char* key_name[4] = {"tpm", "average", "per75", "per95"};
        py::list out;
        for (const auto& r : rows) {
          const WinStat& w = std::get<3>(r);
          out.append(py::make_tuple(key_name[std::get<0>(r) & 3], std::get<1>(r), std::get<2>(r),
                                    w.tpm, w.avg, w.p75, w.p95));
        }
        return out;
      })
      .def("winstats", [](Engine& e) {
        std::vector<WinStat> w;
        e.download_winstats(w);
        std::vector<std::tuple<int, int, double, double, double, double>> out;
        for (int i = 0; i < e.n_series(); ++i) out.emplace_back(w[i].active, w[i].n, w[i].tpm, w[i].avg, w[i].p75, w[i].p95);
        return out;
      });

  py::class_<JoinHarness>(m, "JoinHarness")
      .def(py::init<const py::dict&>())
      .def("add_file", &JoinHarness::add_file)
      .def("process", &JoinHarness::process)
      .def("counters", &JoinHarness::counters);

  m.def("alloc_pinned", &Engine::alloc_pinned);
  // re-shard merge of old ranks' checkpoints (runtime/merge.h), host only
  m.def("checkpoint_batches", &checkpoint_batches, py::arg("path"));
  m.def("merge_checkpoints", [](const std::vector<std::string>& inputs, const std::vector<std::string>& servers,
                                const std::string& out, const py::bytes& extra, uint64_t batch_no) {
    MergeResult r;
    const std::string ex = extra;
    {
      py::gil_scoped_release rel;
      r = merge_checkpoints(inputs, servers, out, ex, batch_no);
    }
    py::dict d;
    d["batch_no"] = r.batch_no; d["series"] = r.series; d["keys"] = r.keys; d["need"] = r.need;
    d["pending"] = r.pending; d["raw"] = r.raw; d["files"] = r.files; d["servers"] = r.servers;
    d["used"] = r.used;
    py::list ex_l;
    for (const auto& e : r.extras) ex_l.append(py::bytes(e));
    d["extras"] = ex_l;
    return d;
  }, py::arg("inputs"), py::arg("servers"), py::arg("out"), py::arg("extra") = py::bytes(""), py::arg("batch_no") = 0);
  m.def("free_pinned", &Engine::free_pinned);
  m.def("memcpy_to", [](uintptr_t dst, py::bytes b, uint64_t off) {
    std::string_view v = b;
    std::memcpy((char*)dst + off, v.data(), v.size());
  });
  m.def("copy_encode", [](py::bytes blob) {
    // wire lines -> Postgres COPY text per table type (runtime/sinks.py is the Python twin)
    std::string b = blob;
    std::string out[16];
    int64_t counts[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    {
      py::gil_scoped_release rel;
      copyenc::encode_blob(b, out, counts);
    }
    py::dict d;
    const char* names[16] = {"tx", "fs", "al", "jx", "fb", "lh", "wp", "sl", "tk", "sv", "rw", "sb", "tf", "po", "ls", "ic"};
    for (int k = 0; k < 16; ++k) d[names[k]] = py::make_tuple(py::bytes(out[k]), counts[k]);
    return d;
  });
  m.def("set_blocking_sync", [](int device) {
    // before anything else creates the device's runtime state (bench.py, ranks sharing a GPU):
    // stream / event waits block instead of spinning
    HIP_OK(hipSetDevice(device));
    return hipSetDeviceFlags(hipDeviceScheduleBlockingSync) == hipSuccess;
  });
  m.def("release_bench", [](int64_t n, int iters, uint64_t seed) {
    std::vector<double> r;
    {
      py::gil_scoped_release rel;
      r = apm_release_bench(n, iters, seed);
    }
    py::dict d;
    const char* k[7] = {"lines", "wire_bytes", "copy_bytes", "gather_us", "txcopy_us", "txcopy_write_us", "fallbacks"};
    for (int i = 0; i < 7; ++i) d[k[i]] = r[(size_t)i];
    return d;
  }, py::arg("n") = 60000, py::arg("iters") = 20, py::arg("seed") = 1);
  m.def("dj_rebuild_selftest", [](uint32_t cap, double load, double dead, uint64_t seed, bool copy) {
    std::vector<double> r;
    {
      py::gil_scoped_release rel;
      r = apm_dj_rebuild_selftest(cap, load, dead, seed, copy);
    }
    py::dict d;
    const char* k[8] = {"live", "want_live", "found", "dead_left", "occupied", "probes_before", "probes_after", "us"};
    for (int i = 0; i < 8; ++i) d[k[i]] = r[(size_t)i];
    return d;
  }, py::arg("cap"), py::arg("load") = 0.55, py::arg("dead") = 0.3, py::arg("seed") = 1, py::arg("copy") = false);
  m.def("txcopy_lines", [](py::bytes blob) {
    // newline-terminated wire tx lines -> (COPY rows from the GPU encoder, fallback count)
    std::string b = blob;
    std::vector<uint64_t> off{0};
    for (size_t i = 0; i < b.size(); ++i)
      if (b[i] == '\n') off.push_back(i + 1);
    if (off.back() != b.size()) throw std::invalid_argument("txcopy_lines: the last line needs its newline");
    const int64_t n = (int64_t)off.size() - 1;
    std::string rows;
    int fb = 0;
    {
      py::gil_scoped_release rel;
      uint64_t cap = 1;
      while (cap < b.size() + 64) cap <<= 1;
      char* d = nullptr;
      HIP_OK(hipMalloc(&d, cap));
      HIP_OK(hipMemset(d, 0, cap));
      HIP_OK(hipMemcpy(d, b.data(), b.size(), hipMemcpyHostToDevice));
      fb = n ? apm_txcopy_lines(d, off.data(), n, rows) : 0;
      HIP_OK(hipFree(d));
    }
    return py::make_tuple(py::bytes(rows), fb);
  });
  m.def("flatmap_selftest", [](int n_ops, uint64_t seed, int key_space) {
    // randomized FlatMap / SmallVec vs std containers (CPU test of the join's data structures)
    FlatMap<int64_t> fm(16);
    std::unordered_map<uint64_t, int64_t> ref;
    uint64_t x = seed | 1;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int i = 0; i < n_ops; ++i) {
      const uint64_t k = 1 + rnd() % (uint64_t)key_space;
      const int op = (int)(rnd() % 3);
      if (op == 0) { fm[k] = (int64_t)i; ref[k] = i; }
      else if (op == 1) { if (fm.erase(k) != (ref.erase(k) == 1)) return false; }
      else {
        int64_t* v = fm.find(k);
        auto it = ref.find(k);
        if ((v != nullptr) != (it != ref.end())) return false;
        if (v && *v != it->second) return false;
      }
      if (fm.size() != ref.size()) return false;
    }
    SmallVec<int, 2> sv;
    std::vector<int> rv;
    for (int i = 0; i < 2000; ++i) {
      if (rnd() % 3 || rv.empty()) { sv.push_back(i); rv.push_back(i); }
      else {
        const size_t j = rnd() % rv.size();
        sv.erase(sv.begin() + j);
        rv.erase(rv.begin() + j);
      }
      if (sv.size() != rv.size() || !std::equal(rv.begin(), rv.end(), sv.begin())) return false;
    }
    return true;
  });
  m.def("gpu_to_fixed", [](const std::vector<double>& xs, int f, const std::string& mode) {
    // K12 number printer on the device (test hook), per value: "nf" nf(x, f), "json" / "copy"
    // js_fixed(x, f) as a JSON number / a COPY field
    const int md = mode == "nf" ? 0 : mode == "json" ? 1 : mode == "copy" ? 2 : -1;
    if (md < 0) throw std::invalid_argument("gpu_to_fixed: mode is nf, json or copy");
    if (f != 1 && f != 2) throw std::invalid_argument("gpu_to_fixed: f is 1 or 2");
    const int n = (int)xs.size();
    std::vector<char> h((size_t)n * 32);
    DevMem dx((size_t)n * 8), dout(h.size());
    HIP_OK(hipMemcpy(dx.p, xs.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    apm_format_fixed_batch(dx.as<double>(), n, f, md, dout.as<char>(), 0);
    HIP_OK(hipMemcpy(h.data(), dout.p, h.size(), hipMemcpyDeviceToHost));
    std::vector<std::string> r;
    for (int i = 0; i < n; ++i) r.emplace_back(h.data() + (size_t)i * 32);
    return r;
  }, py::arg("xs"), py::arg("f"), py::arg("mode") = "nf");
  m.def("gpu_fleet_rows", [](const std::vector<double>& moments, const std::vector<std::string>& names,
                             const std::vector<int32_t>& lag_values, int32_t slot_lo, int32_t n_slots, bool copy,
                             int64_t edge_ts) {
    // the fb row formatter alone (test hook): moments [slot][lag][stat]{n, sum, sum of squares} of
    // every slot in `names`, rows of slots [slot_lo, slot_lo + n_slots)
    const int n_lags = (int)lag_values.size();
    if (n_lags < 1 || n_lags > MAX_LAGS) throw std::invalid_argument("gpu_fleet_rows: 1..MAX_LAGS lag values");
    if (slot_lo < 0 || n_slots < 0 || (size_t)slot_lo + (size_t)n_slots > names.size())
      throw std::invalid_argument("gpu_fleet_rows: slots outside names");
    if (moments.size() != names.size() * (size_t)n_lags * NSTAT * 3)
      throw std::invalid_argument("gpu_fleet_rows: moments hold names x lags x 3 x 3 doubles");
    std::vector<int32_t> nm;
    std::string chars;
    size_t longest = 0;
    for (const std::string& s : names) {
      nm.push_back((int32_t)chars.size());
      nm.push_back((int32_t)s.size());
      chars += s;
      longest = std::max(longest, s.size());
    }
    const int32_t rows = n_slots * n_lags;
    const uint32_t blocks = apm_fleet_format_blocks(rows);
    const size_t cap = apm_fleet_out_bound(rows, longest);
    // `cap` holds any row the grammar allows (apm_fleet_out_bound), so the kernels cannot write
    // past it; the check of `total` below only guards the copy back
    DevMem m_mom(moments.size() * 8), m_nm(nm.size() * 4), m_out(cap);
    DevMem m_chars(chars.size() + 64);                // (16-byte over-reading name loads)
    DevMem m_status((size_t)blocks * 8 + 64);         // [blocks] wave totals, then {total, fallback}
    double* d_mom = m_mom.as<double>();
    int32_t* d_nm = m_nm.as<int32_t>();
    char *d_chars = m_chars.as<char>(), *d_out = m_out.as<char>();
    unsigned long long* d_status = m_status.as<unsigned long long>();
    HIP_OK(hipMemset(d_chars, 0, chars.size() + 64));
    HIP_OK(hipMemset(d_status, 0, (size_t)blocks * 8 + 64));
    HIP_OK(hipMemcpy(d_mom, moments.data(), moments.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_nm, nm.data(), nm.size() * 4, hipMemcpyHostToDevice));
    if (!chars.empty()) HIP_OK(hipMemcpy(d_chars, chars.data(), chars.size(), hipMemcpyHostToDevice));
    FleetFormatArgs fa{};
    fa.moments = d_mom;
    fa.names = reinterpret_cast<const int2*>(d_nm);
    fa.chars = d_chars;
    fa.slot_lo = slot_lo;
    fa.n_slots = n_slots;
    fa.n_lags = n_lags;
    std::vector<int> order(n_lags);
    for (int l = 0; l < n_lags; ++l) order[l] = l;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return lag_values[a] < lag_values[b]; });
    for (int l = 0; l < n_lags; ++l) { fa.lag_order[l] = order[l]; fa.lag_value[l] = lag_values[l]; }
    fa.edge_ts = edge_ts;
    fa.copy = copy ? 1 : 0;
    fa.ts_len = Engine::pg_timestamp(edge_ts, fa.ts);
    fa.status = d_status;
    fa.total = reinterpret_cast<uint32_t*>(d_status + blocks);
    fa.out = d_out;
    fa.fallback = reinterpret_cast<int32_t*>(d_status + blocks) + 1;
    apm_fleet_format(&fa, 0);
    uint32_t total = 0;
    HIP_OK(hipMemcpy(&total, fa.total, 4, hipMemcpyDeviceToHost));
    if (total > cap) throw std::runtime_error("gpu_fleet_rows: rows longer than the output bound");
    std::string out(total, '\0');
    if (total) HIP_OK(hipMemcpy(&out[0], d_out, total, hipMemcpyDeviceToHost));
    return py::bytes(out);
  }, py::arg("moments"), py::arg("names"), py::arg("lag_values"), py::arg("slot_lo"), py::arg("n_slots"),
     py::arg("copy"), py::arg("edge_ts"));
  m.def("js_to_fixed", [](double x, int f) { return js::to_fixed(x, f); });
  m.def("js_num_str", [](double x) { return js::num_str(x); });
  m.def("js_parse_int", [](const std::string& s) { return js::parse_int(s); });
  m.def("js_convert_date", [](const std::string& s, const py::dict& tz) {
    double v;
    TzTable t = tz_from(tz);
    if (!js::convert_date(s, t, v)) return py::object(py::none());
    return py::object(py::float_(v));
  });
  m.def("js_round_fixed", [](double x, int f) { return js_round_fixed(x, f); });
  // lh histogram (hist.hip): the device bin rule as the host compiles it, and the sample count
  // up to which the count pass keeps a series in its 32-lane group (tests bracket it)
  m.def("hist_bin", [](int32_t v) { return hist_bin(v); });
  m.def("hist_lower", [](int b) { return hist_lower(b); });
  m.def("hist_group_max", []() { return apm_hist_group_max(); });
  // wp percentiles (winpct.hip): the sample count and window length up to which the value pass
  // keeps a series in its 32-lane group (tests bracket them)
  m.def("winpct_group_max", []() { return apm_winpct_group_max(); });
  m.def("winpct_group_win", []() { return apm_winpct_group_win(); });
  // sl threshold counts (slo.hip): the sample count up to which the value pass keeps a series in
  // its 32-lane group, and the write pass' LDS stage (tests bracket them)
  m.def("slo_group_max", []() { return apm_slo_group_max(); });
  m.def("slo_stage_bytes", []() { return apm_slo_stage_bytes(); });
  // tk leaderboards (topk.hip): emission positions per block of the tile pass, and the survivors the
  // final block reads per sweep (tests bracket both)
  // sv service windows (svcwin.hip): the sample total and window length up to which the value pass
  // keeps a service in its 32-lane group (tests bracket them)
  m.def("svcwin_group_max", []() { return apm_svcwin_group_max(); });
  m.def("svcwin_group_win", []() { return apm_svcwin_group_win(); });
  // rw recent windows (recent.hip): the largest span's sample count and the window length up to
  // which the value pass keeps a series in its 32-lane group (tests bracket them)
  m.def("recent_group_max", []() { return apm_recent_group_max(); });
  m.def("recent_group_win", []() { return apm_recent_group_win(); });
  // sb burn rates (burn.hip): the sample count up to which the value pass keeps a series in its
  // 32-lane group (tests bracket it), and the exact inequality the kernels decide a rule with
  // (burncmp.h, the same routine compiled for the host): m >= min_samples and
  // bad * 10^8 >= f * m * b
  m.def("burn_group_max", []() { return apm_burn_group_max(); });
  m.def("burn_fires", [](int64_t bad, int64_t mm, int64_t b, int64_t f, int64_t min_samples) {
    if (bad < 0 || bad > 0x7fffffff || mm < 0 || mm > 0x7fffffff || b < 1 || b > 99999 || f < 1 || f > 1000000 ||
        min_samples < 1 || min_samples > 0x7fffffff)
      throw std::invalid_argument("burn_fires: bad, m in 0 .. 2147483647, b in 1 .. 99999, f in 1 .. 1000000, min_samples >= 1");
    return burn_fires((uint32_t)bad, (uint32_t)mm, (uint32_t)b, (uint32_t)f, (uint32_t)min_samples);
  }, py::arg("bad"), py::arg("m"), py::arg("b"), py::arg("f"), py::arg("min_samples"));
  // tf traffic (traffic.hip): the window length up to which the value pass sorts in registers and the
  // longest it takes at all, the series per block of that path (tests bracket them), and the exact
  // verdict the kernels decide a rule with (trafficcmp.h, the same routine compiled for the host):
  // "D", "S" or "N" from the recent samples R, twice the median, four times the MAD, the baseline
  // buckets B and the clipped span kk
  m.def("traffic_group_win", []() { return apm_traffic_group_win(); });
  m.def("traffic_max_win", []() { return apm_traffic_max_win(); });
  m.def("traffic_tile", []() { return apm_traffic_tile(); });
  m.def("traffic_verdict", [](int64_t R, int64_t med2, int64_t mad4, int64_t B, int64_t kk, int64_t r_d, int64_t r_s,
                              int64_t z, int64_t min_rate, int64_t min_buckets) {
    // (the bounds trafficcmp.h's width argument rests on: R < 2^37, med2 < 2^32, mad4 <= 2^33)
    if (R < 0 || R > 64 * (int64_t)0x7fffffff || med2 < 0 || med2 > 2 * (int64_t)0x7fffffff || mad4 < 0 ||
        mad4 > ((int64_t)1 << 33) || B < 0 || B > 0x7fffffff || kk < 1 || kk > 64 || r_d < 0 || r_d > 999 ||
        (r_s != 0 && (r_s < 1001 || r_s > 1000000)) || z < 0 || z > 100000 || min_rate < 1 || min_rate > 0x7fffffff ||
        min_buckets < 0 || min_buckets > 0x7fffffff)
      throw std::invalid_argument("traffic_verdict: R in 0 .. 64 (2^31 - 1), med2 in 0 .. 2^32 - 2, mad4 in 0 .. 2^33, kk in "
                                  "1 .. 64, r_d in 0 .. 999, r_s 0 or in 1001 .. 1000000, z in 0 .. 100000, min_rate >= 1");
    const int v = traffic_verdict(R, med2, mad4, (int32_t)B, (int32_t)kk, (int32_t)r_d, (int32_t)r_s, (int32_t)z,
                                  (int32_t)min_rate, (int32_t)min_buckets);
    return std::string(v == TF_D ? "D" : v == TF_S ? "S" : "N");
  }, py::arg("R"), py::arg("med2"), py::arg("mad4"), py::arg("B"), py::arg("kk"), py::arg("r_d"), py::arg("r_s"),
     py::arg("z"), py::arg("min_rate"), py::arg("min_buckets"));
  // po peers (peers.hip): the members up to which a group is ranked by 32 lanes in registers (tests
  // bracket it; larger groups take the block pass), and the exact verdict the kernels decide a
  // member with (peercmp.h, the same routine compiled for the host): "H", "L" or "N"
  m.def("peer_group_max", []() { return apm_peer_group_max(); });
  m.def("peer_verdict", [](int64_t x, int64_t X2, int64_t D4, int64_t E, int64_t r_h, int64_t r_l, int64_t z,
                           int64_t min_value, int64_t min_delta, int64_t min_peers) {
    // (the bounds peercmp.h's width argument rests on: |x| < 2^32, |X2| < 2^33, D4 < 2^36)
    const int64_t b32 = (int64_t)1 << 32;
    if (x <= -b32 || x >= b32 || X2 <= -2 * b32 || X2 >= 2 * b32 || D4 < 0 || D4 >= 16 * b32 || E < 0 || E > 0x7fffffff ||
        (r_h != 0 && (r_h < 1001 || r_h > 1000000)) || r_l < 0 || r_l > 999 || z < 0 || z > 100000 || min_value < 1 ||
        min_value > 0x7fffffff || min_delta < 0 || min_delta > 0x7fffffff || min_peers < 0 || min_peers > 0x7fffffff)
      throw std::invalid_argument("peer_verdict: |x| < 2^32, |X2| < 2^33, D4 in 0 .. 2^36 - 1, r_h 0 or in 1001 .. 1000000, "
                                  "r_l in 0 .. 999, z in 0 .. 100000, min_value >= 1, min_delta >= 0");
    const int v = peer_verdict(x, X2, D4, (int32_t)E, (int32_t)r_h, (int32_t)r_l, (int32_t)z, (int32_t)min_value,
                               (int32_t)min_delta, (int32_t)min_peers);
    return std::string(v == PO_H ? "H" : v == PO_L ? "L" : "N");
  }, py::arg("x"), py::arg("X2"), py::arg("D4"), py::arg("E"), py::arg("r_h"), py::arg("r_l"), py::arg("z"),
     py::arg("min_value"), py::arg("min_delta"), py::arg("min_peers"));
  // ls shifts (shift.hip): the window length and the sample count up to which the value pass keeps a
  // series in its 32-lane group (tests bracket them), and the exact verdict the kernels decide a rule
  // with (shiftcmp.h, the same routine compiled for the host): "U", "D" or "N"
  m.def("shift_group_max", []() { return apm_shift_group_max(); });
  m.def("shift_group_win", []() { return apm_shift_group_win(); });
  m.def("shift_verdict", [](int64_t a, int64_t b, int64_t mR, int64_t mB, int64_t T2, int64_t X2, int64_t q, int64_t r_u,
                            int64_t r_d, int64_t z, int64_t min_delta, int64_t min_recent, int64_t min_baseline) {
    // (the bounds shiftcmp.h's width argument rests on)
    const int64_t b32 = (int64_t)1 << 32;
    if (mR < 0 || mR > 0x7fffffff || mB < 0 || mB > 0x7fffffff || a < 0 || b < 0 || a + b > mR || T2 <= -b32 || T2 >= b32 ||
        X2 <= -b32 || X2 >= b32 || q < 1 || q > 99999 || (r_u != 0 && (r_u < 1001 || r_u > 1000000)) ||
        (r_d != 0 && (r_d < 1001 || r_d > 1000000)) || z < 0 || z > 100000 || min_delta < 1 || min_delta > 1073741823 ||
        min_recent < 1 || min_recent > 0x7fffffff || min_baseline < 1 || min_baseline > 0x7fffffff)
      throw std::invalid_argument("shift_verdict: mR, mB in 0 .. 2147483647, a + b <= mR, |T2|, |X2| < 2^32, q in 1 .. 99999, "
                                  "r_u, r_d 0 or in 1001 .. 1000000, z in 0 .. 100000, min_delta in 1 .. 1073741823, "
                                  "min_recent, min_baseline >= 1");
    const int v = shift_verdict((int32_t)a, (int32_t)b, (int32_t)mR, (int32_t)mB, T2, X2, (int32_t)q, (int32_t)r_u, (int32_t)r_d,
                                (int32_t)z, (int32_t)min_delta, (int32_t)min_recent, (int32_t)min_baseline);
    return std::string(v == LS_U ? "U" : v == LS_D ? "D" : "N");
  }, py::arg("a"), py::arg("b"), py::arg("mR"), py::arg("mB"), py::arg("T2"), py::arg("X2"), py::arg("q"), py::arg("r_u"),
     py::arg("r_d"), py::arg("z"), py::arg("min_delta"), py::arg("min_recent"), py::arg("min_baseline"));
  // ic incidents (incident.hip): one step of the state machine the kernel runs (incidentcmp.h, the
  // same routine compiled for the host).  state = (code0 "" or a letter, since_ts, age, hot_run,
  // clear_run); returns (state, event "" / "O" / "S" / "C", code0 the row prints, run the row prints)
  m.def("incident_step", [](const std::tuple<std::string, int64_t, uint64_t, int, int>& state, bool hot, const std::string& code,
                            int64_t edge_ts, int64_t open_after, int64_t close_after, int64_t remind_every) {
    const std::string& c0 = std::get<0>(state);
    const uint64_t age = std::get<2>(state);
    const int hr = std::get<3>(state), cr = std::get<4>(state);
    if (c0.size() > 1 || age > 0xffffffffull || hr < 0 || hr > 255 || cr < 0 || cr > 255 || open_after < 1 || open_after > 255 ||
        close_after < 1 || close_after > 255 || remind_every < 0 || remind_every > 65535 || (hot && code.size() != 1) ||
        (hot && code[0] == 0))
      throw std::invalid_argument("incident_step: code0 at most one letter, age below 2^32, runs in 0 .. 255, open_after and "
                                  "close_after in 1 .. 255, remind_every in 0 .. 65535, one letter of code when hot");
    IncidentState st{};
    st.code0 = c0.empty() ? 0 : (uint8_t)c0[0];
    st.since_ts = std::get<1>(state);
    st.age = (uint32_t)age;
    st.hot_run = (uint8_t)hr;
    st.clear_run = (uint8_t)cr;
    const IncidentOut o = incident_step(st, hot, hot ? (uint8_t)code[0] : 0, edge_ts, (uint32_t)open_after, (uint32_t)close_after,
                                        (uint32_t)remind_every);
    return py::make_tuple(py::make_tuple(st.code0 ? std::string(1, (char)st.code0) : std::string(), (int64_t)st.since_ts,
                                         (uint64_t)st.age, (int)st.hot_run, (int)st.clear_run),
                          o.event ? std::string(1, (char)o.event) : std::string(),
                          o.code0 ? std::string(1, (char)o.code0) : std::string(), (int)o.run);
  }, py::arg("state"), py::arg("hot"), py::arg("code"), py::arg("edge_ts"), py::arg("open_after"), py::arg("close_after"),
     py::arg("remind_every"));
  m.def("incident_row_bound", [](uint64_t name_bytes) { return (uint64_t)apm_incident_row_bound((size_t)name_bytes); });
  m.def("incident_kernels", [](py::bytes state, py::bytes ev, const std::vector<py::object>& words, py::bytes active,
                               int32_t n_series, const std::vector<int32_t>& open_after, const std::vector<int32_t>& close_after,
                               int32_t remind_every, int64_t edge_ts, const std::vector<int32_t>& perm,
                               const std::vector<std::tuple<int32_t, int32_t, int32_t, int32_t>>& series_names, py::bytes names) {
    // the K25 kernels alone (test hook) over `cap` slots: state is cap * 4 * 16 bytes, ev cap * 4,
    // active cap; words holds per source None (off) or cap int32 verdict words (stride 4); perm the
    // series in emission order (empty: no text pass).  Returns (state, ev, open counts, text).
    const std::string st = state, e0 = ev, act = active, nm = names;
    const size_t cap = act.size();
    if (st.size() != cap * 64 || e0.size() != cap * 4 || words.size() != 4 || open_after.size() != 4 || close_after.size() != 4 ||
        n_series < 0 || (size_t)n_series > cap || series_names.size() != cap || remind_every < 0 || remind_every > 65535)
      throw std::invalid_argument("incident_kernels: state cap * 64 bytes, ev cap * 4, four sources, n_series <= cap");
    size_t longest = 0;
    for (const auto& t : series_names) {
      const int64_t so = std::get<0>(t), sl = std::get<1>(t), vo = std::get<2>(t), vl = std::get<3>(t);
      if (so < 0 || sl < 0 || vo < 0 || vl < 0 || (size_t)(so + sl) > nm.size() || (size_t)(vo + vl) > nm.size())
        throw std::invalid_argument("incident_kernels: a name lies outside `names`");
      longest = std::max(longest, (size_t)(sl + vl));
    }
    for (int32_t s : perm)
      if (s < 0 || s >= n_series) throw std::invalid_argument("incident_kernels: perm names no series");
    DevMem dst(cap * 64), dev(cap * 4), dcodes(cap * 8), dact(cap), dopen(16), dnames(nm.size() + 64), dsn(cap * 16);
    std::vector<std::unique_ptr<DevMem>> dw;
    IncidentArgs a{};
    for (int k = 0; k < 4; ++k) {
      a.src[k].kind = k;
      a.src[k].stride_bytes = 4;
      a.open_after[k] = open_after[k];
      a.close_after[k] = close_after[k];
      if (words[k].is_none()) continue;
      const auto w = words[k].cast<std::vector<int32_t>>();
      if (w.size() != cap || open_after[k] < 1 || open_after[k] > 255 || close_after[k] < 1 || close_after[k] > 255)
        throw std::invalid_argument("incident_kernels: cap words per source, open_after and close_after in 1 .. 255");
      dw.emplace_back(new DevMem(cap * 4));
      if (cap) HIP_OK(hipMemcpy(dw.back()->p, w.data(), cap * 4, hipMemcpyHostToDevice));
      a.src[k].word = dw.back()->as<int32_t>();
    }
    if (cap) {
      HIP_OK(hipMemcpy(dst.p, st.data(), st.size(), hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(dev.p, e0.data(), e0.size(), hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(dact.p, act.data(), cap, hipMemcpyHostToDevice));
      std::vector<int32_t> sn;
      for (const auto& t : series_names) {
        sn.push_back(std::get<0>(t)); sn.push_back(std::get<1>(t)); sn.push_back(std::get<2>(t)); sn.push_back(std::get<3>(t));
      }
      HIP_OK(hipMemcpy(dsn.p, sn.data(), cap * 16, hipMemcpyHostToDevice));
    }
    HIP_OK(hipMemset(dcodes.p, 0, std::max<size_t>(cap * 8, 8)));
    HIP_OK(hipMemset(dopen.p, 0, 16));
    HIP_OK(hipMemset(dnames.p, 0, nm.size() + 64));
    if (!nm.empty()) HIP_OK(hipMemcpy(dnames.p, nm.data(), nm.size(), hipMemcpyHostToDevice));
    a.active = dact.as<uint8_t>();
    a.n_series = n_series;
    a.remind_every = remind_every;
    a.edge_ts = edge_ts;
    a.state = dst.as<IncidentState>();
    a.ev = dev.as<uint8_t>();
    a.codes = dcodes.as<uint8_t>();
    a.open_n = dopen.as<int32_t>();
    apm_incident_step(&a, 0);
    std::string text;
    const int32_t n = (int32_t)perm.size();
    if (n > 0) {
      const int32_t np = n * IC_MAX_SOURCES;
      const size_t bound = (size_t)np * apm_incident_row_bound(longest) + 64;
      const size_t tmpb = apm_incident_tmp_bytes(n);
      DevMem dperm((size_t)n * 4), dlen(((size_t)np + 1) * 4), doff(((size_t)np + 1) * 4), dtmp(tmpb), dout(bound);
      HIP_OK(hipMemcpy(dperm.p, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice));
      IncidentTextArgs t{};
      t.state = a.state; t.ev = a.ev; t.codes = a.codes;
      t.perm = dperm.as<int32_t>();
      t.series_names = dsn.as<int4>();
      t.names = dnames.as<char>();
      t.n = np;
      t.n_series = n_series;
      t.ts_len = std::snprintf(t.ts, sizeof t.ts, "%lld|", (long long)edge_ts);
      t.len = dlen.as<uint32_t>();
      t.off = doff.as<uint32_t>();
      t.out = dout.as<char>();
      if (apm_incident_plan(&t, dtmp.p, tmpb, 0) != 0) throw std::runtime_error("incident_kernels: scan failed");
      apm_incident_write(&t, 0);
      uint32_t total = 0;
      HIP_OK(hipMemcpy(&total, t.off + np, 4, hipMemcpyDeviceToHost));
      if (total > bound) throw std::runtime_error("incident_kernels: the rows pass the row bound");
      text.resize(total);
      if (total) HIP_OK(hipMemcpy(&text[0], dout.p, total, hipMemcpyDeviceToHost));
    }
    HIP_OK(hipDeviceSynchronize());
    std::string st1(cap * 64, '\0'), ev1(cap * 4, '\0');
    int32_t open_n[4] = {0, 0, 0, 0};
    if (cap) {
      HIP_OK(hipMemcpy(&st1[0], dst.p, st1.size(), hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(&ev1[0], dev.p, ev1.size(), hipMemcpyDeviceToHost));
    }
    HIP_OK(hipMemcpy(open_n, dopen.p, 16, hipMemcpyDeviceToHost));
    return py::make_tuple(py::bytes(st1), py::bytes(ev1), py::make_tuple(open_n[0], open_n[1], open_n[2], open_n[3]),
                          py::bytes(text));
  }, py::arg("state"), py::arg("ev"), py::arg("words"), py::arg("active"), py::arg("n_series"), py::arg("open_after"),
     py::arg("close_after"), py::arg("remind_every"), py::arg("edge_ts"), py::arg("perm"), py::arg("series_names"),
     py::arg("names"));
  m.def("apm_topk_tile", []() { return apm_topk_tile(); });
  m.def("apm_topk_final_span", []() { return apm_topk_final_span(); });
  m.def("topk_select", [](const std::vector<std::tuple<double, double, double, double, int32_t>>& win_rows,
                          const std::vector<int32_t>& perm, int32_t k, const std::vector<int32_t>& by, double min_tpm) {
    // the two K18 kernels alone (test hook): win_rows are (tpm, avg, p75, p95, active) per series,
    // perm the series in emission order; returns per board [(series, position)] in rank order
    if (k < 1 || k > TK_MAX_K) throw std::invalid_argument("topk_select: k is 1 .. 128");
    if (by.empty() || by.size() > (size_t)TK_MAX_BOARDS) throw std::invalid_argument("topk_select: 1 to 4 boards");
    for (int32_t c : by)
      if (c < TK_TPM || c > TK_P95) throw std::invalid_argument("topk_select: keys are 0 .. 3");
    for (int32_t s : perm)
      if (s < 0 || (size_t)s >= win_rows.size()) throw std::invalid_argument("topk_select: perm names no series");
    const int32_t n = (int32_t)perm.size(), S = (int32_t)win_rows.size(), nb = (int32_t)by.size();
    std::vector<WinStat> win((size_t)S);
    for (int32_t s = 0; s < S; ++s) {
      win[s].tpm = std::get<0>(win_rows[s]); win[s].avg = std::get<1>(win_rows[s]);
      win[s].p75 = std::get<2>(win_rows[s]); win[s].p95 = std::get<3>(win_rows[s]);
      win[s].n = 0; win[s].active = std::get<4>(win_rows[s]);
    }
    DevMem dwin((size_t)S * sizeof(WinStat)), dperm((size_t)n * 4), dsc(apm_topk_scratch_bytes(n, k, nb));
    DevMem dout((size_t)nb * k * sizeof(TopKRec)), dn(64);
    if (S) HIP_OK(hipMemcpy(dwin.p, win.data(), (size_t)S * sizeof(WinStat), hipMemcpyHostToDevice));
    if (n) HIP_OK(hipMemcpy(dperm.p, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    TopKArgs a{};
    a.win = dwin.as<WinStat>(); a.perm = dperm.as<int32_t>(); a.n = n; a.n_series = S; a.k = k; a.nb = nb;
    for (int32_t b = 0; b < nb; ++b) a.by[b] = by[b];
    a.min_tpm = min_tpm;
    a.out = dout.as<TopKRec>(); a.out_n = dn.as<int32_t>();
    apm_topk(&a, dsc.p, 0);
    std::vector<TopKRec> rec((size_t)nb * k);
    int32_t cnt[TK_MAX_BOARDS] = {0, 0, 0, 0};
    HIP_OK(hipMemcpy(cnt, dn.p, (size_t)nb * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rec.data(), dout.p, rec.size() * sizeof(TopKRec), hipMemcpyDeviceToHost));
    py::list out;
    for (int32_t b = 0; b < nb; ++b) {
      py::list rows;
      for (int32_t r = 0; r < std::min(std::max(cnt[b], 0), k); ++r)
        rows.append(py::make_tuple(rec[(size_t)b * k + r].series, rec[(size_t)b * k + r].pos));
      out.append(rows);
    }
    return out;
  }, py::arg("win_rows"), py::arg("perm"), py::arg("k"), py::arg("by"), py::arg("min_tpm") = 0.0);

  register_tailer(m);
  register_synth(m);
  register_procstat(m);
  register_dbsink(m);
}
