// K13: wire records -> Postgres COPY text rows (host, C++).
//
// The reference converts every db_insert message to a row object (entries.js toPostgresObject
// :23-42, :120-151, :218-240, :310-331) and ships them with multi-row INSERTs built by
// pg-promise (stream_insert_db.js:298).  At the fused engine's output rate (one fs row per
// series per LAG every 10 s: ~160k rows per interval per GPU) that per-row object path would
// dominate, so the sink encodes COPY text directly from the wire lines here.  The Python
// definition is runtime/sinks.py (copy_encode_lines); tests/test_sinks.py checks both agree
// byte for byte.
//
// Field rules (as the Python/JS path produces them):
//   timestamps      parseInt -> 'YYYY-MM-DD HH:MM:SS.mmm+00' (UTC), NaN -> \N
//   numbers         parseInt / parseFloat, printed as String(x); NaN/Infinity -> \N (JSON null)
//   strings         COPY-escaped (\\, \t, \n, \r); missing field -> \N
//   fs.lag          kept as the string it was on the wire (JSON: a string)
//   stats / entry   JSON.stringify text (jsonb), dates as toISOString()
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../kernels/common.h"
#include "jsutil.h"

namespace apm {
namespace copyenc {

namespace {

constexpr std::string_view kNull = "\\N";

// JS parseFloat
double parse_float(std::string_view s) {
  const uint8_t* p = (const uint8_t*)s.data();
  const uint8_t* e = p + s.size();
  while (p < e) { int w = js::ws_len(p, e); if (!w) break; p += w; }
  const char* b = (const char*)p;
  const char* q = b;
  const char* end = (const char*)e;
  if (q < end && (*q == '+' || *q == '-')) ++q;
  if ((size_t)(end - q) >= 8 && std::memcmp(q, "Infinity", 8) == 0)
    return *b == '-' ? -INFINITY : INFINITY;
  const char* d0 = q;
  while (q < end && *q >= '0' && *q <= '9') ++q;
  bool digits = q > d0;
  if (q < end && *q == '.') {
    ++q;
    const char* f0 = q;
    while (q < end && *q >= '0' && *q <= '9') ++q;
    digits |= q > f0;
  }
  if (!digits) return js::nan();
  if (q < end && (*q == 'e' || *q == 'E')) {
    const char* x = q + 1;
    if (x < end && (*x == '+' || *x == '-')) ++x;
    const char* x0 = x;
    while (x < end && *x >= '0' && *x <= '9') ++x;
    if (x > x0) q = x;
  }
  return std::strtod(std::string(b, q).c_str(), nullptr);
}

void civil(int64_t days, int& y, unsigned& m, unsigned& d) {
  days += 719468;
  const int64_t era = (days >= 0 ? days : days - 146096) / 146097;
  const unsigned doe = (unsigned)(days - era * 146097);
  const unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const unsigned mp = (5 * doy + 2) / 153;
  d = doy - (153 * mp + 2) / 5 + 1;
  m = mp < 10 ? mp + 3 : mp - 9;
  y = (int)(yoe + era * 400) + (m <= 2);
}

// ms since epoch -> "YYYY-MM-DD?HH:MM:SS.mmm" (sep ' ' or 'T')
bool ts_text(double ms, char sep, std::string& out) {
  if (!(ms == ms) || std::isinf(ms) || std::fabs(ms) > 8.64e15) return false;
  const int64_t t = (int64_t)ms;
  int64_t days = t / 86400000, rem = t % 86400000;
  if (rem < 0) { rem += 86400000; --days; }
  int y;
  unsigned mo, d;
  civil(days, y, mo, d);
  char buf[40];
  std::snprintf(buf, sizeof(buf), "%04d-%02u-%02u%c%02d:%02d:%02d.%03d", y, mo, d, sep, (int)(rem / 3600000),
                (int)(rem / 60000 % 60), (int)(rem / 1000 % 60), (int)(rem % 1000));
  out += buf;
  return true;
}

void copy_escape(std::string& out, std::string_view s) {
  for (char c : s) {
    switch (c) {
      case '\\': out += "\\\\"; break;
      case '\t': out += "\\t"; break;
      case '\n': out += "\\n"; break;
      case '\r': out += "\\r"; break;
      default: out += c;
    }
  }
}

void json_str(std::string& out, std::string_view s) {
  out += '"';
  for (unsigned char c : s) {
    switch (c) {
      case '"': out += "\\\""; break;
      case '\\': out += "\\\\"; break;
      case '\n': out += "\\n"; break;
      case '\r': out += "\\r"; break;
      case '\t': out += "\\t"; break;
      case '\b': out += "\\b"; break;
      case '\f': out += "\\f"; break;
      default:
        if (c < 0x20) {
          char b[8];
          std::snprintf(b, sizeof(b), "\\u%04x", c);
          out += b;
        } else {
          out += (char)c;
        }
    }
  }
  out += '"';
}

struct Fields {
  std::string_view f[32];
  int n = 0;
  bool has(int i) const { return i < n; }
};

void split(std::string_view s, char d, Fields& o) {
  o.n = 0;
  size_t i = 0;
  for (;;) {
    size_t j = s.find(d, i);
    if (o.n < 32) o.f[o.n++] = s.substr(i, j == std::string_view::npos ? std::string_view::npos : j - i);
    if (j == std::string_view::npos) break;
    i = j + 1;
  }
}

void c_str(std::string& out, const Fields& a, int i) {
  if (a.has(i)) copy_escape(out, a.f[i]); else out += kNull;
}
void c_num(std::string& out, double v) {
  if (v == v && !std::isinf(v)) js::append_num(out, v); else out += kNull;
}
void c_ts(std::string& out, const Fields& a, int i) {
  if (!a.has(i) || !ts_text(js::parse_int(a.f[i]), ' ', out)) { out += kNull; return; }
  out += "+00";
}
void j_num(std::string& out, double v) {
  if (v == v && !std::isinf(v)) js::append_num(out, v); else out += "null";
}

// stats object of FullStatEntry.toPostgresObject (entries.js:120-151)
void fs_stats_json(std::string& out, const Fields& a) {
  static const char* names[3] = {"average", "per75", "per95"};
  static const char* suff[5] = {"", "avg", "lb", "ub", "signal"};
  out += '{';
  for (int k = 0; k < 3; ++k) {
    Fields p;
    if (a.has(6 + k)) split(a.f[6 + k], ':', p);
    for (int j = 0; j < 5; ++j) {
      if (k || j) out += ',';
      out += '"';
      out += names[k];
      out += suff[j];
      out += "\":";
      const double v = !p.has(j) ? js::nan() : (j == 4 ? js::parse_int(p.f[j]) : parse_float(p.f[j]));
      j_num(out, v);
    }
  }
  out += '}';
}

void fs_row_json(std::string& out, const Fields& a) {
  out += "{\"timestamp\":";
  std::string ts;
  if (a.has(1) && ts_text(js::parse_int(a.f[1]), 'T', ts)) { out += '"'; out += ts; out += "Z\""; }
  else out += "null";
  out += ",\"server\":";
  if (a.has(2)) json_str(out, a.f[2]); else out += "null";
  out += ",\"service\":";
  if (a.has(3)) json_str(out, a.f[3]); else out += "null";
  out += ",\"tpm\":";
  j_num(out, a.has(5) ? parse_float(a.f[5]) : js::nan());
  out += ",\"lag\":";
  if (a.has(4)) json_str(out, a.f[4]); else out += "null";
  out += ",\"stats\":";
  fs_stats_json(out, a);
  out += '}';
}

}  // namespace

// wp pairs (utils/records.py _pct_from_text / _half_from_text hold the same rules): integers only.
bool all_digits(std::string_view s, size_t max_len) {
  if (s.empty() || s.size() > max_len) return false;
  for (char ch : s) if (ch < '0' || ch > '9') return false;
  return true;
}
// "99.9" -> q = 99900 (1..100000, at most three decimals); -1: malformed
int64_t pct_from_text(std::string_view s) {
  const size_t d = s.find('.');
  const std::string_view ip = s.substr(0, d);
  if (!all_digits(ip, 3)) return -1;
  int64_t q = 0;
  for (char ch : ip) q = q * 10 + (ch - '0');
  q *= 1000;
  if (d != std::string_view::npos) {
    const std::string_view fr = s.substr(d + 1);
    if (!all_digits(fr, 3)) return -1;
    int64_t f = 0;
    for (char ch : fr) f = f * 10 + (ch - '0');
    for (size_t k = fr.size(); k < 3; ++k) f *= 10;
    q += f;
  }
  return q >= 1 && q <= 100000 ? q : -1;
}
// "-340.5" -> sum2 = -681 (twice the value: an integer, or an integer and ".5"); false: malformed
bool half_from_text(std::string_view s, int64_t& sum2) {
  const bool neg = !s.empty() && s[0] == '-';
  if (neg) s.remove_prefix(1);
  const size_t d = s.find('.');
  const std::string_view ip = s.substr(0, d);
  if (!all_digits(ip, 10)) return false;
  if (d != std::string_view::npos && s.substr(d + 1) != "5") return false;
  int64_t v = 0;
  for (char ch : ip) v = v * 10 + (ch - '0');
  v = 2 * v + (d != std::string_view::npos ? 1 : 0);
  sum2 = neg ? -v : v;
  return true;
}
void append_i64(std::string& o, int64_t v) { o += std::to_string(v); }
// "<p>:<v>,<p>:<v>,..." (wp and sv rows) -> the members of a JSON object appended to js ("{" is
// there already); a malformed pair is dropped
void append_pct_pairs(std::string& js, std::string_view rest) {
  while (!rest.empty()) {
    const size_t e = rest.find(',');
    const std::string_view pr = rest.substr(0, e);
    rest = e == std::string_view::npos ? std::string_view() : rest.substr(e + 1);
    const size_t c = pr.find(':');
    const int64_t q = pct_from_text(pr.substr(0, c));
    int64_t sum2 = 0;
    if (q < 0 || c == std::string_view::npos || !half_from_text(pr.substr(c + 1), sum2)) continue;  // (dropped)
    if (js.size() > 1) js += ',';
    // the canonical texts again: q / 1000 without trailing zeros, sum2 / 2 as an integer or x.5
    js += '"';
    append_i64(js, q / 1000);
    if (q % 1000) {
      char fr[4] = {(char)('0' + q % 1000 / 100), (char)('0' + q % 100 / 10), (char)('0' + q % 10), 0};
      int n = 3;
      while (fr[n - 1] == '0') --n;
      js += '.';
      js.append(fr, (size_t)n);
    }
    js += "\":";
    const int64_t m = sum2 < 0 ? -sum2 : sum2;
    if (sum2 < 0) js += '-';
    append_i64(js, m / 2);
    if (m & 1) js += ".5";
  }
}

// Returns the type index (0 tx, 1 fs, 2 al, 3 jx, 4 fb, 5 lh, 6 wp, 7 sl, 8 tk, 9 sv, 10 rw, 11 sb, 12 tf,
// 13 po, 14 ls, 15 ic) the row was appended to, or -1.
int encode_line(std::string_view line, std::string* out /*[16]*/) {
  Fields a;
  split(line, '|', a);
  const std::string_view t = a.f[0];
  if (t == "tx") {
    std::string& o = out[0];
    c_ts(o, a, 6); o += '\t';
    c_ts(o, a, 5); o += '\t';
    c_str(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    c_num(o, a.has(4) ? js::parse_int(a.f[4]) : js::nan()); o += '\t';
    c_num(o, a.has(7) ? js::parse_int(a.f[7]) : js::nan()); o += '\t';
    c_str(o, a, 8); o += '\n';
    return 0;
  }
  if (t == "fs") {
    std::string& o = out[1];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    c_num(o, a.has(5) ? parse_float(a.f[5]) : js::nan()); o += '\t';
    c_str(o, a, 4); o += '\t';
    std::string js;
    fs_stats_json(js, a);
    copy_escape(o, js);
    o += '\n';
    return 1;
  }
  if (t == "al") {
    std::string& o = out[2];
    c_ts(o, a, 2); o += '\t';
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 3); o += '\t';
    c_str(o, a, 4); o += '\t';
    c_str(o, a, 5); o += '\t';
    Fields e;
    split(a.has(6) ? a.f[6] : std::string_view(), '&', e);
    std::string js;
    fs_row_json(js, e);
    copy_escape(o, js);
    o += '\n';
    return 2;
  }
  if (t == "fb") {  // fleet baseline: timestamp, service, lag, nseries, stats json
    std::string& o = out[4];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    c_num(o, a.has(4) ? js::parse_int(a.f[4]) : js::nan()); o += '\t';
    static const char* names[3] = {"average", "per75", "per95"};
    std::string js = "{";
    for (int k = 0; k < 3; ++k) {
      Fields p;
      if (a.has(5 + k)) split(a.f[5 + k], ':', p);
      for (int j = 0; j < 2; ++j) {
        if (k || j) js += ',';
        js += '"';
        js += names[k];
        js += j ? "std\":" : "mean\":";
        j_num(js, p.has(j) ? parse_float(p.f[j]) : js::nan());
      }
    }
    js += '}';
    copy_escape(o, js);
    o += '\n';
    return 4;
  }
  if (t == "lh") {  // latency histogram: timestamp, server, service, count, nan, bins json
    std::string& o = out[5];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    c_num(o, a.has(4) ? js::parse_int(a.f[4]) : js::nan()); o += '\t';
    c_num(o, a.has(5) ? js::parse_int(a.f[5]) : js::nan()); o += '\t';
    std::string js = "{";
    std::string_view rest = a.has(6) ? a.f[6] : std::string_view();
    while (!rest.empty()) {
      const size_t e = rest.find(',');
      const std::string_view pr = rest.substr(0, e);
      rest = e == std::string_view::npos ? std::string_view() : rest.substr(e + 1);
      const size_t c = pr.find(':');
      const double lo = js::parse_int(pr.substr(0, c));
      const double n = c == std::string_view::npos ? js::nan() : js::parse_int(pr.substr(c + 1));
      if (lo != lo || n != n) continue;  // (a malformed pair is dropped)
      if (js.size() > 1) js += ',';
      js += '"';
      js::append_num(js, lo);
      js += "\":";
      js::append_num(js, n);
    }
    js += '}';
    copy_escape(o, js);
    o += '\n';
    return 5;
  }
  if (t == "wp") {  // window percentiles: timestamp, server, service, count, nan, pcts json
    std::string& o = out[6];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    c_num(o, a.has(4) ? js::parse_int(a.f[4]) : js::nan()); o += '\t';
    c_num(o, a.has(5) ? js::parse_int(a.f[5]) : js::nan()); o += '\t';
    std::string js = "{";
    append_pct_pairs(js, a.has(6) ? a.f[6] : std::string_view());
    js += '}';
    copy_escape(o, js);
    o += '\n';
    return 6;
  }
  if (t == "sl") {  // window threshold counts: timestamp, server, service, count, nan, le json
    std::string& o = out[7];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    c_num(o, a.has(4) ? js::parse_int(a.f[4]) : js::nan()); o += '\t';
    c_num(o, a.has(5) ? js::parse_int(a.f[5]) : js::nan()); o += '\t';
    std::string js = "{";
    std::string_view rest = a.has(6) ? a.f[6] : std::string_view();
    int64_t last_t = -1;
    while (!rest.empty()) {
      const size_t e = rest.find(',');
      const std::string_view pr = rest.substr(0, e);
      rest = e == std::string_view::npos ? std::string_view() : rest.substr(e + 1);
      const size_t c = pr.find(':');
      // (utils/records.py slo_pairs_from_text holds the same rules) T and c: 1 to 10 digits,
      // T <= INT32_MAX and above the last pair kept
      if (c == std::string_view::npos || !all_digits(pr.substr(0, c), 10) || !all_digits(pr.substr(c + 1), 10)) continue;
      int64_t tv = 0, cv = 0;
      for (char ch : pr.substr(0, c)) tv = tv * 10 + (ch - '0');
      for (char ch : pr.substr(c + 1)) cv = cv * 10 + (ch - '0');
      if (tv > 2147483647 || tv <= last_t) continue;  // (dropped)
      last_t = tv;
      if (js.size() > 1) js += ',';
      js += '"';
      append_i64(js, tv);
      js += "\":";
      append_i64(js, cv);
    }
    js += '}';
    copy_escape(o, js);
    o += '\n';
    return 7;
  }
  if (t == "tk") {  // leaderboard: timestamp, board, rank, server, service, tpm, average, per75, per95
    // (utils/records.py entry_from_csv holds the same rules) a row with an unknown board, or a rank
    // that is not 1 to 3 plain digits in 1 .. 128, is dropped
    const std::string_view board = a.has(2) ? a.f[2] : std::string_view();
    if (board != "tpm" && board != "average" && board != "per75" && board != "per95") return -1;
    if (!a.has(3) || !all_digits(a.f[3], 3)) return -1;
    int64_t rank = 0;
    for (char ch : a.f[3]) rank = rank * 10 + (ch - '0');
    if (rank < 1 || rank > 128) return -1;
    std::string& o = out[8];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    append_i64(o, rank); o += '\t';
    c_str(o, a, 4); o += '\t';
    c_str(o, a, 5);
    for (int i = 6; i < 10; ++i) {  // (numbers as the fs row's tpm: not finite -> NULL)
      o += '\t';
      c_num(o, a.has(i) ? parse_float(a.f[i]) : js::nan());
    }
    o += '\n';
    return 8;
  }
  if (t == "sv") {  // service window: timestamp, service, servers, count, nan, elapsed_sum, pcts json
    // (utils/records.py entry_from_csv holds the same rules) a row whose servers, count or nan is not
    // 1 to 10 plain digits, or whose sum is not 1 to 18 digits after an optional '-', is dropped
    for (int i = 3; i <= 5; ++i)
      if (!a.has(i) || !all_digits(a.f[i], 10)) return -1;
    if (!a.has(6)) return -1;
    const bool sneg = !a.f[6].empty() && a.f[6][0] == '-';
    const std::string_view sdig = sneg ? a.f[6].substr(1) : a.f[6];
    if (!all_digits(sdig, 18)) return -1;
    std::string& o = out[9];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    for (int i = 3; i <= 5; ++i) {
      int64_t v = 0;
      for (char ch : a.f[i]) v = v * 10 + (ch - '0');
      append_i64(o, v); o += '\t';
    }
    int64_t sv = 0;
    for (char ch : sdig) sv = sv * 10 + (ch - '0');
    append_i64(o, sneg ? -sv : sv); o += '\t';
    std::string js = "{";
    append_pct_pairs(js, a.has(7) ? a.f[7] : std::string_view());
    js += '}';
    copy_escape(o, js);
    o += '\n';
    return 9;
  }
  if (t == "rw") {  // recent window: timestamp, server, service, buckets, count, nan, elapsed_sum, pcts json
    // (utils/records.py entry_from_csv holds the same rules, those of sv) a row whose buckets, count
    // or nan is not 1 to 10 plain digits, or whose sum is not 1 to 18 digits after an optional '-',
    // is dropped
    for (int i = 4; i <= 6; ++i)
      if (!a.has(i) || !all_digits(a.f[i], 10)) return -1;
    if (!a.has(7)) return -1;
    const bool sneg = !a.f[7].empty() && a.f[7][0] == '-';
    const std::string_view sdig = sneg ? a.f[7].substr(1) : a.f[7];
    if (!all_digits(sdig, 18)) return -1;
    std::string& o = out[10];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    for (int i = 4; i <= 6; ++i) {
      int64_t v = 0;
      for (char ch : a.f[i]) v = v * 10 + (ch - '0');
      append_i64(o, v); o += '\t';
    }
    int64_t sv = 0;
    for (char ch : sdig) sv = sv * 10 + (ch - '0');
    append_i64(o, sneg ? -sv : sv); o += '\t';
    std::string js = "{";
    append_pct_pairs(js, a.has(8) ? a.f[8] : std::string_view());
    js += '}';
    copy_escape(o, js);
    o += '\n';
    return 10;
  }
  if (t == "sb") {  // SLO burn: timestamp, server, service, threshold, target_q, count, bad, nan, rules json
    // (utils/records.py entry_from_csv and burn_rules_from_text hold the same rules) a row whose T,
    // q, m, bad or nan is not 1 to 10 plain digits, or whose last field is not 1 to 4 groups
    // k:f:m:bad:fired of such numbers with fired 0 or 1, is dropped whole
    for (int i = 4; i <= 8; ++i)
      if (!a.has(i) || !all_digits(a.f[i], 10)) return -1;
    if (!a.has(9) || a.f[9].empty()) return -1;
    std::string js = "[";
    {
      static const char* key[5] = {"{\"k\":", ",\"f\":", ",\"m\":", ",\"bad\":", ",\"fired\":"};
      std::string_view rest = a.f[9];
      int groups = 0;
      for (;;) {
        const size_t e = rest.find(',');
        std::string_view g = rest.substr(0, e);
        if (++groups > 4) return -1;
        if (groups > 1) js += ',';
        for (int p = 0; p < 5; ++p) {
          const size_t c = g.find(':');
          if ((p < 4) == (c == std::string_view::npos)) return -1;  // (exactly five parts)
          const std::string_view num = g.substr(0, c);
          if (!all_digits(num, 10)) return -1;
          js += key[p];
          if (p == 4) {
            if (num != "0" && num != "1") return -1;
            js += num == "1" ? "true" : "false";
          } else {
            int64_t v = 0;
            for (char ch : num) v = v * 10 + (ch - '0');
            append_i64(js, v);
            g = g.substr(c + 1);
          }
        }
        js += '}';
        if (e == std::string_view::npos) break;
        rest = rest.substr(e + 1);
      }
    }
    js += ']';
    std::string& o = out[11];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    for (int i = 4; i <= 8; ++i) {
      int64_t v = 0;
      for (char ch : a.f[i]) v = v * 10 + (ch - '0');
      append_i64(o, v); o += '\t';
    }
    copy_escape(o, js);
    o += '\n';
    return 11;
  }
  if (t == "tf") {  // traffic: timestamp, server, service, count, min_rate, rules json
    // (utils/records.py entry_from_csv and traffic_rules_from_text hold the same rules) a row whose n
    // or minRate is not 1 to 10 plain digits, or whose last field is not 1 to 4 groups
    // k:B:R:med2:mad4:V of such numbers with V one of D, S, N, is dropped whole
    for (int i = 4; i <= 5; ++i)
      if (!a.has(i) || !all_digits(a.f[i], 10)) return -1;
    if (!a.has(6) || a.f[6].empty()) return -1;
    std::string js = "[";
    {
      static const char* key[6] = {"{\"k\":", ",\"buckets\":", ",\"recent\":", ",\"med2\":", ",\"mad4\":", ",\"verdict\":"};
      std::string_view rest = a.f[6];
      int groups = 0;
      for (;;) {
        const size_t e = rest.find(',');
        std::string_view g = rest.substr(0, e);
        if (++groups > 4) return -1;
        if (groups > 1) js += ',';
        for (int p = 0; p < 6; ++p) {
          const size_t c = g.find(':');
          if ((p < 5) == (c == std::string_view::npos)) return -1;  // (exactly six parts)
          const std::string_view part = g.substr(0, c);
          js += key[p];
          if (p == 5) {
            if (part != "D" && part != "S" && part != "N") return -1;
            js += '"';
            js += part;
            js += '"';
          } else {
            if (!all_digits(part, 10)) return -1;
            int64_t v = 0;
            for (char ch : part) v = v * 10 + (ch - '0');
            append_i64(js, v);
            g = g.substr(c + 1);
          }
        }
        js += '}';
        if (e == std::string_view::npos) break;
        rest = rest.substr(e + 1);
      }
    }
    js += ']';
    std::string& o = out[12];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    for (int i = 4; i <= 5; ++i) {
      int64_t v = 0;
      for (char ch : a.f[i]) v = v * 10 + (ch - '0');
      append_i64(o, v); o += '\t';
    }
    copy_escape(o, js);
    o += '\n';
    return 12;
  }
  if (t == "po") {  // peer outlier: timestamp, server, service, count, pct, value2, peers, median2x2, mad4, verdict
    // (utils/records.py entry_from_csv holds the same rules) a row is dropped whole unless it has
    // exactly ten fields, m and E are 1 to 10 plain digits, the pair is <p>:<x> with p a percentile
    // of at most three decimals and x 1 to 10 digits after an optional '-', X2 1 to 11 digits after
    // an optional '-', D4 1 to 11 plain digits and the verdict H or L
    if (a.n != 10) return -1;
    if (!all_digits(a.f[4], 10) || !all_digits(a.f[6], 10) || !all_digits(a.f[8], 11)) return -1;
    if (a.f[9] != "H" && a.f[9] != "L") return -1;
    const size_t c = a.f[5].find(':');
    if (c == std::string_view::npos) return -1;
    const int64_t q = pct_from_text(a.f[5].substr(0, c));
    if (q < 0) return -1;
    const auto sint = [](std::string_view s, size_t max_len, int64_t& v) {
      const bool neg = !s.empty() && s[0] == '-';
      if (neg) s.remove_prefix(1);
      if (!all_digits(s, max_len)) return false;
      v = 0;
      for (char ch : s) v = v * 10 + (ch - '0');
      if (neg) v = -v;
      return true;
    };
    int64_t x = 0, X2 = 0, m = 0, E = 0, D4 = 0;
    if (!sint(a.f[5].substr(c + 1), 10, x) || !sint(a.f[7], 11, X2)) return -1;
    sint(a.f[4], 10, m); sint(a.f[6], 10, E); sint(a.f[8], 11, D4);
    std::string& o = out[13];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    append_i64(o, m); o += '\t';
    append_i64(o, q / 1000);  // (the canonical text again: q / 1000 without trailing zeros)
    if (q % 1000) {
      char fr[4] = {(char)('0' + q % 1000 / 100), (char)('0' + q % 100 / 10), (char)('0' + q % 10), 0};
      int n = 3;
      while (fr[n - 1] == '0') --n;
      o += '.';
      o.append(fr, (size_t)n);
    }
    o += '\t';
    append_i64(o, x); o += '\t';
    append_i64(o, E); o += '\t';
    append_i64(o, X2); o += '\t';
    append_i64(o, D4); o += '\t';
    o += a.f[9];
    o += '\n';
    return 13;
  }
  if (t == "ls") {  // latency shift: timestamp, server, service, count, min_delta, rules json
    // (utils/records.py entry_from_csv and shift_rules_from_text hold the same rules) a row is dropped
    // whole unless it has exactly seven fields, n and minDelta are 1 to 10 plain digits and the last
    // field is 1 to 4 groups k:p:mB:T2:mR:X2:a:b:V -- k, mB, mR, a, b 1 to 10 plain digits, p a
    // percentile of at most three decimals below 100, T2 and X2 1 to 10 digits after an optional '-',
    // V one of U, D, N
    if (a.n != 7) return -1;
    for (int i = 4; i <= 5; ++i)
      if (!all_digits(a.f[i], 10)) return -1;
    if (a.f[6].empty()) return -1;
    std::string js = "[";
    {
      static const char* key[9] = {"{\"k\":", ",\"p\":", ",\"base\":", ",\"t2\":", ",\"recent\":", ",\"x2\":",
                                   ",\"above\":", ",\"below\":", ",\"verdict\":"};
      std::string_view rest = a.f[6];
      int groups = 0;
      for (;;) {
        const size_t e = rest.find(',');
        std::string_view g = rest.substr(0, e);
        if (++groups > 4) return -1;
        if (groups > 1) js += ',';
        for (int p = 0; p < 9; ++p) {
          const size_t c = g.find(':');
          if ((p < 8) == (c == std::string_view::npos)) return -1;  // (exactly nine parts)
          std::string_view part = g.substr(0, c);
          js += key[p];
          if (p == 8) {
            if (part != "U" && part != "D" && part != "N") return -1;
            js += '"';
            js += part;
            js += '"';
          } else if (p == 1) {
            const int64_t q = pct_from_text(part);
            if (q < 0 || q > 99999) return -1;
            js += '"';
            append_i64(js, q / 1000);  // (the canonical text again: q / 1000 without trailing zeros)
            if (q % 1000) {
              char fr[4] = {(char)('0' + q % 1000 / 100), (char)('0' + q % 100 / 10), (char)('0' + q % 10), 0};
              int n = 3;
              while (fr[n - 1] == '0') --n;
              js += '.';
              js.append(fr, (size_t)n);
            }
            js += '"';
          } else {
            const bool neg = (p == 3 || p == 5) && !part.empty() && part[0] == '-';
            if (neg) part.remove_prefix(1);
            if (!all_digits(part, 10)) return -1;
            int64_t v = 0;
            for (char ch : part) v = v * 10 + (ch - '0');
            append_i64(js, neg ? -v : v);
          }
          if (p < 8) g = g.substr(c + 1);
        }
        js += '}';
        if (e == std::string_view::npos) break;
        rest = rest.substr(e + 1);
      }
    }
    js += ']';
    std::string& o = out[14];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    for (int i = 4; i <= 5; ++i) {
      int64_t v = 0;
      for (char ch : a.f[i]) v = v * 10 + (ch - '0');
      append_i64(o, v); o += '\t';
    }
    copy_escape(o, js);
    o += '\n';
    return 14;
  }
  if (t == "ic") {  // incident: timestamp, server, service, source, event, code0, code, since, age, run
    // (utils/records.py entry_from_csv holds the same rules) a row is dropped whole unless it has
    // exactly eleven fields, the source is one of sb, tf, po, ls, the event one of O, S, C, code0 one
    // of B, D, S, H, L, U and code one of those or '-', since 1 to 15 plain digits and at most
    // 253402300799999 (the last ms of the year 9999), age 1 to 10 plain digits and run 1 to 3
    if (a.n != 11) return -1;
    const std::string_view src = a.f[4], ev = a.f[5], c0 = a.f[6], c1 = a.f[7];
    if (src != "sb" && src != "tf" && src != "po" && src != "ls") return -1;
    if (ev != "O" && ev != "S" && ev != "C") return -1;
    static const std::string_view kCodes = "BDSHLU";
    if (c0.size() != 1 || kCodes.find(c0[0]) == std::string_view::npos) return -1;
    if (c1.size() != 1 || (c1[0] != '-' && kCodes.find(c1[0]) == std::string_view::npos)) return -1;
    const std::string_view since = a.f[8];
    if (!all_digits(since, 15) || !all_digits(a.f[9], 10) || !all_digits(a.f[10], 3)) return -1;
    int64_t sv = 0;
    for (char ch : since) sv = sv * 10 + (ch - '0');
    std::string since_txt;
    if (sv > 253402300799999LL || !ts_text((double)sv, ' ', since_txt)) return -1;
    std::string& o = out[15];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2); o += '\t';
    c_str(o, a, 3); o += '\t';
    o += src; o += '\t';
    o += ev; o += '\t';
    o += c0; o += '\t';
    o += c1; o += '\t';
    o += since_txt; o += "+00\t";
    for (int i = 9; i <= 10; ++i) {
      int64_t v = 0;
      for (char ch : a.f[i]) v = v * 10 + (ch - '0');
      append_i64(o, v);
      o += i == 9 ? '\t' : '\n';
    }
    return 15;
  }
  if (t == "jx") {
    std::string& o = out[3];
    c_ts(o, a, 1); o += '\t';
    c_str(o, a, 2);
    for (int k = 0; k < 16; ++k) {
      o += '\t';
      const int i = 3 + k;
      c_num(o, !a.has(i) ? js::nan() : (k == 9 ? parse_float(a.f[i]) : js::parse_int(a.f[i])));
    }
    o += '\n';
    return 3;
  }
  return -1;
}

// Encode a newline-separated blob; counts[k] rows appended to out[k].
void encode_blob(std::string_view blob, std::string* out, int64_t* counts) {
  size_t i = 0;
  while (i < blob.size()) {
    size_t j = blob.find('\n', i);
    if (j == std::string_view::npos) j = blob.size();
    if (j > i) {
      const int k = encode_line(blob.substr(i, j - i), out);
      if (k >= 0) ++counts[k];
    }
    i = j + 1;
  }
}

}  // namespace copyenc
}  // namespace apm
