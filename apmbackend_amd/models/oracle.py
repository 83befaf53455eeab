"""Exact sequential CPU model of the reference pipeline semantics ("the oracle").

This module is the executable specification that every GPU kernel is tested against.  It
models *behaviour* of the reference stages, record-at-a-time, in double precision:

* ``ParseOracle``  -- log line -> ``tx`` records (``stream_parse_transactions.js:210-812``):
  SOAP account capture, EJB / standard CommonTiming entry-exit joins, BAF account salvage,
  the audit-trail state machine, and the three TTL caches (``NodeCache`` semantics with an
  injectable clock; expiry is lazy on ``get``/``has`` plus a sweep at every batch boundary).
* ``StatsOracle``  -- ``tx`` -> ``st`` + released ``tx`` (``stream_calc_stats.js:28-204,331-371``):
  10 s buckets, rollover on a newer bucket, the 31-bucket window / 30-bucket TPM divisor (Q2),
  the reference percentile formula (Q3), ordered release through a port of the JS binary heap.
* ``ZScoreOracle`` -- ``st`` -> ``fs`` (``stream_calc_z_score.js:66-311``): smoothed z-score per
  LAG with ``sqrt(mean)`` as sigma (Q1) and influence on the previous stored value.
* ``AlertsOracle`` -- ``fs`` -> ``al`` (``stream_process_alerts.js:348-471``): hard max, signal
  gates, alertOnBothOnly, the leaky counter (Q6) and the per-service cooldown (Q7).

Where the reference depends on wall-clock time (NodeCache TTLs, alert timestamps) the oracle
takes an explicit clock, which is what makes GPU-vs-oracle comparisons deterministic.
"""
from __future__ import annotations

import math
import re
import statistics
from collections import OrderedDict
from typing import Any, Callable, Dict, Iterable, List, Optional, Tuple

from ..utils import jsfmt
from ..utils.config import (as_bool, check_incidents, incidents, check_latency_shift, latency_shift, check_peer_outliers, check_recent_windows, check_slo_burn, check_traffic_watch,
                            gpu_opt, peer_outliers, slo_burn,
                            latency_objectives, leaderboard, recent_windows, service_window, traffic_watch,
                            window_percentiles, zscore_lag_settings)
from ..utils.records import (AlertEntry, FullStatEntry, IncidentEntry, LatencyHistEntry, LatencyShiftEntry, LeaderboardEntry, PeerEntry, RecentWindowEntry,
                             ServiceWindowEntry, SloBurnEntry, TrafficEntry,
                             StatEntry, TxEntry, WindowPctEntry, WindowSloEntry, entry_from_csv, hist_bin, hist_lower,
                             pct_ranks)
from ..utils.timeparse import TzOffset, convert_string_date_to_ms, default_tz

NAN = float("nan")


# ----------------------------------------------------------------------------- JS helpers

def _valid(v) -> bool:
    return v is not None and not (isinstance(v, float) and math.isnan(v))


def js_average(values: Iterable) -> Optional[float]:
    """Array.prototype.average (util_methods.js:10-24): mean of defined, non-NaN entries,
    summed left to right from 0 in double precision; ``None`` when there are none.

    A history list that offers ``float_view()`` (a float64 array, NaN = undefined; used by the
    bench-scale tests for LAG 8640) is summed by ``np.add.accumulate``: the same sequential
    left-to-right double additions, in C."""
    view = getattr(values, "float_view", None)
    if view is not None:
        import numpy as np
        a = view()
        a = a[~np.isnan(a)]
        return float(np.add.accumulate(a)[-1] / a.size) if a.size else None
    cnt = 0
    s = 0
    for v in values:
        if _valid(v):
            cnt += 1
            s = s + float(v)
    if cnt > 0:
        return s / cnt
    return None


def js_stddev(values: Iterable) -> Optional[float]:
    """Array.prototype.standardDeviation *as the reference computes it* (Q1):
    ``average()`` ignores its argument, so the result is ``sqrt(mean)`` (``None`` if the mean
    is 0/undefined, NaN if negative)."""
    vals = values if hasattr(values, "float_view") else list(values)
    avg = js_average(vals)
    if avg is None or (isinstance(avg, float) and math.isnan(avg)):
        return None
    avg_sq = avg  # the bug: this.average(squareDiffs) === this.average()
    if avg_sq and avg_sq != 0:
        return math.sqrt(avg_sq) if avg_sq > 0 else NAN
    return None


def true_stddev(values: Iterable) -> Optional[float]:
    vals = [float(v) for v in values if _valid(v)]
    if not vals:
        return None
    m = sum(vals) / len(vals)
    var = sum((v - m) ** 2 for v in vals) / len(vals)
    return math.sqrt(var) if var != 0 else None


def js_binary_insert(arr: List[float], v: float) -> None:
    """Array.prototype.binaryInsert(v, duplicate=true) (util_methods.js:57-95) with the default
    comparator.  NaN compares 'equal' to everything, so once a NaN is in the array the result
    is no longer sorted and depends on the insertion order -- reproduced exactly here."""
    lo, hi = 0, len(arr) - 1
    while lo <= hi:
        m = (lo + hi) >> 1
        a = arr[m]
        if a < v:
            lo = m + 1
        elif a > v:
            hi = m - 1
        else:  # equal, or either side NaN
            arr.insert(m, v)
            return
    arr.insert(lo, v)


def js_window_array(bucket_arrays) -> List[float]:
    """windowSortedElapTimes of generateAllStatsToQueue (stream_calc_stats.js:172-178): the
    window buckets binaryConcat'ed in key order.  Without NaN this is just the sorted union."""
    out: List[float] = []
    if not any(v != v for arr in bucket_arrays for v in arr):
        for arr in bucket_arrays:
            out.extend(arr)
        out.sort()
        return out
    for arr in bucket_arrays:
        for v in arr:
            js_binary_insert(out, v)
    return out


def calc_percentile(arr: List[float], percentile: float):
    """Array.prototype.calcPercentile (util_methods.js:112-142) on a sorted array."""
    n = len(arr)
    if n == 0:
        return None
    if percentile == 0:
        return arr[0]
    if percentile == 100:
        return arr[-1]
    index = (percentile / 100.0) * n - 1.0
    if n == 1 or index % 1 == 0:
        return arr[int(index)]
    index = int(math.ceil(index))
    if index == n - 1:
        return arr[index]
    return (arr[index] + arr[index + 1]) / 2


def percentile_ranks(n: int, percentile: float) -> Tuple[int, int]:
    """The (lo, hi) sorted ranks calc_percentile reads for a window of n samples; the value is
    ``(a[lo] + a[hi]) / 2`` when ``lo != hi`` else ``a[lo]``.  Shared with the GPU kernel."""
    if n <= 0:
        return (-1, -1)
    if percentile == 0:
        return (0, 0)
    if percentile == 100:
        return (n - 1, n - 1)
    index = (percentile / 100.0) * n - 1.0
    if n == 1 or index % 1 == 0:
        i = int(index)
        return (i, i)
    i = int(math.ceil(index))
    if i == n - 1:
        return (i, i)
    return (i, i + 1)


class JsBinaryHeap:
    """Port of binary_heap.js (min-heap by score) -- kept so the oracle reproduces the
    reference release order exactly, including the order of equal scores."""

    def __init__(self, score: Callable[[Any], float]):
        self.content: List[Any] = []
        self.score = score

    def push(self, el):
        self.content.append(el)
        self._bubble_up(len(self.content) - 1)

    def pop(self):
        result = self.content[0]
        end = self.content.pop()
        if self.content:
            self.content[0] = end
            self._sink_down(0)
        return result

    def peek(self):
        return self.content[0]

    def size(self):
        return len(self.content)

    def pop_all_le(self, score):
        out = []
        while self.content and self.score(self.peek()) <= score:
            out.append(self.pop())
        return out

    def _bubble_up(self, n):
        el = self.content[n]
        sc = self.score(el)
        while n > 0:
            pn = (n + 1) // 2 - 1
            parent = self.content[pn]
            if sc >= self.score(parent):
                break
            self.content[pn] = el
            self.content[n] = parent
            n = pn

    def _sink_down(self, n):
        length = len(self.content)
        el = self.content[n]
        es = self.score(el)
        while True:
            c2 = (n + 1) * 2
            c1 = c2 - 1
            swap = None
            c1s = None
            if c1 < length:
                c1s = self.score(self.content[c1])
                if c1s < es:
                    swap = c1
            if c2 < length:
                c2s = self.score(self.content[c2])
                if c2s < (es if swap is None else c1s):
                    swap = c2
            if swap is None:
                break
            self.content[n] = self.content[swap]
            self.content[swap] = el
            n = swap


# ----------------------------------------------------------------------------- TTL cache

class TTLCache:
    """NodeCache (v5) semantics with an injectable clock.

    ``set`` stamps expiry = now + ttl; ``get``/``has`` lazily expire (strict ``expiry < now``),
    emitting ``on_expired(key, value)``; ``sweep`` is the periodic ``_checkData``.
    """

    def __init__(self, ttl_s: float, clock: Callable[[], float],
                 on_expired: Optional[Callable[[str, Any], None]] = None):
        self.ttl_ms = ttl_s * 1000.0
        self.clock = clock
        self.on_expired = on_expired
        self.data: "OrderedDict[str, Tuple[Any, float]]" = OrderedDict()
        self.stats = {"hits": 0, "misses": 0, "keys": 0}

    def _check(self, key) -> bool:
        val, t = self.data[key]
        if t != 0 and t < self.clock():
            del self.data[key]
            if self.on_expired:
                self.on_expired(key, val)
            return False
        return True

    def set(self, key, value):
        # JS object semantics: re-setting an existing key keeps its position
        self.data[key] = (value, self.clock() + self.ttl_ms)
        return True

    def get(self, key):
        if key in self.data and self._check(key):
            self.stats["hits"] += 1
            return self.data[key][0]
        self.stats["misses"] += 1
        return None

    def has(self, key) -> bool:
        return key in self.data and self._check(key)

    def sweep(self):
        for key in list(self.data.keys()):
            if key in self.data:
                self._check(key)

    def __len__(self):
        return len(self.data)


# ----------------------------------------------------------------------------- parse oracle

_WS_SPLIT = re.compile(r"\s+")
_SOAP_LOG = re.compile(r"soap_io")
_SERVER_LOG = re.compile(r"server\.log")
_EJB_ENTRY = re.compile(r"INFO *\[CommonTiming] The EJB")
_EJB_EXIT = re.compile(r"INFO *\[CommonTiming] Total time")
_CT_ENTRY = re.compile(r"INFO *CommonTiming::Start")
_CT_EXIT = re.compile(r"INFO *CommonTiming::Stop")
_SOAP_IN = re.compile(r"^=== jbossId.*IO=I")
_SOAP_OUT = re.compile(r"^=== jbossId.*IO=O")
_SOAP_ACCT = re.compile(r"<accountNumber>", re.I)
_SOAP_ALT_KEY = re.compile(r"<key>AccountNumber</key>", re.I)
_SOAP_ALT_VALUE = re.compile(r"<value>")
_BAF_RX = re.compile(r"\[[^ ]+] +INFO ")
_AUTR_MAP = re.compile(r"INFO  auditTrailId=")
_AUTR_HDR = re.compile(r"^Audit Trail id *:")
_EL_START = re.compile(r": RequestTrace \[stopWatchList=")
_EL_END = re.compile(r"^]")
_SW_START = re.compile(r"<stopWatchList>")
_SW_END = re.compile(r"</stopWatchList>")
_SW_NAME = re.compile(r"<name>")
_SW_START_TS = re.compile(r"<startTime>")
_SW_STOP_TS = re.compile(r"<stopTime>")
_TOPLEVEL = re.compile(r"^S:")
_PROVIDER = re.compile(r"Provider\[", re.I)
_DIGITS = re.compile(r"^[0-9]+$")
_BRACKETS = re.compile(r"[\[\]]")


def _tok(arr: List[str], i: int) -> Optional[str]:
    return arr[i] if 0 <= i < len(arr) else None


def _s(x: Optional[str]) -> str:
    """Template-literal interpolation: undefined -> 'undefined'."""
    return "undefined" if x is None else x


def js_split_ws(s: str) -> List[str]:
    return _WS_SPLIT.split(s)


def xml_inner(line: str) -> str:
    """``line.replace(/<\\/.*/,'').replace(/.*>/,'')``"""
    return re.sub(r".*>", "", re.sub(r"</.*", "", line, count=1), count=1)


def normalize_service(service: str) -> str:
    """outputRecord's rewrite: first ``Provider[`` (any case) -> ``Provider:``, then the first ``]``
    removed (stream_parse_transactions.js:274)."""
    service = _PROVIDER.sub("Provider:", service, count=1)
    return service.replace("]", "", 1)


def file_kind(path: str) -> str:
    name = path.split("/")[-1]
    if _SOAP_LOG.search(name):
        return "SOAP"
    if _SERVER_LOG.search(name):
        return "SERVER"
    return "APP"


def server_of(path: str) -> str:
    parts = path.split("/")
    return parts[2] if len(parts) > 2 else "undefined"


class ParseOracle:
    """Sequential model of the transaction parser.

    ``emit(queue, csv_line)`` receives every produced record; ``queue`` is ``'transactions'``
    (the stats stage) or ``'db_insert'`` (non-Provider audit records, Q18).
    The clock is set with ``begin_batch(now_ms)``, which also performs the periodic sweep.
    """

    def __init__(self, emit: Callable[[str, str], None], tz: Optional[TzOffset] = None,
                 record_ttl=120, acct_ttl=120, need_ttl=30, server_fn: Callable[[str], str] = None):
        self.emit = emit
        self.server_fn = server_fn or server_of  # path -> server (reference: split('/')[2])
        self.tz = tz or default_tz()
        self.now = 0.0
        clock = lambda: self.now
        self.context: Dict[str, Dict[str, Any]] = {}
        self.acct_cache = TTLCache(acct_ttl, clock)
        self.record_cache = TTLCache(record_ttl, clock, self._record_expired)
        self.need_cache = TTLCache(need_ttl, clock, self._need_expired)
        self.counters = {"lines": 0, "expired_partials": 0, "need_expired": 0,
                         "ejb_exit_unmatched": 0, "invalid_acct": 0, "audit_errors": 0}

    # -- clock
    def begin_batch(self, now_ms: float):
        self.now = float(now_ms)
        # periodic check: need-cache checkperiod 10 s, others 30 s -- modelled as a sweep at
        # every batch boundary (the engine does the same).
        self.record_cache.sweep()
        self.need_cache.sweep()
        self.acct_cache.sweep()

    def _record_expired(self, log_id, m):
        self.counters["expired_partials"] += len(m)

    def _need_expired(self, log_id, need_map):
        for service, rec in list(need_map.items()):
            self.counters["need_expired"] += 1
            alt = rec.get("altAcctNum") or ""
            self.output_record(rec.get("server"), service, log_id, alt, rec.get("startTs"),
                               rec.get("endTs"), rec.get("elapsed"), rec.get("insertToDb") or False)

    # -- output
    def output_record(self, server, service, log_id, acct_num, start_ts, end_ts, elapsed,
                      insert_to_db=False):
        start_ms = convert_string_date_to_ms(start_ts, self.tz) if isinstance(start_ts, str) else start_ts
        end_ms = convert_string_date_to_ms(end_ts, self.tz) if isinstance(end_ts, str) else end_ts
        service = normalize_service(_s(service))
        if not jsfmt.js_truthy_num(start_ms):
            e = 0.0 if end_ms is None else end_ms  # JS: '' - n === -n
            start_ms = e - jsfmt.parse_int(elapsed)
        tx = TxEntry.make(server, service, _s(log_id) if log_id is not None else "undefined",
                          acct_num if acct_num is not None else "undefined",
                          start_ms, end_ms if end_ms is not None else "", elapsed,
                          "Y" if _TOPLEVEL.search(service) else "N")
        self.emit("db_insert" if insert_to_db else "transactions", tx.to_csv())

    # -- account handling
    def save_acct_num(self, acct: str, fp: str, source: str, alt_log_id: Optional[str] = None):
        acct = acct.strip()
        if not _DIGITS.match(acct):
            # reference: logs (and, through the $currLogFp typo, throws -- Q16 fixed)
            self.counters["invalid_acct"] += 1
            return
        if source == "bafmetainfo":
            log_id = alt_log_id
            if not log_id:
                return
        else:
            log_id = self.context[fp]["logId"]
        self.acct_cache.set(log_id, acct)
        if source != "bafmetainfo":
            self.context.pop(fp, None)
        need_map = self.need_cache.get(log_id)
        if need_map:
            srv = self.server_fn(fp)
            for service, rec in list(need_map.items()):
                self.output_record(srv, service, log_id, acct, rec.get("startTs"), rec.get("endTs"),
                                   rec.get("elapsed"))
                del need_map[service]

    def _baf_acct(self, line: str, fp: str, log_id: str, arr: List[str]) -> str:
        acct = ""
        if _BAF_RX.search(line):
            t = _tok(arr, 3) or ""
            t = re.sub(r".*]\[", "", t, count=1)
            t = _BRACKETS.sub("", t)
            parts = t.split(":")
            acct = parts[-1]
            if acct:
                self.save_acct_num(acct, fp, "bafmetainfo", log_id)
        return acct

    # -- SOAP
    def _soap(self, line: str, fp: str):
        if _SOAP_IN.search(line):
            tok = _tok(js_split_ws(line), 1)
            parts = (tok or "").split("=")
            self.context[fp] = {"logId": parts[1] if len(parts) > 1 else None}
        elif _SOAP_OUT.search(line):
            self.context.pop(fp, None)
        elif fp in self.context:
            if _SOAP_ACCT.search(line):
                parts = re.split(r"<|>", line.strip())
                self.save_acct_num(parts[2] if len(parts) > 2 else "", fp, "standard")
            elif _SOAP_ALT_KEY.search(line):
                self.context[fp] = dict(self.context[fp], pullNextValueFlag=True)
            elif _SOAP_ALT_VALUE.search(line) and self.context[fp].get("pullNextValueFlag"):
                parts = re.split(r"<|>", line.strip())
                self.save_acct_num(parts[2] if len(parts) > 2 else "", fp, "riskStrategy")

    # -- CommonTiming
    def _ejb_entry(self, line: str, server: str):
        arr = js_split_ws(line)
        log_id = _BRACKETS.sub("", arr[0])
        start_ts = f"{_s(_tok(arr, 1))} {_s(_tok(arr, 2))}"
        if log_id == "":
            return
        service = f"S:{_s(_tok(arr, 13))}"
        if not self.record_cache.has(log_id):
            self.record_cache.set(log_id, OrderedDict())
        m = self.record_cache.get(log_id)
        m[service] = {"server": server, "startTs": start_ts}  # Map.set keeps position

    def _ejb_exit(self, line: str, server: str):
        arr = js_split_ws(line)
        log_id = _BRACKETS.sub("", arr[0])
        end_ts = f"{_s(_tok(arr, 1))} {_s(_tok(arr, 2))}"
        service = f"S:{_s(_tok(arr, 9))}"
        elapsed = _tok(arr, 11)
        if log_id == "":
            self.output_record(server, service, "", "", "", end_ts, elapsed)
            return
        m = self.record_cache.get(log_id)
        if m is None:
            self.counters["ejb_exit_unmatched"] += 1
            return
        part = m.get(service)
        if part is None:
            self.counters["ejb_exit_unmatched"] += 1
            return
        acct = self.acct_cache.get(log_id)
        if acct:
            self.output_record(server, service, log_id, acct, part["startTs"], end_ts, elapsed)
        else:
            if not self.need_cache.has(log_id):
                self.need_cache.set(log_id, OrderedDict())
            nm = self.need_cache.get(log_id)
            nm[service] = dict(part, endTs=end_ts, elapsed=elapsed)
        del m[service]

    @staticmethod
    def _after_info(line: str) -> List[str]:
        parts = line.split("INFO")
        seg = parts[1] if len(parts) > 1 else ""
        return js_split_ws(seg.strip())

    def _ct_entry(self, line: str, server: str):
        arr = js_split_ws(line)
        log_id = _BRACKETS.sub("", arr[0])
        start_ts = f"{_s(_tok(arr, 1))} {_s(_tok(arr, 2))}"
        service = _s(_tok(self._after_info(line), 1))
        if log_id == "":
            return
        if not self.record_cache.has(log_id):
            self.record_cache.set(log_id, OrderedDict())
        m = self.record_cache.get(log_id)
        m[service] = {"server": server, "startTs": start_ts}  # Map.set keeps position

    def _salvage(self, line, fp, log_id, arr, server, service, end_ts, elapsed):
        acct = self._baf_acct(line, fp, log_id, arr)
        self.output_record(server, service, "", acct, "", end_ts, elapsed)

    def _ct_exit(self, line: str, fp: str, server: str):
        arr = js_split_ws(line)
        second = self._after_info(line)
        log_id = _BRACKETS.sub("", arr[0])
        end_ts = f"{_s(_tok(arr, 1))} {_s(_tok(arr, 2))}"
        service = _s(_tok(second, 1))
        elapsed = _tok(second, 5)
        m = self.record_cache.get(log_id)
        if log_id == "":
            self._salvage(line, fp, log_id, arr, server, service, end_ts, elapsed)
            return
        if m is None:
            self._salvage(line, fp, log_id, arr, server, service, end_ts, elapsed)
            return
        part = m.get(service)
        if part is None:
            self._salvage(line, fp, log_id, arr, server, service, end_ts, elapsed)
            return
        acct = self.acct_cache.get(log_id)
        if acct:
            self.output_record(server, service, log_id, acct, part["startTs"], end_ts, elapsed)
        else:
            if not self.need_cache.has(log_id):
                self.need_cache.set(log_id, OrderedDict())
            alt = self._baf_acct(line, fp, log_id, arr)
            nm = self.need_cache.get(log_id)
            if nm is None:  # expired between has() and get() cannot happen with a fixed clock
                nm = OrderedDict()
            nm[service] = dict(part, endTs=end_ts, elapsed=elapsed, altAcctNum=alt)
        del m[service]

    # -- audit trail
    def _app(self, line: str, fp: str, server: str):
        if _AUTR_MAP.search(line):
            arr = js_split_ws(line)
            log_id = _BRACKETS.sub("", arr[0])
            t5 = _tok(arr, 5) or ""
            parts = t5.split("=")
            autr_id = parts[1] if len(parts) > 1 else None
            if fp not in self.context:
                self.context[fp] = {"autrIdMap": OrderedDict()}
            ctx = self.context[fp]
            ctx.setdefault("autrIdMap", OrderedDict())
            alt = self._baf_acct(line, fp, log_id, arr)
            ctx["autrIdMap"][autr_id] = {"logId": log_id, "altAcctNum": alt}
        elif _AUTR_HDR.search(line):
            if fp in self.context:
                autr_id = line.split(":")[1].strip()
                ctx = self.context[fp]
                obj = (ctx.get("autrIdMap") or {}).get(autr_id)
                if not obj or not obj.get("logId"):
                    self.counters["audit_errors"] += 1
                else:
                    ctx["serviceMap"] = OrderedDict()
                    ctx["activeAutrId"] = autr_id
                    ctx["activeLogId"] = obj["logId"]
                    ctx["activeAltAcctNum"] = obj["altAcctNum"]
                    ctx["elapsedFlag"] = False
                    ctx["swFlag"] = False
                    ctx["activeService"] = None
                    del ctx["autrIdMap"][autr_id]
            else:
                self.counters["audit_errors"] += 1
        elif fp in self.context and self.context[fp].get("activeLogId"):
            ctx = self.context[fp]
            if _EL_START.search(line):
                ctx["elapsedFlag"] = True
            elif ctx.get("elapsedFlag"):
                if _EL_END.search(line):
                    ctx["elapsedFlag"] = False
                else:
                    arr = line.split(":")
                    service = arr[0].strip()
                    el_tok = js_split_ws(arr[1])[0] if len(arr) > 1 else ""
                    elapsed = _BRACKETS.sub("", el_tok)
                    ctx["serviceMap"].setdefault(service, []).append({"elapsed": elapsed})
            elif _SW_START.search(line):
                ctx["swFlag"] = True
            elif ctx.get("swFlag"):
                if _SW_END.search(line):
                    for k in ("activeAutrId", "activeLogId", "activeAltAcctNum", "activeService",
                              "serviceMap"):
                        ctx[k] = None
                    ctx["elapsedFlag"] = False
                    ctx["swFlag"] = False
                elif _SW_NAME.search(line):
                    ctx["activeService"] = xml_inner(line)
                elif ctx.get("activeService"):
                    svc = ctx["activeService"]
                    if _SW_START_TS.search(line):
                        lst = ctx["serviceMap"].get(svc)
                        if not lst:
                            self.counters["audit_errors"] += 1
                            return
                        lst[0]["startTs"] = xml_inner(line)
                    elif _SW_STOP_TS.search(line):
                        end_ts = xml_inner(line)
                        lst = ctx["serviceMap"].get(svc)
                        if not lst:
                            self.counters["audit_errors"] += 1
                            return
                        obj = lst.pop(0)
                        log_id = ctx["activeLogId"]
                        acct = self.acct_cache.get(log_id)
                        insert_to_db = not _PROVIDER.search(svc)
                        if acct:
                            self.output_record(server, svc, log_id, acct, obj.get("startTs"), end_ts,
                                               obj.get("elapsed"), insert_to_db)
                        else:
                            if not self.need_cache.has(log_id):
                                self.need_cache.set(log_id, OrderedDict())
                            nm = self.need_cache.get(log_id)
                            nm[svc] = {"server": server, "logId": log_id,
                                       "startTs": obj.get("startTs"), "endTs": end_ts,
                                       "elapsed": obj.get("elapsed"),
                                       "altAcctNum": ctx.get("activeAltAcctNum"),
                                       "insertToDb": insert_to_db}

    # -- dispatcher
    def read_line(self, fp: str, line: str):
        if not line:
            return
        self.counters["lines"] += 1
        server = self.server_fn(fp)
        kind = file_kind(fp)
        if kind == "SOAP":
            self._soap(line, fp)
        elif kind == "SERVER":
            if _EJB_ENTRY.search(line):
                self._ejb_entry(line, server)
            elif _EJB_EXIT.search(line):
                self._ejb_exit(line, server)
            elif _CT_ENTRY.search(line):
                self._ct_entry(line, server)
            elif _CT_EXIT.search(line):
                self._ct_exit(line, fp, server)
        else:
            if _CT_ENTRY.search(line):
                self._ct_entry(line, server)
            elif _CT_EXIT.search(line):
                self._ct_exit(line, fp, server)
            else:
                self._app(line, fp, server)


# ----------------------------------------------------------------------------- stats oracle

class StatsOracle:
    """``StatParser`` + ``consumeMsg`` of stream_calc_stats.js."""

    def __init__(self, emit_stat: Callable[[str], None], emit_db: Callable[[str], None],
                 interval_len=10, window=30, buffer=6, emit_hist: Optional[Callable[[str], None]] = None,
                 emit_pct: Optional[Callable[[str], None]] = None, percentiles: Iterable[int] = (),
                 emit_slo: Optional[Callable[[str], None]] = None, objectives: Optional[Dict[str, Any]] = None,
                 emit_top: Optional[Callable[[str], None]] = None, board: Optional[Dict[str, Any]] = None,
                 emit_svc: Optional[Callable[[str], None]] = None, svc_percentiles: Iterable[int] = (),
                 emit_recent: Optional[Callable[[str], None]] = None, recent_buckets: Iterable[int] = (),
                 recent_percentiles: Iterable[int] = (),
                 emit_burn: Optional[Callable[[str], None]] = None, burn: Optional[Dict[str, Any]] = None,
                 emit_traffic: Optional[Callable[[str], None]] = None, traffic: Optional[Dict[str, Any]] = None,
                 emit_peer: Optional[Callable[[str], None]] = None, peer: Optional[Dict[str, Any]] = None,
                 emit_shift: Optional[Callable[[str], None]] = None, shift: Optional[Dict[str, Any]] = None,
                 emit_incident: Optional[Callable[[str], None]] = None, incident: Optional[Dict[str, Any]] = None):
        self.emit_incident = emit_incident  # ic rows (docs/INCIDENTS.md); None = stream off
        self.incident = incident            # config.parse_incidents' result
        # (server, service, source) -> [code0 or "", since_ts, age, hot_run, clear_run]
        self.incident_state: Dict[Tuple[str, str, str], List[Any]] = {}
        self.emit_shift = emit_shift  # ls rows (docs/SHIFT.md); None = stream off
        self.shift = shift            # config.parse_latency_shift's result
        self.emit_peer = emit_peer  # po rows (docs/PEERS.md); None = stream off
        self.peer = peer            # config.parse_peer_outliers's result
        self.emit_traffic = emit_traffic  # tf rows (docs/TRAFFIC.md); None = stream off
        self.traffic = traffic            # config.parse_traffic_watch's result
        self.emit_burn = emit_burn  # sb rows (docs/BURN.md); None = stream off
        self.burn = burn            # config.parse_slo_burn's result
        self.emit_recent = emit_recent  # rw rows (docs/RECENT.md); None = stream off
        self.recent_buckets = [int(k) for k in recent_buckets]  # spans in buckets, ascending
        self.recent_percentiles = [int(q) for q in recent_percentiles]  # q = p * 1000
        self.emit_svc = emit_svc    # sv rows (docs/SERVICEWINDOW.md); None = stream off
        self.svc_percentiles = [int(q) for q in svc_percentiles]  # q = p * 1000 (config.service_window)
        self.emit_top = emit_top    # tk rows (docs/LEADERBOARD.md); None = stream off
        self.board = board          # config.parse_leaderboard's result: {"k", "by", "minTpm"}
        self.emit_slo = emit_slo    # sl rows (docs/OBJECTIVES.md); None = stream off
        # config.parse_latency_objectives' result: {"default": [T, ...], "services": {name: [T, ...]}}
        self.objectives = objectives or {"default": [], "services": {}}
        self.emit_hist = emit_hist  # lh rows (docs/HISTOGRAM.md); None = stream off
        self.emit_pct = emit_pct    # wp rows (docs/PERCENTILES.md); None = stream off
        self.percentiles = [int(q) for q in percentiles]  # q = p * 1000 (config.window_percentiles)
        self.emit_stat = emit_stat
        self.emit_db = emit_db
        self.interval_len = interval_len
        self.window = window
        self.buffer = buffer
        self.keep = window + buffer
        self.servers: "OrderedDict[str, OrderedDict[str, Dict[int, List[int]]]]" = OrderedDict()
        self.latest = 0
        self.heap = JsBinaryHeap(lambda tx: tx.endTs)
        self.rollovers = 0

    @staticmethod
    def bucket_label(end_ts) -> Optional[int]:
        s = jsfmt.js_str(end_ts)
        lab = s[:-4] if len(s) > 4 else ""
        try:
            return int(lab)
        except ValueError:
            return None

    def consume(self, csv_line: str):
        tx = entry_from_csv(csv_line)
        self.consume_tx(tx)

    def consume_tx(self, tx: TxEntry):
        lab = self.bucket_label(tx.endTs)
        if lab is None:
            return  # NaN/short endTs: the reference would wedge its heap (fix)
        if lab > self.latest:
            prev, self.latest = self.latest, lab
            self.rollover(prev)
        srv = self.servers.setdefault(tx.server, OrderedDict())
        svc = srv.setdefault(tx.service, {})
        svc.setdefault(lab, []).append(jsfmt.parse_int(tx.elapsed))
        self.heap.push(tx)

    def advance_to(self, latest: int):
        """Multi-rank lock-step (parallel/dist): another rank saw bucket ``latest`` -- roll
        over as the single reference stats process would have at that tx."""
        if latest > self.latest:
            prev, self.latest = self.latest, latest
            self.rollover(prev)

    def hist_rows(self, prev: int) -> List[str]:
        """The lh rows of the rollover from ``prev`` to ``self.latest``: every bucket that enters
        the window now (max(prev - buffer, latest - keep - 1) < b <= latest - buffer), ascending;
        inside a bucket the series in st order, those with a sample in it only."""
        rows = []
        lo = max(prev - self.buffer, self.latest - self.keep - 1)
        for b in range(lo + 1, self.latest - self.buffer + 1):
            for server, srv in self.servers.items():
                for service, svc in srv.items():
                    arr = svc.get(b)
                    if not arr:
                        continue
                    bins: Dict[int, int] = {}
                    nan = 0
                    for v in arr:
                        # the engine stores int32; anything else is its NaN sentinel (engine.cpp)
                        if v != v or not -2147483647 <= v <= 2147483647:
                            nan += 1
                        else:
                            k = hist_bin(int(v))
                            bins[k] = bins.get(k, 0) + 1
                    rows.append(LatencyHistEntry(b * 10000, server, service, len(arr), nan,
                                                 [(hist_lower(k), bins[k]) for k in sorted(bins)]).to_csv())
        return rows

    def pct_row(self, edge_ts: int, server: str, service: str, win: List[List[int]]) -> Optional[str]:
        """The wp row of one window (its buckets in key order): the percentiles of the samples
        that are not NaN, sorted ascending, by the integer rank rule; None when there is none."""
        flat = [v for arr in win for v in arr]
        # the engine stores int32; anything else is its NaN sentinel (engine.cpp)
        fin = sorted(int(v) for v in flat if v == v and -2147483647 <= v <= 2147483647)
        if not fin:
            return None
        pcts = []
        for q in self.percentiles:
            lo, hi = pct_ranks(len(fin), q)
            pcts.append((q, fin[lo] + fin[hi]))
        return WindowPctEntry(edge_ts, server, service, len(fin), len(flat) - len(fin), pcts).to_csv()

    def slo_row(self, edge_ts: int, server: str, service: str, win: List[List[int]]) -> Optional[str]:
        """The sl row of one window: for each threshold T of the service's objective, the number of
        samples that are not NaN with v <= T; None without a threshold or without such a sample."""
        thr = self.objectives["services"].get(service, self.objectives["default"])
        flat = [v for arr in win for v in arr]
        # the engine stores int32; anything else is its NaN sentinel (engine.cpp)
        fin = [int(v) for v in flat if v == v and -2147483647 <= v <= 2147483647]
        if not thr or not fin:
            return None
        le = [(t, sum(1 for v in fin if v <= t)) for t in thr]
        return WindowSloEntry(edge_ts, server, service, len(fin), len(flat) - len(fin), le).to_csv()

    def top_rows(self, st_rows: List[str]) -> List[str]:
        """The tk rows of one rollover from its st rows (in emission order): per board of
        ``self.board["by"]`` the k rows with the largest value of that field -- the value the st
        row carries, i.e. after its rounding -- among the rows whose value is not NaN and whose
        tpm is at least minTpm; ties keep the st order."""
        ents = [entry_from_csv(r) for r in st_rows]
        out: List[str] = []
        for key in self.board["by"]:
            cands = []
            for pos, e in enumerate(ents):
                v = getattr(e, key)
                if v is None or v != v or not e.tpm >= self.board["minTpm"]:
                    continue
                cands.append((-v, pos))
            cands.sort()
            for rank, (_, pos) in enumerate(cands[:self.board["k"]], 1):
                e = ents[pos]
                out.append(LeaderboardEntry(e.timestamp, key, rank, e.server, e.service, e.tpm, e.average, e.per75,
                                            e.per95).to_csv())
        return out

    def svc_rows(self, edge_ts: int, wins: "OrderedDict[str, List[List[int]]]") -> List[str]:
        """The sv rows of one rollover.  ``wins`` maps a service to the windows (flat sample lists)
        of its series with an st row, services in the order of their first st row: per service the
        series count, the samples that are not NaN (count, sum, percentiles by the integer rank
        rule over their union) and the NaN count; no row without such a sample."""
        rows = []
        for service, members in wins.items():
            flat = [v for w in members for v in w]
            # the engine stores int32; anything else is its NaN sentinel (engine.cpp)
            fin = sorted(int(v) for v in flat if v == v and -2147483647 <= v <= 2147483647)
            if not fin:
                continue
            pcts = []
            for q in self.svc_percentiles:
                lo, hi = pct_ranks(len(fin), q)
                pcts.append((q, fin[lo] + fin[hi]))
            rows.append(ServiceWindowEntry(edge_ts, service, len(members), len(fin), len(flat) - len(fin), sum(fin),
                                           pcts).to_csv())
        return rows

    def recent_rows(self, edge_ts: int, server: str, service: str, svc: Dict[int, List[int]]) -> List[str]:
        """The rw rows of one series with an st row: per configured span of k buckets, the samples
        of the window buckets newer than ``latest - buffer - min(k, window buckets)``: the count of
        those that are not NaN, the NaN count, the sum and the percentiles of the former by the
        integer rank rule (none when there is no such sample).  No row when the whole window is
        empty."""
        newest = self.latest - self.buffer
        n_win = self.keep - self.buffer + 1
        if not any(arr for b, arr in svc.items() if self.latest - self.keep <= b <= newest):
            return []
        rows = []
        for k in self.recent_buckets:
            lo = newest - min(k, n_win)
            flat = [v for b in sorted(svc) if lo < b <= newest for v in svc[b]]
            # the engine stores int32; anything else is its NaN sentinel (engine.cpp)
            fin = sorted(int(v) for v in flat if v == v and -2147483647 <= v <= 2147483647)
            pcts = []
            for q in self.recent_percentiles if fin else ():
                r0, r1 = pct_ranks(len(fin), q)
                pcts.append((q, fin[r0] + fin[r1]))
            rows.append(RecentWindowEntry(edge_ts, server, service, k, len(fin), len(flat) - len(fin), sum(fin),
                                          pcts).to_csv())
        return rows

    @staticmethod
    def _burn_counts(flat: List[Any], T: int) -> Tuple[int, int, int]:
        """(m, bad, nan) of a list of samples: the finite ones, those of them above T, the others."""
        # the engine stores int32; anything else is its NaN sentinel (engine.cpp)
        fin = [int(v) for v in flat if v == v and -2147483647 <= v <= 2147483647]
        return len(fin), sum(1 for v in fin if v > T), len(flat) - len(fin)

    def burn_row(self, edge_ts: int, server: str, service: str, svc: Dict[int, List[int]]) -> Optional[str]:
        """The sb row of one series with an st row: None unless its service has an objective and, for
        at least one rule (k, f), both the whole window and its newest min(k, window buckets)
        buckets hold at least minSamples finite samples and satisfy bad * 10^8 >= f * m * b
        (b = 100000 - q), in integers."""
        named = self.burn["services"]
        obj = named[service] if service in named else self.burn["default"]  # (a service named with null: no row)
        if obj is None:
            return None
        T, q = obj
        b = 100000 - q
        ms = self.burn["minSamples"]
        newest = self.latest - self.buffer
        n_win = self.keep - self.buffer + 1

        def burns(m: int, bad: int, f: int) -> bool:
            return m >= ms and bad * 10 ** 8 >= f * m * b

        m, bad, nan = self._burn_counts([v for k in sorted(svc) if self.latest - self.keep <= k <= newest
                                         for v in svc[k]], T)
        rules = []
        for k, f in self.burn["rules"]:
            lo = newest - min(k, n_win)
            mk, badk, _ = self._burn_counts([v for bk in sorted(svc) if lo < bk <= newest for v in svc[bk]], T)
            rules.append((k, f, mk, badk, burns(m, bad, f) and burns(mk, badk, f)))
        if not any(r[4] for r in rules):
            return None
        return SloBurnEntry(edge_ts, server, service, T, q, m, bad, nan, rules).to_csv()

    @staticmethod
    def traffic_rule(counts: List[int], k: int, r_d: int, r_s: int, z: int, min_rate: int,
                     min_buckets: int) -> Tuple[int, int, int, int, str]:
        """(B, R, med2, mad4, verdict) of one rule over the per-bucket counts of a window, oldest
        first: the newest min(k, len) buckets against the median / MAD of the others, in integers
        (docs/TRAFFIC.md)."""
        kk = min(k, len(counts))
        base = counts[:len(counts) - kk]
        B = len(base)
        R = sum(counts[B:])
        med2 = mad4 = 0
        if B:
            med2 = statistics.median_low(base) + statistics.median_high(base)
            dev = [abs(2 * c - med2) for c in base]
            mad4 = statistics.median_low(dev) + statistics.median_high(dev)
        verdict = "N"
        if B >= min_buckets and med2 >= 2 * min_rate:
            if r_d and 2000 * R <= r_d * kk * med2 and 4000 * R <= kk * (2000 * med2 - z * mad4):
                verdict = "D"
            elif r_s and 2000 * R >= r_s * kk * med2 and 4000 * R >= kk * (2000 * med2 + z * mad4):
                verdict = "S"
        return B, R, med2, mad4, verdict

    def traffic_row(self, edge_ts: int, server: str, service: str, svc: Dict[int, List[int]]) -> Optional[str]:
        """The tf row of one series with an st row: None unless its service has a minRate and at least
        one rule says D or S.  A bucket's count is its stored samples, NaN ones included; an absent
        bucket counts 0."""
        named = self.traffic["services"]
        min_rate = named[service] if service in named else self.traffic["default"]  # (named with null: no row)
        if min_rate is None:
            return None
        newest = self.latest - self.buffer
        counts = [len(svc.get(b, ())) for b in range(self.latest - self.keep, newest + 1)]
        rules = [(k,) + self.traffic_rule(counts, k, r_d, r_s, z, min_rate, self.traffic["minBuckets"])
                 for k, r_d, r_s, z in self.traffic["rules"]]
        if all(r[5] == "N" for r in rules):
            return None
        return TrafficEntry(edge_ts, server, service, sum(counts), min_rate, rules).to_csv()

    @staticmethod
    def peer_verdict(x: int, X2: int, D4: int, E: int, po: Dict[str, Any], min_value: int) -> str:
        """H, L or N of one eligible member (docs/PEERS.md), in integers."""
        if E < po["minPeers"] or X2 < 4 * min_value:
            return "N"
        r_h, r_l, z, floor4 = po["high"], po["low"], po["z"], 4 * po["minDelta"]
        if r_h and 2000 * x >= r_h * X2 and 4000 * x >= 2000 * X2 + z * D4 and 2 * x - X2 >= floor4:
            return "H"
        if r_l and 2000 * x <= r_l * X2 and 4000 * x <= 2000 * X2 - z * D4 and X2 - 2 * x >= floor4:
            return "L"
        return "N"

    def peer_member(self, win: List[List[int]]) -> Tuple[int, int]:
        """(m, x) of one window: its finite samples and the sum of the one or two ranks the integer
        rank rule reads for the configured percentile (twice the percentile; 0 without a sample)."""
        fin = sorted(int(v) for arr in win for v in arr if v == v and -2147483647 <= v <= 2147483647)
        if not fin:
            return 0, 0
        lo, hi = pct_ranks(len(fin), self.peer["percentile"])
        return len(fin), fin[lo] + fin[hi]

    def peer_rows(self, edge_ts: int, members: List[Tuple[str, str, int, int]]) -> List[str]:
        """The po rows of one rollover.  ``members``: (server, service, m, x) per st row, in st order.
        Per service the eligible members (a minValue, m >= minSamples) give X2 = x_lo + x_hi and
        D4 = d_lo + d_hi, d = |2 x - X2|; a row per eligible member with verdict H or L, in st order."""
        po = self.peer
        groups: Dict[str, List[int]] = {}
        for server, service, m, x in members:
            min_value = po["services"][service] if service in po["services"] else po["default"]
            if min_value is not None and m >= po["minSamples"]:
                groups.setdefault(service, []).append(x)
        base: Dict[str, Tuple[int, int, int]] = {}
        for service, xs in groups.items():
            X2 = statistics.median_low(xs) + statistics.median_high(xs)
            dev = [abs(2 * x - X2) for x in xs]
            base[service] = (len(xs), X2, statistics.median_low(dev) + statistics.median_high(dev))
        rows = []
        for server, service, m, x in members:
            min_value = po["services"][service] if service in po["services"] else po["default"]
            if min_value is None or m < po["minSamples"]:
                continue
            E, X2, D4 = base[service]
            v = self.peer_verdict(x, X2, D4, E, po, min_value)
            if v != "N":
                rows.append(PeerEntry(edge_ts, server, service, m, po["percentile"], x, E, X2, D4, v).to_csv())
        return rows

    @staticmethod
    def shift_rule(base: List[Any], recent: List[Any], q: int, r_u: int, r_d: int, z: int, min_delta: int,
                   min_recent: int, min_baseline: int) -> Tuple[int, int, int, int, int, int, str]:
        """(mB, T2, mR, X2, a, b, verdict) of one rule over the samples of the baseline buckets and of the
        recent span: the share of recent samples beyond the baseline's percentile against the share the
        percentile predicts, in integers (docs/SHIFT.md)."""
        S = 100000
        # the engine stores int32; anything else is its NaN sentinel (engine.cpp)
        fb = sorted(int(v) for v in base if v == v and -2147483647 <= v <= 2147483647)
        fr = sorted(int(v) for v in recent if v == v and -2147483647 <= v <= 2147483647)
        mB, mR = len(fb), len(fr)
        T2 = X2 = a = b = 0
        if mB:
            lo, hi = pct_ranks(mB, q)
            T2 = fb[lo] + fb[hi]
            a = sum(1 for v in fr if 2 * v > T2)
            b = sum(1 for v in fr if 2 * v < T2)
        if mR:
            lo, hi = pct_ranks(mR, q)
            X2 = fr[lo] + fr[hi]
        verdict = "N"
        if mB >= min_baseline and mR >= min_recent:
            var = z * z * mR * q * (S - q)
            if (r_u and X2 - T2 >= 2 * min_delta and 1000 * a * S >= r_u * mR * (S - q) and a * S >= mR * (S - q)
                    and (a * S - mR * (S - q)) ** 2 * 10 ** 6 >= var):
                verdict = "U"
            elif (r_d and T2 - X2 >= 2 * min_delta and 1000 * b * S >= r_d * mR * q and b * S >= mR * q
                    and (b * S - mR * q) ** 2 * 10 ** 6 >= var):
                verdict = "D"
        return mB, T2, mR, X2, a, b, verdict

    def shift_row(self, edge_ts: int, server: str, service: str, svc: Dict[int, List[int]]) -> Optional[str]:
        """The ls row of one series with an st row: None unless its service has a minDelta and at least
        one rule says U or D.  Rule (k, q, ...) sets the newest min(k, window buckets) buckets against
        the other buckets of the window."""
        named = self.shift["services"]
        min_delta = named[service] if service in named else self.shift["default"]  # (named with null: no row)
        if min_delta is None:
            return None
        newest = self.latest - self.buffer
        oldest = self.latest - self.keep
        n_win = self.keep - self.buffer + 1
        rules = []
        for k, q, r_u, r_d, z in self.shift["rules"]:
            lo = newest - min(k, n_win)
            base = [v for bk in sorted(svc) if oldest <= bk <= lo for v in svc[bk]]
            recent = [v for bk in sorted(svc) if lo < bk <= newest for v in svc[bk]]
            rules.append((k, q) + self.shift_rule(base, recent, q, r_u, r_d, z, min_delta, self.shift["minRecent"],
                                                  self.shift["minBaseline"]))
        if all(r[8] == "N" for r in rules):
            return None
        n = sum(len(svc[bk]) for bk in svc if oldest <= bk <= newest)
        return LatencyShiftEntry(edge_ts, server, service, n, min_delta, rules).to_csv()

    @staticmethod
    def incident_code(source: str, row: Optional[str]) -> str:
        """The code of one source at this rollover from the row its stream printed for the series
        ("" = not hot): sb ``B`` for any row; tf / ls the verdict of the lowest-numbered rule that is
        not N; po its letter."""
        if row is None:
            return ""
        if source == "sb":
            return "B"
        e = entry_from_csv(row)
        if source == "po":
            return e.verdict if e.verdict in ("H", "L") else ""
        for r in e.rules:
            if r[-1] != "N":
                return r[-1]
        return ""

    def incident_rows(self, edge_ts: int, codes: "OrderedDict[Tuple[str, str], Dict[str, str]]") -> List[str]:
        """One step of every (series, source) incident and the rows of the steps with an event.
        ``codes``: per series with an st row, in st order, its code per configured source.  This
        oracle prints an st row for every series it has ever seen, at every rollover, so every state
        it holds is stepped here, in st order: the "series without an st row" of docs/INCIDENTS.md
        cannot occur in it."""
        ic = self.incident
        remind = ic["remindEvery"]
        rows = []
        for server, service in codes:
            for src, (open_after, close_after) in ic["sources"].items():
                code = codes.get((server, service), {}).get(src, "")
                st = self.incident_state.setdefault((server, service, src), ["", 0, 0, 0, 0])
                hot = code != ""
                was_open = st[0] != ""
                if hot:
                    st[3], st[4] = min(st[3] + 1, 255), 0
                else:
                    st[4], st[3] = min(st[4] + 1, 255), 0
                event = ""
                if not was_open:
                    if hot and st[3] >= open_after:
                        st[0], st[1], st[2] = code, edge_ts, 0
                        event = "O"
                else:
                    st[2] = min(st[2] + 1, 2 ** 32 - 1)
                    if not hot and st[4] >= close_after:
                        event = "C"
                    elif remind and st[2] % remind == 0:
                        event = "S"
                if event:
                    rows.append(IncidentEntry(edge_ts, server, service, src, event, st[0], code or "-", st[1], st[2],
                                              st[3] if hot else st[4]).to_csv())
                if event == "C":
                    st[0] = ""
        return rows

    def rollover(self, prev: Optional[int] = None):
        self.rollovers += 1
        for srv in self.servers.values():
            for svc in srv.values():
                for b in [b for b in svc if b < self.latest - self.keep]:
                    del svc[b]
        edge_ts = (self.latest - self.buffer - 1) * 10000
        for tx in self.heap.pop_all_le(edge_ts):
            self.emit_db(tx.to_csv())
        if self.emit_hist is not None:
            for row in self.hist_rows(self.latest - 1 if prev is None else prev):
                self.emit_hist(row)
        st_rows: List[str] = []
        svc_wins: "OrderedDict[str, List[List[int]]]" = OrderedDict()
        peer_members: List[Tuple[str, str, int, int]] = []
        ic_codes: "OrderedDict[Tuple[str, str], Dict[str, str]]" = OrderedDict()
        ic_src = self.incident["sources"] if self.emit_incident is not None else {}
        for server, srv in self.servers.items():
            for service, svc in srv.items():
                win: List[List[int]] = []
                cnt = 0
                total = 0
                # bucket keys are integer-like, so Object.entries visits them ascending
                for b in sorted(svc):
                    arr = svc[b]
                    if self.latest - self.keep <= b <= self.latest - self.buffer:
                        cnt += len(arr)
                        for v in arr:
                            total += v
                        win.append(arr)
                avg = p75 = p95 = None
                if cnt != 0:
                    vals = js_window_array(win)
                    avg = total / cnt
                    p75 = calc_percentile(vals, 75)
                    p95 = calc_percentile(vals, 95)
                tpm = cnt / (self.window * self.interval_len / 60.0)
                st = StatEntry.make(edge_ts, server, service, tpm, avg, p75, p95)
                self.emit_stat(st.to_csv())
                if self.emit_top is not None:
                    st_rows.append(st.to_csv())
                if self.emit_svc is not None:
                    svc_wins.setdefault(service, []).append([v for arr in win for v in arr])
                if self.emit_pct is not None and cnt != 0:
                    row = self.pct_row(edge_ts, server, service, win)
                    if row is not None:
                        self.emit_pct(row)
                if self.emit_slo is not None and cnt != 0:
                    row = self.slo_row(edge_ts, server, service, win)
                    if row is not None:
                        self.emit_slo(row)
                if self.emit_recent is not None and cnt != 0:
                    for row in self.recent_rows(edge_ts, server, service, svc):
                        self.emit_recent(row)
                if self.emit_incident is not None:
                    ic_codes[(server, service)] = {}
                if self.emit_burn is not None:
                    row = self.burn_row(edge_ts, server, service, svc)
                    if row is not None:
                        self.emit_burn(row)
                    if "sb" in ic_src:
                        ic_codes[(server, service)]["sb"] = self.incident_code("sb", row)
                if self.emit_traffic is not None:
                    row = self.traffic_row(edge_ts, server, service, svc)
                    if row is not None:
                        self.emit_traffic(row)
                    if "tf" in ic_src:
                        ic_codes[(server, service)]["tf"] = self.incident_code("tf", row)
                if self.emit_peer is not None:
                    peer_members.append((server, service) + self.peer_member(win))
                if self.emit_shift is not None:
                    row = self.shift_row(edge_ts, server, service, svc)
                    if row is not None:
                        self.emit_shift(row)
                    if "ls" in ic_src:
                        ic_codes[(server, service)]["ls"] = self.incident_code("ls", row)
        if self.emit_top is not None:
            for row in self.top_rows(st_rows):
                self.emit_top(row)
        if self.emit_svc is not None:
            for row in self.svc_rows(edge_ts, svc_wins):
                self.emit_svc(row)
        if self.emit_peer is not None:
            for row in self.peer_rows(edge_ts, peer_members):
                self.emit_peer(row)
                if "po" in ic_src:
                    e = entry_from_csv(row)
                    ic_codes[(e.server, e.service)]["po"] = self.incident_code("po", row)
        if self.emit_incident is not None:
            for row in self.incident_rows(edge_ts, ic_codes):
                self.emit_incident(row)


# ----------------------------------------------------------------------------- z-score oracle

def process_zscore_stats(lag: int, threshold: float, influence: float, x: float,
                         prev: List[float], sigma_mode: str = "sqrt_mean"):
    """processZScoreStats (stream_calc_z_score.js:66-104). Returns (stored, avg, lb, ub, signal)."""
    infl = x
    avg = sd = lb = ub = None
    signal = 0
    if len(prev) >= lag:
        avg = js_average(prev)
        sd = js_stddev(prev) if sigma_mode == "sqrt_mean" else true_stddev(prev)
        ok = lambda v: v is not None and not (isinstance(v, float) and math.isnan(v))
        if ok(avg) and ok(sd):
            lb = avg - threshold * sd
            ub = avg + threshold * sd
        if not ok(avg) or not ok(sd):
            signal = 0
        elif not _valid(x):
            signal = 0
        elif abs(x - avg) > threshold * sd:
            signal = 1 if x > avg else -1
            last = prev[-1]
            if _valid(last):
                infl = influence * x + (1 - influence) * last
        else:
            signal = 0
    return infl, avg, lb, ub, signal


class ZScoreOracle:
    def __init__(self, cfg: Dict[str, Any], emit: Callable[[str], None],
                 emulate_aliasing: bool = False, sigma_mode: str = "sqrt_mean"):
        self.cfg = cfg
        self.emit = emit
        self.emulate_aliasing = emulate_aliasing
        self.sigma_mode = sigma_mode
        self.servers: "OrderedDict[str, OrderedDict[str, Dict[int, Dict[str, Any]]]]" = OrderedDict()

    def settings(self, service):
        return zscore_lag_settings(self.cfg, service, self.emulate_aliasing)

    def reload(self, cfg: Dict[str, Any]):
        """The watcher callback (stream_calc_z_score.js:362-382): updateAllServiceSettings --
        every series gets the new THRESHOLD / INFLUENCE of every configured LAG, a new LAG an
        empty history -- then removeStaleLagData drops the LAGs no longer configured."""
        self.cfg = cfg
        for srv in self.servers.values():
            for service, lags in srv.items():
                settings = self.settings(service)
                for el in settings:
                    lag = int(el["LAG"])
                    if lag in lags:
                        lags[lag]["THRESHOLD"], lags[lag]["INFLUENCE"] = el["THRESHOLD"], el["INFLUENCE"]
                    else:
                        lags[lag] = {"THRESHOLD": el["THRESHOLD"], "INFLUENCE": el["INFLUENCE"],
                                     "avgList": [], "per75List": [], "per95List": []}
                keep = {int(el["LAG"]) for el in settings}
                for lag in [x for x in lags if x not in keep]:
                    del lags[lag]

    def consume(self, csv_line: str):
        e = entry_from_csv(csv_line)
        if e is not None and e.type == "st":
            for fs in self.process(e):
                self.emit(fs.to_csv())

    def process(self, st: StatEntry) -> List[FullStatEntry]:
        srv = self.servers.setdefault(st.server, OrderedDict())
        if st.service not in srv:
            lags: Dict[int, Dict[str, Any]] = {}
            for el in self.settings(st.service):
                lags[int(el["LAG"])] = {"THRESHOLD": el["THRESHOLD"], "INFLUENCE": el["INFLUENCE"],
                                        "avgList": [], "per75List": [], "per95List": []}
            srv[st.service] = lags
        out = []
        for lag in sorted(srv[st.service].keys()):
            o = srv[st.service][lag]
            T, I = o["THRESHOLD"], o["INFLUENCE"]
            a = process_zscore_stats(lag, T, I, st.average, o["avgList"], self.sigma_mode)
            p = process_zscore_stats(lag, T, I, st.per75, o["per75List"], self.sigma_mode)
            q = process_zscore_stats(lag, T, I, st.per95, o["per95List"], self.sigma_mode)
            for key in ("avgList", "per75List", "per95List"):
                if len(o[key]) >= lag:
                    o[key].pop(0)
            f = lambda v: NAN if v is None else v
            out.append(FullStatEntry.make(
                st.timestamp, st.server, st.service, st.tpm, str(lag),
                st.average, f(a[1]), f(a[2]), f(a[3]), a[4],
                st.per75, f(p[1]), f(p[2]), f(p[3]), p[4],
                st.per95, f(q[1]), f(q[2]), f(q[3]), q[4]))
            o["avgList"].append(a[0])
            o["per75List"].append(p[0])
            o["per95List"].append(q[0])
        return out


# ----------------------------------------------------------------------------- alerts oracle

ALERT_CAUSES = ["average exceeded hard ms threshold", "per75 exceeded hard ms threshold",
                "average UB exceeded", "per75 UB exceeded", "average and per75 UB exceeded"]


class AlertsOracle:
    def __init__(self, cfg: Dict[str, Any], clock: str = "entry",
                 wall: Callable[[], float] = None, cooldown_key: str = "service"):
        self.cfg = cfg
        self.clock = clock
        self.wall = wall
        self.cooldown_key = cooldown_key
        self.recent: Dict[Tuple[str, str, str], int] = {}
        self.alerts: Dict[str, AlertEntry] = {}
        self.alert_buffer: List[AlertEntry] = []

    def process(self, en: FullStatEntry) -> Optional[AlertEntry]:
        ac = self.cfg["streamProcessAlerts"]
        key = (en.server, en.service, str(en.lag))
        cnt = self.recent.get(key, 0)
        window = int(ac["rollingAlertWindowSizeInIntervals"])
        thresh = int(ac["requiredNumberBadIntervalsInAlertWindowToTrigger"])
        state = {"cnt": cnt, "inc": False, "trigger": False}
        causes: List[str] = []

        def alert(cause):
            if not state["inc"]:
                if state["cnt"] <= window:
                    state["cnt"] += 1
                state["inc"] = True
            if window and window > 1 and thresh and thresh > 1:
                if state["cnt"] >= thresh:
                    state["trigger"] = True
                    causes.append(cause)
            else:
                state["trigger"] = True
                causes.append(cause)

        ovr = ((ac.get("overrides") or {}).get("services") or {}).get(en.service)
        lag_i = jsfmt.parse_int(en.lag)
        if lag_i not in [int(x) for x in ac.get("suppressedLags", [])]:
            if en.service not in ac.get("suppressedServices", []):
                hard_max = ac["hardMaxMsAlertThreshold"]
                if ovr is not None and ovr.get("hardMaxMsAlertThreshold"):
                    hard_max = ovr["hardMaxMsAlertThreshold"]
                gt = lambda a, b: _valid(a) and a > b
                if gt(en.average, hard_max):
                    alert(ALERT_CAUSES[0])
                if gt(en.per75, hard_max):
                    alert(ALERT_CAUSES[1])
                both = 0
                mn, mt = ac["hardMinMsAlertThreshold"], ac["hardMinTpmAlertThreshold"]
                if gt(en.averageSignal, 0) and gt(en.average, mn) and gt(en.tpm, mt):
                    if not ac["alertOnBothOnly"]:
                        alert(ALERT_CAUSES[2])
                    else:
                        both += 1
                if gt(en.per75Signal, 0) and gt(en.per75, mn) and gt(en.tpm, mt):
                    if not ac["alertOnBothOnly"]:
                        alert(ALERT_CAUSES[3])
                    else:
                        both += 1
                if ac["alertOnBothOnly"] and both >= 2:
                    alert(ALERT_CAUSES[4])
        if not state["inc"] and state["cnt"] > 0:
            state["cnt"] -= 1
        if state["cnt"] < 0:
            state["cnt"] = 0
        self.recent[key] = state["cnt"]
        if not state["trigger"]:
            return None
        now = en.timestamp if self.clock == "entry" else self.wall()
        al = AlertEntry.make(now, en.timestamp, en.server, en.service, ",".join(causes), en.to_csv())
        return al if self.admit(al) else None

    def cooldown_key_of(self, server: str, service: str) -> str:
        return service if self.cooldown_key == "service" else f"{server}\x00{service}"

    def admit(self, al: AlertEntry) -> bool:
        """The per-service cooldown (:436-468): the first candidate in emission order wins."""
        ac = self.cfg["streamProcessAlerts"]
        ck = self.cooldown_key_of(al.server, al.service)
        last = self.alerts.get(ck)
        if last is None or (al.alertTimestamp - last.alertTimestamp) / 1000 > ac["perServiceAlertCooldownInMinutes"] * 60:
            self.alerts[ck] = al
            self.alert_buffer.append(al)
            return True
        return False

    def evaluate(self, en: FullStatEntry) -> Optional[AlertEntry]:
        """The leaky counter alone: the candidate an fs row raises, before the cooldown."""
        saved, self.admit = self.admit, (lambda al: True)
        try:
            return self.process(en)
        finally:
            self.admit = saved


# ----------------------------------------------------------------------------- full chain

class PipelineOracle:
    """parse -> stats -> z-score -> alerts, with the queues modelled as in-order FIFOs."""

    def __init__(self, cfg: Dict[str, Any], tz: Optional[TzOffset] = None, alert_clock="entry",
                 server_fn: Callable[[str], str] = None,
                 node_exchange: Optional[Callable[[list], list]] = None,
                 server_index: Optional[Dict[str, int]] = None):
        """``node_exchange`` (multi-rank, servers sharded over ranks): the cooldown is decided
        node-wide.  Alert candidates are queued with their global emission-order key and, after
        every batch, ``node_exchange(mine)`` returns every rank's candidates; each rank applies
        the same cooldown in the same order and keeps its own winners (engine.cpp "node-wide
        cooldown").  ``server_index``: node-wide server positions (the key's tie-break within
        one batch)."""
        self.cfg = cfg
        self.node_exchange = node_exchange
        self.server_index = server_index or {}
        self._batch_no = 0
        self._first_batch: Dict[str, int] = {}
        self._svc_seq: Dict[Tuple[str, str], int] = {}
        self._node_q: list = []
        self._fs_no = 0
        self.tx_db: List[str] = []
        self.audit_db: List[str] = []
        self.stats: List[str] = []
        self.fs: List[str] = []
        self.al: List[str] = []
        self.tx_out: List[str] = []
        self.lh: List[str] = []
        self.wp: List[str] = []
        self.sl: List[str] = []
        self.tk: List[str] = []
        self.sv: List[str] = []
        self.rw: List[str] = []
        self.sb: List[str] = []
        self.tf: List[str] = []
        self.po: List[str] = []
        self.ls: List[str] = []
        self.ic: List[str] = []
        g = cfg.get("gpu", {})
        self.zs = ZScoreOracle(cfg, self._on_fs, g.get("emulateOverrideAliasing", False),
                               g.get("zscoreSigma", "sqrt_mean"))
        self.alerts = AlertsOracle(cfg, alert_clock, cooldown_key=g.get("cooldownKey", "service"))
        sc = cfg["streamCalcStats"]
        # (as APMEngine does: a span is at most windowSizeInIntervals at construction; reload() may
        # shorten the window later, and the span then reads the whole window)
        check_recent_windows(recent_windows(cfg), int(sc["windowSizeInIntervals"]))
        check_slo_burn(slo_burn(cfg), int(sc["windowSizeInIntervals"]))  # (likewise)
        check_traffic_watch(traffic_watch(cfg), int(sc["windowSizeInIntervals"]))  # (likewise)
        check_peer_outliers(peer_outliers(cfg))
        check_latency_shift(latency_shift(cfg), int(sc["windowSizeInIntervals"]))  # (as check_traffic_watch)
        check_incidents(incidents(cfg), cfg)
        self.st = StatsOracle(self._on_st, self.tx_db.append, int(sc["intervalLengthInSeconds"]),
                              int(sc["windowSizeInIntervals"]), int(sc["bufferSizeInIntervals"]),
                              emit_hist=self.lh.append if as_bool(gpu_opt(cfg, "latencyHistogram")) else None,
                              emit_pct=self.wp.append if window_percentiles(cfg) else None,
                              percentiles=window_percentiles(cfg),
                              emit_slo=self.sl.append if latency_objectives(cfg) else None,
                              objectives=latency_objectives(cfg),
                              emit_top=self.tk.append if leaderboard(cfg) else None,
                              board=leaderboard(cfg),
                              emit_svc=self.sv.append if service_window(cfg) else None,
                              svc_percentiles=service_window(cfg),
                              emit_recent=self.rw.append if recent_windows(cfg) else None,
                              recent_buckets=(recent_windows(cfg) or {}).get("buckets", ()),
                              recent_percentiles=(recent_windows(cfg) or {}).get("percentiles", ()),
                              emit_burn=self.emit_burn if slo_burn(cfg) else None, burn=slo_burn(cfg),
                              emit_traffic=self.tf.append if traffic_watch(cfg) else None, traffic=traffic_watch(cfg),
                              emit_peer=self.po.append if peer_outliers(cfg) else None, peer=peer_outliers(cfg),
                              emit_shift=self.ls.append if latency_shift(cfg) else None, shift=latency_shift(cfg),
                              emit_incident=self.ic.append if incidents(cfg) else None, incident=incidents(cfg))
        self.parse = ParseOracle(self._on_tx, tz, g.get("recordTtlSeconds", 120),
                                 g.get("acctTtlSeconds", 120), g.get("needTtlSeconds", 30), server_fn=server_fn)

    def reload(self, cfg: Dict[str, Any]):
        """Config hot reload between two batches: z-score settings / LAG set (ZScoreOracle.reload)
        and every alert gate (read from the config per fs entry)."""
        self.cfg = cfg
        self.zs.reload(cfg)
        self.alerts.cfg = cfg
        # stream_calc_stats.js watcher (:228-261): getParseSettings re-read, used from the next
        # rollover (removeOldBuckets / window / TPM divisor / edge)
        sc = cfg["streamCalcStats"]
        st = self.st
        st.interval_len = int(sc["intervalLengthInSeconds"])
        st.window = int(sc["windowSizeInIntervals"])
        st.buffer = int(sc["bufferSizeInIntervals"])
        st.keep = st.window + st.buffer

    def _on_tx(self, queue, line):
        if queue == "db_insert":
            self.audit_db.append(line)
        else:
            self.tx_out.append(line)
            n = len(self.st.servers)
            self.st.consume(line)
            if len(self.st.servers) != n:  # a server's first series: its node-wide order key
                for srv in list(self.st.servers)[n:]:
                    self._first_batch.setdefault(srv, self._batch_no)

    def emit_burn(self, line):
        """One sb row (docs/BURN.md) of the stats stage: kept in ``self.sb``."""
        self.sb.append(line)

    def _on_st(self, line):
        self.stats.append(line)
        self.zs.consume(line)

    def _on_fs(self, line):
        self.fs.append(line)
        en = entry_from_csv(line)
        if self.node_exchange is not None:
            al = self.alerts.evaluate(en)
            if al is not None:
                sk = (en.server, en.service)
                if sk not in self._svc_seq:
                    self._svc_seq[sk] = list(self.st.servers[en.server]).index(en.service)
                self._fs_no += 1
                key = (int(en.timestamp), self._first_batch.get(en.server, -1),
                       self.server_index.get(en.server, 0), self._svc_seq[sk], self._fs_no)
                self._node_q.append((key, al.to_csv()))
            return
        al = self.alerts.process(en)
        if al is not None:
            self.al.append(al.to_csv())

    def _node_resolve(self):
        mine = set(c for _k, c in self._node_q)
        every = self.node_exchange(self._node_q)
        self._node_q = []
        for _key, csv in sorted(every):
            al = entry_from_csv(csv)
            if self.alerts.admit(al) and csv in mine:
                self.al.append(csv)

    def run_batches(self, batches: Iterable[Tuple[float, List[Tuple[str, List[str]]]]],
                    sync_latest: Optional[Callable[[int], int]] = None):
        """batches: (now_ms, [(file_path, [lines...]), ...]).  ``sync_latest`` (multi-rank)
        maps this rank's latest bucket to the global one after every batch."""
        for now, chunks in batches:
            self.parse.begin_batch(now)
            for fp, lines in chunks:
                for ln in lines:
                    self.parse.read_line(fp, ln)
            if sync_latest is not None:
                self.st.advance_to(sync_latest(self.st.latest))
            if self.node_exchange is not None:
                self._node_resolve()
            self._batch_no += 1
