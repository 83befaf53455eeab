"""Record types and wire codecs (reference ``entries.js:1-342``).

Five record kinds travel between stages, pipe-delimited UTF-8 text:

====  =====================================================================================
tx    ``tx|server|service|logId|acctNum|startTs|endTs|elapsed|topLevel``        (entries.js:19)
st    ``st|ts|server|service|tpm(.2)|avg(.1)|p75(.1)|p95(.1)``                  (entries.js:72)
fs    ``fs|ts|server|service|lag|tpm|avg:avgAvg:avgLB:avgUB:avgSig|p75:...|p95:...`` (:117)
al    ``al|alertTs|entryTs|server|service|cause|<fs with '|' -> '&'>``            (:215)
jx    ``jx|ts|server|<16 JVM gauges>``                                             (:307)
====  =====================================================================================

Every numeric field is parsed with JS ``parseInt``/``parseFloat`` semantics and printed
with JS ``toFixed``/``String`` semantics (``jsfmt``), so a record that round-trips through
this module is byte-identical to what the reference stages produce.
``to_pg_row`` mirrors ``toPostgresObject`` (the inferred Postgres schema).
"""
from __future__ import annotations

import datetime as _dt
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Union

from .jsfmt import js_str, nf, parse_float, parse_int

Num = Union[int, float]


def _ms_to_dt(ms: Num) -> Optional[_dt.datetime]:
    if ms is None or (isinstance(ms, float) and math.isnan(ms)):
        return None
    return _dt.datetime.fromtimestamp(float(ms) / 1000.0, tz=_dt.timezone.utc)


def _num_or_none(x):
    if x is None or (isinstance(x, float) and math.isnan(x)):
        return None
    return x


@dataclass
class TxEntry:
    server: str
    service: str
    logId: str
    acctNum: Num
    startTs: Num
    endTs: Num
    elapsed: Num
    topLevel: str
    type: str = "tx"

    @classmethod
    def make(cls, server, service, logId, acctNum, startTs, endTs, elapsed, topLevel) -> "TxEntry":
        return cls(server, service, logId, parse_int(acctNum), parse_int(startTs),
                   parse_int(endTs), parse_int(elapsed), topLevel)

    def to_csv(self) -> str:
        return (f"tx|{self.server}|{self.service}|{self.logId}|{js_str(self.acctNum)}|"
                f"{js_str(self.startTs)}|{js_str(self.endTs)}|{js_str(self.elapsed)}|{self.topLevel}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {
            "endts": _ms_to_dt(self.endTs),
            "startts": _ms_to_dt(self.startTs),
            "server": self.server,
            "service": self.service,
            "logid": self.logId,
            "acctnum": _num_or_none(self.acctNum),
            "elapsed": _num_or_none(self.elapsed),
            "toplevel": self.topLevel,
        }


@dataclass
class StatEntry:
    timestamp: Num
    server: str
    service: str
    tpm: float
    average: float
    per75: float
    per95: float
    type: str = "st"

    @classmethod
    def make(cls, timestamp, server, service, tpm, average, per75, per95) -> "StatEntry":
        return cls(parse_int(timestamp), server, service, parse_float(tpm), parse_float(average),
                   parse_float(per75), parse_float(per95))

    def to_csv(self) -> str:
        return (f"st|{js_str(self.timestamp)}|{self.server}|{self.service}|{nf(self.tpm, 2)}|"
                f"{nf(self.average)}|{nf(self.per75)}|{nf(self.per95)}")


@dataclass
class FullStatEntry:
    timestamp: Num
    server: str
    service: str
    tpm: float
    lag: Any
    average: float
    averageAvg: float
    averageLB: float
    averageUB: float
    averageSignal: Num
    per75: float
    per75Avg: float
    per75LB: float
    per75UB: float
    per75Signal: Num
    per95: float
    per95Avg: float
    per95LB: float
    per95UB: float
    per95Signal: Num
    type: str = "fs"

    @classmethod
    def make(cls, timestamp, server, service, tpm, lag, average, averageAvg, averageLB, averageUB,
             averageSignal, per75, per75Avg, per75LB, per75UB, per75Signal, per95, per95Avg,
             per95LB, per95UB, per95Signal) -> "FullStatEntry":
        pf, pi = parse_float, parse_int
        return cls(pi(timestamp), server, service, pf(tpm), lag,
                   pf(average), pf(averageAvg), pf(averageLB), pf(averageUB), pi(averageSignal),
                   pf(per75), pf(per75Avg), pf(per75LB), pf(per75UB), pi(per75Signal),
                   pf(per95), pf(per95Avg), pf(per95LB), pf(per95UB), pi(per95Signal))

    def to_csv(self) -> str:
        # averageSignal is printed raw, the percentile signals through nf (entries.js:117, Q22)
        return (f"fs|{js_str(self.timestamp)}|{self.server}|{self.service}|{self.lag}|{nf(self.tpm, 2)}|"
                f"{nf(self.average)}:{nf(self.averageAvg)}:{nf(self.averageLB)}:{nf(self.averageUB)}:"
                f"{js_str(self.averageSignal)}|"
                f"{nf(self.per75)}:{nf(self.per75Avg)}:{nf(self.per75LB)}:{nf(self.per75UB)}:"
                f"{nf(self.per75Signal)}|"
                f"{nf(self.per95)}:{nf(self.per95Avg)}:{nf(self.per95LB)}:{nf(self.per95UB)}:"
                f"{nf(self.per95Signal)}")

    def to_pg_row(self) -> Dict[str, Any]:
        n = _num_or_none
        return {
            "timestamp": _ms_to_dt(self.timestamp),
            "server": self.server,
            "service": self.service,
            "tpm": n(self.tpm),
            "lag": self.lag,
            "stats": {
                "average": n(self.average), "averageavg": n(self.averageAvg),
                "averagelb": n(self.averageLB), "averageub": n(self.averageUB),
                "averagesignal": n(self.averageSignal),
                "per75": n(self.per75), "per75avg": n(self.per75Avg), "per75lb": n(self.per75LB),
                "per75ub": n(self.per75UB), "per75signal": n(self.per75Signal),
                "per95": n(self.per95), "per95avg": n(self.per95Avg), "per95lb": n(self.per95LB),
                "per95ub": n(self.per95UB), "per95signal": n(self.per95Signal),
            },
        }


@dataclass
class AlertEntry:
    alertTimestamp: Num
    entryTimestamp: Num
    server: str
    service: str
    cause: str
    entry: str  # fs CSV with '|' replaced by '&'
    type: str = "al"

    @classmethod
    def make(cls, alertTimestamp, entryTimestamp, server, service, cause, entry) -> "AlertEntry":
        return cls(parse_int(alertTimestamp), parse_int(entryTimestamp), server, service, cause,
                   entry.replace("|", "&"))

    def to_csv(self) -> str:
        return (f"al|{js_str(self.alertTimestamp)}|{js_str(self.entryTimestamp)}|{self.server}|"
                f"{self.service}|{self.cause}|{self.entry}")

    def fs_entry(self) -> "FullStatEntry":
        return entry_from_csv(self.entry, "&")  # type: ignore[return-value]

    def to_pg_row(self) -> Dict[str, Any]:
        return {
            "alerttimestamp": _ms_to_dt(self.alertTimestamp),
            "entrytimestamp": _ms_to_dt(self.entryTimestamp),
            "server": self.server,
            "service": self.service,
            "cause": self.cause,
            "entry": self.fs_entry().to_pg_row(),
        }


JMX_FIELDS = ["dsInUseNodes", "dsActiveNodes", "dsAvailableNodes", "heapUsed", "heapCommitted",
              "heapMax", "metaUsed", "metaCommitted", "metaMax", "sysLoad", "classCnt",
              "threadCnt", "daemonThreadCnt", "beanPoolAvailableCount", "beanPoolCurrentSize",
              "beanPoolMaxSize"]
JMX_PG = ["dsinusenodes", "dsactivenodes", "dsavailablenodes", "heapused", "heapcommitted",
          "heapmax", "metaused", "metacommitted", "metamax", "sysload", "classcnt", "threadcnt",
          "daemonthreadcnt", "beanpoolavailablecnt", "beanpoolcurrentsize", "beanpoolmaxsize"]


@dataclass
class JmxEntry:
    timestamp: Num
    server: str
    values: List[Num] = field(default_factory=list)
    type: str = "jx"

    @classmethod
    def from_stats(cls, timestamp, server, stats: Dict[str, Any]) -> "JmxEntry":
        """Constructor used by the poller (entries.js:246-273)."""
        pi = parse_int
        r = lambda k: stats[k]["result"]
        vals = [
            pi(r("ds")["InUseCount"]), pi(r("ds")["ActiveCount"]), pi(r("ds")["AvailableCount"]),
            pi(r("heap")["used"]), pi(r("heap")["committed"]), pi(r("heap")["max"]),
            pi(r("meta")["used"]), pi(r("meta")["committed"]), pi(r("meta")["max"]),
            parse_float(r("sysload")),
            pi(r("classcnt")),
            pi(r("threading")["thread-count"]), pi(r("threading")["daemon-thread-count"]),
            pi(r("bean")[0]["result"]["pool-available-count"]),
            pi(r("bean")[0]["result"]["pool-current-size"]),
            pi(r("bean")[0]["result"]["pool-max-size"]),
        ]
        return cls(pi(timestamp), server, vals)

    @classmethod
    def make(cls, timestamp, server, *vals) -> "JmxEntry":
        out = []
        for name, v in zip(JMX_FIELDS, vals):
            out.append(parse_float(v) if name == "sysLoad" else parse_int(v))
        return cls(parse_int(timestamp), server, out)

    def to_csv(self) -> str:
        return "jx|" + "|".join([js_str(self.timestamp), self.server] + [js_str(v) for v in self.values])

    def to_pg_row(self) -> Dict[str, Any]:
        row = {"timestamp": _ms_to_dt(self.timestamp), "server": self.server}
        for k, v in zip(JMX_PG, self.values):
            row[k] = _num_or_none(v)
        return row


def _pad(arr: List[str], n: int) -> List[Optional[str]]:
    return list(arr) + [None] * max(0, n - len(arr))


@dataclass
class FleetEntry:
    """``fb|ts|service|lag|nseries|avgMean:avgStd|p75Mean:p75Std|p95Mean:p95Std`` -- the
    fleet-merged per-service baseline (no reference counterpart: the reference has one process
    per stage and no cross-JVM view).  Emitted by rank 0 after each interval's RCCL merge."""
    timestamp: Num
    service: str
    lag: str
    nseries: Num
    stats: List[Num]  # [avg mean, avg std, p75 mean, p75 std, p95 mean, p95 std]
    type: str = "fb"

    def to_csv(self) -> str:
        g = [f"{nf(self.stats[2 * k], 1)}:{nf(self.stats[2 * k + 1], 1)}" for k in range(3)]
        return f"fb|{js_str(self.timestamp)}|{self.service}|{self.lag}|{js_str(self.nseries)}|" + "|".join(g)

    def to_pg_row(self) -> Dict[str, Any]:
        keys = ("averagemean", "averagestd", "per75mean", "per75std", "per95mean", "per95std")
        return {"timestamp": _ms_to_dt(self.timestamp), "service": self.service, "lag": self.lag,
                "nseries": _num_or_none(self.nseries),
                "stats": {k: _num_or_none(v) for k, v in zip(keys, self.stats)}}


# ---- lh: per-interval latency histogram (docs/HISTOGRAM.md).  Integer-only log-linear bins:
# four sub-bins per power of two, 120 bins for the int32 range (the device rule: kernels/common.h).
HIST_BINS = 120


def hist_bin(v: int) -> int:
    """Bin of an elapsed value (the stored int32): v <= 0 -> 0, 1..3 -> v, else 4 * (e - 1) + sub
    with e = floor(log2 v) and sub the two bits below the leading one."""
    v = int(v)
    if v <= 0:
        return 0
    if v < 4:
        return v
    e = v.bit_length() - 1
    return 4 * (e - 1) + ((v >> (e - 2)) & 3)


def hist_lower(b: int) -> int:
    """Smallest value of bin b (bin 0 also holds everything below 1)."""
    return b if b < 4 else (4 + b % 4) << (b // 4 - 1)


@dataclass
class LatencyHistEntry:
    """``lh|bucketStartMs|server|service|count|nan|lo:c,lo:c,...`` -- the elapsed times of one
    (10 s bucket, series) as a sparse histogram (no reference counterpart).  ``count`` includes the
    ``nan`` samples; ``bins`` holds (bin lower bound, samples) pairs, non-zero bins ascending."""
    timestamp: Num
    server: str
    service: str
    count: Num
    nan: Num
    bins: List[tuple]
    type: str = "lh"

    def to_csv(self) -> str:
        pairs = ",".join(f"{lo}:{c}" for lo, c in self.bins)
        return (f"lh|{js_str(self.timestamp)}|{self.server}|{self.service}|{js_str(self.count)}|"
                f"{js_str(self.nan)}|{pairs}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "count": _num_or_none(self.count), "nan": _num_or_none(self.nan),
                "bins": {str(lo): c for lo, c in self.bins}}


# ---- wp: exact window percentiles (docs/PERCENTILES.md).  Integers only: a percentile is
# q = p * 1000 (1..100000), a value the sum of the one or two ranks read (one rank: twice it).
PCT_SCALE = 100000


def pct_text(q: int) -> str:
    """Canonical text of percentile q / 1000: trailing zeros and a trailing point dropped."""
    q = int(q)
    s = f"{q // 1000}.{q % 1000:03d}".rstrip("0")
    return s[:-1] if s.endswith(".") else s


def pct_ranks(m: int, q: int) -> tuple:
    """calcPercentile's (lo, hi) ranks among m >= 1 ascending samples for percentile q / 1000, in
    integers: t = q * m; t a multiple of 100000 -> rank t / 100000 - 1; else i = ceil(t / 100000) - 1
    and (i, i + 1), or (i, i) at the last sample.  m == 1 -> (0, 0)."""
    if m == 1:
        return (0, 0)
    t = int(q) * int(m)
    if t % PCT_SCALE == 0:
        i = t // PCT_SCALE - 1
        return (i, i)
    i = t // PCT_SCALE  # ceil(t / 100000) - 1 of a non-multiple
    return (i, i) if i == m - 1 else (i, i + 1)


def half_text(sum2: int) -> str:
    """sum2 / 2 in decimal: the integer half, '.5' when sum2 is odd, '-' when negative (-1 -> -0.5)."""
    sum2 = int(sum2)
    a = abs(sum2)
    return ("-" if sum2 < 0 else "") + str(a // 2) + (".5" if a & 1 else "")


def _pct_from_text(s: str) -> Optional[int]:
    ip, sep, fr = s.partition(".")
    if not (ip.isascii() and ip.isdigit() and len(ip) <= 3) or (sep and not (fr.isascii() and fr.isdigit() and len(fr) <= 3)):
        return None
    q = int(ip) * 1000 + (int(fr.ljust(3, "0")) if sep else 0)
    return q if 1 <= q <= PCT_SCALE else None


def _half_from_text(s: str) -> Optional[int]:
    neg = s.startswith("-")
    ip, sep, fr = (s[1:] if neg else s).partition(".")
    if not (ip.isascii() and ip.isdigit() and len(ip) <= 10) or (sep and fr != "5"):
        return None
    v = 2 * int(ip) + (1 if sep else 0)
    return -v if neg else v


@dataclass
class WindowPctEntry:
    """``wp|ts|server|service|m|nan|p:v,p:v,...`` -- exact percentiles of the K8 window's ``m``
    non-NaN samples (``nan`` counts the others), one row per st row with m >= 1 (no reference
    counterpart).  ``pcts`` holds (q, sum2) integer pairs: q = p * 1000, sum2 = twice the value."""
    timestamp: Num
    server: str
    service: str
    count: Num
    nan: Num
    pcts: List[tuple]
    type: str = "wp"

    def to_csv(self) -> str:
        pairs = ",".join(f"{pct_text(q)}:{half_text(v)}" for q, v in self.pcts)
        return (f"wp|{js_str(self.timestamp)}|{self.server}|{self.service}|{js_str(self.count)}|"
                f"{js_str(self.nan)}|{pairs}")

    def to_pg_row(self) -> Dict[str, Any]:
        # (|sum2| < 2^33: the half is exact in a double)
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "count": _num_or_none(self.count), "nan": _num_or_none(self.nan),
                "pcts": {pct_text(q): (v // 2 if v % 2 == 0 else v / 2) for q, v in self.pcts}}


# ---- sl: exact window threshold counts per service objective (docs/OBJECTIVES.md).  Integers only.
SLO_T_MAX = 2147483647


def _slo_int(s: str, max_len: int = 10) -> Optional[int]:
    """A plain decimal of at most ``max_len`` digits (no sign, no spaces); None: malformed."""
    if not (s.isascii() and s.isdigit() and len(s) <= max_len):
        return None
    return int(s)


def slo_pairs_from_text(text: str) -> List[tuple]:
    """``T:c,T:c,...`` -> [(T, c)]; a malformed pair is dropped (copyenc.cpp holds the same rules:
    T and c of 1 to 10 digits, T <= 2147483647 and above the last pair kept)."""
    out = []
    for pr in (text or "").split(","):
        t, sep, c = pr.partition(":")
        tv, cv = _slo_int(t), _slo_int(c)
        if sep and tv is not None and cv is not None and tv <= SLO_T_MAX and (not out or tv > out[-1][0]):
            out.append((tv, cv))
    return out


@dataclass
class WindowSloEntry:
    """``sl|ts|server|service|m|nan|T:c,T:c,...`` -- for each threshold T of the service's latency
    objective the number c of the K8 window's ``m`` non-NaN samples with elapsed <= T (cumulative;
    ``nan`` counts the others), one row per st row with m >= 1 and at least one threshold (no
    reference counterpart).  ``le`` holds (T, c) integer pairs in list order."""
    timestamp: Num
    server: str
    service: str
    count: Num
    nan: Num
    le: List[tuple]
    type: str = "sl"

    def to_csv(self) -> str:
        pairs = ",".join(f"{int(t)}:{int(c)}" for t, c in self.le)
        return (f"sl|{js_str(self.timestamp)}|{self.server}|{self.service}|{js_str(self.count)}|"
                f"{js_str(self.nan)}|{pairs}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "count": _num_or_none(self.count), "nan": _num_or_none(self.nan),
                "le": {str(int(t)): int(c) for t, c in self.le}}


# ---- tk: per-rollover top-K series leaderboards (docs/LEADERBOARD.md)
LEADERBOARD_KEYS = ("tpm", "average", "per75", "per95")
LEADERBOARD_MAX_K = 128


def leaderboard_rank_from_text(s: Optional[str]) -> Optional[int]:
    """A rank of 1 to 3 plain digits in 1 .. 128; None: malformed (copyenc.cpp holds the same rule)."""
    r = _slo_int(s, 3) if s is not None else None
    return r if r is not None and 1 <= r <= LEADERBOARD_MAX_K else None


@dataclass
class LeaderboardEntry:
    """``tk|ts|board|rank|server|service|tpm|average|per75|per95`` -- at a rollover, the series of
    rank ``rank`` (1 = largest) on the board of key ``board`` (tpm, average, per75 or per95) among
    this rank's series, with the four numbers of the series' st row of the same rollover (no
    reference counterpart)."""
    timestamp: Num
    board: str
    rank: int
    server: str
    service: str
    tpm: float
    average: float
    per75: float
    per95: float
    type: str = "tk"

    def to_csv(self) -> str:
        return (f"tk|{js_str(self.timestamp)}|{self.board}|{int(self.rank)}|{self.server}|{self.service}|"
                f"{nf(self.tpm, 2)}|{nf(self.average)}|{nf(self.per75)}|{nf(self.per95)}")

    def to_pg_row(self) -> Dict[str, Any]:
        n = _num_or_none
        return {"timestamp": _ms_to_dt(self.timestamp), "board": self.board, "rank": int(self.rank),
                "server": self.server, "service": self.service, "tpm": n(self.tpm), "average": n(self.average),
                "per75": n(self.per75), "per95": n(self.per95)}


# ---- sv: exact per-service window stats across servers (docs/SERVICEWINDOW.md).  Integers only.
def _svc_int(s: Optional[str], max_len: int = 10, signed: bool = False) -> Optional[int]:
    """A plain decimal of 1 to ``max_len`` digits, with a leading '-' when ``signed``; None: malformed
    (copyenc.cpp holds the same rule)."""
    if s is None:
        return None
    neg = signed and s.startswith("-")
    d = s[1:] if neg else s
    if not (d.isascii() and d.isdigit() and len(d) <= max_len):
        return None
    return -int(d) if neg else int(d)


@dataclass
class ServiceWindowEntry:
    """``sv|ts|service|servers|m|nan|sum|p:v,p:v,...`` -- at a rollover, the union of the K8 windows
    of a service's ``servers`` contributing series: ``m`` non-NaN samples (``nan`` counts the
    others), their int64 ``sum`` and their exact percentiles (no reference counterpart).  ``pcts``
    holds (q, sum2) integer pairs as WindowPctEntry does."""
    timestamp: Num
    service: str
    servers: int
    count: int
    nan: int
    elapsed_sum: int
    pcts: List[tuple]
    type: str = "sv"

    def to_csv(self) -> str:
        pairs = ",".join(f"{pct_text(q)}:{half_text(v)}" for q, v in self.pcts)
        return (f"sv|{js_str(self.timestamp)}|{self.service}|{int(self.servers)}|{int(self.count)}|"
                f"{int(self.nan)}|{int(self.elapsed_sum)}|{pairs}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "service": self.service, "servers": int(self.servers),
                "count": int(self.count), "nan": int(self.nan), "elapsed_sum": int(self.elapsed_sum),
                "pcts": {pct_text(q): (v // 2 if v % 2 == 0 else v / 2) for q, v in self.pcts}}


# ---- rw: exact stats of the newest window buckets (docs/RECENT.md).  Integers only.
@dataclass
class RecentWindowEntry:
    """``rw|ts|server|service|k|m|nan|sum|p:v,p:v,...`` -- at a rollover, the newest ``buckets``
    buckets of the series' K8 window: ``count`` non-NaN samples (``nan`` counts the others), their
    int64 ``elapsed_sum`` and their exact percentiles (no reference counterpart).  ``pcts`` holds
    (q, sum2) integer pairs as WindowPctEntry does; it is empty when ``count`` is 0."""
    timestamp: Num
    server: str
    service: str
    buckets: int
    count: int
    nan: int
    elapsed_sum: int
    pcts: List[tuple]
    type: str = "rw"

    def to_csv(self) -> str:
        pairs = ",".join(f"{pct_text(q)}:{half_text(v)}" for q, v in self.pcts)
        return (f"rw|{js_str(self.timestamp)}|{self.server}|{self.service}|{int(self.buckets)}|{int(self.count)}|"
                f"{int(self.nan)}|{int(self.elapsed_sum)}|{pairs}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "buckets": int(self.buckets), "count": int(self.count), "nan": int(self.nan),
                "elapsed_sum": int(self.elapsed_sum),
                "pcts": {pct_text(q): (v // 2 if v % 2 == 0 else v / 2) for q, v in self.pcts}}


# ---- sb: SLO burn-rate breaches (docs/BURN.md).  Integers only.
BURN_MAX_RULES = 4


def burn_rules_from_text(text: Optional[str]) -> Optional[List[tuple]]:
    """``k:f:m:bad:fired,...`` -> [(k, f, m, bad, fired)], 1 to 4 groups of five plain decimals of 1
    to 10 digits, the last 0 or 1; None: malformed (copyenc.cpp holds the same rules)."""
    groups = (text or "").split(",")
    if not text or len(groups) > BURN_MAX_RULES:
        return None
    out = []
    for g in groups:
        parts = g.split(":")
        if len(parts) != 5:
            return None
        vals = [_svc_int(p) for p in parts]
        if any(v is None for v in vals) or parts[4] not in ("0", "1"):
            return None
        out.append(tuple(vals))
    return out


@dataclass
class SloBurnEntry:
    """``sb|ts|server|service|T|q|m|bad|nan|k:f:m_k:bad_k:fired,...`` -- at a rollover, a series
    whose K8 window and whose newest ``k`` buckets both burn the error budget of its objective
    (``threshold`` T, ``target_q`` = target * 1000) at least ``f`` / 1000 times as fast as the
    objective allows, for at least one rule: ``count`` non-NaN window samples, ``bad`` of them above
    T, ``nan`` others; ``rules`` holds (k, f, m_k, bad_k, fired) per configured rule (no reference
    counterpart)."""
    timestamp: Num
    server: str
    service: str
    threshold: int
    target_q: int
    count: int
    bad: int
    nan: int
    rules: List[tuple]
    type: str = "sb"

    def to_csv(self) -> str:
        groups = ",".join(f"{int(k)}:{int(f)}:{int(m)}:{int(b)}:{1 if fired else 0}" for k, f, m, b, fired in self.rules)
        return (f"sb|{js_str(self.timestamp)}|{self.server}|{self.service}|{int(self.threshold)}|{int(self.target_q)}|"
                f"{int(self.count)}|{int(self.bad)}|{int(self.nan)}|{groups}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "threshold": int(self.threshold), "target_q": int(self.target_q), "count": int(self.count),
                "bad": int(self.bad), "nan": int(self.nan),
                "rules": [{"k": int(k), "f": int(f), "m": int(m), "bad": int(b), "fired": bool(fired)}
                          for k, f, m, b, fired in self.rules]}


# ---- tf: traffic drops and surges (docs/TRAFFIC.md).  Integers only.
TRAFFIC_MAX_RULES = 4


def traffic_rules_from_text(text: Optional[str]) -> Optional[List[tuple]]:
    """``k:B:R:med2:mad4:V,...`` -> [(k, B, R, med2, mad4, V)], 1 to 4 groups of five plain decimals
    of 1 to 10 digits and a verdict D, S or N; None: malformed (copyenc.cpp holds the same rules)."""
    groups = (text or "").split(",")
    if not text or len(groups) > TRAFFIC_MAX_RULES:
        return None
    out = []
    for g in groups:
        parts = g.split(":")
        if len(parts) != 6 or parts[5] not in ("D", "S", "N"):
            return None
        vals = [_svc_int(p) for p in parts[:5]]
        if any(v is None for v in vals):
            return None
        out.append(tuple(vals) + (parts[5],))
    return out


@dataclass
class TrafficEntry:
    """``tf|ts|server|service|n|minRate|k:B:R:med2:mad4:V,...`` -- at a rollover, a series whose
    newest ``k`` window buckets hold far fewer (``D``) or far more (``S``) samples than the other
    ``B`` buckets of its K8 window, for at least one rule: ``count`` is the window's samples,
    ``min_rate`` the class' gate; ``rules`` holds (k, B, R, med2, mad4, verdict) per configured rule,
    R the samples of the newest buckets, med2 twice the median and mad4 four times the median absolute
    deviation of the baseline buckets' counts (no reference counterpart)."""
    timestamp: Num
    server: str
    service: str
    count: int
    min_rate: int
    rules: List[tuple]
    type: str = "tf"

    def to_csv(self) -> str:
        groups = ",".join(f"{int(k)}:{int(b)}:{int(r)}:{int(m2)}:{int(m4)}:{v}" for k, b, r, m2, m4, v in self.rules)
        return (f"tf|{js_str(self.timestamp)}|{self.server}|{self.service}|{int(self.count)}|{int(self.min_rate)}|"
                f"{groups}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "count": int(self.count), "min_rate": int(self.min_rate),
                "rules": [{"k": int(k), "buckets": int(b), "recent": int(r), "med2": int(m2), "mad4": int(m4),
                           "verdict": v} for k, b, r, m2, m4, v in self.rules]}


# ---- po: peer-outlier servers per service (docs/PEERS.md).  Integers only.
def pct_text(q: int) -> str:
    """q = p * 1000 as the canonical text of p: trailing zeros and a trailing point dropped."""
    q = int(q)
    return f"{q // 1000}.{q % 1000:03d}".rstrip("0").rstrip(".") if q % 1000 else str(q // 1000)


@dataclass
class PeerEntry:
    """``po|ts|server|service|m|p:x|E|X2|D4|V`` -- at a rollover, a series whose window percentile
    ``p`` lies far above (``H``) or below (``L``) the median of the same percentile over the ``peers``
    eligible series of its service: ``count`` is the window's finite samples, ``q`` = p * 1000,
    ``value2`` twice the series' percentile, ``median2x2`` x_lo + x_hi of the peers' sorted value2
    (four times the median percentile), ``mad4`` d_lo + d_hi of the sorted abs(2 value2 - median2x2)
    (no reference counterpart)."""
    timestamp: Num
    server: str
    service: str
    count: int
    q: int
    value2: int
    peers: int
    median2x2: int
    mad4: int
    verdict: str
    type: str = "po"

    def to_csv(self) -> str:
        return (f"po|{js_str(self.timestamp)}|{self.server}|{self.service}|{int(self.count)}|{pct_text(self.q)}:"
                f"{int(self.value2)}|{int(self.peers)}|{int(self.median2x2)}|{int(self.mad4)}|{self.verdict}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "count": int(self.count), "pct": pct_text(self.q), "value2": int(self.value2), "peers": int(self.peers),
                "median2x2": int(self.median2x2), "mad4": int(self.mad4), "verdict": self.verdict}


# ---- ls: latency shifts against the window's own past (docs/SHIFT.md).  Integers only.
SHIFT_MAX_RULES = 4


def shift_rules_from_text(text: Optional[str]) -> Optional[List[tuple]]:
    """``k:p:mB:T2:mR:X2:a:b:V,...`` -> [(k, q, mB, T2, mR, X2, a, b, V)], 1 to 4 groups: k, mB, mR, a
    and b plain decimals of 1 to 10 digits, p a percentile of at most three decimals below 100
    (q = p * 1000), T2 and X2 1 to 10 digits after an optional '-', V one of U, D, N; None: malformed
    (copyenc.cpp holds the same rules)."""
    groups = (text or "").split(",")
    if not text or len(groups) > SHIFT_MAX_RULES:
        return None
    out = []
    for g in groups:
        parts = g.split(":")
        if len(parts) != 9 or parts[8] not in ("U", "D", "N"):
            return None
        q = _pct_from_text(parts[1])
        vals = [_svc_int(parts[0]), q, _svc_int(parts[2]), _svc_int(parts[3], 10, True), _svc_int(parts[4]),
                _svc_int(parts[5], 10, True), _svc_int(parts[6]), _svc_int(parts[7])]
        if any(v is None for v in vals) or q >= PCT_SCALE:
            return None
        out.append(tuple(vals) + (parts[8],))
    return out


@dataclass
class LatencyShiftEntry:
    """``ls|ts|server|service|n|minDelta|k:p:mB:T2:mR:X2:a:b:V,...`` -- at a rollover, a series whose
    newest ``k`` window buckets are slower (``U``) or faster (``D``) than the other buckets of its K8
    window, for at least one rule: ``count`` is the window's samples, ``min_delta`` the class' gate;
    ``rules`` holds (k, q, mB, T2, mR, X2, a, b, verdict) per configured rule, q = p * 1000, mB / mR
    the finite samples of the baseline / the recent span, T2 / X2 twice their percentile p, a / b the
    recent finite samples strictly above / below the baseline's percentile (no reference
    counterpart)."""
    timestamp: Num
    server: str
    service: str
    count: int
    min_delta: int
    rules: List[tuple]
    type: str = "ls"

    def to_csv(self) -> str:
        groups = ",".join(f"{int(k)}:{pct_text(q)}:{int(mb)}:{int(t2)}:{int(mr)}:{int(x2)}:{int(a)}:{int(b)}:{v}"
                          for k, q, mb, t2, mr, x2, a, b, v in self.rules)
        return (f"ls|{js_str(self.timestamp)}|{self.server}|{self.service}|{int(self.count)}|{int(self.min_delta)}|"
                f"{groups}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "count": int(self.count), "min_delta": int(self.min_delta),
                "rules": [{"k": int(k), "p": pct_text(q), "base": int(mb), "t2": int(t2), "recent": int(mr),
                           "x2": int(x2), "above": int(a), "below": int(b), "verdict": v}
                          for k, q, mb, t2, mr, x2, a, b, v in self.rules]}


# ---- ic: incidents opened and closed over the sb / tf / po / ls verdicts (docs/INCIDENTS.md).
INCIDENT_SOURCES = ("sb", "tf", "po", "ls")
INCIDENT_EVENTS = ("O", "S", "C")
INCIDENT_CODES = ("B", "D", "S", "H", "L", "U")
INCIDENT_SINCE_MAX = 253402300799999  # the last ms of the year 9999


@dataclass
class IncidentEntry:
    """``ic|ts|server|service|source|event|code0|code|since|age|run`` -- at a rollover, an incident of
    one series and one source (sb, tf, po, ls) opened (``O``), is still open at a reminder step
    (``S``) or closed (``C``): ``code0`` is the code it opened with, ``code`` this rollover's (``-``
    when the source is not hot), ``since`` the timestamp of the rollover that opened it, ``age`` the
    rollovers since then and ``run`` the consecutive hot (or, when not hot, clear) rollovers (no
    reference counterpart)."""
    timestamp: Num
    server: str
    service: str
    source: str
    event: str
    code0: str
    code: str
    since: int
    age: int
    run: int
    type: str = "ic"

    def to_csv(self) -> str:
        return (f"ic|{js_str(self.timestamp)}|{self.server}|{self.service}|{self.source}|{self.event}|{self.code0}|"
                f"{self.code}|{int(self.since)}|{int(self.age)}|{int(self.run)}")

    def to_pg_row(self) -> Dict[str, Any]:
        return {"timestamp": _ms_to_dt(self.timestamp), "server": self.server, "service": self.service,
                "source": self.source, "event": self.event, "code0": self.code0, "code": self.code,
                # (integer arithmetic: a float of seconds is a microsecond off near the year 9999)
                "since": _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc) + _dt.timedelta(milliseconds=int(self.since)),
                "age": int(self.age), "run": int(self.run)}


def entry_from_csv(line: Union[str, bytes], delim: str = "|"):
    """EntryFactory.getEntryFromCSV (entries.js:174-193). Returns None for unknown types."""
    if isinstance(line, bytes):
        line = line.decode("utf-8")
    arr = line.split(delim)
    t = arr[0]
    if t == "tx":
        a = _pad(arr, 9)
        return TxEntry.make(a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8])
    if t == "st":
        a = _pad(arr, 8)
        return StatEntry.make(a[1], a[2], a[3], a[4], a[5], a[6], a[7])
    if t == "fs":
        a = _pad(arr, 9)
        # a truncated record throws in entries.js (undefined.split); here missing groups are
        # read as all-undefined so one bad line cannot take the consumer down
        av = _pad(a[6].split(":") if a[6] is not None else [], 5)
        p75 = _pad(a[7].split(":") if a[7] is not None else [], 5)
        p95 = _pad(a[8].split(":") if a[8] is not None else [], 5)
        return FullStatEntry.make(a[1], a[2], a[3], a[5], a[4], *av, *p75, *p95)
    if t == "al":
        a = _pad(arr, 7)
        return AlertEntry(parse_int(a[1]), parse_int(a[2]), a[3], a[4], a[5], a[6])
    if t == "jx":
        a = _pad(arr, 19)
        return JmxEntry.make(a[1], a[2], *a[3:19])
    if t == "fb":
        a = _pad(arr, 8)
        st: List[Num] = []
        for g in a[5:8]:
            p = _pad(g.split(":") if g is not None else [], 2)
            st += [parse_float(p[0]), parse_float(p[1])]
        return FleetEntry(parse_int(a[1]), a[2], a[3], parse_int(a[4]), st)
    if t == "lh":
        a = _pad(arr, 7)
        bins = []
        for pr in (a[6] or "").split(","):
            lo, _sep, c = pr.partition(":")
            lo, c = parse_int(lo), parse_int(c)
            if lo == lo and c == c:  # (a malformed pair is dropped, as copyenc.cpp does)
                bins.append((int(lo), int(c)))
        return LatencyHistEntry(parse_int(a[1]), a[2], a[3], parse_int(a[4]), parse_int(a[5]), bins)
    if t == "wp":
        a = _pad(arr, 7)
        pcts = []
        for pr in (a[6] or "").split(","):
            p, _sep, v = pr.partition(":")
            q, s2 = _pct_from_text(p), _half_from_text(v)
            if q is not None and s2 is not None:  # (a malformed pair is dropped, as copyenc.cpp does)
                pcts.append((q, s2))
        return WindowPctEntry(parse_int(a[1]), a[2], a[3], parse_int(a[4]), parse_int(a[5]), pcts)
    if t == "sl":
        a = _pad(arr, 7)
        return WindowSloEntry(parse_int(a[1]), a[2], a[3], parse_int(a[4]), parse_int(a[5]),
                              slo_pairs_from_text(a[6]))
    if t == "tk":
        a = _pad(arr, 10)
        rank = leaderboard_rank_from_text(a[3])
        if a[2] not in LEADERBOARD_KEYS or rank is None:  # (a malformed row is dropped, as copyenc.cpp does)
            return None
        pf = parse_float
        return LeaderboardEntry(parse_int(a[1]), a[2], rank, a[4], a[5], pf(a[6]), pf(a[7]), pf(a[8]), pf(a[9]))
    if t == "sv":
        a = _pad(arr, 8)
        srv, cnt, nan = _svc_int(a[3]), _svc_int(a[4]), _svc_int(a[5])
        tot = _svc_int(a[6], 18, signed=True)
        if srv is None or cnt is None or nan is None or tot is None:  # (a malformed row is dropped, as copyenc.cpp does)
            return None
        pcts = []
        for pr in (a[7] or "").split(","):
            p, _sep, v = pr.partition(":")
            q, s2 = _pct_from_text(p), _half_from_text(v)
            if q is not None and s2 is not None:  # (a malformed pair is dropped, likewise)
                pcts.append((q, s2))
        return ServiceWindowEntry(parse_int(a[1]), a[2], srv, cnt, nan, tot, pcts)
    if t == "rw":
        a = _pad(arr, 9)
        k, cnt, nan = _svc_int(a[4]), _svc_int(a[5]), _svc_int(a[6])
        tot = _svc_int(a[7], 18, signed=True)
        if k is None or cnt is None or nan is None or tot is None:  # (a malformed row is dropped, as copyenc.cpp does)
            return None
        pcts = []
        for pr in (a[8] or "").split(","):
            p, _sep, v = pr.partition(":")
            q, s2 = _pct_from_text(p), _half_from_text(v)
            if q is not None and s2 is not None:  # (a malformed pair is dropped, likewise)
                pcts.append((q, s2))
        return RecentWindowEntry(parse_int(a[1]), a[2], a[3], k, cnt, nan, tot, pcts)
    if t == "sb":
        a = _pad(arr, 10)
        nums = [_svc_int(x) for x in a[4:9]]
        rules = burn_rules_from_text(a[9])
        if any(v is None for v in nums) or rules is None:  # (a malformed row is dropped, as copyenc.cpp does)
            return None
        return SloBurnEntry(parse_int(a[1]), a[2], a[3], *nums, rules)
    if t == "tf":
        a = _pad(arr, 7)
        nums = [_svc_int(x) for x in a[4:6]]
        rules = traffic_rules_from_text(a[6])
        if any(v is None for v in nums) or rules is None:  # (a malformed row is dropped, as copyenc.cpp does)
            return None
        return TrafficEntry(parse_int(a[1]), a[2], a[3], *nums, rules)
    if t == "po":
        # (copyenc.cpp holds the same rules) exactly ten fields; m and E 1 to 10 digits; <p>:<x> with x
        # 1 to 10 digits after an optional '-'; X2 1 to 11 digits after an optional '-'; D4 1 to 11
        # digits; the verdict H or L; anything else is dropped
        if len(arr) != 10 or arr[9] not in ("H", "L"):
            return None
        p, sep, x = arr[5].partition(":")
        q = _pct_from_text(p) if sep else None
        nums = [_svc_int(arr[4]), _svc_int(x, 10, True), _svc_int(arr[6]), _svc_int(arr[7], 11, True), _svc_int(arr[8], 11)]
        if q is None or any(v is None for v in nums):
            return None
        return PeerEntry(parse_int(arr[1]), arr[2], arr[3], nums[0], q, nums[1], nums[2], nums[3], nums[4], arr[9])
    if t == "ls":
        # (copyenc.cpp holds the same rules) exactly seven fields; n and minDelta 1 to 10 digits; the
        # groups by shift_rules_from_text; anything else is dropped
        if len(arr) != 7:
            return None
        nums = [_svc_int(x) for x in arr[4:6]]
        rules = shift_rules_from_text(arr[6])
        if any(v is None for v in nums) or rules is None:
            return None
        return LatencyShiftEntry(parse_int(arr[1]), arr[2], arr[3], *nums, rules)
    if t == "ic":
        # (copyenc.cpp holds the same rules) exactly eleven fields; the source, the event and the two
        # codes from their sets; since 1 to 15 digits up to the year 9999, age 1 to 10, run 1 to 3;
        # anything else is dropped
        if len(arr) != 11:
            return None
        if (arr[4] not in INCIDENT_SOURCES or arr[5] not in INCIDENT_EVENTS or arr[6] not in INCIDENT_CODES
                or arr[7] not in INCIDENT_CODES + ("-",)):
            return None
        since, age, run = _svc_int(arr[8], 15), _svc_int(arr[9]), _svc_int(arr[10], 3)
        if since is None or age is None or run is None or since > INCIDENT_SINCE_MAX:
            return None
        return IncidentEntry(parse_int(arr[1]), arr[2], arr[3], arr[4], arr[5], arr[6], arr[7], since, age, run)
    return None


RECORD_TYPES = ("tx", "st", "fs", "al", "jx", "fb", "lh", "wp", "sl", "tk", "sv", "rw", "sb", "tf", "po", "ls", "ic")
