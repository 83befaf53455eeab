"""APM config loader, compatible with the reference ``config/apm_config.json``.

Behaviour parity (reference ``util_methods.js:253-348``):

* ``json_strip`` removes ``[^:]//.*`` (global), *including the character before* ``//``
  (quirk Q20: ``"a": 1,// c`` loses its comma, ``amqp://h`` survives).
* ``read_apm_config`` returns ``None`` on a JSON error (caller keeps the previous config),
  and adds ``apmConfigFilePath``.
* ``ConfigWatcher`` polls the file (md5 + size, 500 ms debounce, like ``watchAPMConfig``),
  logs a warning for every changed key in ``restart_required`` and invokes the callback.

New keys live under a ``gpu`` section (see ``GPU_DEFAULTS``); unknown keys there are
reported, never silently ignored.
"""
from __future__ import annotations

import copy
import decimal
import hashlib
import json
import logging
import math
import os
import re
import threading
import time
from typing import Any, Callable, Dict, Iterable, List, Optional, Tuple

log = logging.getLogger("apm.config")

_STRIP_RE = re.compile(r"[^:]//(.*)")

DEFAULT_CONFIG_PATH = os.path.join(
    os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
    "config", "apm_config.json")

# New section: everything the MI355X engine needs that the reference did not have.
GPU_DEFAULTS: Dict[str, Any] = {
    "device": 0,                      # local device index (rank's LOCAL_RANK overrides)
    "maxSeries": 1 << 17,             # (server, service) series capacity per GPU
    "maxServices": 1 << 16,           # distinct service-name capacity
    "maxServers": 1024,
    "bucketCellCapacity": 16,         # samples per (series, 10 s bucket) kept inline
    "bucketRingSlots": 0,             # bucket ring slots (0 = window + buffer + 1, at least 40; grows on reload)
    "bucketOverflowCapacity": 1 << 22,  # spill area for hot series
    "batchBytes": 32 << 20,           # bytes of raw log per ingest batch
    "maxLinesPerBatch": 1 << 20,
    "ringDtype": "float64",          # z-score history ring: float64 | float32 | bfloat16
    "pinThreads": False,             # pin join workers / stats / output lanes to GPU-local cores
    "zscoreMeanMode": "rolling",      # rolling (O(1) compensated) | exact (sequential, JS-bit-exact)
    "zscoreSigma": "sqrt_mean",       # sqrt_mean (reference quirk Q1) | stddev (true sigma)
    "exactRecomputeEveryIntervals": 360,
    "emulateOverrideAliasing": False,  # quirk Q4 (per-service overrides leak into defaults)
    "alertClock": "wall",             # wall (reference: stream_process_alerts.js:437,449-467) | entry (log time: replay)
    "cooldownKey": "service",         # service (reference Q7) | series
    "recordTtlSeconds": 120,          # recordCache stdTTL (stream_parse_transactions.js:215)
    "acctTtlSeconds": 120,            # acctCache stdTTL (:213)
    "needTtlSeconds": 30,             # needNumRecordCache stdTTL (:218)
    "timezone": "local",              # tz for 'YYYY-MM-DD HH:MM:SS,mmm' timestamps
    "fleetBaseline": True,            # RCCL all-reduce of per-service moments + lock-step clocks
    "joinThreads": 0,                 # host join worker threads (0 = auto; joinOnDevice false)
    "joinOnDevice": True,             # K4/K6 join + tx encoding on the GPU (false: host join workers)
    "joinTableSlots": 1 << 21,        # GPU join key table (logId keys, 128 B per slot) -- grows
    "needArenaEntries": 1 << 18,      # GPU needNumRecordCache entries (512 B each) -- grows
    "joinChainBlocks": 0,             # GPU join overflow chains (256 B blocks; 0 = auto) -- grows
    "txTextRingMB": 4096,             # HBM ring holding pending (unreleased) tx lines
    "maxRawServices": 1 << 18,        # distinct (server, raw service name) pairs
    "collectiveTimeoutSeconds": 300,  # RCCL watchdog: abort + exit when a collective hangs this long
    "collectiveInitTimeoutSeconds": 120,  # RCCL communicator init deadline (a peer that never joins -> clear error)
    "collectiveBackend": "rccl",      # node-wide exchanges: rccl (xGMI) or host (TCP via rank 0, ranks sharing a GPU)
    "checkpointDir": "",              # binary engine checkpoints (+ tail offsets) per rank
    "checkpointEverySeconds": 60,
    "checkpointStageMB": 2048,        # HBM staging of a checkpoint's z-score ring rows (larger bases stream)
    "importReferenceResume": False,   # seed a fresh engine from the reference's JSON resume files
    "outputMode": "inproc",           # inproc (DB insert stage in-process) | amqp (queue bridge) | none
    "bridgeQueues": [],               # amqp mode: also mirror "transactions" / "stats"
    "tailFromStart": False,           # File::Tail starts at EOF; true reads existing content
    "serverRollup": False,            # K14 "sx" stream: per-JVM rollup fused with JMX / VM gauges
    "fuseJmx": False,                 # JMX poller inside the engine process feeding K14
    "syntheticJmx": False,            # use the synthetic WildFly CLI (tests / benchmarks)
    "logFilePrefix": "apm_engine",
    "faultInjection": {},             # {"rank", "dropBatchEvery", "duplicateBatchEvery", "exitAtBatch"}
}

# Opt-in keys of the gpu section that have no entry in a config that does not name them (the
# loaded default config stays byte for byte what it was, and with it the config text the recorded
# reference answers under tests/golden/refjs are keyed by): read with gpu_opt(cfg, key).
GPU_OPTIONAL: Dict[str, Any] = {
    "latencyHistogram": False,        # K15 "lh" stream: per-interval latency histograms (docs/HISTOGRAM.md)
    "histQueue": "latency_hist",      # amqp mode: the queue the lh records go to
    "windowPercentiles": [],          # K16 "wp" stream: exact window percentiles, e.g. [50, 90, 99, 99.9] (docs/PERCENTILES.md)
    "pctQueue": "window_pct",         # amqp mode: the queue the wp records go to
    "latencyObjectives": None,        # K17 "sl" stream: per-service latency thresholds, {"default": [500, 2000], "services": {...}} (docs/OBJECTIVES.md)
    "sloQueue": "window_slo",         # amqp mode: the queue the sl records go to
    "leaderboard": None,              # K18 "tk" stream: per-rollover top-K series, {"k": 20, "by": ["per95", "average", "tpm"], "minTpm": 0} (docs/LEADERBOARD.md)
    "topQueue": "leaderboard",        # amqp mode: the queue the tk records go to
    "serviceWindow": None,            # K19 "sv" stream: exact per-service window stats across servers, {"percentiles": [50, 75, 95, 99]} (docs/SERVICEWINDOW.md)
    "svcQueue": "service_window",     # amqp mode: the queue the sv records go to
    "recentWindows": None,            # K20 "rw" stream: exact stats of the newest window buckets, {"buckets": [1, 6], "percentiles": [50, 95, 99]} (docs/RECENT.md)
    "recentQueue": "recent_window",   # amqp mode: the queue the rw records go to
    "sloBurn": None,                  # K21 "sb" stream: multi-window SLO burn-rate breaches, {"default": {"threshold": 2000, "target": 99}, "services": {...}, "rules": [{"short": 1, "factor": 14.4}], "minSamples": 20} (docs/BURN.md)
    "burnQueue": "slo_burn",          # amqp mode: the queue the sb records go to
    "trafficWatch": None,             # K22 "tf" stream: traffic drops and surges against the window's median / MAD baseline, {"default": {"minRate": 5}, "services": {...}, "rules": [{"short": 1, "drop": 0.1, "z": 4}], "minBuckets": 8} (docs/TRAFFIC.md)
    "trafficQueue": "traffic",        # amqp mode: the queue the tf records go to
    "peerOutliers": None,             # K23 "po" stream: servers whose window percentile lies far from the median over the servers of the same service, {"percentile": 95, "default": {"minValue": 20}, "services": {...}, "high": 2, "low": 0.25, "z": 3, "minDelta": 10, "minPeers": 5, "minSamples": 20} (docs/PEERS.md)
    "peerQueue": "peer_outliers",     # amqp mode: the queue the po records go to
    "latencyShift": None,             # K24 "ls" stream: latency shifts of a series' newest buckets against the rest of its own window, {"default": {"minDelta": 50}, "services": {...}, "rules": [{"short": 6, "percentile": 95, "up": 3, "z": 4}], "minRecent": 20, "minBaseline": 100} (docs/SHIFT.md)
    "shiftQueue": "latency_shift",    # amqp mode: the queue the ls records go to
    "incidents": None,                # K25 "ic" stream: incidents opened and closed over the sb / tf / po / ls verdicts, {"sources": {"sb": {"openAfter": 2, "closeAfter": 6}, ...}, "remindEvery": 90, "email": true} (docs/INCIDENTS.md)
    "incidentQueue": "incidents",     # amqp mode: the queue the ic records go to
}

def gpu_opt(cfg: Dict[str, Any], key: str) -> Any:
    """An optional gpu key's value, GPU_OPTIONAL's default when the config does not name it."""
    return (cfg.get("gpu") or {}).get(key, GPU_OPTIONAL[key])


MAX_WINDOW_PCTS = 8   # kernel_api.h WP_MAX_Q
PCT_SCALE = 100000    # q = p * 1000: a percentile with three decimals as an integer, 100 % = 100000


def parse_window_percentiles(v: Any) -> List[int]:
    """gpu.windowPercentiles -> [q], q = p * 1000 (1 <= q <= 100000), strictly ascending, at most
    eight.  Each entry goes through its decimal text (a float's shortest repr, which is the text
    the config held), never through float arithmetic.  None / [] -> [] (stream off); anything
    else that is not such a list raises ValueError."""
    if v is None:
        return []
    if isinstance(v, (str, bytes)) or not isinstance(v, (list, tuple)):
        raise ValueError(f"gpu.windowPercentiles: a list of percentiles, got {v!r}")
    if len(v) > MAX_WINDOW_PCTS:
        raise ValueError(f"gpu.windowPercentiles: at most {MAX_WINDOW_PCTS} percentiles, got {len(v)}")
    out: List[int] = []
    for p in v:
        if isinstance(p, bool) or not isinstance(p, (int, float, str, decimal.Decimal)):
            raise ValueError(f"gpu.windowPercentiles: {p!r} is not a number")
        try:
            d = decimal.Decimal(repr(p) if isinstance(p, float) else str(p).strip())
        except decimal.InvalidOperation:
            raise ValueError(f"gpu.windowPercentiles: {p!r} is not a number") from None
        if not d.is_finite():
            raise ValueError(f"gpu.windowPercentiles: {p!r} is not finite")
        q = d * 1000
        if q != q.to_integral_value():
            raise ValueError(f"gpu.windowPercentiles: {p!r} has more than three decimals")
        q = int(q)
        if not 1 <= q <= PCT_SCALE:
            raise ValueError(f"gpu.windowPercentiles: {p!r} is outside (0, 100]")
        if out and q <= out[-1]:
            raise ValueError(f"gpu.windowPercentiles: {p!r} does not ascend strictly")
        out.append(q)
    return out


def window_percentiles(cfg: Dict[str, Any]) -> List[int]:
    """The validated gpu.windowPercentiles of a config as integers q = p * 1000 ([]: off)."""
    return parse_window_percentiles(gpu_opt(cfg, "windowPercentiles"))


MAX_SLO_THRESHOLDS = 8   # kernel_api.h SL_MAX_T
SLO_T_MAX = 2147483647   # samples are int32


def _parse_threshold_list(where: str, v: Any) -> List[int]:
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"gpu.latencyObjectives: {where} must be a list of integers, got {v!r}")
    if len(v) > MAX_SLO_THRESHOLDS:
        raise ValueError(f"gpu.latencyObjectives: {where} holds {len(v)} thresholds, at most {MAX_SLO_THRESHOLDS}")
    out: List[int] = []
    for t in v:
        if isinstance(t, bool) or not isinstance(t, int):
            raise ValueError(f"gpu.latencyObjectives: {where}: {t!r} is not an integer")
        if not 0 <= t <= SLO_T_MAX:
            raise ValueError(f"gpu.latencyObjectives: {where}: {t!r} is outside 0 .. {SLO_T_MAX}")
        if out and t <= out[-1]:
            raise ValueError(f"gpu.latencyObjectives: {where}: {t!r} does not ascend strictly")
        out.append(t)
    return out


def parse_latency_objectives(v: Any) -> Optional[Dict[str, Any]]:
    """gpu.latencyObjectives -> {"default": [T, ...], "services": {name: [T, ...]}} with every
    list 0 to 8 strictly ascending integers in 0 .. 2147483647 (bool, float and str entries are
    rejected: a threshold is compared with int32 samples, nothing is rounded).  None, or an object
    without a non-empty list -> None (stream off); anything else raises ValueError."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.latencyObjectives: an object with 'default' and / or 'services', got {v!r}")
    extra = set(v) - {"default", "services"}
    if extra:
        raise ValueError(f"gpu.latencyObjectives: unknown key(s) {sorted(extra)!r}")
    default = _parse_threshold_list("default", v["default"]) if v.get("default") is not None else []
    services = v.get("services")
    if services is None:
        services = {}
    if not isinstance(services, dict):
        raise ValueError(f"gpu.latencyObjectives: services must be an object, got {services!r}")
    named: Dict[str, List[int]] = {}
    for name, lst in services.items():
        if not isinstance(name, str):
            raise ValueError(f"gpu.latencyObjectives: service name {name!r} is not a string")
        named[name] = _parse_threshold_list(f"services[{name!r}]", lst)
    if not default and not any(named.values()):
        return None
    return {"default": default, "services": named}


def latency_objectives(cfg: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The validated gpu.latencyObjectives of a config (None: off)."""
    return parse_latency_objectives(gpu_opt(cfg, "latencyObjectives"))


def slo_tables(obj: Optional[Dict[str, Any]]) -> Tuple[List[List[int]], Dict[str, int], int]:
    """(classes, service -> class, default class) as the engine takes them: class 0 is "no row",
    class 1 the default list when it is not empty, then one class per named service with a
    non-empty list, in config order; a service named with [] maps to class 0."""
    if not obj:
        return [], {}, 0
    classes: List[List[int]] = [[]]
    default_class = 0
    if obj["default"]:
        classes.append(list(obj["default"]))
        default_class = 1
    services: Dict[str, int] = {}
    for name, lst in obj["services"].items():
        if lst:
            classes.append(list(lst))
            services[name] = len(classes) - 1
        else:
            services[name] = 0
    return classes, services, default_class


LEADERBOARD_KEYS = ("tpm", "average", "per75", "per95")  # kernel_api.h TopKKey, in code order
LEADERBOARD_MAX_K = 128                                  # kernel_api.h TK_MAX_K
LEADERBOARD_MAX_BOARDS = 4


def parse_leaderboard(v: Any) -> Optional[Dict[str, Any]]:
    """gpu.leaderboard -> {"k": int, "by": [name, ...], "minTpm": float}: ``k`` a JSON integer in
    1 .. 128 (bool, float and str are rejected), ``by`` 1 to 4 distinct names out of tpm, average,
    per75, per95 (the boards, in row order), ``minTpm`` optional (default 0), a finite number >= 0.
    None -> None (stream off); anything else raises ValueError."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.leaderboard: an object with 'k', 'by' and optionally 'minTpm', got {v!r}")
    extra = set(v) - {"k", "by", "minTpm"}
    if extra:
        raise ValueError(f"gpu.leaderboard: unknown key(s) {sorted(extra, key=str)!r}")
    k = v.get("k")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= LEADERBOARD_MAX_K:
        raise ValueError(f"gpu.leaderboard: k must be an integer in 1 .. {LEADERBOARD_MAX_K}, got {k!r}")
    by = v.get("by")
    if not isinstance(by, (list, tuple)) or not 1 <= len(by) <= LEADERBOARD_MAX_BOARDS:
        raise ValueError(f"gpu.leaderboard: by must list 1 to {LEADERBOARD_MAX_BOARDS} keys, got {by!r}")
    for name in by:
        if not isinstance(name, str) or name not in LEADERBOARD_KEYS:
            raise ValueError(f"gpu.leaderboard: by: {name!r} is not one of {', '.join(LEADERBOARD_KEYS)}")
    if len(set(by)) != len(by):
        raise ValueError(f"gpu.leaderboard: by names a key twice: {list(by)!r}")
    m = v.get("minTpm", 0)
    if isinstance(m, bool) or not isinstance(m, (int, float)) or not math.isfinite(m) or m < 0:
        raise ValueError(f"gpu.leaderboard: minTpm must be a finite number >= 0, got {m!r}")
    return {"k": k, "by": list(by), "minTpm": float(m)}


def leaderboard(cfg: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The validated gpu.leaderboard of a config (None: off)."""
    return parse_leaderboard(gpu_opt(cfg, "leaderboard"))


def parse_service_window(v: Any) -> List[int]:
    """gpu.serviceWindow -> [q] (q = p * 1000) of its ``percentiles`` list, which follows the rules
    of gpu.windowPercentiles (parse_window_percentiles) and must hold at least one entry.
    None -> [] (stream off); an object without such a list, with any other member, or a value of
    any other type raises ValueError."""
    if v is None:
        return []
    if not isinstance(v, dict):
        raise ValueError(f"gpu.serviceWindow: an object with 'percentiles', got {v!r}")
    extra = set(v) - {"percentiles"}
    if extra:
        raise ValueError(f"gpu.serviceWindow: unknown key(s) {sorted(extra, key=str)!r}")
    try:
        qs = parse_window_percentiles(v.get("percentiles"))
    except ValueError as e:
        raise ValueError(str(e).replace("gpu.windowPercentiles", "gpu.serviceWindow.percentiles", 1)) from None
    if not qs:
        raise ValueError("gpu.serviceWindow: percentiles must list 1 to 8 percentiles")
    return qs


def service_window(cfg: Dict[str, Any]) -> List[int]:
    """The validated gpu.serviceWindow percentiles of a config as integers q = p * 1000 ([]: off)."""
    return parse_service_window(gpu_opt(cfg, "serviceWindow"))


RECENT_MAX_SPANS = 4


def parse_recent_windows(v: Any) -> Optional[Dict[str, List[int]]]:
    """gpu.recentWindows -> {"buckets": [k, ...], "percentiles": [q, ...]} (q = p * 1000).
    ``buckets``: 1 to 4 JSON integers (no bool, float or string), strictly ascending, each at least
    1; the bound against the window is the engine's (check_recent_windows).  ``percentiles``: the
    rules of gpu.windowPercentiles, at least one entry.  None -> None (stream off); an object
    without either list, with any other member, or a value of any other type raises ValueError."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.recentWindows: an object with 'buckets' and 'percentiles', got {v!r}")
    extra = set(v) - {"buckets", "percentiles"}
    if extra:
        raise ValueError(f"gpu.recentWindows: unknown key(s) {sorted(extra, key=str)!r}")
    b = v.get("buckets")
    if not isinstance(b, list) or not 1 <= len(b) <= RECENT_MAX_SPANS:
        raise ValueError(f"gpu.recentWindows: buckets must list 1 to {RECENT_MAX_SPANS} bucket counts, got {b!r}")
    for i, k in enumerate(b):
        if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > 0x7fffffff:
            raise ValueError(f"gpu.recentWindows.buckets: integers >= 1, got {k!r}")
        if i and k <= b[i - 1]:
            raise ValueError(f"gpu.recentWindows.buckets: strictly ascending, got {b!r}")
    try:
        qs = parse_window_percentiles(v.get("percentiles"))
    except ValueError as e:
        raise ValueError(str(e).replace("gpu.windowPercentiles", "gpu.recentWindows.percentiles", 1)) from None
    if not qs:
        raise ValueError("gpu.recentWindows: percentiles must list 1 to 8 percentiles")
    return {"buckets": [int(k) for k in b], "percentiles": qs}


def recent_windows(cfg: Dict[str, Any]) -> Optional[Dict[str, List[int]]]:
    """The validated gpu.recentWindows object of a config (None: off)."""
    return parse_recent_windows(gpu_opt(cfg, "recentWindows"))


def check_recent_windows(rw: Optional[Dict[str, List[int]]], window: int) -> None:
    """The bound an engine puts on the spans when it is constructed: at most windowSizeInIntervals."""
    if rw and rw["buckets"][-1] > int(window):
        raise ValueError(f"gpu.recentWindows.buckets: at most windowSizeInIntervals ({int(window)}), "
                         f"got {rw['buckets'][-1]}")


BURN_MAX_RULES = 4          # kernel_api.h SB_MAX_RULES
BURN_Q_SCALE = 100000       # target_q = target * 1000; the error budget is b = 100000 - q
BURN_F_MAX = 1000000        # factor * 1000


def _burn_decimal(where: str, p: Any, lo: int, hi: int) -> int:
    """A decimal with at most three places as the integer ``p * 1000`` in lo .. hi, read from its
    text the way parse_window_percentiles reads a percentile (never through float arithmetic)."""
    if isinstance(p, bool) or not isinstance(p, (int, float, str, decimal.Decimal)):
        raise ValueError(f"gpu.sloBurn: {where}: {p!r} is not a number")
    try:
        d = decimal.Decimal(repr(p) if isinstance(p, float) else str(p).strip())
    except decimal.InvalidOperation:
        raise ValueError(f"gpu.sloBurn: {where}: {p!r} is not a number") from None
    if not d.is_finite():
        raise ValueError(f"gpu.sloBurn: {where}: {p!r} is not finite")
    q = d * 1000
    if q != q.to_integral_value():
        raise ValueError(f"gpu.sloBurn: {where}: {p!r} has more than three decimals")
    q = int(q)
    if not lo <= q <= hi:
        raise ValueError(f"gpu.sloBurn: {where}: {p!r} is outside {lo / 1000:g} .. {hi / 1000:g}")
    return q


def _parse_burn_objective(where: str, v: Any) -> Optional[Tuple[int, int]]:
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.sloBurn: {where} must be an object with 'threshold' and 'target' (or null), got {v!r}")
    extra = set(v) - {"threshold", "target"}
    if extra:
        raise ValueError(f"gpu.sloBurn: {where}: unknown key(s) {sorted(extra, key=str)!r}")
    if "threshold" not in v or "target" not in v:
        raise ValueError(f"gpu.sloBurn: {where} needs both 'threshold' and 'target', got {v!r}")
    t = v["threshold"]
    if isinstance(t, bool) or not isinstance(t, int):
        raise ValueError(f"gpu.sloBurn: {where}: threshold {t!r} is not an integer")
    if not 0 <= t <= SLO_T_MAX:
        raise ValueError(f"gpu.sloBurn: {where}: threshold {t!r} is outside 0 .. {SLO_T_MAX}")
    return int(t), _burn_decimal(f"{where}: target", v["target"], 1, BURN_Q_SCALE - 1)


def parse_slo_burn(v: Any) -> Optional[Dict[str, Any]]:
    """gpu.sloBurn -> {"default": (T, q) | None, "services": {name: (T, q) | None},
    "rules": [(short, f), ...], "minSamples": n}.  An objective is a JSON integer ``threshold`` in
    0 .. 2147483647 (bool, float and str are rejected) and a ``target`` percentage with at most three
    decimals, q = target * 1000 in 1 .. 99999; ``default`` may be absent or null, a service named
    with null gets no rows.  ``rules``: 1 to 4 objects {"short": k, "factor": x}, ``short`` a JSON
    integer >= 1, strictly ascending (its bound against the window is the engine's,
    check_slo_burn), ``factor`` a decimal with at most three places, f = factor * 1000 in
    1 .. 1000000.  ``minSamples``: a JSON integer >= 1 (default 1).  None, or an object in which no
    service has an objective -> None (stream off); anything else raises ValueError."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.sloBurn: an object with 'default' and / or 'services', and 'rules', got {v!r}")
    extra = set(v) - {"default", "services", "rules", "minSamples"}
    if extra:
        raise ValueError(f"gpu.sloBurn: unknown key(s) {sorted(extra, key=str)!r}")
    default = _parse_burn_objective("default", v.get("default"))
    services = v.get("services")
    if services is None:
        services = {}
    if not isinstance(services, dict):
        raise ValueError(f"gpu.sloBurn: services must be an object, got {services!r}")
    named: Dict[str, Optional[Tuple[int, int]]] = {}
    for name, o in services.items():
        if not isinstance(name, str):
            raise ValueError(f"gpu.sloBurn: service name {name!r} is not a string")
        named[name] = _parse_burn_objective(f"services[{name!r}]", o)
    rules = v.get("rules")
    if not isinstance(rules, list) or not 1 <= len(rules) <= BURN_MAX_RULES:
        raise ValueError(f"gpu.sloBurn: rules must list 1 to {BURN_MAX_RULES} rules, got {rules!r}")
    out_rules: List[Tuple[int, int]] = []
    for i, r in enumerate(rules):
        if not isinstance(r, dict):
            raise ValueError(f"gpu.sloBurn: rules[{i}] must be an object with 'short' and 'factor', got {r!r}")
        extra = set(r) - {"short", "factor"}
        if extra:
            raise ValueError(f"gpu.sloBurn: rules[{i}]: unknown key(s) {sorted(extra, key=str)!r}")
        if "short" not in r or "factor" not in r:
            raise ValueError(f"gpu.sloBurn: rules[{i}] needs both 'short' and 'factor', got {r!r}")
        k = r["short"]
        if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > 0x7fffffff:
            raise ValueError(f"gpu.sloBurn: rules[{i}]: short must be an integer >= 1, got {k!r}")
        if out_rules and k <= out_rules[-1][0]:
            raise ValueError(f"gpu.sloBurn: rules[{i}]: short {k!r} does not ascend strictly")
        out_rules.append((int(k), _burn_decimal(f"rules[{i}]: factor", r["factor"], 1, BURN_F_MAX)))
    ms = v.get("minSamples", 1)
    if isinstance(ms, bool) or not isinstance(ms, int) or ms < 1 or ms > 0x7fffffff:
        raise ValueError(f"gpu.sloBurn: minSamples must be an integer >= 1, got {ms!r}")
    if default is None and not any(o is not None for o in named.values()):
        return None
    return {"default": default, "services": named, "rules": out_rules, "minSamples": int(ms)}


def slo_burn(cfg: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The validated gpu.sloBurn object of a config (None: off)."""
    return parse_slo_burn(gpu_opt(cfg, "sloBurn"))


def check_slo_burn(sb: Optional[Dict[str, Any]], window: int) -> None:
    """The bound an engine puts on the rules' spans when it is constructed: at most
    windowSizeInIntervals (as check_recent_windows)."""
    if sb and sb["rules"][-1][0] > int(window):
        raise ValueError(f"gpu.sloBurn.rules: short at most windowSizeInIntervals ({int(window)}), "
                         f"got {sb['rules'][-1][0]}")


def burn_tables(sb: Optional[Dict[str, Any]]) -> Tuple[List[List[int]], Dict[str, int], int]:
    """(classes, service -> class, default class) as the engine takes them, by sl's scheme
    (slo_tables): class 0 is "no row" (an empty list), class 1 the default objective [T, q] when
    there is one, then one class per named service with an objective, in config order; a service
    named with null maps to class 0."""
    if not sb:
        return [], {}, 0
    classes: List[List[int]] = [[]]
    default_class = 0
    if sb["default"] is not None:
        classes.append(list(sb["default"]))
        default_class = 1
    services: Dict[str, int] = {}
    for name, o in sb["services"].items():
        if o is not None:
            classes.append(list(o))
            services[name] = len(classes) - 1
        else:
            services[name] = 0
    return classes, services, default_class


TRAFFIC_MAX_RULES = 4       # kernel_api.h TF_MAX_RULES
TRAFFIC_SHORT_MAX = 64      # buckets of a rule's recent span (the bound the 64-bit products rest on)
TRAFFIC_Z_DEFAULT = 3000    # z * 1000


def _traffic_decimal(where: str, p: Any, lo: int, hi: int) -> int:
    """A decimal with at most three places as the integer ``p * 1000`` in lo .. hi, read from its
    text (never through float arithmetic), as _burn_decimal."""
    if isinstance(p, bool) or not isinstance(p, (int, float, str, decimal.Decimal)):
        raise ValueError(f"gpu.trafficWatch: {where}: {p!r} is not a number")
    try:
        d = decimal.Decimal(repr(p) if isinstance(p, float) else str(p).strip())
    except decimal.InvalidOperation:
        raise ValueError(f"gpu.trafficWatch: {where}: {p!r} is not a number") from None
    if not d.is_finite():
        raise ValueError(f"gpu.trafficWatch: {where}: {p!r} is not finite")
    q = d * 1000
    if q != q.to_integral_value():
        raise ValueError(f"gpu.trafficWatch: {where}: {p!r} has more than three decimals")
    q = int(q)
    if not lo <= q <= hi:
        raise ValueError(f"gpu.trafficWatch: {where}: {p!r} is outside {lo / 1000:g} .. {hi / 1000:g}")
    return q


def _parse_traffic_class(where: str, v: Any) -> Optional[int]:
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.trafficWatch: {where} must be an object with 'minRate' (or null), got {v!r}")
    extra = set(v) - {"minRate"}
    if extra:
        raise ValueError(f"gpu.trafficWatch: {where}: unknown key(s) {sorted(extra, key=str)!r}")
    if "minRate" not in v:
        raise ValueError(f"gpu.trafficWatch: {where} needs 'minRate', got {v!r}")
    r = v["minRate"]
    if isinstance(r, bool) or not isinstance(r, int):
        raise ValueError(f"gpu.trafficWatch: {where}: minRate {r!r} is not an integer")
    if not 1 <= r <= SLO_T_MAX:
        raise ValueError(f"gpu.trafficWatch: {where}: minRate {r!r} is outside 1 .. {SLO_T_MAX}")
    return int(r)


def parse_traffic_watch(v: Any) -> Optional[Dict[str, Any]]:
    """gpu.trafficWatch -> {"default": minRate | None, "services": {name: minRate | None},
    "rules": [(short, r_d, r_s, z), ...], "minBuckets": n}.  ``minRate`` is a JSON integer in
    1 .. 2147483647 (bool, float and str are rejected); ``default`` may be absent or null, a service
    named with null gets no rows.  ``rules``: 1 to 4 objects {"short": k, "drop": x, "surge": y,
    "z": w}, ``short`` a JSON integer in 1 .. 64, strictly ascending (its bound against the window is
    the engine's, check_traffic_watch); ``drop`` a decimal with at most three places, r_d = drop *
    1000 in 1 .. 999; ``surge`` likewise, r_s = surge * 1000 in 1001 .. 1000000; at least one of the
    two (the missing one is 0 in the result); ``z`` likewise, z * 1000 in 0 .. 100000, default 3.
    ``minBuckets``: a JSON integer >= 3 (default 8).  None, or an object in which no service has a
    minRate -> None (stream off); anything else raises ValueError."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.trafficWatch: an object with 'default' and / or 'services', and 'rules', got {v!r}")
    extra = set(v) - {"default", "services", "rules", "minBuckets"}
    if extra:
        raise ValueError(f"gpu.trafficWatch: unknown key(s) {sorted(extra, key=str)!r}")
    default = _parse_traffic_class("default", v.get("default"))
    services = v.get("services")
    if services is None:
        services = {}
    if not isinstance(services, dict):
        raise ValueError(f"gpu.trafficWatch: services must be an object, got {services!r}")
    named: Dict[str, Optional[int]] = {}
    for name, o in services.items():
        if not isinstance(name, str):
            raise ValueError(f"gpu.trafficWatch: service name {name!r} is not a string")
        named[name] = _parse_traffic_class(f"services[{name!r}]", o)
    rules = v.get("rules")
    if not isinstance(rules, list) or not 1 <= len(rules) <= TRAFFIC_MAX_RULES:
        raise ValueError(f"gpu.trafficWatch: rules must list 1 to {TRAFFIC_MAX_RULES} rules, got {rules!r}")
    out_rules: List[Tuple[int, int, int, int]] = []
    for i, r in enumerate(rules):
        if not isinstance(r, dict):
            raise ValueError(f"gpu.trafficWatch: rules[{i}] must be an object with 'short' and 'drop' and / or 'surge', got {r!r}")
        extra = set(r) - {"short", "drop", "surge", "z"}
        if extra:
            raise ValueError(f"gpu.trafficWatch: rules[{i}]: unknown key(s) {sorted(extra, key=str)!r}")
        if "short" not in r or ("drop" not in r and "surge" not in r):
            raise ValueError(f"gpu.trafficWatch: rules[{i}] needs 'short' and at least one of 'drop' and 'surge', got {r!r}")
        k = r["short"]
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= TRAFFIC_SHORT_MAX:
            raise ValueError(f"gpu.trafficWatch: rules[{i}]: short must be an integer in 1 .. {TRAFFIC_SHORT_MAX}, got {k!r}")
        if out_rules and k <= out_rules[-1][0]:
            raise ValueError(f"gpu.trafficWatch: rules[{i}]: short {k!r} does not ascend strictly")
        rd = _traffic_decimal(f"rules[{i}]: drop", r["drop"], 1, 999) if "drop" in r else 0
        rs = _traffic_decimal(f"rules[{i}]: surge", r["surge"], 1001, 1000000) if "surge" in r else 0
        z = _traffic_decimal(f"rules[{i}]: z", r["z"], 0, 100000) if "z" in r else TRAFFIC_Z_DEFAULT
        out_rules.append((int(k), rd, rs, z))
    mb = v.get("minBuckets", 8)
    if isinstance(mb, bool) or not isinstance(mb, int) or mb < 3 or mb > 0x7fffffff:
        raise ValueError(f"gpu.trafficWatch: minBuckets must be an integer >= 3, got {mb!r}")
    if default is None and not any(o is not None for o in named.values()):
        return None
    return {"default": default, "services": named, "rules": out_rules, "minBuckets": int(mb)}


def traffic_watch(cfg: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The validated gpu.trafficWatch object of a config (None: off)."""
    return parse_traffic_watch(gpu_opt(cfg, "trafficWatch"))


def check_traffic_watch(tf: Optional[Dict[str, Any]], window: int) -> None:
    """The bound an engine puts on the rules' spans when it is constructed: at most
    windowSizeInIntervals (as check_slo_burn)."""
    if tf and tf["rules"][-1][0] > int(window):
        raise ValueError(f"gpu.trafficWatch.rules: short at most windowSizeInIntervals ({int(window)}), "
                         f"got {tf['rules'][-1][0]}")


def traffic_tables(tf: Optional[Dict[str, Any]]) -> Tuple[List[List[int]], Dict[str, int], int]:
    """(classes, service -> class, default class) as the engine takes them, by sl's scheme
    (burn_tables): class 0 is "no row" (an empty list), class 1 the default [minRate] when there is
    one, then one class per named service with a minRate, in config order; a service named with
    null maps to class 0."""
    if not tf:
        return [], {}, 0
    classes: List[List[int]] = [[]]
    default_class = 0
    if tf["default"] is not None:
        classes.append([tf["default"]])
        default_class = 1
    services: Dict[str, int] = {}
    for name, o in tf["services"].items():
        if o is not None:
            classes.append([o])
            services[name] = len(classes) - 1
        else:
            services[name] = 0
    return classes, services, default_class


PEER_PCT_DEFAULT = 95000    # percentile * 1000
PEER_Z_DEFAULT = 3000       # z * 1000
PEER_KEYS = ("percentile", "default", "services", "high", "low", "z", "minDelta", "minPeers", "minSamples")


def _peer_decimal(where: str, p: Any, lo: int, hi: int) -> int:
    """A decimal with at most three places as the integer ``p * 1000`` in lo .. hi, read from its
    text (never through float arithmetic), as _traffic_decimal."""
    if isinstance(p, bool) or not isinstance(p, (int, float, str, decimal.Decimal)):
        raise ValueError(f"gpu.peerOutliers: {where}: {p!r} is not a number")
    try:
        d = decimal.Decimal(repr(p) if isinstance(p, float) else str(p).strip())
    except decimal.InvalidOperation:
        raise ValueError(f"gpu.peerOutliers: {where}: {p!r} is not a number") from None
    if not d.is_finite():
        raise ValueError(f"gpu.peerOutliers: {where}: {p!r} is not finite")
    q = d * 1000
    if q != q.to_integral_value():
        raise ValueError(f"gpu.peerOutliers: {where}: {p!r} has more than three decimals")
    q = int(q)
    if not lo <= q <= hi:
        raise ValueError(f"gpu.peerOutliers: {where}: {p!r} is outside {lo / 1000:g} .. {hi / 1000:g}")
    return q


def _peer_int(where: str, v: Any, lo: int, hi: int = SLO_T_MAX) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"gpu.peerOutliers: {where} {v!r} is not an integer")
    if not lo <= v <= hi:
        raise ValueError(f"gpu.peerOutliers: {where} {v!r} is outside {lo} .. {hi}")
    return int(v)


def _parse_peer_class(where: str, v: Any) -> Optional[int]:
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.peerOutliers: {where} must be an object with 'minValue' (or null), got {v!r}")
    extra = set(v) - {"minValue"}
    if extra:
        raise ValueError(f"gpu.peerOutliers: {where}: unknown key(s) {sorted(extra, key=str)!r}")
    if "minValue" not in v:
        raise ValueError(f"gpu.peerOutliers: {where} needs 'minValue', got {v!r}")
    return _peer_int(f"{where}: minValue", v["minValue"], 1)


def parse_peer_outliers(v: Any) -> Optional[Dict[str, Any]]:
    """gpu.peerOutliers -> {"percentile": q, "default": minValue | None, "services": {name: minValue
    | None}, "high": r_h, "low": r_l, "z": z, "minDelta": n, "minPeers": n, "minSamples": n}.
    ``percentile``: one value under gpu.windowPercentiles' rules, q = p * 1000 (default 95).
    ``minValue`` is a JSON integer in 1 .. 2147483647 (bool, float and str are rejected); ``default``
    may be absent or null, a service named with null gets no rows.  ``high``: a decimal with at most
    three places, r_h = high * 1000 in 1001 .. 1000000; ``low`` likewise, r_l = low * 1000 in
    1 .. 999; at least one of the two (the missing one is 0 in the result); ``z`` likewise, z * 1000
    in 0 .. 100000, default 3.  ``minDelta``: a JSON integer in 0 .. 2147483647 (default 0);
    ``minPeers``: a JSON integer >= 3 (default 5); ``minSamples``: a JSON integer in
    1 .. 2147483647 (default 20).  None, or an object in which no service has a minValue -> None
    (stream off); anything else raises ValueError."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.peerOutliers: an object with 'default' and / or 'services', and 'high' and / or 'low', got {v!r}")
    extra = set(v) - set(PEER_KEYS)
    if extra:
        raise ValueError(f"gpu.peerOutliers: unknown key(s) {sorted(extra, key=str)!r}")
    q = PEER_PCT_DEFAULT
    if "percentile" in v:
        try:
            qs = parse_window_percentiles([v["percentile"]])
        except ValueError as e:
            raise ValueError(str(e).replace("gpu.windowPercentiles", "gpu.peerOutliers: percentile")) from None
        if len(qs) != 1:
            raise ValueError(f"gpu.peerOutliers: percentile: one percentile, got {v['percentile']!r}")
        q = qs[0]
    default = _parse_peer_class("default", v.get("default"))
    services = v.get("services")
    if services is None:
        services = {}
    if not isinstance(services, dict):
        raise ValueError(f"gpu.peerOutliers: services must be an object, got {services!r}")
    named: Dict[str, Optional[int]] = {}
    for name, o in services.items():
        if not isinstance(name, str):
            raise ValueError(f"gpu.peerOutliers: service name {name!r} is not a string")
        named[name] = _parse_peer_class(f"services[{name!r}]", o)
    if "high" not in v and "low" not in v:
        raise ValueError("gpu.peerOutliers: needs at least one of 'high' and 'low'")
    r_h = _peer_decimal("high", v["high"], 1001, 1000000) if "high" in v else 0
    r_l = _peer_decimal("low", v["low"], 1, 999) if "low" in v else 0
    z = _peer_decimal("z", v["z"], 0, 100000) if "z" in v else PEER_Z_DEFAULT
    min_delta = _peer_int("minDelta", v.get("minDelta", 0), 0)
    min_peers = _peer_int("minPeers", v.get("minPeers", 5), 3)
    min_samples = _peer_int("minSamples", v.get("minSamples", 20), 1)
    if default is None and not any(o is not None for o in named.values()):
        return None
    return {"percentile": q, "default": default, "services": named, "high": r_h, "low": r_l, "z": z,
            "minDelta": min_delta, "minPeers": min_peers, "minSamples": min_samples}


def peer_outliers(cfg: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The validated gpu.peerOutliers object of a config (None: off)."""
    return parse_peer_outliers(gpu_opt(cfg, "peerOutliers"))


def check_peer_outliers(po: Optional[Dict[str, Any]]) -> None:
    """What an engine checks of the parsed object when it is constructed (as check_traffic_watch;
    no setting depends on the window): the ranges parse_peer_outliers guarantees, for a caller
    that built the object itself."""
    if not po:
        return
    ok = (1 <= po["percentile"] <= PCT_SCALE and (po["high"] == 0 or 1001 <= po["high"] <= 1000000)
          and (po["low"] == 0 or 1 <= po["low"] <= 999) and (po["high"] or po["low"]) and 0 <= po["z"] <= 100000
          and 0 <= po["minDelta"] <= SLO_T_MAX and 3 <= po["minPeers"] <= SLO_T_MAX and 1 <= po["minSamples"] <= SLO_T_MAX)
    if not ok:
        raise ValueError(f"gpu.peerOutliers: settings out of range: {po!r}")


def peer_tables(po: Optional[Dict[str, Any]]) -> Tuple[List[List[int]], Dict[str, int], int]:
    """(classes, service -> class, default class) as the engine takes them, by sl's scheme
    (traffic_tables): class 0 is "no row" (an empty list), class 1 the default [minValue] when there
    is one, then one class per named service with a minValue, in config order; a service named with
    null maps to class 0."""
    if not po:
        return [], {}, 0
    classes: List[List[int]] = [[]]
    default_class = 0
    if po["default"] is not None:
        classes.append([po["default"]])
        default_class = 1
    services: Dict[str, int] = {}
    for name, o in po["services"].items():
        if o is not None:
            classes.append([o])
            services[name] = len(classes) - 1
        else:
            services[name] = 0
    return classes, services, default_class


SHIFT_MAX_RULES = 4         # kernel_api.h LS_MAX_RULES
SHIFT_SHORT_MAX = 64        # buckets of a rule's recent span
SHIFT_DELTA_MAX = 1073741823  # 2 minDelta stays an int32
SHIFT_Z_DEFAULT = 3000      # z * 1000


def _shift_decimal(where: str, p: Any, lo: int, hi: int) -> int:
    """A decimal with at most three places as the integer ``p * 1000`` in lo .. hi, read from its
    text (never through float arithmetic), as _traffic_decimal."""
    if isinstance(p, bool) or not isinstance(p, (int, float, str, decimal.Decimal)):
        raise ValueError(f"gpu.latencyShift: {where}: {p!r} is not a number")
    try:
        d = decimal.Decimal(repr(p) if isinstance(p, float) else str(p).strip())
    except decimal.InvalidOperation:
        raise ValueError(f"gpu.latencyShift: {where}: {p!r} is not a number") from None
    if not d.is_finite():
        raise ValueError(f"gpu.latencyShift: {where}: {p!r} is not finite")
    q = d * 1000
    if q != q.to_integral_value():
        raise ValueError(f"gpu.latencyShift: {where}: {p!r} has more than three decimals")
    q = int(q)
    if not lo <= q <= hi:
        raise ValueError(f"gpu.latencyShift: {where}: {p!r} is outside {lo / 1000:g} .. {hi / 1000:g}")
    return q


def _shift_int(where: str, v: Any, lo: int, hi: int = SLO_T_MAX) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"gpu.latencyShift: {where} {v!r} is not an integer")
    if not lo <= v <= hi:
        raise ValueError(f"gpu.latencyShift: {where} {v!r} is outside {lo} .. {hi}")
    return int(v)


def _parse_shift_class(where: str, v: Any) -> Optional[int]:
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.latencyShift: {where} must be an object with 'minDelta' (or null), got {v!r}")
    extra = set(v) - {"minDelta"}
    if extra:
        raise ValueError(f"gpu.latencyShift: {where}: unknown key(s) {sorted(extra, key=str)!r}")
    if "minDelta" not in v:
        raise ValueError(f"gpu.latencyShift: {where} needs 'minDelta', got {v!r}")
    return _shift_int(f"{where}: minDelta", v["minDelta"], 1, SHIFT_DELTA_MAX)


def parse_latency_shift(v: Any) -> Optional[Dict[str, Any]]:
    """gpu.latencyShift -> {"default": minDelta | None, "services": {name: minDelta | None},
    "rules": [(short, q, r_u, r_d, z), ...], "minRecent": n, "minBaseline": n}.  ``minDelta`` is a
    JSON integer in 1 .. 1073741823 (bool, float and str are rejected); ``default`` may be absent or
    null, a service named with null gets no rows.  ``rules``: 1 to 4 objects {"short": k,
    "percentile": p, "up": x, "down": y, "z": w} with ``short`` ascending and no (short, percentile)
    pair twice (one span may be judged at several percentiles, in any order); ``short`` a JSON integer in 1 .. 64 (its bound against the window is the engine's,
    check_latency_shift); ``percentile`` one entry by parse_window_percentiles' rules, q = p * 1000 in
    1 .. 99999; ``up`` and ``down`` decimals with at most three places, r * 1000 in 1001 .. 1000000,
    at least one of the two (the missing one is 0 in the result); ``z`` likewise, z * 1000 in
    0 .. 100000, default 3.  ``minRecent``: a JSON integer >= 1 (default 20); ``minBaseline``: >= 2
    (default 100).  None, or an object in which no service has a minDelta -> None (stream off);
    anything else raises ValueError."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.latencyShift: an object with 'default' and / or 'services', and 'rules', got {v!r}")
    extra = set(v) - {"default", "services", "rules", "minRecent", "minBaseline"}
    if extra:
        raise ValueError(f"gpu.latencyShift: unknown key(s) {sorted(extra, key=str)!r}")
    default = _parse_shift_class("default", v.get("default"))
    services = v.get("services")
    if services is None:
        services = {}
    if not isinstance(services, dict):
        raise ValueError(f"gpu.latencyShift: services must be an object, got {services!r}")
    named: Dict[str, Optional[int]] = {}
    for name, o in services.items():
        if not isinstance(name, str):
            raise ValueError(f"gpu.latencyShift: service name {name!r} is not a string")
        named[name] = _parse_shift_class(f"services[{name!r}]", o)
    rules = v.get("rules")
    if not isinstance(rules, list) or not 1 <= len(rules) <= SHIFT_MAX_RULES:
        raise ValueError(f"gpu.latencyShift: rules must list 1 to {SHIFT_MAX_RULES} rules, got {rules!r}")
    out_rules: List[Tuple[int, int, int, int, int]] = []
    for i, r in enumerate(rules):
        if not isinstance(r, dict):
            raise ValueError(f"gpu.latencyShift: rules[{i}] must be an object with 'short', 'percentile' and 'up' and / or 'down', got {r!r}")
        extra = set(r) - {"short", "percentile", "up", "down", "z"}
        if extra:
            raise ValueError(f"gpu.latencyShift: rules[{i}]: unknown key(s) {sorted(extra, key=str)!r}")
        if "short" not in r or "percentile" not in r or ("up" not in r and "down" not in r):
            raise ValueError(f"gpu.latencyShift: rules[{i}] needs 'short', 'percentile' and at least one of 'up' and 'down', got {r!r}")
        k = r["short"]
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= SHIFT_SHORT_MAX:
            raise ValueError(f"gpu.latencyShift: rules[{i}]: short must be an integer in 1 .. {SHIFT_SHORT_MAX}, got {k!r}")
        try:
            qs = parse_window_percentiles([r["percentile"]])
        except ValueError as e:
            raise ValueError(str(e).replace("gpu.windowPercentiles", f"gpu.latencyShift: rules[{i}]: percentile")) from None
        if len(qs) != 1 or qs[0] >= PCT_SCALE:
            raise ValueError(f"gpu.latencyShift: rules[{i}]: percentile {r['percentile']!r} is outside (0, 100)")
        q = qs[0]
        if out_rules and (int(k) < out_rules[-1][0] or any((int(k), q) == o[:2] for o in out_rules)):
            raise ValueError(f"gpu.latencyShift: rules[{i}]: short {k!r} descends, or (short, percentile) "
                             f"({k!r}, {r['percentile']!r}) stands twice")
        ru = _shift_decimal(f"rules[{i}]: up", r["up"], 1001, 1000000) if "up" in r else 0
        rd = _shift_decimal(f"rules[{i}]: down", r["down"], 1001, 1000000) if "down" in r else 0
        z = _shift_decimal(f"rules[{i}]: z", r["z"], 0, 100000) if "z" in r else SHIFT_Z_DEFAULT
        out_rules.append((int(k), q, ru, rd, z))
    min_recent = _shift_int("minRecent", v.get("minRecent", 20), 1)
    min_baseline = _shift_int("minBaseline", v.get("minBaseline", 100), 2)
    if default is None and not any(o is not None for o in named.values()):
        return None
    return {"default": default, "services": named, "rules": out_rules, "minRecent": min_recent,
            "minBaseline": min_baseline}


def latency_shift(cfg: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The validated gpu.latencyShift object of a config (None: off)."""
    return parse_latency_shift(gpu_opt(cfg, "latencyShift"))


def check_latency_shift(ls: Optional[Dict[str, Any]], window: int) -> None:
    """The bound an engine puts on the rules' spans when it is constructed: at most
    windowSizeInIntervals (as check_traffic_watch)."""
    if ls and ls["rules"][-1][0] > int(window):
        raise ValueError(f"gpu.latencyShift.rules: short at most windowSizeInIntervals ({int(window)}), "
                         f"got {ls['rules'][-1][0]}")


def shift_tables(ls: Optional[Dict[str, Any]]) -> Tuple[List[List[int]], Dict[str, int], int]:
    """(classes, service -> class, default class) as the engine takes them, by sl's scheme
    (traffic_tables): class 0 is "no row" (an empty list), class 1 the default [minDelta] when there
    is one, then one class per named service with a minDelta, in config order; a service named with
    null maps to class 0."""
    if not ls:
        return [], {}, 0
    classes: List[List[int]] = [[]]
    default_class = 0
    if ls["default"] is not None:
        classes.append([ls["default"]])
        default_class = 1
    services: Dict[str, int] = {}
    for name, o in ls["services"].items():
        if o is not None:
            classes.append([o])
            services[name] = len(classes) - 1
        else:
            services[name] = 0
    return classes, services, default_class


INCIDENT_SOURCES = ("sb", "tf", "po", "ls")   # incidentcmp.h IC_SB .. IC_LS, the order of a series' rows
# the gpu key of each source's own stream
INCIDENT_SOURCE_KEYS = {"sb": "sloBurn", "tf": "trafficWatch", "po": "peerOutliers", "ls": "latencyShift"}
INCIDENT_RUN_MAX = 255        # the runs saturate there (incidentcmp.h)
INCIDENT_REMIND_MAX = 65535


def _incident_int(where: str, v: Any, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"gpu.incidents: {where} {v!r} is not an integer")
    if not lo <= v <= hi:
        raise ValueError(f"gpu.incidents: {where} {v!r} is outside {lo} .. {hi}")
    return int(v)


def parse_incidents(v: Any) -> Optional[Dict[str, Any]]:
    """gpu.incidents -> {"sources": {name: (openAfter, closeAfter)}, "remindEvery": n, "email": bool}.
    ``sources`` holds one to four of sb, tf, po, ls, each an object with ``openAfter`` and
    ``closeAfter``, JSON integers in 1 .. 255 (bool, float and str are rejected); ``remindEvery`` a
    JSON integer, 0 (never, the default) or 1 .. 65535 rollovers; ``email`` a JSON boolean (default
    false).  Unknown members at any level raise ValueError.  None -> None (stream off).  That a named
    source's own stream is configured is check_incidents' part."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError(f"gpu.incidents: an object with 'sources', got {v!r}")
    extra = set(v) - {"sources", "remindEvery", "email"}
    if extra:
        raise ValueError(f"gpu.incidents: unknown key(s) {sorted(extra, key=str)!r}")
    sources = v.get("sources")
    if not isinstance(sources, dict) or not sources:
        raise ValueError(f"gpu.incidents: sources must be an object naming one to four of {', '.join(INCIDENT_SOURCES)}, "
                         f"got {sources!r}")
    out: Dict[str, Tuple[int, int]] = {}
    for name in INCIDENT_SOURCES:  # (the result's order is the rows' order, whatever the config's)
        if name not in sources:
            continue
        o = sources[name]
        if not isinstance(o, dict):
            raise ValueError(f"gpu.incidents: sources[{name!r}] must be an object with 'openAfter' and 'closeAfter', got {o!r}")
        extra = set(o) - {"openAfter", "closeAfter"}
        if extra:
            raise ValueError(f"gpu.incidents: sources[{name!r}]: unknown key(s) {sorted(extra, key=str)!r}")
        if "openAfter" not in o or "closeAfter" not in o:
            raise ValueError(f"gpu.incidents: sources[{name!r}] needs 'openAfter' and 'closeAfter', got {o!r}")
        out[name] = (_incident_int(f"sources[{name!r}]: openAfter", o["openAfter"], 1, INCIDENT_RUN_MAX),
                     _incident_int(f"sources[{name!r}]: closeAfter", o["closeAfter"], 1, INCIDENT_RUN_MAX))
    extra = set(sources) - set(INCIDENT_SOURCES)
    if extra:
        raise ValueError(f"gpu.incidents: sources: unknown source(s) {sorted(extra, key=str)!r}")
    remind = _incident_int("remindEvery", v.get("remindEvery", 0), 0, INCIDENT_REMIND_MAX)
    email = v.get("email", False)
    if not isinstance(email, bool):
        raise ValueError(f"gpu.incidents: email {email!r} is not a boolean")
    return {"sources": out, "remindEvery": remind, "email": email}


def incidents(cfg: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The validated gpu.incidents object of a config (None: off)."""
    return parse_incidents(gpu_opt(cfg, "incidents"))


def check_incidents(ic: Optional[Dict[str, Any]], cfg: Dict[str, Any]) -> None:
    """What a config, a service and an engine ask of gpu.incidents beyond its own shape: every named
    source's own stream is configured (sb needs gpu.sloBurn, ...)."""
    if not ic:
        return
    parsers = {"sb": slo_burn, "tf": traffic_watch, "po": peer_outliers, "ls": latency_shift}
    for name in ic["sources"]:
        if not parsers[name](cfg):
            raise ValueError(f"gpu.incidents: source {name!r} needs gpu.{INCIDENT_SOURCE_KEYS[name]} to be set")


def incident_tables(ic: Optional[Dict[str, Any]]) -> Tuple[List[int], List[int]]:
    """(openAfter, closeAfter) per source in the order sb, tf, po, ls as the engine takes them; 0 / 0
    for a source that is not configured."""
    src = ic["sources"] if ic else {}
    return ([src[k][0] if k in src else 0 for k in INCIDENT_SOURCES],
            [src[k][1] if k in src else 0 for k in INCIDENT_SOURCES])


_BOOL_STRINGS = {"true": True, "false": False, "1": True, "0": False, "yes": True, "no": False}


def json_strip(txt: str) -> str:
    """The reference JSONstrip (util_methods.js:265-268), including its quirk."""
    return _STRIP_RE.sub("", txt)


def parse_config_text(txt: str) -> Dict[str, Any]:
    return json.loads(json_strip(txt))


def read_apm_config(path: Optional[str] = None, first_run: bool = False) -> Optional[Dict[str, Any]]:
    path = os.path.abspath(path or os.environ.get("APM_CONFIG", DEFAULT_CONFIG_PATH))
    if not os.path.exists(path):
        raise FileNotFoundError(f"APM config file does not exist: {path}")
    with open(path, "r", encoding="utf-8") as fh:
        content = fh.read()
    try:
        cfg = parse_config_text(content)
    except json.JSONDecodeError as e:
        log.error("Could not parse JSON content from APM config file %s: %s", path, e)
        return None
    cfg["apmConfigFilePath"] = path
    cfg.setdefault("gpu", {})
    unknown = set(cfg["gpu"]) - set(GPU_DEFAULTS) - set(GPU_OPTIONAL)
    for k in sorted(unknown):
        log.warning("unknown key gpu.%s in %s (ignored)", k, path)
    merged = dict(GPU_DEFAULTS)
    merged.update({k: v for k, v in cfg["gpu"].items() if k in GPU_DEFAULTS or k in GPU_OPTIONAL})
    cfg["gpu"] = merged
    if "windowPercentiles" in merged:
        parse_window_percentiles(merged["windowPercentiles"])  # ValueError: a bad list stops the load
    if "latencyObjectives" in merged:
        parse_latency_objectives(merged["latencyObjectives"])  # likewise
    if "leaderboard" in merged:
        parse_leaderboard(merged["leaderboard"])  # likewise
    if "serviceWindow" in merged:
        parse_service_window(merged["serviceWindow"])  # likewise
    if "recentWindows" in merged:
        parse_recent_windows(merged["recentWindows"])  # likewise
    if "sloBurn" in merged:
        parse_slo_burn(merged["sloBurn"])  # likewise
    if "trafficWatch" in merged:
        parse_traffic_watch(merged["trafficWatch"])  # likewise
    if "peerOutliers" in merged:
        parse_peer_outliers(merged["peerOutliers"])  # likewise
    if "latencyShift" in merged:
        parse_latency_shift(merged["latencyShift"])  # likewise
    if "incidents" in merged:
        check_incidents(parse_incidents(merged["incidents"]), cfg)  # likewise; a source needs its own stream
    return cfg


def resolve(path: str, obj: Any, sep: str = ".") -> Any:
    """``resolve`` from util_methods.js:248-251."""
    cur = obj
    for p in path.split(sep):
        if cur is None:
            return None
        if isinstance(cur, dict):
            cur = cur.get(p)
        else:
            return None
    return cur


def as_bool(v: Any) -> bool:
    """Fix for quirk Q8: ``"false"`` disables (the reference treated any string as true)."""
    if isinstance(v, str):
        return _BOOL_STRINGS.get(v.strip().lower(), bool(v))
    return bool(v)


def default_config(replay: bool = False) -> Dict[str, Any]:
    """The shipped config.  ``replay=True`` switches the alert clock to log time
    (``gpu.alertClock = "entry"``): alert timestamps and cooldowns then depend only on the input,
    which is what replays, benchmarks and oracle comparisons need.  The shipped default is the
    reference's wall clock."""
    cfg = read_apm_config(DEFAULT_CONFIG_PATH)
    assert cfg is not None
    if replay:
        cfg["gpu"]["alertClock"] = "entry"
    return cfg


def overrides_for(cfg: Dict[str, Any], section: str) -> Dict[str, Any]:
    return ((cfg.get(section) or {}).get("overrides") or {}).get("services") or {}


class ConfigWatcher:
    """Poll-based equivalent of ``watchAPMConfig`` (md5 + size + 500 ms debounce)."""

    def __init__(self, cfg: Dict[str, Any], callback: Callable[[Dict[str, Any]], None],
                 restart_required: Iterable[str] = (), poll_s: float = 0.5):
        self.cfg = cfg
        self.path = cfg["apmConfigFilePath"]
        self.callback = callback
        self.restart_required = list(restart_required)
        self.poll_s = poll_s
        self._prev = self._digest()
        self._stop = threading.Event()
        self._th: Optional[threading.Thread] = None

    def _digest(self):
        try:
            with open(self.path, "rb") as fh:
                b = fh.read()
            return hashlib.md5(b).hexdigest(), len(b)
        except OSError:
            return None

    def check_once(self) -> bool:
        cur = self._digest()
        if cur is None or cur == self._prev:
            return False
        time.sleep(0.5 if self.poll_s >= 0.5 else 0)  # let the file settle (debounce)
        cur = self._digest()
        self._prev = cur
        new = read_apm_config(self.path)
        if new is None:
            log.warning("config JSON could not be processed; keeping the previous config")
            return False
        for var in self.restart_required:
            old_v, new_v = resolve(var, self.cfg), resolve(var, new)
            if json.dumps(old_v, sort_keys=True) != json.dumps(new_v, sort_keys=True):
                log.warning("%s was changed on settings reload, but this will not take effect "
                            "without a restart.", var)
        self.cfg = new
        self.callback(new)
        return True

    def _run(self):
        while not self._stop.wait(self.poll_s):
            try:
                self.check_once()
            except Exception as e:  # pragma: no cover - defensive
                log.error("config watcher error: %s", e)

    def start(self) -> "ConfigWatcher":
        self._th = threading.Thread(target=self._run, name="apm-config-watch", daemon=True)
        self._th.start()
        return self

    def stop(self):
        self._stop.set()


def zscore_lag_settings(cfg: Dict[str, Any], service: str,
                        emulate_aliasing: bool = False) -> List[Dict[str, Any]]:
    """Per-service z-score settings (stream_calc_z_score.js:106-132).

    With ``emulate_aliasing`` the reference bug Q4 is reproduced: the override is written
    into ``cfg['streamCalcZScore']['defaults']`` itself, so it leaks to later services.
    Q5 (an override of 0 is ignored because it is falsy) is kept in both modes only when
    emulating; otherwise an explicit 0 is honoured.
    """
    zc = cfg["streamCalcZScore"]
    defaults = zc["defaults"]
    settings = defaults if emulate_aliasing else copy.deepcopy(defaults)
    ovr = ((zc.get("overrides") or {}).get("services") or {}).get(service)
    if ovr:
        for idx, el in enumerate(settings):
            for lag, vals in ovr.items():
                if str(el["LAG"]) == str(lag) or _num_eq(el["LAG"], lag):
                    if emulate_aliasing:
                        if vals.get("THRESHOLD"):
                            settings[idx]["THRESHOLD"] = vals["THRESHOLD"]
                        if vals.get("INFLUENCE"):
                            settings[idx]["INFLUENCE"] = vals["INFLUENCE"]
                    else:
                        if vals.get("THRESHOLD") is not None:
                            settings[idx]["THRESHOLD"] = vals["THRESHOLD"]
                        if vals.get("INFLUENCE") is not None:
                            settings[idx]["INFLUENCE"] = vals["INFLUENCE"]
    return settings


def _num_eq(a, b) -> bool:
    try:
        return float(a) == float(b)
    except (TypeError, ValueError):
        return False
