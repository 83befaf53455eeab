"""The flagship model: the fused MI355X APM pipeline.

``APMEngine`` maps the reference configuration (``config/apm_config.json`` sections
``streamParseTransactions`` .. ``streamProcessAlerts`` + the new ``gpu`` section) onto the native
``_apm_native.Engine`` and exposes a batch API:

    eng = APMEngine(cfg)
    eng.process([(path, bytes), ...])          # one ingest batch (whole lines per file)
    eng.take("fs"), eng.take("al"), ...        # reference wire-format records (keep_text=True)

One engine == one GPU == one process; the multi-GPU runner (``parallel.dist``) shards JVM hosts
across ranks.
"""
from __future__ import annotations

import logging
import math
import os
import time
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

from .. import _native
from ..models.oracle import file_kind, server_of
from ..ops.parse_ref import tz_table
from ..utils.config import (LEADERBOARD_KEYS, burn_tables, check_incidents, incident_tables, incidents, check_latency_shift, check_peer_outliers, check_recent_windows,
                            check_slo_burn, latency_shift, shift_tables,
                            check_traffic_watch, latency_objectives, leaderboard, peer_outliers, peer_tables, recent_windows, service_window, slo_burn, slo_tables,
                            traffic_tables, traffic_watch, window_percentiles)
from ..utils.timeparse import TzOffset

log = logging.getLogger("apm.pipeline")

KIND_CODE = {"SOAP": 0, "SERVER": 1, "APP": 2}

# Output streams (engine.h OutKind); the bit index is the position in this tuple.
OUT_KINDS = ("transactions", "audit_db", "db", "st", "fs", "al", "sx", "fb", "lh")
# Streams added after lh continue the enum here: OUT_KINDS keeps ending in "lh", which
# tests/test_hist_engine_gpu.py pins.
ALL_OUT_KINDS = OUT_KINDS + ("wp",)
# ... and tests/test_winpct_engine_gpu.py pins ALL_OUT_KINDS; ENGINE_OUT_KINDS is engine.h's OutKind
# up to sl.
ENGINE_OUT_KINDS = ALL_OUT_KINDS + ("sl",)
# ... and tests/test_slo_model.py pins ENGINE_OUT_KINDS; NATIVE_OUT_KINDS is engine.h's OutKind up
# to tk.
NATIVE_OUT_KINDS = ENGINE_OUT_KINDS + ("tk",)
# ... and tests/test_topk_model.py pins NATIVE_OUT_KINDS; DEVICE_OUT_KINDS is engine.h's OutKind up
# to sv.
DEVICE_OUT_KINDS = NATIVE_OUT_KINDS + ("sv",)
# ... and tests/test_svcwin_model.py pins DEVICE_OUT_KINDS and its last element; STREAM_OUT_KINDS is
# engine.h's OutKind up to rw.
STREAM_OUT_KINDS = DEVICE_OUT_KINDS + ("rw",)
# ... and tests/test_recent_*.py pin STREAM_OUT_KINDS; FULL_OUT_KINDS is engine.h's OutKind up to sb.
FULL_OUT_KINDS = STREAM_OUT_KINDS + ("sb",)
# ... and tests/test_burn_*.py pin FULL_OUT_KINDS; EVERY_OUT_KINDS is engine.h's OutKind up to tf.
EVERY_OUT_KINDS = FULL_OUT_KINDS + ("tf",)
# ... and tests/test_traffic_*.py pin EVERY_OUT_KINDS; WHOLE_OUT_KINDS is engine.h's OutKind up to po.
WHOLE_OUT_KINDS = EVERY_OUT_KINDS + ("po",)
# ... and tests/test_peers_*.py pin WHOLE_OUT_KINDS; COMPLETE_OUT_KINDS is engine.h's OutKind up to ls.
COMPLETE_OUT_KINDS = WHOLE_OUT_KINDS + ("ls",)
# ... and tests/test_shift_*.py pin COMPLETE_OUT_KINDS; TOTAL_OUT_KINDS is engine.h's OutKind in full and
# the tuple a stream's bit index comes from.
TOTAL_OUT_KINDS = COMPLETE_OUT_KINDS + ("ic",)
# keep_text=True materialises these; lh (K15 latency histograms), wp (K16 window percentiles),
# sl (K17 threshold counts), tk (K18 leaderboards), sv (K19 per-service window stats), rw (K20
# stats of the newest window buckets), sb (K21 SLO burn-rate breaches), tf (K22 traffic drops and
# surges), po (K23 peer-outlier servers), ls (K24 latency shifts) and ic (K25 incidents) are opt-in through
# `outputs` only
KEEP_TEXT_KINDS = tuple(k for k in OUT_KINDS if k != "lh")
# What the reference persists (db_insert queue): released + audit tx, fs, al.  `transactions`
# and `st` are internal hand-offs that only the AMQP bridge needs.
DB_OUTPUTS = ("audit_db", "db", "fs", "al")
MAX_LAGS = 16  # apm_types.h MAX_LAGS: LAG capacity per engine (each LAG is an HBM ring; see there)


def output_mask(kinds) -> int:
    m = 0
    for k in kinds:
        m |= 1 << TOTAL_OUT_KINDS.index(k)
    return m


def engine_config(cfg: Dict[str, Any], device: int = 0, keep_text: bool = False, outputs=None,
                  tz: Optional[TzOffset] = None, tz_centre_ms: Optional[int] = None, **kw) -> Dict[str, Any]:
    """Engine settings from the reference config keys + the `gpu` section.  keep_text=True
    materialises every stream but the opt-in lh / wp / sl / tk / sv / rw / sb / tf / po / ls / ic; `outputs` (iterable of TOTAL_OUT_KINDS) selects explicitly.
    The two add up: keep_text=True with outputs=("lh",) is every stream (before the lh stream
    existed, `outputs` was ignored under keep_text).  "wp" takes its percentiles from
    gpu.windowPercentiles (ValueError when the list is missing or malformed), "sl" its thresholds
    from gpu.latencyObjectives (likewise), "tk" its boards from gpu.leaderboard (likewise), "sv" its percentiles
    from gpu.serviceWindow (likewise), "rw" its spans and percentiles from gpu.recentWindows (likewise; the
    bound of a span against windowSizeInIntervals is checked where an engine is constructed, not here: a
    reload reads the settings through this function too), "sb" its objectives and rules from gpu.sloBurn
    (likewise, the bound of a rule's span included), "tf" its classes and rules from gpu.trafficWatch
    (likewise), "po" its percentile, classes and ratios from gpu.peerOutliers (likewise), "ls" its classes and rules from gpu.latencyShift (likewise), "ic" its sources from gpu.incidents (likewise; every source it names must be in `outputs` too).  `tz` (a TzOffset) stands in for gpu.timezone; the zone's
    transition table is centred on `tz_centre_ms` (default: the wall clock now, see
    ops.parse_ref.tz_table)."""
    g = cfg.get("gpu", {})
    win_pcts = window_percentiles(cfg)
    if "wp" in (outputs or ()) and not win_pcts:
        raise ValueError('outputs names "wp" but gpu.windowPercentiles is empty')
    slo_classes, slo_services, slo_default = slo_tables(latency_objectives(cfg))
    if "sl" in (outputs or ()) and not slo_classes:
        raise ValueError('outputs names "sl" but gpu.latencyObjectives holds no threshold')
    board = leaderboard(cfg)
    if "tk" in (outputs or ()) and not board:
        raise ValueError('outputs names "tk" but gpu.leaderboard is not set')
    svc_pcts = service_window(cfg)
    if "sv" in (outputs or ()) and not svc_pcts:
        raise ValueError('outputs names "sv" but gpu.serviceWindow is not set')
    recent = recent_windows(cfg)
    if "rw" in (outputs or ()) and not recent:
        raise ValueError('outputs names "rw" but gpu.recentWindows is not set')
    burn = slo_burn(cfg)
    if "sb" in (outputs or ()) and not burn:
        raise ValueError('outputs names "sb" but gpu.sloBurn is not set')
    sb_classes, sb_services, sb_default = burn_tables(burn)
    traffic = traffic_watch(cfg)
    if "tf" in (outputs or ()) and not traffic:
        raise ValueError('outputs names "tf" but gpu.trafficWatch is not set')
    tf_classes, tf_services, tf_default = traffic_tables(traffic)
    peers = peer_outliers(cfg)
    if "po" in (outputs or ()) and not peers:
        raise ValueError('outputs names "po" but gpu.peerOutliers is not set')
    po_classes, po_services, po_default = peer_tables(peers)
    shift = latency_shift(cfg)
    if "ls" in (outputs or ()) and not shift:
        raise ValueError('outputs names "ls" but gpu.latencyShift is not set')
    ls_classes, ls_services, ls_default = shift_tables(shift)
    ic = incidents(cfg)
    if "ic" in (outputs or ()):
        if not ic:
            raise ValueError('outputs names "ic" but gpu.incidents is not set')
        check_incidents(ic, cfg)
        for name in ic["sources"]:
            if name not in outputs:
                raise ValueError(f'outputs names "ic" and gpu.incidents the source {name!r}, but outputs does not name {name!r}')
    ic_open, ic_close = incident_tables(ic)
    # (the spans' bound against the window holds at construction only -- APMEngine.__init__ and the
    # native constructor: a reload may shorten the window below a span, which then reads all of it)
    zc = cfg["streamCalcZScore"]
    ac = cfg["streamProcessAlerts"]
    sc = cfg["streamCalcStats"]
    lags = sorted(((int(d["LAG"]), float(d["THRESHOLD"]), float(d["INFLUENCE"])) for d in zc["defaults"]),
                  key=lambda x: x[0])
    if len(lags) > MAX_LAGS:
        raise ValueError(f"at most {MAX_LAGS} LAG settings are supported per engine")
    suppressed_lags = {int(x) for x in ac.get("suppressedLags", [])}
    ring = {"float64": 8, "float32": 4, "bfloat16": 2, "bf16": 2}.get(g.get("ringDtype", "float64"), 8)
    if tz is None:
        tz = TzOffset(g.get("timezone", "local"))
    d = {
        "device": device,
        "max_series": int(g.get("maxSeries", 1 << 17)),
        "cell_cap": int(g.get("bucketCellCapacity", 16)),
        "spill_cap": int(g.get("bucketOverflowCapacity", 1 << 22)) // 40 or 1,
        "max_batch_bytes": int(g.get("batchBytes", 32 << 20)) * 2,
        # (below 2^21: the device join packs its per-event selection counts into 21-bit fields)
        "max_lines": min(int(g.get("maxLinesPerBatch", 1 << 20)) * 2, (1 << 21) - 1),
        # host-join tx staging per batch (grows by doubling when a batch needs more)
        "max_tx_per_batch": int(g.get("maxTxPerBatch", int(g.get("maxLinesPerBatch", 1 << 20)) * 2)),
        "ring_bytes": ring,
        "exact_mean": 1 if g.get("zscoreMeanMode", "rolling") == "exact" else 0,
        "sigma_stddev": 1 if g.get("zscoreSigma", "sqrt_mean") == "stddev" else 0,
        "resync_k": int(g.get("exactRecomputeEveryIntervals", 360)),
        "resync_mfma": bool(g.get("resyncOnMatrixCores", False)),
        "emulate_aliasing": 1 if g.get("emulateOverrideAliasing", False) else 0,
        "lags": lags,
        "lag_suppressed": [1 if l[0] in suppressed_lags else 0 for l in lags],
        "alert_window": int(ac["rollingAlertWindowSizeInIntervals"]),
        "alert_threshold": int(ac["requiredNumberBadIntervalsInAlertWindowToTrigger"]),
        "hard_min_ms": float(ac["hardMinMsAlertThreshold"]),
        "hard_min_tpm": float(ac["hardMinTpmAlertThreshold"]),
        "hard_max_ms": float(ac["hardMaxMsAlertThreshold"]),
        "both_only": 1 if ac.get("alertOnBothOnly") else 0,
        "cooldown_ms": float(ac["perServiceAlertCooldownInMinutes"]) * 60000.0,
        "cooldown_by_service": 1 if g.get("cooldownKey", "service") == "service" else 0,
        "alert_clock_entry": 1 if g.get("alertClock", "entry") == "entry" else 0,
        "interval_len": int(sc["intervalLengthInSeconds"]),
        "window": int(sc["windowSizeInIntervals"]),
        # bucket ring slots (0: window + buffer + 1, at least 40); a reload to a longer window grows it
        "nslot": int(g.get("bucketRingSlots", 0)),
        # HBM staging of a base checkpoint's ring rows; a larger ring streams (checkpoint.cpp)
        "ck_stage_bytes": int(float(g.get("checkpointStageMB", 2048)) * (1 << 20)),
        "buffer": int(sc["bufferSizeInIntervals"]),
        "record_ttl_ms": float(g.get("recordTtlSeconds", 120)) * 1000.0,
        "acct_ttl_ms": float(g.get("acctTtlSeconds", 120)) * 1000.0,
        "need_ttl_ms": float(g.get("needTtlSeconds", 30)) * 1000.0,
        "tz_table": tz_table(tz, tz_centre_ms),
        "join_threads": int(g.get("joinThreads", 0)),
        "pin_threads": bool(g.get("pinThreads", False)),
        "coll_timeout_ms": float(g.get("collectiveTimeoutSeconds", 300)) * 1000.0,
        "coll_init_timeout_ms": float(g.get("collectiveInitTimeoutSeconds", 120)) * 1000.0,
        # lock-step ranks decide the alert cooldown node-wide (one alert per service per node)
        "node_cooldown": 1 if g.get("nodeCooldown", True) else 0,
        # K4/K6 join on the GPU (devjoin.hip); false = host join workers (join.cpp)
        "device_join": 1 if g.get("joinOnDevice", True) else 0,
        "join_table_bits": max(10, (int(g.get("joinTableSlots", 1 << 21)) - 1).bit_length()),
        "need_arena": int(g.get("needArenaEntries", 1 << 18)),
        "join_chain_blocks": int(g.get("joinChainBlocks", 0)),
        # the ring holds every tx line not yet released (~70 s of tx text); small test engines
        # keep it proportional to their batch size
        "tx_ring_bytes": min(int(g.get("txTextRingMB", 4096)), max(256, (128 * int(g.get("batchBytes", 32 << 20))) >> 20)) << 20,
        "max_raw_services": max(int(g.get("maxRawServices", 1 << 18)), 2 * int(g.get("maxSeries", 1 << 17))),
        "outputs": output_mask(KEEP_TEXT_KINDS if keep_text else ()) | output_mask(outputs or ()),
        # K16: the percentiles of the wp stream as q = p * 1000, read at construction (a reload that
        # changes them is reported as needing a restart, like every other non-live setting)
        "win_pcts": win_pcts,
        # K17: the sl stream's threshold table (class 0: no row) and each named service's class,
        # likewise read at construction
        "slo_classes": slo_classes,
        "slo_services": slo_services,
        "slo_default": slo_default,
        # K18: the tk stream's rows per board, the boards' keys (kernel_api.h TopKKey codes, in row
        # order) and the tpm floor, likewise read at construction (None: gpu.leaderboard is not set)
        "tk_k": board["k"] if board else None,
        "tk_by": [LEADERBOARD_KEYS.index(b) for b in board["by"]] if board else [],
        "tk_min_tpm": board["minTpm"] if board else 0.0,
        # K19: the percentiles of the sv stream as q = p * 1000, likewise read at construction
        "svc_pcts": svc_pcts,
        # K20: the spans (buckets) and percentiles (q = p * 1000) of the rw stream, likewise
        "rw_buckets": recent["buckets"] if recent else [],
        "rw_pcts": recent["percentiles"] if recent else [],
        # K21: the class tables of the sb stream ([T, q] per class), its rules (span in buckets and
        # f = factor * 1000) and minSamples, likewise
        "sb_classes": sb_classes,
        "sb_services": sb_services,
        "sb_default": sb_default,
        "sb_short": [k for k, _f in burn["rules"]] if burn else [],
        "sb_factor": [f for _k, f in burn["rules"]] if burn else [],
        "sb_min_samples": burn["minSamples"] if burn else 1,
        # K22: the class tables of the tf stream ([minRate] per class), its rules (span in buckets,
        # r_d = drop * 1000 or 0, r_s = surge * 1000 or 0, z * 1000) and minBuckets, likewise
        "tf_classes": tf_classes,
        "tf_services": tf_services,
        "tf_default": tf_default,
        "tf_short": [r[0] for r in traffic["rules"]] if traffic else [],
        "tf_drop": [r[1] for r in traffic["rules"]] if traffic else [],
        "tf_surge": [r[2] for r in traffic["rules"]] if traffic else [],
        "tf_z": [r[3] for r in traffic["rules"]] if traffic else [],
        "tf_min_buckets": traffic["minBuckets"] if traffic else 8,
        # K23: the percentile (q = p * 1000), the class tables of the po stream ([minValue] per class),
        # r_h = high * 1000 or 0, r_l = low * 1000 or 0, z * 1000, minDelta, minPeers and minSamples, likewise
        "po_pct": peers["percentile"] if peers else 0,
        "po_classes": po_classes,
        "po_services": po_services,
        "po_default": po_default,
        "po_high": peers["high"] if peers else 0,
        "po_low": peers["low"] if peers else 0,
        "po_z": peers["z"] if peers else 3000,
        "po_min_delta": peers["minDelta"] if peers else 0,
        "po_min_peers": peers["minPeers"] if peers else 5,
        "po_min_samples": peers["minSamples"] if peers else 20,
        # K24: the class tables of the ls stream ([minDelta] per class), its rules (span in buckets,
        # q = percentile * 1000, r_u = up * 1000 or 0, r_d = down * 1000 or 0, z * 1000), minRecent and
        # minBaseline, likewise
        "ls_classes": ls_classes,
        "ls_services": ls_services,
        "ls_default": ls_default,
        "ls_short": [r[0] for r in shift["rules"]] if shift else [],
        "ls_pct": [r[1] for r in shift["rules"]] if shift else [],
        "ls_up": [r[2] for r in shift["rules"]] if shift else [],
        "ls_down": [r[3] for r in shift["rules"]] if shift else [],
        "ls_z": [r[4] for r in shift["rules"]] if shift else [],
        "ls_min_recent": shift["minRecent"] if shift else 20,
        "ls_min_baseline": shift["minBaseline"] if shift else 100,
        # K25: openAfter / closeAfter per source (sb, tf, po, ls; 0: not configured) and remindEvery, likewise
        "ic_open_after": ic_open,
        "ic_close_after": ic_close,
        "ic_remind_every": ic["remindEvery"] if ic else 0,
    }
    # intervalLengthInSeconds only scales the TPM divisor: the bucket label is endTs without its
    # last 4 digits whatever the interval (stream_calc_stats.js:89-96, :186), as here
    w, b = d["window"], d["buffer"]
    if not (w >= 1 and b >= 0 and d["interval_len"] >= 1):
        raise ValueError(f"stats window: windowSizeInIntervals >= 1, bufferSizeInIntervals >= 0, "
                         f"intervalLengthInSeconds >= 1 (got {w} / {b} / {d['interval_len']})")
    d.update(kw)
    return d


def service_overrides(cfg: Dict[str, Any]) -> Dict[str, Dict[str, Any]]:
    """Per-service override table: z-score THRESHOLD/INFLUENCE per LAG, alert hard max, suppression."""
    zc = cfg["streamCalcZScore"]
    ac = cfg["streamProcessAlerts"]
    lags = sorted(int(d["LAG"]) for d in zc["defaults"])
    out: Dict[str, Dict[str, Any]] = {}
    for svc, per_lag in ((zc.get("overrides") or {}).get("services") or {}).items():
        o = out.setdefault(svc, {"thr": [None] * len(lags), "infl": [None] * len(lags)})
        for lag_key, vals in per_lag.items():
            try:
                li = lags.index(int(float(lag_key)))
            except ValueError:
                continue
            if "THRESHOLD" in vals:
                o["thr"][li] = float(vals["THRESHOLD"])
            if "INFLUENCE" in vals:
                o["infl"][li] = float(vals["INFLUENCE"])
    for svc, vals in ((ac.get("overrides") or {}).get("services") or {}).items():
        o = out.setdefault(svc, {"thr": [None] * len(lags), "infl": [None] * len(lags)})
        hm = vals.get("hardMaxMsAlertThreshold")
        if hm:
            o["hard_max"] = float(hm)
    for svc in ac.get("suppressedServices", []) or []:
        o = out.setdefault(svc, {"thr": [None] * len(lags), "infl": [None] * len(lags)})
        o["suppressed"] = True
    return out


_last_gen = [0]


def _reload_generation(cfg: Dict[str, Any]) -> int:
    """Reload generation: the config file's mtime in ms (identical on every rank of a node, so
    the ranks agree on which reload they apply), else a local counter."""
    path = cfg.get("apmConfigFilePath")
    g = 0
    if path and os.path.exists(path):
        g = os.stat(path).st_mtime_ns // 1_000_000
    if g <= 0:
        g = _last_gen[0] + 1
    _last_gen[0] = max(_last_gen[0], g)
    return g


class APMEngine:
    def __init__(self, cfg: Dict[str, Any], device: int = 0, keep_text: bool = False, outputs=None,
                 tz: Optional[TzOffset] = None, tz_centre_ms: Optional[int] = None, **kw):
        self.cfg = cfg
        # K20: a span is at most windowSizeInIntervals when the engine is constructed (a later reload
        # may shorten the window: the span then reads the whole window)
        check_recent_windows(recent_windows(cfg), int(cfg["streamCalcStats"]["windowSizeInIntervals"]))
        check_slo_burn(slo_burn(cfg), int(cfg["streamCalcStats"]["windowSizeInIntervals"]))  # K21: likewise
        check_traffic_watch(traffic_watch(cfg), int(cfg["streamCalcStats"]["windowSizeInIntervals"]))  # K22: likewise
        check_peer_outliers(peer_outliers(cfg))  # K23 (no setting depends on the window)
        check_latency_shift(latency_shift(cfg), int(cfg["streamCalcStats"]["windowSizeInIntervals"]))  # K24: as K22
        check_incidents(incidents(cfg), cfg)  # K25: a source needs its own stream configured
        self.N = _native.load()
        # the engine's zone (tz, else gpu.timezone as read now) and the time its transition table is
        # centred on (the wall clock at construction).  Both are kept: the zone is not applied live,
        # and a reload neither searches the zone's transitions again nor moves the table
        self.tz = tz if tz is not None else TzOffset(cfg.get("gpu", {}).get("timezone", "local"))
        self.tz_centre_ms = int(time.time() * 1000) if tz_centre_ms is None else int(tz_centre_ms)
        self.ecfg = engine_config(cfg, device, keep_text, outputs, tz=self.tz, tz_centre_ms=self.tz_centre_ms, **kw)
        self.eng = self.N.Engine(self.ecfg)
        self.file_ids: Dict[str, int] = {}
        self.apply_overrides(cfg)

    def apply_overrides(self, cfg: Dict[str, Any]):
        self.eng.clear_overrides()
        for svc, o in service_overrides(cfg).items():
            self.eng.set_override(svc, o)

    # engine settings a reload applies live (reconfig.cpp); any other change needs a restart
    LIVE_KEYS = ("lags", "lag_suppressed", "alert_window", "alert_threshold", "hard_min_ms", "hard_min_tpm",
                 "hard_max_ms", "both_only", "cooldown_ms", "interval_len", "window", "buffer")

    @classmethod
    def restart_required(cls, old: Dict[str, Any], new: Dict[str, Any]) -> List[str]:
        """The engine settings that differ between two engine_config results and are not applied
        live (win_pcts, the slo_* tables, the tk_* settings, svc_pcts, rw_buckets, rw_pcts, the sb_*, tf_*, po_*, ls_* and ic_* settings, ...)."""
        return sorted(k for k in new if k not in cls.LIVE_KEYS and k not in ("outputs", "tz_table")
                      and new[k] != old.get(k))

    def reload(self, cfg: Dict[str, Any], gen: Optional[int] = None) -> List[str]:
        """Config hot reload (the reference's watchAPMConfig callbacks): z-score defaults and
        per-service overrides re-applied to every series, LAGs added (empty history) or removed
        (removeStaleLagData), every alert gate replaced -- staged now, applied by the engine at the
        next batch boundary (the same boundary on every lock-step rank).  Returns the engine
        settings that changed but need a restart (they are not applied)."""
        new = engine_config(cfg, self.ecfg["device"], outputs=(), tz=self.tz, tz_centre_ms=self.tz_centre_ms)
        restart = self.restart_required(self.ecfg, new)
        if restart:
            log.warning("config reload: %s changed but need a restart (not applied)", ", ".join(restart))
        if gen is None:
            gen = _reload_generation(cfg)
        self.eng.stage_reconfig(new, service_overrides(cfg), int(gen))
        for k in self.LIVE_KEYS:
            self.ecfg[k] = new[k]
        self.cfg = cfg
        return restart

    def add_file(self, path: str, kind: Optional[str] = None, server: Optional[str] = None) -> int:
        if path in self.file_ids:
            return self.file_ids[path]
        k = KIND_CODE[kind or file_kind(path)]
        fid = self.eng.add_file(path, k, server or server_of(path))
        self.file_ids[path] = fid
        return fid

    def process(self, chunks: Sequence[Tuple[Union[str, int], bytes]], now: Optional[float] = None):
        parts, table = [], []
        off = 0
        for f, data in chunks:
            if not data:
                continue
            if not data.endswith(b"\n"):
                data = data + b"\n"
            fid = f if isinstance(f, int) else self.add_file(f)
            parts.append(data)
            table.append((fid, off, off + len(data)))
            off += len(data)
        buf = b"".join(parts)
        self.eng.process_batch(buf, table, -1.0 if now is None else float(now))

    def process_lines(self, chunks: Sequence[Tuple[str, List[str]]], now: Optional[float] = None):
        self.process([(fp, ("\n".join(ls) + "\n").encode("utf-8")) for fp, ls in chunks if ls], now)

    def take(self, kind: str) -> List[str]:
        return self.eng.take(kind)

    def save_state(self, path: str, extra: bytes = b"") -> int:
        """Binary checkpoint of the whole pipeline (engine + join caches + pending output);
        ``extra`` is stored with it (one atomic file)."""
        return self.eng.save_state(path, extra)

    def checkpoint_async(self, prefix: str, extra: bytes = b"", force_base: bool = False) -> int:
        """Incremental asynchronous checkpoint (``<prefix>.ckpt`` chain manifest): returns its
        sequence number, or -1 if the previous one is still being written."""
        return self.eng.checkpoint_async(prefix, extra, force_base)

    def checkpoint_wait(self) -> int:
        return self.eng.checkpoint_wait()

    def checkpoint_info(self) -> dict:
        return self.eng.checkpoint_info()

    def load_state(self, path: str) -> bytes:
        """Resume from save_state() / checkpoint_async() output; this engine must be fresh (no
        files, no batches).  Returns the ``extra`` blob stored with the state."""
        extra = self.eng.load_state(path)
        self.file_ids = {p: i for i, (p, _k, _s) in enumerate(self.eng.files())}
        return extra

    def take_bytes(self, kind: str) -> bytes:
        return self.eng.take_bytes(kind)

    def dump_trace(self, path: str, pid: int = 0) -> int:
        """Write the recorded stage intervals (set_trace(True) first) as a Chrome trace."""
        import json
        ev = self.eng.take_trace()
        names = {0: "ingest (parse + join)", 1: "stats thread", 2: "device join phases", 3: "next-batch lane", 4: "output lane"}
        out = [{"name": "thread_name", "ph": "M", "pid": pid, "tid": t, "args": {"name": n}} for t, n in names.items()]
        for name, t0, t1, tid, batch in ev:
            out.append({"name": name, "ph": "X", "ts": t0 * 1000.0, "dur": max(0.0, (t1 - t0) * 1000.0), "pid": pid,
                        "tid": tid, "args": {"batch": batch}})
        with open(path, "w") as f:
            json.dump({"traceEvents": out, "displayTimeUnit": "ms"}, f)
        return len(ev)

    def set_server_context(self, jx_line: str, vm_load: float = 0.0) -> bool:
        """Feed a JMX ``jx`` record (pull_jvm_stats) into the per-JVM gauge table fused by K14."""
        from ..utils.records import entry_from_csv
        e = entry_from_csv(jx_line)
        if e is None or e.type != "jx":
            return False
        vals = [float("nan") if v is None else float(v) for v in e.values]
        return self.eng.set_server_context(e.server, float(e.timestamp), vals, float(vm_load))

    NODE_METRICS = ("ranks", "batches", "lines", "events", "bytes", "tx", "tx_db", "released", "rollovers",
                    "alert_candidates", "alerts", "series")

    def node_metrics(self) -> Dict[str, float]:
        """Node-wide sums of the per-rank counters as of the last interval edge (one RCCL
        all-reduce per interval on the collective stream); empty before the first edge or when
        no fleet exchange is configured."""
        return dict(zip(self.NODE_METRICS, self.eng.node_metrics()))

    def metrics(self) -> Dict[str, Any]:
        m = self.eng.metrics()
        m.update({"join": self.eng.join_counters(), "series": self.eng.n_series(),
                  "device_bytes": self.eng.device_bytes()})
        return m
