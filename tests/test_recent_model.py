"""The rw stream (exact stats of the newest window buckets, docs/RECENT.md) on the CPU: the config
key, the oracle's rows against an independent reference (tests/recent_ref.py), the record codec,
both COPY encoders, the service's route to the table and the reload report."""
import copy
import json
import os
import random

import pytest

from apmbackend_amd.models.cpu_engine import CpuOracleEngine
from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models.pipeline import (DEVICE_OUT_KINDS, STREAM_OUT_KINDS, APMEngine, engine_config, output_mask)
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import RecentWindowEntry, entry_from_csv

import recent_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

INT32_MAX = 2 ** 31 - 1
NAN = R.ELAPSED_NAN
QS = [1, 1000, 50000, 75000, 95000, 99900, 99999, 100000]
KEY = {"buckets": [1, 6], "percentiles": [50, 95, 99]}


# ------------------------------------------------------------------------------- config

def test_config_key_accepted_forms():
    assert config.parse_recent_windows(KEY) == {"buckets": [1, 6], "percentiles": [50000, 95000, 99000]}
    assert config.parse_recent_windows({"buckets": [3], "percentiles": ["0.001", 100]}) == \
        {"buckets": [3], "percentiles": [1, 100000]}
    assert config.parse_recent_windows({"buckets": [1, 2, 3, 4], "percentiles": [50]})["buckets"] == [1, 2, 3, 4]
    assert config.parse_recent_windows(None) is None
    C = config.parse_config_text('{"gpu": {"recentWindows": {"buckets": [1, 6], "percentiles": [50, 99.9]}}}')
    assert config.recent_windows(C) == {"buckets": [1, 6], "percentiles": [50000, 99900]}
    assert config.recent_windows({"gpu": {}}) is None and config.recent_windows({"gpu": {"recentWindows": None}}) is None
    assert config.gpu_opt({}, "recentQueue") == "recent_window"
    for key in ("recentWindows", "recentQueue"):
        assert key in config.GPU_OPTIONAL and key not in config.GPU_DEFAULTS
        assert key not in config.default_config()["gpu"]
    assert config.GPU_OPTIONAL["recentWindows"] is None


def test_default_config_text_is_unchanged():
    with open(config.DEFAULT_CONFIG_PATH, encoding="utf-8") as fh:
        txt = fh.read()
    assert "recentWindows" not in txt and "recentQueue" not in txt and "dbRecentTable" not in txt
    assert "recentWindows" not in config.read_apm_config(config.DEFAULT_CONFIG_PATH)["gpu"]


P_OK = [50, 95]
BAD = [{}, {"buckets": [1, 6]}, {"percentiles": P_OK}, {"buckets": [], "percentiles": P_OK},
       {"buckets": None, "percentiles": P_OK}, {"buckets": [0], "percentiles": P_OK},
       {"buckets": [-1], "percentiles": P_OK}, {"buckets": [6, 1], "percentiles": P_OK},
       {"buckets": [6, 6], "percentiles": P_OK}, {"buckets": [1, 2, 3, 4, 5], "percentiles": P_OK},
       {"buckets": [True], "percentiles": P_OK}, {"buckets": [6.0], "percentiles": P_OK},
       {"buckets": ["6"], "percentiles": P_OK}, {"buckets": 6, "percentiles": P_OK},
       {"buckets": "6", "percentiles": P_OK}, {"buckets": [1, None], "percentiles": P_OK},
       {"buckets": [1], "percentiles": []}, {"buckets": [1], "percentiles": None},
       {"buckets": [1], "percentiles": [0]}, {"buckets": [1], "percentiles": [100.001]},
       {"buckets": [1], "percentiles": [99, 50]}, {"buckets": [1], "percentiles": [1, 2, 3, 4, 5, 6, 7, 8, 9]},
       {"buckets": [1], "percentiles": [True]}, {"buckets": [1], "percentiles": "50"},
       {"buckets": [1], "percentiles": P_OK, "extra": 1}, {"spans": [1], "percentiles": P_OK},
       [1, 6], 6, "6", True, False, 0, []]


@pytest.mark.parametrize("bad", BAD)
def test_config_validation_raises(bad, tmp_path):
    with pytest.raises(ValueError):
        config.parse_recent_windows(bad)
    C = config.default_config(replay=True)
    C["gpu"]["recentWindows"] = bad
    with pytest.raises(ValueError):       # engine construction (the settings every engine is built from)
        engine_config(C, outputs=("st",))
    with pytest.raises(ValueError):
        CpuOracleEngine(C)
    p = tmp_path / "cfg.json"             # config load
    p.write_text(json.dumps({"gpu": {"recentWindows": bad}}))
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))


def test_spans_are_bounded_by_the_window_at_construction(tmp_path):
    C = config.default_config(replay=True)
    w = int(C["streamCalcStats"]["windowSizeInIntervals"])
    C["gpu"]["recentWindows"] = {"buckets": [1, w], "percentiles": [50]}
    assert engine_config(C, outputs=("st", "rw"))["rw_buckets"] == [1, w]
    assert CpuOracleEngine(C).take("rw") == [] and PipelineOracle(copy.deepcopy(C), UTC).st.recent_buckets == [1, w]
    C["gpu"]["recentWindows"]["buckets"] = [1, w + 1]
    assert config.recent_windows(C)["buckets"] == [1, w + 1]   # (the list itself is well-formed)
    # every engine refuses it when it is constructed, before anything else happens ...
    for make in (lambda: APMEngine(C, outputs=("st", "rw")), lambda: APMEngine(C, keep_text=True),
                 lambda: CpuOracleEngine(C), lambda: PipelineOracle(copy.deepcopy(C), UTC)):
        with pytest.raises(ValueError, match="windowSizeInIntervals"):
            make()
    C2, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C2["gpu"]["recentWindows"] = {"buckets": [1, int(C2["streamCalcStats"]["windowSizeInIntervals"]) + 1],
                                  "percentiles": [50]}
    with pytest.raises(ValueError, match="windowSizeInIntervals"):
        IngestService(C2, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
    # ... but the settings a reload reads do not: the window is applied live, and may get shorter
    assert engine_config(C, outputs=())["rw_buckets"] == [1, w + 1]
    C["streamCalcStats"]["windowSizeInIntervals"] = w + 1
    assert engine_config(C, outputs=("st", "rw"))["rw_buckets"] == [1, w + 1]
    assert CpuOracleEngine(C).take("rw") == []


def test_a_reload_that_shortens_the_window_clips_the_span():
    """windowSizeInIntervals 30 -> 3 between two batches (4 window buckets): the spans 6 and 9 then
    read the whole window -- their rows carry what the series' wp row carries -- and still print the
    configured k."""
    from apmbackend_amd.utils.synth import Generator, SynthConfig, batches, with_watermarks
    sc = SynthConfig(servers=2, duration_s=200, tx_per_sec_per_server=4, seed=9, ejb_services=6, provider_services=4)
    bl = with_watermarks(batches(Generator(sc).generate(), sc.start_ms, 5.0), UTC)
    C0 = config.default_config(replay=True)
    C0["gpu"].update({"timezone": "UTC", "windowPercentiles": [50, 95, 99],
                      "recentWindows": {"buckets": [1, 6, 9], "percentiles": [50, 95, 99]}})
    C1 = copy.deepcopy(C0)
    C1["streamCalcStats"]["windowSizeInIntervals"] = 3
    cut = len(bl) // 2
    P = PipelineOracle(copy.deepcopy(C0), UTC)
    P.run_batches(bl[:cut])
    n_before = len(P.rw)
    P.reload(copy.deepcopy(C1))
    P.run_batches(bl[cut:])
    after = [r.split("|") for r in P.rw[n_before:]]
    assert n_before > 30 and len(after) > 90 and {f[4] for f in after} == {"1", "6", "9"}
    wp = {tuple(f[1:4]): f for f in (r.split("|") for r in P.wp)}
    whole = 0
    for f in after[-60:]:                         # (the last rollovers: the window shrank before them)
        w = wp.get(tuple(f[1:4]))
        if f[4] != "1" and w is not None:
            assert [f[5], f[6], f[8]] == w[4:7], (f, w)
            whole += 1
    assert whole >= 20
    assert any(f[4] == "1" and f[5] != g[5] for f, g in zip(after[0::3], after[1::3]))   # span 1 stays shorter


def test_service_rejects_a_bad_key(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C["gpu"]["recentWindows"] = {"buckets": [6, 1], "percentiles": [50]}
    with pytest.raises(ValueError):
        IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)


def test_outputs_naming_rw_needs_the_key(tmp_path):
    assert STREAM_OUT_KINDS == DEVICE_OUT_KINDS + ("rw",) and DEVICE_OUT_KINDS[-1] == "sv"
    bit = STREAM_OUT_KINDS.index("rw")
    assert bit == 13 and output_mask(("rw",)) == 1 << 13 and output_mask(("sv", "st")) == (1 << 12) | (1 << 3)
    C = config.default_config(replay=True)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "rw"))
    C["gpu"]["recentWindows"] = copy.deepcopy(KEY)
    e = engine_config(C, outputs=("st", "rw"))
    assert e["rw_buckets"] == [1, 6] and e["rw_pcts"] == [50000, 95000, 99000] and (e["outputs"] >> bit) & 1
    assert not (engine_config(C, keep_text=True)["outputs"] >> bit) & 1   # keep_text alone leaves it off
    d = engine_config(config.default_config(replay=True))
    assert d["rw_buckets"] == [] and d["rw_pcts"] == []
    p = tmp_path / "cfg.json"
    p.write_text('{"gpu": {"recentWindows": {"buckets": [2], "percentiles": [50, 99.9]}, "recentQueue": "q"}}')
    assert config.recent_windows(config.read_apm_config(str(p))) == {"buckets": [2], "percentiles": [50000, 99900]}


def test_a_reload_that_changes_either_list_needs_a_restart():
    C = config.default_config(replay=True)
    C["gpu"]["recentWindows"] = copy.deepcopy(KEY)
    old = engine_config(C, outputs=("st", "rw"))
    assert APMEngine.restart_required(old, engine_config(copy.deepcopy(C), outputs=())) == []
    C2 = copy.deepcopy(C)
    C2["gpu"]["recentWindows"]["percentiles"] = [50, 99]
    assert APMEngine.restart_required(old, engine_config(C2, outputs=())) == ["rw_pcts"]
    C3 = copy.deepcopy(C)
    C3["gpu"]["recentWindows"]["buckets"] = [1, 3]
    assert APMEngine.restart_required(old, engine_config(C3, outputs=())) == ["rw_buckets"]
    C4 = copy.deepcopy(C)
    del C4["gpu"]["recentWindows"]
    assert APMEngine.restart_required(old, engine_config(C4, outputs=())) == ["rw_buckets", "rw_pcts"]
    assert "rw_buckets" not in APMEngine.LIVE_KEYS and "rw_pcts" not in APMEngine.LIVE_KEYS


# ------------------------------------------------------------------------------- oracle

def tx(server, service, end, elapsed):
    return f"tx|{server}|{service}|id|1|{end - 5}|{end}|{elapsed}|Y"


def test_stats_oracle_rows_literal():
    rw, st = [], []
    so = StatsOracle(st.append, lambda _l: None, 10, 3, 1, emit_recent=rw.append, recent_buckets=[1, 2, 9],
                     recent_percentiles=[1000, 50000, 99900])
    B = 1000
    so.latest = B
    t = lambda b, ms=1: b * 10000 + ms
    # the rollover to B + 2 reads the window [B - 2, B + 1]: newest entry B + 1, then B, ...
    for ln in (tx("a", "x", t(B + 1), -1), tx("a", "x", t(B), 0), tx("a", "x", t(B - 2), 9),
               tx("a", "nan", t(B + 1), "abc"), tx("a", "nan", t(B), 7),
               tx("a", "quiet", t(B - 1), 5), tx("a", "quiet", t(B - 2), INT32_MAX),
               tx("a", "old", t(B - 9), 5)):                              # outside the window: st row, no rw row
        so.consume(ln)
    assert rw == []
    so.consume(tx("d", "t", t(B + 2), 5))
    ts = (B + 2 - 1 - 1) * 10000
    assert rw == [f"rw|{ts}|a|x|1|1|0|-1|1:-1,50:-1,99.9:-1",
                  f"rw|{ts}|a|x|2|2|0|-1|1:-0.5,50:-1,99.9:0",
                  f"rw|{ts}|a|x|9|3|0|8|1:-0.5,50:4.5,99.9:9",              # 9 > 4 buckets: the whole window
                  f"rw|{ts}|a|nan|1|0|1|0|",                              # all NaN: empty pairs
                  f"rw|{ts}|a|nan|2|1|1|7|1:7,50:7,99.9:7",
                  f"rw|{ts}|a|nan|9|1|1|7|1:7,50:7,99.9:7",
                  f"rw|{ts}|a|quiet|1|0|0|0|",                            # went quiet
                  f"rw|{ts}|a|quiet|2|0|0|0|",
                  f"rw|{ts}|a|quiet|9|2|0|2147483652|1:1073741826,50:5,99.9:2147483647"]
    assert [l.split("|")[3] for l in st] == ["x", "nan", "quiet", "old"]
    off = StatsOracle(lambda _l: None, lambda _l: None, 10, 3, 2)
    assert off.emit_recent is None and off.recent_buckets == [] and off.recent_percentiles == []


def test_oracle_rows_against_the_independent_reference():
    rng = random.Random(20)
    rw, st = [], []
    window, buffer = 7, 2
    spans = [1, 3, 8, 11]      # 8 = the window's buckets, 11 beyond it
    so = StatsOracle(st.append, lambda _l: None, 10, window, buffer, emit_recent=rw.append, recent_buckets=spans,
                     recent_percentiles=QS)
    B = 3000
    so.latest = B
    labels = list(range(B + 1 - window - buffer, B + 1 - buffer + 1))   # the window of the rollover to B + 1
    assert len(labels) == window + 1
    want = []
    ts = (B + 1 - buffer - 1) * 10000
    kinds = 0
    for i in range(120):
        server, service = f"s{i % 3}", f"S:{i}"
        entries = []
        for j, b in enumerate(labels):
            mode = rng.randrange(5)
            n = 0 if mode == 0 or (i % 4 == 1 and j >= len(labels) - 3) else rng.choice([1, 2, 3, 9, 40])
            vals = [rng.choice([rng.randint(-50, 10 ** 6), INT32_MAX, -INT32_MAX, 0, NAN]) for _ in range(n)]
            if i % 7 == 3 and j == len(labels) - 1 and vals:
                vals = [NAN] * len(vals)          # a newest bucket that is all NaN
            entries.append(vals)
        if i % 10 == 9:
            entries = [[] for _ in labels]         # nothing in the window (a tx outside keeps the st row)
        for b, vals in zip(labels, entries):
            for v in vals:
                so.consume(tx(server, service, b * 10000 + 1, "abc" if v == NAN else v))
        so.consume(tx(server, service, (labels[0] - 1) * 10000 + 1, 123456))   # older than the window
        so.consume(tx(server, service, (labels[-1] + 1) * 10000 + 1, 654321))  # newer than the window
        got = R.rows(ts, server, service, entries, spans, QS)
        kinds |= (1 if any(r.split("|")[5] == "0" for r in got) and got else 0) | (2 if not got else 0)
        want.append(((server, service), got))
    so.consume(tx("t", "T", (B + 1) * 10000 + 1, 1))
    assert kinds == 3
    # st order: server by server, services in first-seen order
    order = [(l.split("|")[2], l.split("|")[3]) for l in st]
    by = dict(want)
    flat = [r for key in order for r in by.get(key, [])]
    assert rw == flat and len(rw) > 300
    assert any("|8|" in r for r in rw) and any(r.split("|")[8] == "" and r.split("|")[6] != "0" for r in rw)
    # a span equal to the window and one beyond it read the same samples
    for r8, r11 in zip([r for r in rw if r.split("|")[4] == "8"], [r for r in rw if r.split("|")[4] == "11"]):
        assert r8.split("|")[5:] == r11.split("|")[5:]


def test_pipeline_oracle_and_cpu_engine_carry_the_stream():
    C = config.default_config(replay=True)
    assert PipelineOracle(copy.deepcopy(C), UTC).st.emit_recent is None
    C["gpu"]["recentWindows"] = copy.deepcopy(KEY)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    assert P.st.emit_recent is not None and P.st.recent_buckets == [1, 6] and P.rw == []
    assert P.st.recent_percentiles == [50000, 95000, 99000]
    assert CpuOracleEngine(C).take("rw") == []


# ------------------------------------------------------------------------------- codec, encoders

RW_LINES = ["rw|1578391200000|jvm00|S:getSvc0001|6|7|1|2040|50:12,99.9:340.5",
            "rw|1578391210000|j\tx|S:a\tb\\c|1|2|0|-1|0.001:-0.5,50:-1,100:0",
            "rw|1578391220000|jvm01|S:max|31|3|2|6442450941|50:2147483647,75:2147483646.5,99.999:-2147483647",
            "rw|1578391230000|jvm01|S:quiet|1|0|0|0|",
            "rw|1578391230000|jvm01|S:allnan|6|0|4|0|",
            "rw|1578391240000|jvm02|S:wide|31|300000000|0|644245094100000000|50:2147483647"]


def test_codec_round_trip_and_pg_row():
    for ln in RW_LINES:
        e = entry_from_csv(ln)
        assert isinstance(e, RecentWindowEntry) and e.type == "rw" and e.to_csv() == ln
    e = entry_from_csv(RW_LINES[0])
    assert (e.server, e.service, e.buckets, e.count, e.nan, e.elapsed_sum, e.pcts) == \
        ("jvm00", "S:getSvc0001", 6, 7, 1, 2040, [(50000, 24), (99900, 681)])
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["rw"][1]
    assert row["pcts"] == {"50": 12, "99.9": 340.5} and row["elapsed_sum"] == 2040 and row["buckets"] == 6
    assert entry_from_csv(RW_LINES[3]).to_pg_row()["pcts"] == {}
    assert "rw" in records.RECORD_TYPES and "rw" in sinks.TYPES and sinks.COLUMNS["rw"][0] == "dbRecentTable"
    assert sinks.DEFAULT_TABLES["rw"] == "apm_recent_window"
    for bad in ("rw|12|s|v|x|1|0|5|50:5", "rw|12|s|v|1|-1|0|5|50:5", "rw|12|s|v|1|1||5|50:5",
                "rw|12|s|v|1|1|0|5.5|50:5", "rw|12|s|v|1|1|0|--5|50:5", "rw|12|s|v|1|1|0|1234567890123456789|50:5",
                "rw|12|s|v|1|1|0", "rw|12|s|v|1 |1|0|5|50:5", "rw|12|s|v|12345678901|1|0|5|50:5"):
        assert entry_from_csv(bad) is None, bad


def test_copy_encode_lines_rw():
    got = sinks.copy_encode_lines(RW_LINES)["rw"]
    assert got[0] == '2020-01-07 10:00:00.000+00\tjvm00\tS:getSvc0001\t6\t7\t1\t2040\t{"50":12,"99.9":340.5}\n'
    assert got[1] == '2020-01-07 10:00:10.000+00\tj\\tx\tS:a\\tb\\\\c\t1\t2\t0\t-1\t{"0.001":-0.5,"50":-1,"100":0}\n'
    assert got[2].endswith('\t31\t3\t2\t6442450941\t{"50":2147483647,"75":2147483646.5,"99.999":-2147483647}\n')
    assert got[3].endswith('\tS:quiet\t1\t0\t0\t0\t{}\n')                  # m == 0: an empty object
    assert got[4].endswith('\tS:allnan\t6\t0\t4\t0\t{}\n')
    assert got[5].endswith('\t31\t300000000\t0\t644245094100000000\t{"50":2147483647}\n')   # past 2^53: digits
    assert 644245094100000000 > 2 ** 53
    for ln, row in zip(RW_LINES, got):
        assert sinks.pg_row_from_copy("rw", row) == entry_from_csv(ln).to_pg_row()


def test_native_copy_encoder_matches_python_for_rw():
    lines = RW_LINES + ["rw|12|a|b|6|4|1|9|50:4,bad,75:,99.9:2.5,101:1,50.0001:1,90:1.25,095:-0,7.50:3,:5,0:1",
                        "rw|12|a|b|x|4|1|9|50:4",      # malformed rows: dropped
                        "rw|12|a|b|6|4|1|9.5|50:4",
                        "rw|12|a|b|6|4|1",
                        "rw|12|a|b|6|4|1|1234567890123456789|50:4",
                        "rw|13|a|c|1|2|0|-1|50:-0.5"]
    nat = sinks.copy_encode_native(lines)
    assert nat is not None, "the native extension does not import: build it (a broken build must not pass as a skip)"
    want = sinks.copy_encode_lines(lines)
    assert len(want["rw"]) == 8
    assert nat["rw"][1] == 8 and nat["rw"][0].decode("utf-8") == "".join(want["rw"])
    assert want["rw"][6].endswith('\ta\tb\t6\t4\t1\t9\t{"50":4,"99.9":2.5,"95":0,"7.5":3}\n')
    assert want["rw"][7].endswith('\ta\tc\t1\t2\t0\t-1\t{"50":-0.5}\n')


# ------------------------------------------------------------------------------- service

def run_service(tmp_path, key):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    if key:
        C["gpu"]["recentWindows"] = key
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    assert ("rw" in svc.outputs) == bool(key)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_service_spools_the_recent_window_table(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    P, on = run_service(tmp_path / "on", {"buckets": [1, 6], "percentiles": [50, 95, 99]})
    P0, off = run_service(tmp_path / "off", None)
    assert len(P.rw) > 20 and P0.rw == []
    assert {r.split("|")[4] for r in P.rw} == {"1", "6"}
    assert on["apm_recent_window.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.rw)["rw"])
    assert [c.strip() for c in on["apm_recent_window.columns"].decode().strip().split(",")] == sinks.COLUMNS["rw"][1]
    assert not any(f.startswith("apm_recent_window") for f in off)
    assert {f: b for f, b in on.items() if not f.startswith("apm_recent_window")} == off and len(off) >= 4
