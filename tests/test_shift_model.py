"""K24 ls rows on the CPU: the config key, the class tables, the oracle against an independent
reference (tests/shift_ref.py), the record codec, both COPY encoders, the exact verdict routine
against Python integers, and the service's routing."""
import copy
import os
import random

import pytest

from apmbackend_amd.models.cpu_engine import CpuOracleEngine
from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models.pipeline import COMPLETE_OUT_KINDS, WHOLE_OUT_KINDS, APMEngine, engine_config, output_mask
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import LatencyShiftEntry, entry_from_csv

import shift_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

KEY = {"default": {"minDelta": 50},
       "services": {"S:nightlyBatch": None, "S:checkout": {"minDelta": 20}},
       "rules": [{"short": 6, "percentile": 95, "up": 3, "z": 4},
                 {"short": 6, "percentile": 25, "down": 2}],
       "minRecent": 20, "minBaseline": 100}


# ------------------------------------------------------------------------------- config

def test_config_key_accepted_forms():
    ls = config.parse_latency_shift(copy.deepcopy(KEY))
    assert ls == {"default": 50, "services": {"S:nightlyBatch": None, "S:checkout": 20},
                  "rules": [(6, 95000, 3000, 0, 4000), (6, 25000, 0, 2000, 3000)], "minRecent": 20, "minBaseline": 100}
    assert config.parse_latency_shift(None) is None
    # off: no service has a minDelta
    assert config.parse_latency_shift({"rules": KEY["rules"]}) is None
    assert config.parse_latency_shift({"default": None, "services": {"a": None}, "rules": KEY["rules"]}) is None
    # defaults, decimals from text, the extremes of every range
    ls = config.parse_latency_shift({"services": {"a": {"minDelta": 1073741823}},
                                     "rules": [{"short": 1, "percentile": "0.001", "up": "1.001"},
                                               {"short": 1, "percentile": 99.999, "down": 1000, "up": 1000, "z": 0},
                                               {"short": 64, "percentile": 0.001, "down": 1.5, "z": "100"}]})
    assert ls["default"] is None and ls["minRecent"] == 20 and ls["minBaseline"] == 100
    assert ls["rules"] == [(1, 1, 1001, 0, 3000), (1, 99999, 1000000, 1000000, 0), (64, 1, 0, 1500, 100000)]
    assert config.parse_latency_shift(dict(KEY, minRecent=1, minBaseline=2))["minBaseline"] == 2
    C = config.default_config(replay=True)
    assert config.latency_shift(C) is None
    assert config.gpu_opt(C, "shiftQueue") == "latency_shift"
    assert "latencyShift" not in C["gpu"] and "latencyShift" in config.GPU_OPTIONAL


def test_default_config_text_is_unchanged():
    import json
    txt = json.dumps(config.default_config(replay=True))
    assert "latencyShift" not in txt and "shiftQueue" not in txt and "dbShiftTable" not in txt


O = {"minDelta": 50}
RU = [{"short": 1, "percentile": 95, "up": 3}]


def rule(**kw):
    return {"default": O, "rules": [kw]}


BAD = [[], "x", 5, {"rules": RU, "extra": 1, "default": O}, {"default": O}, {"default": O, "rules": []},
       {"default": O, "rules": None}, {"default": O, "rules": RU * 5}, {"default": O, "rules": {"short": 1}},
       {"default": O, "rules": ["x"]}, {"default": 50, "rules": RU}, {"default": {}, "rules": RU},
       {"default": {"minDelta": True}, "rules": RU}, {"default": {"minDelta": 50.0}, "rules": RU},
       {"default": {"minDelta": "50"}, "rules": RU}, {"default": {"minDelta": 0}, "rules": RU},
       {"default": {"minDelta": 1073741824}, "rules": RU}, {"default": {"minDelta": 5, "x": 1}, "rules": RU},
       {"default": O, "services": [], "rules": RU}, {"default": O, "services": {"a": 5}, "rules": RU},
       {"default": O, "services": {"a": {"minDelta": -1}}, "rules": RU}, {"default": O, "services": {1: O}, "rules": RU},
       rule(short=0, percentile=95, up=3), rule(short=65, percentile=95, up=3), rule(short=True, percentile=95, up=3),
       rule(short=1.0, percentile=95, up=3), rule(short="1", percentile=95, up=3), rule(percentile=95, up=3),
       rule(short=1, up=3), rule(short=1, percentile=95), rule(short=1, percentile=100, up=3),
       rule(short=1, percentile=0, up=3), rule(short=1, percentile=95.0001, up=3), rule(short=1, percentile=True, up=3),
       rule(short=1, percentile=[95], up=3), rule(short=1, percentile="x", up=3), rule(short=1, percentile=95, up=1),
       rule(short=1, percentile=95, up=1000.001), rule(short=1, percentile=95, up=1.0001), rule(short=1, percentile=95, up=True),
       rule(short=1, percentile=95, down=1), rule(short=1, percentile=95, down=0.5), rule(short=1, percentile=95, down="x"),
       rule(short=1, percentile=95, up=3, z=-1), rule(short=1, percentile=95, up=3, z=100.001),
       rule(short=1, percentile=95, up=3, z=None), rule(short=1, percentile=95, up=3, extra=1),
       {"default": O, "rules": [{"short": 6, "percentile": 95, "up": 3}, {"short": 1, "percentile": 95, "up": 3}]},
       {"default": O, "rules": [{"short": 6, "percentile": 95, "up": 3}, {"short": 6, "percentile": 95, "down": 3}]},
       {"default": O, "rules": [{"short": 6, "percentile": 25, "up": 3}, {"short": 6, "percentile": 95, "down": 3},
                                {"short": 6, "percentile": 25, "down": 3}]},
       {"default": O, "rules": RU, "minRecent": 0}, {"default": O, "rules": RU, "minRecent": 2.0},
       {"default": O, "rules": RU, "minRecent": True}, {"default": O, "rules": RU, "minBaseline": 1},
       {"default": O, "rules": RU, "minBaseline": "100"}]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_config_key_rejections(i):
    with pytest.raises(ValueError):
        config.parse_latency_shift(BAD[i])


def test_read_apm_config_stops_on_a_bad_key(tmp_path):
    p = tmp_path / "cfg.json"
    p.write_text('{"gpu": {"latencyShift": {"default": {"minDelta": 5}, "rules": [{"short": 0, "percentile": 95, "up": 2}]}}}')
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    p.write_text('{"gpu": {"latencyShift": {"default": {"minDelta": 9}, "rules": [{"short": 2, "percentile": 50, "up": 2.5}]}, '
                 '"shiftQueue": "q"}}')
    C = config.read_apm_config(str(p))
    assert config.latency_shift(C)["default"] == 9 and config.gpu_opt(C, "shiftQueue") == "q"


def test_span_bound_is_the_engines_not_the_parsers():
    key = {"default": O, "rules": [{"short": 1, "percentile": 95, "up": 2}, {"short": 31, "percentile": 95, "up": 2}]}
    ls = config.parse_latency_shift(key)
    config.check_latency_shift(ls, 31)
    config.check_latency_shift(None, 3)
    with pytest.raises(ValueError):
        config.check_latency_shift(ls, 30)
    C = config.default_config(replay=True)
    C["gpu"]["latencyShift"] = key
    assert int(C["streamCalcStats"]["windowSizeInIntervals"]) == 30
    assert engine_config(C, outputs=("st", "ls"))["ls_short"] == [1, 31]   # (a reload reads it through here)
    with pytest.raises(ValueError):
        PipelineOracle(copy.deepcopy(C), UTC)
    with pytest.raises(ValueError):
        CpuOracleEngine(copy.deepcopy(C))
    C["streamCalcStats"]["windowSizeInIntervals"] = 31
    PipelineOracle(copy.deepcopy(C), UTC)


def test_class_table():
    classes, services, default = config.shift_tables(config.parse_latency_shift(KEY))
    assert classes == [[], [50], [20]]
    assert services == {"S:nightlyBatch": 0, "S:checkout": 2} and default == 1
    nodef = dict(KEY, default=None)
    classes, services, default = config.shift_tables(config.parse_latency_shift(nodef))
    assert classes == [[], [20]] and services == {"S:nightlyBatch": 0, "S:checkout": 1} and default == 0
    assert config.shift_tables(None) == ([], {}, 0)
    # the other streams' tables are untouched by the key
    C = config.default_config(replay=True)
    C["gpu"]["latencyShift"] = copy.deepcopy(KEY)
    e = engine_config(C, outputs=("st", "ls"))
    assert e["slo_classes"] == [] and e["sb_classes"] == [] and e["tf_classes"] == [] and e["po_classes"] == []
    assert e["ls_classes"] == [[], [50], [20]] and e["ls_services"] == {"S:nightlyBatch": 0, "S:checkout": 2}
    assert e["ls_default"] == 1 and e["ls_short"] == [6, 6] and e["ls_pct"] == [95000, 25000]
    assert e["ls_up"] == [3000, 0] and e["ls_down"] == [0, 2000] and e["ls_z"] == [4000, 3000]
    assert e["ls_min_recent"] == 20 and e["ls_min_baseline"] == 100


def test_outputs_naming_ls_needs_the_key():
    assert COMPLETE_OUT_KINDS == WHOLE_OUT_KINDS + ("ls",) and WHOLE_OUT_KINDS[-1] == "po"
    bit = COMPLETE_OUT_KINDS.index("ls")
    assert bit == 17 and output_mask(("ls",)) == 1 << 17 and output_mask(("po", "st")) == (1 << 16) | (1 << 3)
    C = config.default_config(replay=True)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "ls"))
    C["gpu"]["latencyShift"] = copy.deepcopy(KEY)
    assert (engine_config(C, outputs=("st", "ls"))["outputs"] >> bit) & 1
    assert not (engine_config(C, keep_text=True)["outputs"] >> bit) & 1   # keep_text alone leaves it off
    d = engine_config(config.default_config(replay=True))
    assert d["ls_classes"] == [] and d["ls_short"] == [] and d["ls_pct"] == [] and d["ls_min_baseline"] == 100


def test_a_reload_that_changes_the_key_needs_a_restart():
    C = config.default_config(replay=True)
    C["gpu"]["latencyShift"] = copy.deepcopy(KEY)
    old = engine_config(C, outputs=("st", "ls"))
    assert APMEngine.restart_required(old, engine_config(copy.deepcopy(C), outputs=())) == []
    C2 = copy.deepcopy(C)
    C2["gpu"]["latencyShift"]["rules"][0]["up"] = 2
    assert APMEngine.restart_required(old, engine_config(C2, outputs=())) == ["ls_up"]
    C3 = copy.deepcopy(C)
    C3["gpu"]["latencyShift"]["rules"] = [{"short": 2, "percentile": 50, "down": 3, "z": 1}]
    assert APMEngine.restart_required(old, engine_config(C3, outputs=())) == ["ls_down", "ls_pct", "ls_short", "ls_up", "ls_z"]
    C4 = copy.deepcopy(C)
    C4["gpu"]["latencyShift"]["minBaseline"] = 50
    C4["gpu"]["latencyShift"]["minRecent"] = 5
    C4["gpu"]["latencyShift"]["services"]["S:checkout"]["minDelta"] = 40
    assert APMEngine.restart_required(old, engine_config(C4, outputs=())) == ["ls_classes", "ls_min_baseline", "ls_min_recent"]
    C5 = copy.deepcopy(C)
    del C5["gpu"]["latencyShift"]
    assert APMEngine.restart_required(old, engine_config(C5, outputs=())) == \
        ["ls_classes", "ls_default", "ls_down", "ls_pct", "ls_services", "ls_short", "ls_up", "ls_z"]
    assert not {k for k in old if k.startswith("ls_")} & set(APMEngine.LIVE_KEYS)


# ------------------------------------------------------------------------------- oracle

def tx(server, service, end, elapsed):
    return f"tx|{server}|{service}|id|1|{end - 5}|{end}|{elapsed}|Y"


def test_stats_oracle_rows_literal():
    ls, st = [], []
    key = config.parse_latency_shift({"default": {"minDelta": 10}, "services": {"off": None, "strict": {"minDelta": 500}},
                                      "rules": [{"short": 1, "percentile": 50, "up": 1.5, "down": 1.5, "z": 0}],
                                      "minRecent": 4, "minBaseline": 6})
    so = StatsOracle(st.append, lambda _l: None, 10, 3, 1, emit_shift=ls.append, shift=key)
    B = 1000
    so.latest = B + 1
    t = lambda b, ms=1: b * 10000 + ms
    # the rollover to B + 2 reads the window [B - 2, B + 1]: three baseline buckets, newest entry B + 1

    def feed(service, base, recent):
        for b in (B - 2, B - 1, B):
            for v in base:
                so.consume(tx("a", service, t(b), v))
        for v in recent:
            so.consume(tx("a", service, t(B + 1), v))

    feed("slower", [100, 110], [200, 210, 220, "abc", 230])   # p50 of six samples is rank 2 alone: T2 = 2 * 100, X2 = 2 * 210, a = 4 of 4
    feed("faster", [100, 110], [10, 20, 30, 40])              # b = 4
    feed("same", [100, 110], [100, 110, 100, 110])            # a = 2 of 4 = the share 50 % predicts: below up 1.5
    feed("tied", [100, 100], [100, 100, 100, 100])            # every sample equals the percentile: a = b = 0
    feed("few_recent", [100, 110], [200, 210, 220])           # mR 3 < 4
    feed("few_base", [100], [200, 210, 220, 230])             # mB 3 < 6
    feed("small_delta", [100, 110], [105, 106, 107, 108])     # X2 - T2 = 12 < 20
    feed("at_delta", [100, 110], [109, 110, 111, 112])        # X2 - T2 = 20
    feed("off", [100, 110], [200, 210, 220, 230])
    feed("strict", [100, 110], [200, 210, 220, 230])          # minDelta 500
    assert ls == []
    so.consume(tx("d", "t", t(B + 2), 5))
    ts = (B + 2 - 1 - 1) * 10000
    assert ls == [f"ls|{ts}|a|slower|11|10|1:50:6:200:4:420:4:0:U",
                  f"ls|{ts}|a|faster|10|10|1:50:6:200:4:40:0:4:D",
                  f"ls|{ts}|a|at_delta|10|10|1:50:6:200:4:220:4:0:U"]
    assert [l.split("|")[3] for l in st][:3] == ["slower", "faster", "same"]
    off = StatsOracle(lambda _l: None, lambda _l: None, 10, 3, 2)
    assert off.emit_shift is None and off.shift is None


def test_oracle_rows_against_the_independent_reference():
    rng = random.Random(24)
    ls, st = [], []
    window, buffer = 11, 2
    rules = [(1, 95000, 3000, 0, 4000), (3, 50000, 1500, 1500, 1000), (3, 90000, 2000, 0, 0), (12, 25000, 0, 2000, 3000)]
    deltas = {"S:named": 5, "S:none": None}
    key = {"default": 20, "services": deltas, "rules": rules, "minRecent": 5, "minBaseline": 30}
    so = StatsOracle(st.append, lambda _l: None, 10, window, buffer, emit_shift=ls.append, shift=key)
    B = 3000
    so.latest = B
    labels = list(range(B + 1 - window - buffer, B + 1 - buffer + 1))   # the window of the rollover to B + 1
    assert len(labels) == 12
    ts = (B + 1 - buffer - 1) * 10000
    want, verdicts = {}, set()
    for i in range(160):
        server = f"s{i % 3}"
        service = "S:named" if i % 11 == 0 else "S:none" if i % 13 == 0 else f"S:{i}"
        if (server, service) in want:
            service += f"_{i}"
        delta = deltas.get(service, 20)
        level = rng.choice([-40, 5, 100, 1000, 2 ** 31 - 400])
        spread = rng.choice([0, 3, 50, 300])
        per = rng.choice([0, 2, 8, 15])
        tail = rng.choice([1, 3, 5])
        how = rng.choice(["same", "slow", "fast", "few"])
        entries = []
        for j in range(len(labels)):
            n = per if rng.random() > 0.1 else 0
            e = [level + rng.randint(0, spread) for _ in range(n)]
            if j >= len(labels) - tail:
                e = {"same": e, "slow": [v + rng.randint(0, 4 * spread + 60) for v in e],
                     "fast": [v - rng.randint(0, 4 * spread + 60) for v in e], "few": e[:1]}[how]
            if rng.random() < 0.15:
                e.insert(rng.randint(0, len(e)), "abc")
            entries.append(e)
        for b, e in zip(labels, entries):
            for v in e:
                so.consume(tx(server, service, b * 10000 + 1, v))
        so.consume(tx(server, service, (labels[0] - 1) * 10000 + 1, 1))    # older than the window: not read
        so.consume(tx(server, service, (labels[-1] + 1) * 10000 + 1, 1))   # newer than the window
        ref = [[R.ELAPSED_NAN if v == "abc" else v for v in e] for e in entries]
        want[(server, service)] = None if delta is None else R.row(ts, server, service, ref, rules, delta, 5, 30)
        if delta is not None:
            verdicts |= {p[8] for p in R.series_ints(ref, rules, delta, 5, 30)[1]}
    so.consume(tx("t", "T", (B + 1) * 10000 + 1, 1))
    order = [(l.split("|")[2], l.split("|")[3]) for l in st]
    flat = [want[k] for k in order if want.get(k) is not None]
    assert ls == flat and 10 < len(ls) < 150
    assert verdicts == {"U", "D", "N"}
    assert not any(r.split("|")[3] == "S:none" for r in ls)
    # a span equal to the window has no baseline: mB = 0, T2 = 0, a = b = 0, never judged
    for r in ls:
        g = r.split("|")[6].split(",")[3].split(":")
        assert g[:4] == ["12", "25", "0", "0"] and g[6:] == ["0", "0", "N"]


def test_pipeline_oracle_and_cpu_engine_carry_the_stream():
    C = config.default_config(replay=True)
    assert PipelineOracle(copy.deepcopy(C), UTC).st.emit_shift is None
    C["gpu"]["latencyShift"] = copy.deepcopy(KEY)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    assert P.st.emit_shift is not None and P.st.shift["rules"] == [(6, 95000, 3000, 0, 4000), (6, 25000, 0, 2000, 3000)]
    assert P.ls == [] and CpuOracleEngine(C).take("ls") == []


# ------------------------------------------------------------------------------- codec, encoders

LS_LINES = ["ls|1578391200000|jvm00|S:checkout|310|20|6:95:250:900:60:2400:31:20:U,6:25:250:300:60:310:40:12:N",
            "ls|1578391210000|j\tx|S:a\tb\\c|0|1|64:0.001:0:0:0:0:0:0:N",
            "ls|1578391220000|jvm01|S:max|2147483647|1073741823|"
            "1:99.999:2147483647:4294967294:2147483647:-4294967294:2147483647:0:D,2:50:1:-1:0:0:0:0:N,"
            "3:12.5:2:1:1:1:1:1:U,64:5:6:7:8:9:1:2:N"]

MALFORMED = ["ls|12|s|v|x|5|1:50:3:4:5:6:1:2:U", "ls|12|s|v|5|-1|1:50:3:4:5:6:1:2:U", "ls|12|s|v||5|1:50:3:4:5:6:1:2:U",
             "ls|12|s|v|5|1.5|1:50:3:4:5:6:1:2:U", "ls|12|s|v|12345678901|5|1:50:3:4:5:6:1:2:U",
             "ls|12|s|v|5|5", "ls|12|s|v|5|5|", "ls|12|s|v|5|5|1:50:3:4:5:6:1:2", "ls|12|s|v|5|5|1:50:3:4:5:6:1:U",
             "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:X", "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:u", "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:U:1",
             "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:U,", "ls|12|s|v|5|5|,1:50:3:4:5:6:1:2:U", "ls|12|s|v|5|5|1:50:x:4:5:6:1:2:U",
             "ls|12|s|v|5|5|1:50::4:5:6:1:2:U", "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:",
             "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:U,2:50:3:4:5:6:1:2:N,3:50:3:4:5:6:1:2:N,4:50:3:4:5:6:1:2:N,5:50:3:4:5:6:1:2:N",
             "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:UD", "ls|12|s|v|5 |5|1:50:3:4:5:6:1:2:U", "ls|12|s|v|5|5|1:50:-3:4:5:6:1:2:U",
             "ls|12|s|v|5|5|1:50:3:4:5:6:-1:2:U", "ls|12|s|v|5|5|1:50:3:12345678901:5:6:1:2:U",
             "ls|12|s|v|5|5|1:100:3:4:5:6:1:2:U", "ls|12|s|v|5|5|1:0:3:4:5:6:1:2:U", "ls|12|s|v|5|5|1:5.1234:3:4:5:6:1:2:U",
             "ls|12|s|v|5|5|1:50:3:--4:5:6:1:2:U", "ls|12|s|v|5|5|1:50:3:4:5:6:1:2:U|x"]


def test_codec_round_trip_and_pg_row():
    for ln in LS_LINES:
        e = entry_from_csv(ln)
        assert isinstance(e, LatencyShiftEntry) and e.type == "ls" and e.to_csv() == ln
    e = entry_from_csv(LS_LINES[0])
    assert (e.server, e.service, e.count, e.min_delta) == ("jvm00", "S:checkout", 310, 20)
    assert e.rules == [(6, 95000, 250, 900, 60, 2400, 31, 20, "U"), (6, 25000, 250, 300, 60, 310, 40, 12, "N")]
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["ls"][1] == ["timestamp", "server", "service", "count", "min_delta", "rules"]
    assert row["rules"][0] == {"k": 6, "p": "95", "base": 250, "t2": 900, "recent": 60, "x2": 2400, "above": 31,
                               "below": 20, "verdict": "U"}
    assert "ls" in records.RECORD_TYPES and "ls" in sinks.TYPES and sinks.COLUMNS["ls"][0] == "dbShiftTable"
    assert sinks.DEFAULT_TABLES["ls"] == "apm_latency_shift"
    for bad in MALFORMED:
        assert entry_from_csv(bad) is None, bad


def test_copy_encode_lines_ls():
    got = sinks.copy_encode_lines(LS_LINES)["ls"]
    assert got[0] == ('2020-01-07 10:00:00.000+00\tjvm00\tS:checkout\t310\t20\t'
                      '[{"k":6,"p":"95","base":250,"t2":900,"recent":60,"x2":2400,"above":31,"below":20,"verdict":"U"},'
                      '{"k":6,"p":"25","base":250,"t2":300,"recent":60,"x2":310,"above":40,"below":12,"verdict":"N"}]\n')
    assert got[1] == ('2020-01-07 10:00:10.000+00\tj\\tx\tS:a\\tb\\\\c\t0\t1\t'
                      '[{"k":64,"p":"0.001","base":0,"t2":0,"recent":0,"x2":0,"above":0,"below":0,"verdict":"N"}]\n')
    assert '"t2":4294967294,"recent":2147483647,"x2":-4294967294,' in got[2]
    for ln, row in zip(LS_LINES, got):
        assert sinks.pg_row_from_copy("ls", row) == entry_from_csv(ln).to_pg_row()


def test_native_copy_encoder_matches_python_for_ls():
    lines = LS_LINES + MALFORMED + ["ls|13|a|c|0000000005|01|01:050.50:03:-04:05:06:01:02:N"]
    nat = sinks.copy_encode_native(lines)
    assert nat is not None, "the native extension does not import: build it (a broken build must not pass as a skip)"
    want = sinks.copy_encode_lines(lines)
    assert len(want["ls"]) == 4                           # every malformed row is dropped whole
    assert nat["ls"][1] == 4 and nat["ls"][0].decode("utf-8") == "".join(want["ls"])
    assert want["ls"][3].endswith('\ta\tc\t5\t1\t[{"k":1,"p":"50.5","base":3,"t2":-4,"recent":5,"x2":6,"above":1,'
                                  '"below":2,"verdict":"N"}]\n')
    assert all(nat[t][1] == 0 for t in nat if t != "ls")


# ------------------------------------------------------------------------------- the verdict

def _native():
    from apmbackend_amd import _native as nat
    return nat.load(build_if_missing=False)


S = 100000


def verdict(a, b, mR, mB, T2, X2, q, r_u, r_d, z, min_delta, min_recent, min_baseline):
    """docs/SHIFT.md in Python integers."""
    if mB < min_baseline or mR < min_recent:
        return "N"
    var = z * z * mR * q * (S - q)
    if (r_u and X2 - T2 >= 2 * min_delta and 1000 * a * S >= r_u * mR * (S - q) and a * S >= mR * (S - q)
            and (a * S - mR * (S - q)) ** 2 * 10 ** 6 >= var):
        return "U"
    if (r_d and T2 - X2 >= 2 * min_delta and 1000 * b * S >= r_d * mR * q and b * S >= mR * q
            and (b * S - mR * q) ** 2 * 10 ** 6 >= var):
        return "D"
    return "N"


def test_shift_verdict_against_python_integers():
    N = _native()
    M = 2 ** 31 - 1
    seen = set()

    def both(*args):
        got = N.shift_verdict(*args)
        assert got == verdict(*args), args
        seen.add(got)
        return got

    # the extremes: every product at its widest
    for q in (1, 99999, 50000):
        for r in (1001, 1000000):
            for z in (0, 100000):
                for a, b in ((M, 0), (0, M), (M // 2, M // 2), (M - 1, 1), (0, 0)):
                    both(a, b, M, M, -5, 2 ** 32 - 2, q, r, r, z, 1, 1, 1)
                    both(a, b, M, M, 2 ** 32 - 2, -(2 ** 32 - 2), q, r, r, z, 1073741823, M, M)
                    both(a, b, M, 100, 0, 2 * 1073741823, q, r, 0, z, 1073741823, 20, 100)
                    both(a, b, M, 100, 2 * 1073741823, 0, q, 0, r, z, 1073741823, 20, 100)
    assert both(M, 0, M, M, 0, 10, 99999, 1001, 0, 100000, 5, 1, 1) == "U"      # the squared side near 2^116
    assert both(0, M, M, M, 10, 0, 1, 0, 1001, 100000, 5, 1, 1) == "D"
    assert both(M, 0, M, M, 0, 10, 50000, 1001, 0, 100000, 5, 1, 1) == "U"      # z^2 mR q (S - q) near 2^98
    # the ratio above 64 bits: r mR (S - q) = 10^6 (2^31 - 1) 99999 > 2^64
    assert 10 ** 6 * M * 99999 > 2 ** 64
    assert both(M, 0, M, M, 0, 10, 1, 1000000, 0, 0, 5, 1, 1) == "N"
    assert both(M, 0, M, M, 0, 10, 99999, 1000000, 0, 0, 5, 1, 1) == "U"
    # every inequality at equality, one less and one more
    # ratio: q = 95000, mR = 1000, up 3 -> a = 150 exactly
    for a, w in ((149, "N"), (150, "U"), (151, "U")):
        assert both(a, 0, 1000, 100, 0, 100, 95000, 3000, 0, 0, 50, 20, 100) == w
        assert both(0, a, 1000, 100, 100, 0, 5000, 0, 3000, 0, 50, 20, 100) == w.replace("U", "D")
    # z: q = 50000, mR = 400: sd = 10 samples; z = 4 -> a - 200 >= 40
    for a, w in ((239, "N"), (240, "U"), (241, "U")):
        assert both(a, 0, 400, 100, 0, 100, 50000, 1001, 0, 4000, 50, 20, 100) == w
        assert both(0, a, 400, 100, 100, 0, 50000, 0, 1001, 4000, 50, 20, 100) == w.replace("U", "D")
    # the expectation itself: a S >= mR (S - q) (the ratio test implies it for r > 1; checked on its own by r = 1.001)
    for a, w in ((199, "N"), (201, "U")):
        assert both(a, 0, 400, 100, 0, 100, 50000, 1001, 0, 0, 50, 20, 100) == w
    # minDelta, minRecent, minBaseline
    for d, w in ((99, "N"), (100, "U"), (101, "U")):
        assert both(400, 0, 400, 100, 7, 7 + d, 50000, 2000, 2000, 0, 50, 20, 100) == w
        assert both(0, 400, 400, 100, 7 + d, 7, 50000, 2000, 2000, 0, 50, 20, 100) == ("D" if w == "U" else "N")
        assert both(400, 0, 400, 100, -7 - d, -7, 50000, 2000, 2000, 0, 50, 20, 100) == w
    for mR, w in ((19, "N"), (20, "U"), (21, "U")):
        assert both(mR, 0, mR, 100, 0, 100, 50000, 2000, 0, 0, 50, 20, 100) == w
    for mB, w in ((99, "N"), (100, "U"), (101, "U")):
        assert both(20, 0, 20, mB, 0, 100, 50000, 2000, 0, 0, 50, 20, 100) == w
    # a side that is not configured never fires
    assert both(400, 0, 400, 100, 0, 100, 50000, 0, 2000, 0, 50, 20, 100) == "N"
    assert both(0, 400, 400, 100, 100, 0, 50000, 2000, 0, 0, 50, 20, 100) == "N"
    rng = random.Random(24)
    for _ in range(4000):
        mR = rng.choice([rng.randint(0, 60), rng.randint(0, 5000), rng.randint(0, M)])
        a = rng.randint(0, mR)
        b = rng.randint(0, mR - a)
        T2 = rng.randint(-3000, 3000)
        X2 = T2 + rng.randint(-300, 300)
        both(a, b, mR, rng.randint(0, 300), T2, X2, rng.choice([1, 25000, 50000, 95000, 99000, 99999]),
             rng.choice([0, 1001, 1500, 3000, 1000000]), rng.choice([0, 1001, 2000, 1000000]),
             rng.choice([0, 1000, 3000, 4000, 100000]), rng.choice([1, 10, 50]), rng.choice([1, 20]), rng.choice([1, 100]))
    assert seen == {"U", "D", "N"}
    for bad in ((-1, 0, 5, 5, 0, 0, 50000, 2000, 0, 0, 5, 1, 1), (3, 3, 5, 5, 0, 0, 50000, 2000, 0, 0, 5, 1, 1),
                (1, 0, 5, 5, 0, 0, 100000, 2000, 0, 0, 5, 1, 1), (1, 0, 5, 5, 0, 0, 0, 2000, 0, 0, 5, 1, 1),
                (1, 0, 5, 5, 0, 0, 50000, 1000, 0, 0, 5, 1, 1), (1, 0, 5, 5, 0, 0, 50000, 2000, 1000001, 0, 5, 1, 1),
                (1, 0, 5, 5, 0, 0, 50000, 2000, 0, 100001, 5, 1, 1), (1, 0, 5, 5, 0, 0, 50000, 2000, 0, 0, 0, 1, 1),
                (1, 0, 5, 5, 2 ** 32, 0, 50000, 2000, 0, 0, 5, 1, 1), (1, 0, 2 ** 31, 5, 0, 0, 50000, 2000, 0, 0, 5, 1, 1)):
        with pytest.raises(ValueError):
            N.shift_verdict(*bad)


def test_kernel_constants():
    N = _native()
    assert N.shift_group_max() == 512 and N.shift_group_win() == 32


# ------------------------------------------------------------------------------- service

LOUD = {"default": {"minDelta": 1}, "services": {"S:none": None},
        "rules": [{"short": 1, "percentile": 50, "up": 1.001, "down": 1.001, "z": 0}], "minRecent": 1, "minBaseline": 2}


def run_service(tmp_path, key):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    C["streamCalcStats"]["windowSizeInIntervals"] = 6   # (a window the 20 buckets of the run fill)
    if key:
        C["gpu"]["latencyShift"] = key
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    assert ("ls" in svc.outputs) == bool(key)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_service_spools_the_shift_table_and_leaves_the_others(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    P, on = run_service(tmp_path / "on", copy.deepcopy(LOUD))
    P0, off = run_service(tmp_path / "off", None)
    assert len(P.ls) > 5 and P0.ls == []
    assert on["apm_latency_shift.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.ls)["ls"])
    assert [c.strip() for c in on["apm_latency_shift.columns"].decode().strip().split(",")] == sinks.COLUMNS["ls"][1]
    assert not any(f.startswith("apm_latency_shift") for f in off)
    # every other table is what a run without the key writes
    assert {f: v for f, v in on.items() if not f.startswith("apm_latency_shift")} == off
    # ... and so is every other stream of the CPU engine
    for k in ("stats", "fs", "al", "tx_db", "lh", "wp", "sl", "tk", "sv", "rw", "sb", "tf", "po"):
        assert getattr(P, k) == getattr(P0, k), k


def test_service_routes_the_queue(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    assert config.gpu_opt(C, "shiftQueue") == "latency_shift"
    C["streamInsertDb"]["dbShiftTable"] = "my_shift"
    assert sinks.COLUMNS["ls"][0] == "dbShiftTable"


def test_service_rejects_a_bad_key(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C["gpu"]["latencyShift"] = {"default": {"minDelta": 5}, "rules": [{"short": 6, "percentile": 95, "up": 2},
                                                                      {"short": 1, "percentile": 95, "up": 2}]}
    with pytest.raises(ValueError):
        IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
