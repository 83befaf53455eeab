"""The tf stream (traffic drops and surges, docs/TRAFFIC.md) on the CPU: the config key, the class
table, the oracle's rows against an independent reference (tests/traffic_ref.py), the record codec,
both COPY encoders, the service's route to the table, the reload report, and the exact verdict of
trafficcmp.h through its binding against Python integers."""
import copy
import os
import random

import pytest

from apmbackend_amd.models.cpu_engine import CpuOracleEngine
from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models.pipeline import EVERY_OUT_KINDS, FULL_OUT_KINDS, APMEngine, engine_config, output_mask
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import TrafficEntry, entry_from_csv

import traffic_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

INT32_MAX = 2 ** 31 - 1
KEY = {"default": {"minRate": 5},
       "services": {"S:nightlyBatch": None, "S:checkout": {"minRate": 50}},
       "rules": [{"short": 1, "drop": 0.1, "z": 4}, {"short": 6, "drop": 0.5, "surge": 3, "z": 3}],
       "minBuckets": 8}


# ------------------------------------------------------------------------------- config

def test_config_key_accepted_forms():
    want = {"default": 5, "services": {"S:nightlyBatch": None, "S:checkout": 50},
            "rules": [(1, 100, 0, 4000), (6, 500, 3000, 3000)], "minBuckets": 8}
    assert config.parse_traffic_watch(KEY) == want
    assert config.parse_traffic_watch(None) is None
    # default absent or null, minBuckets and z absent, decimals as text, the bounds themselves
    got = config.parse_traffic_watch({"services": {"a": {"minRate": 1}}, "rules": [{"short": 64, "surge": "1.001"}]})
    assert got == {"default": None, "services": {"a": 1}, "rules": [(64, 0, 1001, 3000)], "minBuckets": 8}
    got = config.parse_traffic_watch({"default": None, "services": {"a": {"minRate": INT32_MAX}},
                                      "rules": [{"short": 1, "drop": 0.001, "z": 0}, {"short": 2, "drop": 0.999, "z": 100},
                                                {"short": 3, "surge": 1000, "z": "0.001"},
                                                {"short": 4, "drop": 0.5, "surge": 2}], "minBuckets": 3})
    assert got["services"]["a"] == INT32_MAX and got["minBuckets"] == 3
    assert got["rules"] == [(1, 1, 0, 0), (2, 999, 0, 100000), (3, 0, 1000000, 1), (4, 500, 2000, 3000)]
    # no service with a minRate: the stream is off
    assert config.parse_traffic_watch({"default": None, "services": {"x": None}, "rules": [{"short": 1, "drop": 0.5}]}) is None
    assert config.parse_traffic_watch({"rules": [{"short": 1, "drop": 0.5}]}) is None
    C = config.parse_config_text('{"gpu": {"trafficWatch": {"default": {"minRate": 7}, '
                                 '"rules": [{"short": 2, "drop": 0.25}]}}}')
    assert config.traffic_watch(C) == {"default": 7, "services": {}, "rules": [(2, 250, 0, 3000)], "minBuckets": 8}
    assert config.traffic_watch({"gpu": {}}) is None and config.traffic_watch({"gpu": {"trafficWatch": None}}) is None
    assert config.gpu_opt({}, "trafficQueue") == "traffic"
    for key in ("trafficWatch", "trafficQueue"):
        assert key in config.GPU_OPTIONAL and key not in config.GPU_DEFAULTS
        assert key not in config.default_config()["gpu"]
    assert config.GPU_OPTIONAL["trafficWatch"] is None


def test_default_config_text_is_unchanged():
    with open(config.DEFAULT_CONFIG_PATH, encoding="utf-8") as fh:
        txt = fh.read()
    assert "trafficWatch" not in txt and "trafficQueue" not in txt and "dbTrafficTable" not in txt
    assert "trafficWatch" not in config.read_apm_config(config.DEFAULT_CONFIG_PATH)["gpu"]


O = {"minRate": 5}
RU = [{"short": 1, "drop": 0.5}]


def rule(**kw):
    return {"default": O, "rules": [kw]}


BAD = [[], "x", 5, {"rules": RU, "extra": 1}, {"default": O}, {"default": O, "rules": []}, {"default": O, "rules": None},
       {"default": O, "rules": {"short": 1, "drop": 0.5}},
       {"default": O, "rules": RU * 2},                                             # short not ascending
       {"default": O, "rules": [{"short": 2, "drop": 0.5}, {"short": 1, "drop": 0.5}]},
       {"default": O, "rules": [{"short": k, "drop": 0.5} for k in range(1, 6)]},   # five rules
       rule(short=0, drop=0.5), rule(short=-1, drop=0.5), rule(short=65, drop=0.5), rule(short=True, drop=0.5),
       rule(short=1.0, drop=0.5), rule(short="1", drop=0.5), rule(short=None, drop=0.5),
       rule(short=1), rule(drop=0.5), rule(short=1, z=3),                           # neither drop nor surge
       rule(short=1, drop=0.5, long=3), {"default": O, "rules": [[1, 0.5]]},
       rule(short=1, drop=0), rule(short=1, drop=1), rule(short=1, drop=0.0001), rule(short=1, drop=-0.5),
       rule(short=1, drop=True), rule(short=1, drop="x"), rule(short=1, drop=None), rule(short=1, drop=float("nan")),
       rule(short=1, drop=0.1234),
       rule(short=1, surge=1), rule(short=1, surge=1.0001), rule(short=1, surge=1000.001), rule(short=1, surge=0.5),
       rule(short=1, surge=True), rule(short=1, surge=None), rule(short=1, surge=float("inf")),
       rule(short=1, drop=0.5, surge=1),                                            # one good, one bad
       rule(short=1, drop=0.5, z=-1), rule(short=1, drop=0.5, z=100.001), rule(short=1, drop=0.5, z=True),
       rule(short=1, drop=0.5, z=None), rule(short=1, drop=0.5, z="abc"), rule(short=1, drop=0.5, z=1.2345),
       {"default": [5], "rules": RU}, {"default": 5, "rules": RU}, {"default": {}, "rules": RU},
       {"default": {"minRate": 5, "x": 1}, "rules": RU}, {"default": {"minRate": True}, "rules": RU},
       {"default": {"minRate": 5.0}, "rules": RU}, {"default": {"minRate": "5"}, "rules": RU},
       {"default": {"minRate": None}, "rules": RU}, {"default": {"minRate": 0}, "rules": RU},
       {"default": {"minRate": -1}, "rules": RU}, {"default": {"minRate": 2 ** 31}, "rules": RU},
       {"default": O, "services": [], "rules": RU}, {"default": O, "services": {"a": 5}, "rules": RU},
       {"default": O, "services": {"a": {"rate": 5}}, "rules": RU}, {"default": O, "services": {1: O}, "rules": RU},
       {"default": O, "rules": RU, "minBuckets": 2}, {"default": O, "rules": RU, "minBuckets": -3},
       {"default": O, "rules": RU, "minBuckets": True}, {"default": O, "rules": RU, "minBuckets": 8.0},
       {"default": O, "rules": RU, "minBuckets": "8"}, {"default": O, "rules": RU, "minBuckets": None},
       # rejected even when no service has a minRate
       {"default": None, "rules": []}, {"services": {"x": None}, "rules": RU, "minBuckets": 0}]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_config_key_rejections(i):
    with pytest.raises(ValueError):
        config.parse_traffic_watch(BAD[i])


def test_read_apm_config_stops_on_a_bad_key(tmp_path):
    p = tmp_path / "cfg.json"
    p.write_text('{"gpu": {"trafficWatch": {"default": {"minRate": 5}, "rules": [{"short": 0, "drop": 0.5}]}}}')
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    p.write_text('{"gpu": {"trafficWatch": {"default": {"minRate": 9}, "rules": [{"short": 2, "surge": 2.5}]}, '
                 '"trafficQueue": "q"}}')
    C = config.read_apm_config(str(p))
    assert config.traffic_watch(C)["default"] == 9 and config.gpu_opt(C, "trafficQueue") == "q"


def test_span_bound_is_the_engines_not_the_parsers():
    tf = config.parse_traffic_watch({"default": O, "rules": [{"short": 1, "drop": 0.5}, {"short": 31, "drop": 0.5}]})
    config.check_traffic_watch(tf, 31)
    config.check_traffic_watch(None, 3)
    with pytest.raises(ValueError):
        config.check_traffic_watch(tf, 30)
    C = config.default_config(replay=True)
    C["gpu"]["trafficWatch"] = {"default": O, "rules": [{"short": 1, "drop": 0.5}, {"short": 31, "drop": 0.5}]}
    assert int(C["streamCalcStats"]["windowSizeInIntervals"]) == 30
    assert engine_config(C, outputs=("st", "tf"))["tf_short"] == [1, 31]   # (a reload reads it through here)
    with pytest.raises(ValueError):
        PipelineOracle(copy.deepcopy(C), UTC)
    with pytest.raises(ValueError):
        CpuOracleEngine(copy.deepcopy(C))
    C["streamCalcStats"]["windowSizeInIntervals"] = 31
    PipelineOracle(copy.deepcopy(C), UTC)


def test_class_table():
    classes, services, default = config.traffic_tables(config.parse_traffic_watch(KEY))
    assert classes == [[], [5], [50]]
    assert services == {"S:nightlyBatch": 0, "S:checkout": 2} and default == 1
    nodef = dict(KEY, default=None)
    classes, services, default = config.traffic_tables(config.parse_traffic_watch(nodef))
    assert classes == [[], [50]] and services == {"S:nightlyBatch": 0, "S:checkout": 1} and default == 0
    assert config.traffic_tables(None) == ([], {}, 0)
    # the other streams' tables are untouched by the key
    C = config.default_config(replay=True)
    C["gpu"]["trafficWatch"] = copy.deepcopy(KEY)
    e = engine_config(C, outputs=("st", "tf"))
    assert e["slo_classes"] == [] and e["sb_classes"] == [] and e["sb_services"] == {}
    assert e["tf_classes"] == [[], [5], [50]] and e["tf_services"] == {"S:nightlyBatch": 0, "S:checkout": 2}
    assert e["tf_default"] == 1 and e["tf_short"] == [1, 6] and e["tf_drop"] == [100, 500]
    assert e["tf_surge"] == [0, 3000] and e["tf_z"] == [4000, 3000] and e["tf_min_buckets"] == 8


def test_outputs_naming_tf_needs_the_key():
    assert EVERY_OUT_KINDS == FULL_OUT_KINDS + ("tf",) and FULL_OUT_KINDS[-1] == "sb"
    bit = EVERY_OUT_KINDS.index("tf")
    assert bit == 15 and output_mask(("tf",)) == 1 << 15 and output_mask(("sb", "st")) == (1 << 14) | (1 << 3)
    C = config.default_config(replay=True)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "tf"))
    C["gpu"]["trafficWatch"] = copy.deepcopy(KEY)
    assert (engine_config(C, outputs=("st", "tf"))["outputs"] >> bit) & 1
    assert not (engine_config(C, keep_text=True)["outputs"] >> bit) & 1   # keep_text alone leaves it off
    d = engine_config(config.default_config(replay=True))
    assert d["tf_classes"] == [] and d["tf_short"] == [] and d["tf_drop"] == [] and d["tf_min_buckets"] == 8


def test_a_reload_that_changes_the_key_needs_a_restart():
    C = config.default_config(replay=True)
    C["gpu"]["trafficWatch"] = copy.deepcopy(KEY)
    old = engine_config(C, outputs=("st", "tf"))
    assert APMEngine.restart_required(old, engine_config(copy.deepcopy(C), outputs=())) == []
    C2 = copy.deepcopy(C)
    C2["gpu"]["trafficWatch"]["rules"][0]["drop"] = 0.2
    assert APMEngine.restart_required(old, engine_config(C2, outputs=())) == ["tf_drop"]
    C3 = copy.deepcopy(C)
    C3["gpu"]["trafficWatch"]["rules"] = [{"short": 2, "surge": 3, "z": 1}]
    assert APMEngine.restart_required(old, engine_config(C3, outputs=())) == ["tf_drop", "tf_short", "tf_surge", "tf_z"]
    C4 = copy.deepcopy(C)
    C4["gpu"]["trafficWatch"]["minBuckets"] = 5
    C4["gpu"]["trafficWatch"]["services"]["S:checkout"]["minRate"] = 40
    assert APMEngine.restart_required(old, engine_config(C4, outputs=())) == ["tf_classes", "tf_min_buckets"]
    C5 = copy.deepcopy(C)
    del C5["gpu"]["trafficWatch"]
    assert APMEngine.restart_required(old, engine_config(C5, outputs=())) == \
        ["tf_classes", "tf_default", "tf_drop", "tf_services", "tf_short", "tf_surge", "tf_z"]
    assert not {k for k in old if k.startswith("tf_")} & set(APMEngine.LIVE_KEYS)


# ------------------------------------------------------------------------------- oracle

def tx(server, service, end, elapsed):
    return f"tx|{server}|{service}|id|1|{end - 5}|{end}|{elapsed}|Y"


def test_stats_oracle_rows_literal():
    tf, st = [], []
    watch = config.parse_traffic_watch({"default": {"minRate": 2}, "services": {"off": None, "busy": {"minRate": 4}},
                                        "rules": [{"short": 1, "drop": 0.5, "surge": 2, "z": 0}], "minBuckets": 3})
    so = StatsOracle(st.append, lambda _l: None, 10, 3, 1, emit_traffic=tf.append, traffic=watch)
    B = 1000
    so.latest = B + 1
    t = lambda b, ms=1: b * 10000 + ms
    # the rollover to B + 2 reads the window [B - 2, B + 1]: three baseline buckets, newest entry B + 1

    def feed(service, per_bucket):
        for b, n in zip((B - 2, B - 1, B, B + 1), per_bucket):
            for i in range(n):
                so.consume(tx("a", service, t(b), "abc" if i == 0 else 7))   # (the first sample of a bucket is a NaN)

    feed("stopped", (4, 4, 4, 0))
    feed("halved", (4, 4, 4, 2))       # 2000 * 2 <= 500 * 1 * 8: exactly on the threshold
    feed("flood", (2, 4, 6, 8))        # med2 8, deviations 4, 0, 4: 2000 * 8 >= 2000 * 8
    feed("steady", (4, 4, 4, 3))
    feed("slow", (1, 1, 1, 0))         # med2 2 < 2 * 2: not judged
    feed("off", (4, 4, 4, 0))
    feed("busy", (3, 3, 3, 0))         # med2 6 < 2 * 4
    assert tf == []
    so.consume(tx("d", "t", t(B + 2), 5))
    ts = (B + 2 - 1 - 1) * 10000
    assert tf == [f"tf|{ts}|a|stopped|12|2|1:3:0:8:0:D",
                  f"tf|{ts}|a|halved|14|2|1:3:2:8:0:D",
                  f"tf|{ts}|a|flood|20|2|1:3:8:8:8:S"]
    assert [l.split("|")[3] for l in st] == ["stopped", "halved", "flood", "steady", "slow", "off", "busy"]
    off = StatsOracle(lambda _l: None, lambda _l: None, 10, 3, 2)
    assert off.emit_traffic is None and off.traffic is None


def test_oracle_rows_against_the_independent_reference():
    rng = random.Random(22)
    tf, st = [], []
    window, buffer = 11, 2
    rules = [(1, 100, 0, 4000), (3, 500, 3000, 3000), (8, 0, 1500, 0), (12, 999, 1001, 0)]   # 12 = the window's buckets
    rates = {"S:named": 20, "S:none": None}
    watch = {"default": 3, "services": rates, "rules": rules, "minBuckets": 3}
    so = StatsOracle(st.append, lambda _l: None, 10, window, buffer, emit_traffic=tf.append, traffic=watch)
    B = 3000
    so.latest = B
    labels = list(range(B + 1 - window - buffer, B + 1 - buffer + 1))   # the window of the rollover to B + 1
    assert len(labels) == 12
    ts = (B + 1 - buffer - 1) * 10000
    want, verdicts = {}, set()
    for i in range(200):
        server = f"s{i % 3}"
        service = "S:named" if i % 11 == 0 else "S:none" if i % 13 == 0 else f"S:{i}"
        if (server, service) in want:
            service += f"_{i}"
        rate = rates.get(service, 3)
        level = rng.choice([0, 2, 3, 6, 10, 40])
        noise = rng.choice([0, 0, 1, 4])
        counts = [max(0, level + rng.randint(-noise, noise)) if rng.random() > 0.1 else 0 for _ in labels]
        tail = rng.choice([1, 3, 8])
        how = rng.choice(["same", "stop", "flood", "half"])
        for j in range(len(labels) - tail, len(labels)):
            counts[j] = {"same": counts[j], "stop": 0, "flood": counts[j] * 4 + 3, "half": counts[j] // 2}[how]
        for b, n in zip(labels, counts):
            for v in range(n):
                so.consume(tx(server, service, b * 10000 + 1, "abc" if v % 5 == 4 else v))
        so.consume(tx(server, service, (labels[0] - 1) * 10000 + 1, 1))    # older than the window: not counted
        so.consume(tx(server, service, (labels[-1] + 1) * 10000 + 1, 1))   # newer than the window
        want[(server, service)] = None if rate is None else R.row(ts, server, service, counts, rules, rate, 3)
        if rate is not None:
            verdicts |= {p[4] for p in R.series_ints(counts, rules, rate, 3)[1]}
    so.consume(tx("t", "T", (B + 1) * 10000 + 1, 1))
    order = [(l.split("|")[2], l.split("|")[3]) for l in st]
    flat = [want[k] for k in order if want.get(k) is not None]
    assert tf == flat and 20 < len(tf) < 190
    assert verdicts == {"D", "S", "N"}
    assert not any(r.split("|")[3] == "S:none" for r in tf)
    # a span equal to the window has no baseline: B = 0, never judged
    for r in tf:
        assert r.split("|")[6].split(",")[3].split(":")[1:] == ["0", r.split("|")[4], "0", "0", "N"]


def test_pipeline_oracle_and_cpu_engine_carry_the_stream():
    C = config.default_config(replay=True)
    assert PipelineOracle(copy.deepcopy(C), UTC).st.emit_traffic is None
    C["gpu"]["trafficWatch"] = copy.deepcopy(KEY)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    assert P.st.emit_traffic is not None and P.st.traffic["rules"] == [(1, 100, 0, 4000), (6, 500, 3000, 3000)]
    assert P.tf == [] and CpuOracleEngine(C).take("tf") == []


# ------------------------------------------------------------------------------- codec, encoders

TF_LINES = ["tf|1578391200000|jvm00|S:checkout|310|50|1:30:0:20:0:D,6:25:300:20:4:S",
            "tf|1578391210000|j\tx|S:a\tb\\c|0|1|64:3:2:1:0:N",
            "tf|1578391220000|jvm01|S:max|2147483647|2147483647|"
            "1:2147483647:4294967295:4294967294:8589934592:S,2:1:0:0:0:N,3:2:1:1:1:D,64:5:6:7:8:N"]


def test_codec_round_trip_and_pg_row():
    for ln in TF_LINES:
        e = entry_from_csv(ln)
        assert isinstance(e, TrafficEntry) and e.type == "tf" and e.to_csv() == ln
    e = entry_from_csv(TF_LINES[0])
    assert (e.server, e.service, e.count, e.min_rate) == ("jvm00", "S:checkout", 310, 50)
    assert e.rules == [(1, 30, 0, 20, 0, "D"), (6, 25, 300, 20, 4, "S")]
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["tf"][1]
    assert row["rules"] == [{"k": 1, "buckets": 30, "recent": 0, "med2": 20, "mad4": 0, "verdict": "D"},
                            {"k": 6, "buckets": 25, "recent": 300, "med2": 20, "mad4": 4, "verdict": "S"}]
    assert "tf" in records.RECORD_TYPES and "tf" in sinks.TYPES and sinks.COLUMNS["tf"][0] == "dbTrafficTable"
    assert sinks.DEFAULT_TABLES["tf"] == "apm_traffic"
    for bad in MALFORMED:
        assert entry_from_csv(bad) is None, bad


MALFORMED = ["tf|12|s|v|x|5|1:2:3:4:5:D", "tf|12|s|v|5|-1|1:2:3:4:5:D", "tf|12|s|v||5|1:2:3:4:5:D",
             "tf|12|s|v|5|1.5|1:2:3:4:5:D", "tf|12|s|v|12345678901|5|1:2:3:4:5:D",
             "tf|12|s|v|5|5", "tf|12|s|v|5|5|", "tf|12|s|v|5|5|1:2:3:4:5", "tf|12|s|v|5|5|1:2:3:4:D",
             "tf|12|s|v|5|5|1:2:3:4:5:X", "tf|12|s|v|5|5|1:2:3:4:5:d", "tf|12|s|v|5|5|1:2:3:4:5:D:1",
             "tf|12|s|v|5|5|1:2:3:4:5:D,", "tf|12|s|v|5|5|,1:2:3:4:5:D", "tf|12|s|v|5|5|1:2:x:4:5:D",
             "tf|12|s|v|5|5|1:2::4:5:D", "tf|12|s|v|5|5|1:2:3:4:5:",
             "tf|12|s|v|5|5|1:2:3:4:5:D,2:2:3:4:5:N,3:2:3:4:5:N,4:2:3:4:5:N,5:2:3:4:5:N",
             "tf|12|s|v|5|5|1:2:3:4:5:DS", "tf|12|s|v|5 |5|1:2:3:4:5:D", "tf|12|s|v|5|5|1:2:-3:4:5:D",
             "tf|12|s|v|5|5|1:2:3:4:12345678901:D"]


def test_copy_encode_lines_tf():
    got = sinks.copy_encode_lines(TF_LINES)["tf"]
    assert got[0] == ('2020-01-07 10:00:00.000+00\tjvm00\tS:checkout\t310\t50\t'
                      '[{"k":1,"buckets":30,"recent":0,"med2":20,"mad4":0,"verdict":"D"},'
                      '{"k":6,"buckets":25,"recent":300,"med2":20,"mad4":4,"verdict":"S"}]\n')
    assert got[1] == ('2020-01-07 10:00:10.000+00\tj\\tx\tS:a\\tb\\\\c\t0\t1\t'
                      '[{"k":64,"buckets":3,"recent":2,"med2":1,"mad4":0,"verdict":"N"}]\n')
    assert got[2].startswith('2020-01-07 10:00:20.000+00\tjvm01\tS:max\t2147483647\t2147483647\t'
                             '[{"k":1,"buckets":2147483647,"recent":4294967295,"med2":4294967294,"mad4":8589934592,'
                             '"verdict":"S"},{"k":2,')
    for ln, row in zip(TF_LINES, got):
        assert sinks.pg_row_from_copy("tf", row) == entry_from_csv(ln).to_pg_row()


def test_native_copy_encoder_matches_python_for_tf():
    lines = TF_LINES + MALFORMED + ["tf|13|a|c|0000000005|01|01:02:03:04:05:N"]
    nat = sinks.copy_encode_native(lines)
    assert nat is not None, "the native extension does not import: build it (a broken build must not pass as a skip)"
    want = sinks.copy_encode_lines(lines)
    assert len(want["tf"]) == 4                           # every malformed row is dropped whole
    assert nat["tf"][1] == 4 and nat["tf"][0].decode("utf-8") == "".join(want["tf"])
    assert want["tf"][3].endswith('\ta\tc\t5\t1\t[{"k":1,"buckets":2,"recent":3,"med2":4,"mad4":5,"verdict":"N"}]\n')
    assert all(nat[t][1] == 0 for t in nat if t != "tf")


# ------------------------------------------------------------------------------- the verdict

def _native():
    from apmbackend_amd import _native as nat
    return nat.load(build_if_missing=False)


def verdict(R_, med2, mad4, B, kk, r_d, r_s, z, min_rate, min_buckets):
    if B < min_buckets or med2 < 2 * min_rate:
        return "N"
    if r_d and 2000 * R_ <= r_d * kk * med2 and 4000 * R_ <= kk * (2000 * med2 - z * mad4):
        return "D"
    if r_s and 2000 * R_ >= r_s * kk * med2 and 4000 * R_ >= kk * (2000 * med2 + z * mad4):
        return "S"
    return "N"


def test_traffic_verdict_against_python_integers():
    N = _native()
    V = N.traffic_verdict
    # drop: the ratio test met exactly and missed by one (med2 20, k' 1, r_d 100: 2000 R <= 2000)
    assert V(1, 20, 0, 8, 1, 100, 0, 3000, 5, 8) == "D" and V(2, 20, 0, 8, 1, 100, 0, 3000, 5, 8) == "N"
    # ... the MAD test met exactly and missed by one with the ratio test satisfied (r_d 999):
    # 4000 R <= 2000 * 20 - 3000 * 4 = 28000
    assert V(7, 20, 4, 8, 1, 999, 0, 3000, 5, 8) == "D" and V(8, 20, 4, 8, 1, 999, 0, 3000, 5, 8) == "N"
    assert 2000 * 8 <= 999 * 20
    # surge: the ratio test (r_s 3000, k' 6: 2000 R >= 360000) and the MAD test (4000 R >= 6 * 52000)
    assert V(180, 20, 0, 8, 6, 0, 3000, 3000, 5, 8) == "S" and V(179, 20, 0, 8, 6, 0, 3000, 3000, 5, 8) == "N"
    assert V(78, 20, 4, 8, 6, 0, 1001, 3000, 5, 8) == "S" and V(77, 20, 4, 8, 6, 0, 1001, 3000, 5, 8) == "N"
    assert 4000 * 78 == 6 * (2000 * 20 + 3000 * 4) and 2000 * 77 >= 1001 * 6 * 20
    # a negative right-hand side of the drop test: not even R = 0 drops
    assert 2000 * 20 - 3000 * 14 < 0
    assert V(0, 20, 14, 8, 1, 999, 0, 3000, 5, 8) == "N" and V(0, 20, 13, 8, 1, 999, 0, 3000, 5, 8) == "D"
    # the gates: med2 below 2 * minRate by one, B = minBuckets - 1
    assert V(0, 10, 0, 8, 1, 100, 0, 3000, 5, 8) == "D" and V(0, 9, 0, 8, 1, 100, 0, 3000, 5, 8) == "N"
    assert V(0, 10, 0, 7, 1, 100, 0, 3000, 5, 8) == "N" and V(0, 10, 0, 3, 1, 100, 0, 3000, 5, 3) == "D"
    # a test that is not configured never decides
    assert V(0, 20, 0, 8, 1, 0, 3000, 3000, 5, 8) == "N" and V(10 ** 6, 20, 0, 8, 1, 100, 0, 3000, 5, 8) == "N"
    # the extremes: c_r = 2^31 - 1 in every bucket, k = 64, r_s = 10^6, z = 10^5
    M = INT32_MAX
    top = dict(R=64 * M, med2=2 * M, mad4=2 ** 33, kk=64, r_s=1000000, z=100000)
    assert top["r_s"] * top["kk"] * top["med2"] > 2 ** 57 and top["kk"] * (2000 * top["med2"] + top["z"] * top["mad4"]) < 2 ** 63
    cases = []
    for med2 in (2 * M, 2 * M - 1, M, 2 ** 31, 2 ** 32 - 2, 40, 2):
        for mad4 in (0, 1, 4, med2 // 2, med2, 2 * med2, 2 ** 33):
            for kk in (1, 6, 63, 64):
                for r_d, r_s, z in ((999, 1000000, 100000), (1, 1001, 0), (500, 3000, 3000), (999, 1001, 1), (0, 1000000, 100000)):
                    edges = {0, 64 * M, kk * M}
                    if r_d:
                        edges |= {r_d * kk * med2 // 2000 + d for d in (-1, 0, 1)}
                        edges |= {kk * (2000 * med2 - z * mad4) // 4000 + d for d in (-1, 0, 1)}
                    edges |= {-(-r_s * kk * med2 // 2000) + d for d in (-1, 0, 1)}
                    edges |= {-(-kk * (2000 * med2 + z * mad4) // 4000) + d for d in (-1, 0, 1)}
                    cases += [(r, med2, min(mad4, 2 ** 33), 30, kk, r_d, r_s, z, 1, 3) for r in edges if 0 <= r <= 64 * M]
    assert (64 * M, 2 * M, 2 ** 33, 30, 64, 999, 1000000, 100000, 1, 3) in cases
    seen = set()
    for c in cases:
        got = V(*c)
        assert got == verdict(*c), c
        seen.add(got)
    assert seen == {"D", "S", "N"}
    rng = random.Random(8)
    for _ in range(20000):
        med2 = rng.choice([rng.randint(0, 2 * M), rng.randint(0, 200)])
        c = (rng.choice([rng.randint(0, 64 * M), rng.randint(0, 4 * med2 + 5)]), med2,
             rng.choice([0, rng.randint(0, 2 ** 33), rng.randint(0, med2 + 1)]), rng.randint(0, 70), rng.randint(1, 64),
             rng.choice([0, 1, 999, rng.randint(1, 999)]), rng.choice([0, 1001, 1000000, rng.randint(1001, 1000000)]),
             rng.choice([0, 100000, rng.randint(0, 100000)]), rng.choice([1, M, rng.randint(1, 100)]), rng.choice([3, 8, 0, 71]))
        assert V(*c) == verdict(*c), c
    for args in ((-1, 2, 0, 8, 1, 100, 0, 0, 1, 3), (64 * M + 1, 2, 0, 8, 1, 100, 0, 0, 1, 3), (0, 2 * M + 1, 0, 8, 1, 100, 0, 0, 1, 3),
                 (0, 2, 2 ** 33 + 1, 8, 1, 100, 0, 0, 1, 3), (0, 2, 0, 8, 0, 100, 0, 0, 1, 3), (0, 2, 0, 8, 65, 100, 0, 0, 1, 3),
                 (0, 2, 0, 8, 1, 1000, 0, 0, 1, 3), (0, 2, 0, 8, 1, 100, 1000, 0, 1, 3), (0, 2, 0, 8, 1, 100, 1000001, 0, 1, 3),
                 (0, 2, 0, 8, 1, 100, 0, 100001, 1, 3), (0, 2, 0, 8, 1, 100, 0, 0, 0, 3)):
        with pytest.raises(ValueError):
            V(*args)


def test_kernel_constants():
    N = _native()
    assert N.traffic_tile() == 64 and N.traffic_group_win() == 128 and N.traffic_max_win() == 2047


# ------------------------------------------------------------------------------- service

LOUD = {"default": {"minRate": 1}, "services": {"S:none": None},
        "rules": [{"short": 1, "drop": 0.9, "surge": 1.1, "z": 0}], "minBuckets": 3}


def run_service(tmp_path, key):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    C["streamCalcStats"]["windowSizeInIntervals"] = 6   # (a window the 20 buckets of the run fill)
    if key:
        C["gpu"]["trafficWatch"] = key
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    assert ("tf" in svc.outputs) == bool(key)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_service_spools_the_traffic_table(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    P, on = run_service(tmp_path / "on", copy.deepcopy(LOUD))
    P0, off = run_service(tmp_path / "off", None)
    assert len(P.tf) > 5 and P0.tf == []
    assert on["apm_traffic.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.tf)["tf"])
    assert [c.strip() for c in on["apm_traffic.columns"].decode().strip().split(",")] == sinks.COLUMNS["tf"][1]
    assert not any(f.startswith("apm_traffic") for f in off)
    # every other table is what a run without the key writes
    assert {f: v for f, v in on.items() if not f.startswith("apm_traffic")} == off


def test_service_rejects_a_bad_key(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C["gpu"]["trafficWatch"] = {"default": {"minRate": 5}, "rules": [{"short": 6, "drop": 0.5}, {"short": 1, "drop": 0.5}]}
    with pytest.raises(ValueError):
        IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
