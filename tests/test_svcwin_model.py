"""The sv stream (exact per-service window stats across servers, docs/SERVICEWINDOW.md) on the CPU:
the config key, the oracle's rows against an independent reference (tests/svcwin_ref.py), the
record codec, both COPY encoders, the service's route to the table and the reload report."""
import copy
import json
import os
import random

import pytest

from apmbackend_amd.models.cpu_engine import CpuOracleEngine
from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models.pipeline import (DEVICE_OUT_KINDS, NATIVE_OUT_KINDS, APMEngine, engine_config)
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import ServiceWindowEntry, entry_from_csv

import svcwin_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

INT32_MAX = 2 ** 31 - 1
NAN = R.ELAPSED_NAN
QS = [1, 1000, 50000, 75000, 95000, 99900, 99999, 100000]


# ------------------------------------------------------------------------------- config

def test_config_key_is_parsed_like_the_percentile_list():
    assert config.parse_service_window({"percentiles": [50, 75, 95, 99]}) == [50000, 75000, 95000, 99000]
    assert config.parse_service_window({"percentiles": ["0.001", 1, "99.999", 100]}) == [1, 1000, 99999, 100000]
    assert config.parse_service_window(None) == []
    C = config.parse_config_text('{"gpu": {"serviceWindow": {"percentiles": [50, 99.9, 99.99]}}}')
    assert config.service_window(C) == [50000, 99900, 99990]
    assert config.service_window({"gpu": {}}) == [] and config.service_window({"gpu": {"serviceWindow": None}}) == []
    assert config.gpu_opt({}, "svcQueue") == "service_window"
    for key in ("serviceWindow", "svcQueue"):
        assert key in config.GPU_OPTIONAL and key not in config.GPU_DEFAULTS
        assert key not in config.default_config()["gpu"]
    assert config.GPU_OPTIONAL["serviceWindow"] is None


def test_default_config_text_is_unchanged():
    with open(config.DEFAULT_CONFIG_PATH, encoding="utf-8") as fh:
        txt = fh.read()
    assert "serviceWindow" not in txt and "svcQueue" not in txt and "dbSvcTable" not in txt
    assert "serviceWindow" not in config.read_apm_config(config.DEFAULT_CONFIG_PATH)["gpu"]


BAD = [{}, {"percentiles": []}, {"percentiles": None}, {"percentiles": [0]}, {"percentiles": [100.001]},
       {"percentiles": [50.0001]}, {"percentiles": [99, 50]}, {"percentiles": [50, 50]},
       {"percentiles": [1, 2, 3, 4, 5, 6, 7, 8, 9]}, {"percentiles": [-1]}, {"percentiles": ["abc"]},
       {"percentiles": [True]}, {"percentiles": 50}, {"percentiles": "50"}, {"percentiles": [float("nan")]},
       {"percentiles": [50], "extra": 1}, {"pcts": [50]}, [50, 95], 50, "50", True, False, 0, []]


@pytest.mark.parametrize("bad", BAD)
def test_config_validation_raises(bad, tmp_path):
    with pytest.raises(ValueError):
        config.parse_service_window(bad)
    C = config.default_config(replay=True)
    C["gpu"]["serviceWindow"] = bad
    with pytest.raises(ValueError):       # engine construction (the settings every engine is built from)
        engine_config(C, outputs=("st",))
    with pytest.raises(ValueError):
        CpuOracleEngine(C)
    p = tmp_path / "cfg.json"             # config load
    p.write_text(json.dumps({"gpu": {"serviceWindow": bad}}))
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))


def test_service_rejects_a_bad_key(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C["gpu"]["serviceWindow"] = {"percentiles": [99, 50]}
    with pytest.raises(ValueError):
        IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)


def test_outputs_naming_sv_needs_the_key(tmp_path):
    assert DEVICE_OUT_KINDS == NATIVE_OUT_KINDS + ("sv",) and DEVICE_OUT_KINDS[-1] == "sv"
    bit = DEVICE_OUT_KINDS.index("sv")
    assert bit == 12
    C = config.default_config(replay=True)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "sv"))
    C["gpu"]["serviceWindow"] = {"percentiles": [50, 99.9]}
    e = engine_config(C, outputs=("st", "sv"))
    assert e["svc_pcts"] == [50000, 99900] and (e["outputs"] >> bit) & 1
    assert not (engine_config(C, keep_text=True)["outputs"] >> bit) & 1   # keep_text alone leaves it off
    assert engine_config(config.default_config(replay=True))["svc_pcts"] == []
    p = tmp_path / "cfg.json"
    p.write_text('{"gpu": {"serviceWindow": {"percentiles": [50, 99.9]}, "svcQueue": "q"}}')
    assert config.service_window(config.read_apm_config(str(p))) == [50000, 99900]


def test_a_reload_that_changes_the_key_needs_a_restart():
    C = config.default_config(replay=True)
    C["gpu"]["serviceWindow"] = {"percentiles": [50, 95]}
    old = engine_config(C, outputs=("st", "sv"))
    assert APMEngine.restart_required(old, engine_config(copy.deepcopy(C), outputs=())) == []
    C2 = copy.deepcopy(C)
    C2["gpu"]["serviceWindow"]["percentiles"] = [50, 99]
    assert APMEngine.restart_required(old, engine_config(C2, outputs=())) == ["svc_pcts"]
    C3 = copy.deepcopy(C)
    del C3["gpu"]["serviceWindow"]
    assert APMEngine.restart_required(old, engine_config(C3, outputs=())) == ["svc_pcts"]
    assert "svc_pcts" not in APMEngine.LIVE_KEYS


# ------------------------------------------------------------------------------- oracle

def tx(server, service, end, elapsed):
    return f"tx|{server}|{service}|id|1|{end - 5}|{end}|{elapsed}|Y"


def test_stats_oracle_rows_literal():
    sv, st = [], []
    so = StatsOracle(st.append, lambda _l: None, 10, 3, 1, emit_svc=sv.append, svc_percentiles=[1000, 50000, 99900])
    B = 1000
    so.latest = B
    t = lambda b, ms=1: b * 10000 + ms
    for ln in (tx("a", "x", t(B), -1), tx("a", "n", t(B), "abc"), tx("a", "y", t(B), 7),
               tx("b", "y", t(B), "abc"), tx("b", "x", t(B), 0), tx("b", "n", t(B), "zz"),
               tx("c", "z", t(B - 1), INT32_MAX), tx("c", "z", t(B), INT32_MAX), tx("c", "z", t(B), INT32_MAX),
               tx("c", "old", t(B - 9), 5)):                                  # outside the window: servers 1, m 0
        so.consume(ln)
    assert sv == []
    so.consume(tx("d", "t", t(B + 2), 5))   # rollover to B + 2: window [B - 2, B + 1]
    ts = (B + 2 - 1 - 1) * 10000
    assert sv == [f"sv|{ts}|x|2|2|0|-1|1:-0.5,50:-1,99.9:0",                 # [-1, 0] over two servers
                  f"sv|{ts}|y|2|1|1|7|1:7,50:7,99.9:7",                       # (only-NaN service n: no row)
                  f"sv|{ts}|z|1|3|0|6442450941|1:2147483647,50:2147483647,99.9:2147483647"]
    assert [l.split("|")[2:4] for l in st] == [["a", "x"], ["a", "n"], ["a", "y"], ["b", "y"], ["b", "x"], ["b", "n"],
                                                ["c", "z"], ["c", "old"]]
    quiet = StatsOracle(lambda _l: None, lambda _l: None, 10, 3, 2)
    assert quiet.emit_svc is None and quiet.svc_percentiles == []


def test_oracle_rows_against_the_independent_reference():
    rng = random.Random(19)
    sv, st = [], []
    so = StatsOracle(st.append, lambda _l: None, 10, 5, 2, emit_svc=sv.append, svc_percentiles=QS)
    B = 2000
    so.latest = B
    series = []   # (service, samples) in st order: server by server, services in first-seen order
    sizes = [1, 2, 3, 7, 20, 100, 999, 1000, 1001]
    for si, server in enumerate(("s0", "s1", "s2")):
        names = [f"S:{i}" for i in range(len(sizes))]
        if si == 1:
            names.reverse()   # opposite order on the second server
        for name in names:
            n = sizes[int(name[2:])] if si != 2 or int(name[2:]) % 2 else 0
            if n == 0:
                continue
            vals = [rng.choice([rng.randint(-50, 10 ** 6), INT32_MAX, -INT32_MAX, 0]) for _ in range(n)]
            if (si + int(name[2:])) % 3 == 1:
                vals[rng.randrange(n)] = "NaN"
            series.append((name, [NAN if v == "NaN" else v for v in vals]))
            for k, v in enumerate(vals):
                so.consume(tx(server, name, (B - 4 + k % 3) * 10000 + 1, v))
    so.consume(tx("t", "T", (B + 1) * 10000 + 1, 1))   # window [B - 6, B - 1]
    ts = (B + 1 - 2 - 1) * 10000
    want, _ints = R.rows_from_series(ts, series, QS)
    assert sv == want and len(sv) == len(sizes)
    assert [r.split("|")[2] for r in sv] == [f"S:{i}" for i in range(len(sizes))]
    assert {r.split("|")[3] for r in sv} == {"2", "3"}


def test_pipeline_oracle_and_cpu_engine_carry_the_stream():
    C = config.default_config(replay=True)
    assert PipelineOracle(copy.deepcopy(C), UTC).st.emit_svc is None
    C["gpu"]["serviceWindow"] = {"percentiles": [50, 95]}
    P = PipelineOracle(copy.deepcopy(C), UTC)
    assert P.st.emit_svc is not None and P.st.svc_percentiles == [50000, 95000] and P.sv == []
    assert CpuOracleEngine(C).take("sv") == []


# ------------------------------------------------------------------------------- codec, encoders

SV_LINES = ["sv|1578391200000|S:getSvc0001|3|7|1|2040|50:12,99.9:340.5",
            "sv|1578391210000|S:a\tb\\c|2|2|0|-1|0.001:-0.5,50:-1,100:0",
            "sv|1578391220000|S:max|4|3|2|6442450941|50:2147483647,75:2147483646.5,99.999:-2147483647",
            "sv|1578391230000|S:neg|1|2|0|-4294967294|50:-2147483647",
            "sv|1578391240000|S:wide|65|300000000|0|644245094100000000|50:2147483647"]


def test_codec_round_trip_and_pg_row():
    for ln in SV_LINES:
        e = entry_from_csv(ln)
        assert isinstance(e, ServiceWindowEntry) and e.type == "sv" and e.to_csv() == ln
    e = entry_from_csv(SV_LINES[0])
    assert (e.service, e.servers, e.count, e.nan, e.elapsed_sum, e.pcts) == \
        ("S:getSvc0001", 3, 7, 1, 2040, [(50000, 24), (99900, 681)])
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["sv"][1]
    assert row["pcts"] == {"50": 12, "99.9": 340.5} and row["elapsed_sum"] == 2040 and row["servers"] == 3
    assert "sv" in records.RECORD_TYPES and "sv" in sinks.TYPES and sinks.COLUMNS["sv"][0] == "dbSvcTable"
    assert sinks.DEFAULT_TABLES["sv"] == "apm_service_window"
    for bad in ("sv|12|s|x|1|0|5|50:5", "sv|12|s|1|-1|0|5|50:5", "sv|12|s|1|1||5|50:5", "sv|12|s|1|1|0|5.5|50:5",
                "sv|12|s|1|1|0|--5|50:5", "sv|12|s|1|1|0|1234567890123456789|50:5", "sv|12|s|1|1|0", "sv|12|s|1 |1|0|5|50:5"):
        assert entry_from_csv(bad) is None, bad


def test_copy_encode_lines_sv():
    got = sinks.copy_encode_lines(SV_LINES)["sv"]
    assert got[0] == '2020-01-07 10:00:00.000+00\tS:getSvc0001\t3\t7\t1\t2040\t{"50":12,"99.9":340.5}\n'
    assert got[1] == '2020-01-07 10:00:10.000+00\tS:a\\tb\\\\c\t2\t2\t0\t-1\t{"0.001":-0.5,"50":-1,"100":0}\n'
    assert got[2].endswith('\t4\t3\t2\t6442450941\t{"50":2147483647,"75":2147483646.5,"99.999":-2147483647}\n')
    assert got[3].endswith('\t1\t2\t0\t-4294967294\t{"50":-2147483647}\n')
    assert got[4].endswith('\t65\t300000000\t0\t644245094100000000\t{"50":2147483647}\n')   # past 2^53: digits
    for ln, row in zip(SV_LINES, got):
        assert sinks.pg_row_from_copy("sv", row) == entry_from_csv(ln).to_pg_row()


def test_native_copy_encoder_matches_python_for_sv():
    lines = SV_LINES + ["sv|12|b|1|4|1|9|50:4,bad,75:,99.9:2.5,101:1,50.0001:1,90:1.25,095:-0,7.50:3,:5,0:1",
                        "sv|12|b|x|4|1|9|50:4",      # malformed rows: dropped
                        "sv|12|b|1|4|1|9.5|50:4",
                        "sv|12|b|1|4|1",
                        "sv|13|c|1|2|0|-1|50:-0.5"]
    nat = sinks.copy_encode_native(lines)
    if nat is None:
        pytest.skip("native extension not built")
    want = sinks.copy_encode_lines(lines)
    assert len(want["sv"]) == 7
    assert nat["sv"][1] == 7 and nat["sv"][0].decode("utf-8") == "".join(want["sv"])
    assert want["sv"][5].endswith('\tb\t1\t4\t1\t9\t{"50":4,"99.9":2.5,"95":0,"7.5":3}\n')
    assert want["sv"][6].endswith('\tc\t1\t2\t0\t-1\t{"50":-0.5}\n')


# ------------------------------------------------------------------------------- service

def run_service(tmp_path, key):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    if key:
        C["gpu"]["serviceWindow"] = key
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    assert ("sv" in svc.outputs) == bool(key)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_service_spools_the_service_window_table(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    P, on = run_service(tmp_path / "on", {"percentiles": [50, 75, 95, 99]})
    P0, off = run_service(tmp_path / "off", None)
    assert len(P.sv) > 20 and P0.sv == []
    assert all("|50:" in r and ",99:" in r for r in P.sv)
    assert on["apm_service_window.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.sv)["sv"])
    assert [c.strip() for c in on["apm_service_window.columns"].decode().strip().split(",")] == sinks.COLUMNS["sv"][1]
    assert not any(f.startswith("apm_service_window") for f in off)
    assert {f: b for f, b in on.items() if not f.startswith("apm_service_window")} == off and len(off) >= 4
