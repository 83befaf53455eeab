"""The tk stream (per-rollover top-K series leaderboards, docs/LEADERBOARD.md) on the CPU: the
config object, the oracle's and the CPU engine's rows against an independent reference
(tests/topk_ref.py), the record codec, both COPY encoders, the service's routes to the table and to
the queue, and the restart-required report of a reload."""
import copy
import os

import pytest

from apmbackend_amd.models.cpu_engine import CpuOracleEngine
from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models.pipeline import (ALL_OUT_KINDS, ENGINE_OUT_KINDS, NATIVE_OUT_KINDS, OUT_KINDS, APMEngine,
                                            engine_config, output_mask)
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.amqp_broker import Broker
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import LeaderboardEntry, entry_from_csv

import topk_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

BOARD = {"k": 20, "by": ["per95", "average", "tpm"], "minTpm": 0}


# ------------------------------------------------------------------------------- config

def test_config_object_is_parsed():
    assert config.parse_leaderboard(BOARD) == {"k": 20, "by": ["per95", "average", "tpm"], "minTpm": 0.0}
    assert config.parse_leaderboard({"k": 1, "by": ["tpm"]}) == {"k": 1, "by": ["tpm"], "minTpm": 0.0}
    assert config.parse_leaderboard({"k": 128, "by": ["tpm", "average", "per75", "per95"], "minTpm": 2.5}) == \
        {"k": 128, "by": ["tpm", "average", "per75", "per95"], "minTpm": 2.5}
    assert config.parse_leaderboard(None) is None
    C = config.parse_config_text('{"gpu": {"leaderboard": {"k": 3, "by": ["per75"], "minTpm": 1}}}')
    assert config.leaderboard(C) == {"k": 3, "by": ["per75"], "minTpm": 1.0}
    assert config.gpu_opt({}, "topQueue") == "leaderboard" and config.gpu_opt({}, "leaderboard") is None
    for key in ("leaderboard", "topQueue"):
        assert key in config.GPU_OPTIONAL and key not in config.GPU_DEFAULTS


@pytest.mark.parametrize("bad", [
    {"k": 0, "by": ["tpm"]}, {"k": 129, "by": ["tpm"]}, {"k": True, "by": ["tpm"]}, {"k": 20.0, "by": ["tpm"]},
    {"k": "20", "by": ["tpm"]}, {"k": -1, "by": ["tpm"]}, {"by": ["tpm"]}, {"k": 20},
    {"k": 20, "by": ["tpm", "tpm"]}, {"k": 20, "by": ["p95"]}, {"k": 20, "by": []}, {"k": 20, "by": "tpm"},
    {"k": 20, "by": ["tpm", "average", "per75", "per95", "tpm"]}, {"k": 20, "by": [0]},
    {"k": 20, "by": ["tpm"], "minTpm": -1}, {"k": 20, "by": ["tpm"], "minTpm": float("nan")},
    {"k": 20, "by": ["tpm"], "minTpm": float("inf")}, {"k": 20, "by": ["tpm"], "minTpm": "0"},
    {"k": 20, "by": ["tpm"], "minTpm": True}, {"k": 20, "by": ["tpm"], "extra": 1},
    [20], "tpm", 20, True, {}])
def test_bad_objects_raise(bad):
    with pytest.raises(ValueError):
        config.parse_leaderboard(bad)
    C = config.default_config(replay=True)
    C["gpu"]["leaderboard"] = bad
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st",))


def test_default_config_text_is_unchanged_and_bad_files_do_not_load(tmp_path):
    D = config.default_config()
    assert "leaderboard" not in D["gpu"] and "topQueue" not in D["gpu"]
    assert "dbTopTable" not in D["streamInsertDb"]
    assert config.leaderboard(D) is None
    p = tmp_path / "cfg.json"
    p.write_text('{"gpu": {"leaderboard": {"k": 0, "by": ["tpm"]}}}')
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    p.write_text('{"gpu": {"leaderboard": {"k": 20.0, "by": ["tpm"]}}}')
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    p.write_text('{"gpu": {"leaderboard": {"k": 5, "by": ["per95", "tpm"]}, "topQueue": "q"}}')
    C = config.read_apm_config(str(p))
    assert config.leaderboard(C) == {"k": 5, "by": ["per95", "tpm"], "minTpm": 0.0} and config.gpu_opt(C, "topQueue") == "q"
    p.write_text('{"gpu": {"leaderboard": null}}')
    assert config.leaderboard(config.read_apm_config(str(p))) is None


def test_engine_settings_and_outputs():
    # the tuples earlier tests pin are as they were; the new one continues the enum
    assert OUT_KINDS == ("transactions", "audit_db", "db", "st", "fs", "al", "sx", "fb", "lh")
    assert ALL_OUT_KINDS == OUT_KINDS + ("wp",) and ENGINE_OUT_KINDS == ALL_OUT_KINDS + ("sl",)
    assert NATIVE_OUT_KINDS == ENGINE_OUT_KINDS + ("tk",) and NATIVE_OUT_KINDS[-1] == "tk"
    bit = NATIVE_OUT_KINDS.index("tk")
    assert bit == 11 and output_mask(("tk",)) == 1 << 11 and output_mask(("sl", "st")) == (1 << 10) | (1 << 3)
    C = config.default_config(replay=True)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "tk"))      # "tk" without the key
    e = engine_config(C, outputs=("st",))
    assert e["tk_k"] is None and e["tk_by"] == [] and e["tk_min_tpm"] == 0.0
    C["gpu"]["leaderboard"] = copy.deepcopy(BOARD)
    e = engine_config(C, outputs=("st", "tk"))
    assert (e["outputs"] >> bit) & 1
    assert e["tk_k"] == 20 and e["tk_by"] == [3, 1, 0] and e["tk_min_tpm"] == 0.0
    assert not (engine_config(C, keep_text=True)["outputs"] >> bit) & 1  # keep_text alone leaves it off
    C["gpu"]["leaderboard"] = None
    with pytest.raises(ValueError):
        engine_config(C, outputs=("tk",))


def test_a_reload_that_changes_the_leaderboard_needs_a_restart():
    C = config.default_config(replay=True)
    C["gpu"]["leaderboard"] = copy.deepcopy(BOARD)
    old = engine_config(C, outputs=("st", "tk"))
    assert APMEngine.restart_required(old, engine_config(copy.deepcopy(C), outputs=())) == []
    C2 = copy.deepcopy(C)
    C2["gpu"]["leaderboard"]["k"] = 21
    assert APMEngine.restart_required(old, engine_config(C2, outputs=())) == ["tk_k"]
    C3 = copy.deepcopy(C)
    C3["gpu"]["leaderboard"]["by"] = ["per95", "tpm"]
    C3["gpu"]["leaderboard"]["minTpm"] = 1
    assert APMEngine.restart_required(old, engine_config(C3, outputs=())) == ["tk_by", "tk_min_tpm"]
    C4 = copy.deepcopy(C)
    del C4["gpu"]["leaderboard"]
    assert APMEngine.restart_required(old, engine_config(C4, outputs=())) == ["tk_by", "tk_k"]
    assert not set(APMEngine.LIVE_KEYS) & {"tk_k", "tk_by", "tk_min_tpm"}


# ------------------------------------------------------------------------------- oracle, CPU engine

def tx(server, service, end, elapsed):
    return f"tx|{server}|{service}|id|1|{end - 5}|{end}|{elapsed}|Y"


def test_stats_oracle_rows_literal():
    tk, st = [], []
    board = config.parse_leaderboard({"k": 2, "by": ["average", "tpm"], "minTpm": 2.0})
    so = StatsOracle(st.append, lambda _l: None, 10, 3, 1, emit_top=tk.append, board=board)
    B = 1000
    so.latest = B
    t = lambda b, ms=1: b * 10000 + ms
    for ln in (tx("a", "x", t(B), 100), tx("a", "x", t(B), 300),           # average 200, tpm 4.00
               tx("a", "n", t(B), "abc"), tx("a", "n", t(B), "zz"),        # only NaN: no average
               tx("a", "lone", t(B), 900),                                 # tpm 2.00, average 900
               tx("b", "y", t(B), 200), tx("b", "y", t(B - 1), 200),       # average 200 again: a tie, later in st order
               tx("b", "z", t(B), 50), tx("b", "z", t(B), 50), tx("b", "z", t(B), 50)):
        so.consume(ln)
    assert tk == []
    so.consume(tx("c", "t", t(B + 2), 5))   # rollover to B + 2: window [B - 2, B + 1]; tpm = n / (3 * 10 / 60) = 2 n
    ts = (B + 2 - 1 - 1) * 10000
    assert [l.split("|")[3] for l in st] == ["x", "n", "lone", "y", "z"]
    assert tk == R.rows_from_st(st, 2, ["average", "tpm"], 2.0)
    assert tk == [f"tk|{ts}|average|1|a|lone|2.00|900.0|900.0|900.0",
                  f"tk|{ts}|average|2|a|x|4.00|200.0|300.0|300.0",
                  f"tk|{ts}|tpm|1|b|z|6.00|50.0|50.0|50.0",
                  f"tk|{ts}|tpm|2|a|x|4.00|200.0|300.0|300.0"]
    quiet = StatsOracle(lambda _l: None, lambda _l: None, 10, 3, 2)   # off by default
    assert quiet.emit_top is None and quiet.board is None


def lines_of(bl_item):
    return [ln for _fp, ls in bl_item[1] for ln in ls]


def test_oracle_and_cpu_engine_rows_against_the_independent_reference(tmp_path):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    C["gpu"]["leaderboard"] = {"k": 3, "by": ["per95", "tpm", "average", "per75"], "minTpm": 1.0}
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    eng = CpuOracleEngine(copy.deepcopy(C))
    svc = IngestService(copy.deepcopy(C), engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    assert len(P.tk) > 40 and len({l.split("|")[4] for l in P.stats}) >= 2   # a multi-server run
    # per rollover: the rows follow from the st rows of the same timestamp alone
    by_ts = {}
    for r in P.stats:
        by_ts.setdefault(r.split("|")[1], []).append(r)
    want = []
    for ts, rows in by_ts.items():
        want += R.rows_from_st(rows, 3, ["per95", "tpm", "average", "per75"], 1.0)
    assert P.tk == want
    assert any(float(r.split("|")[4]) < 1.0 for r in P.stats), "minTpm cuts nothing in this run"
    assert svc.native.P.tk == P.tk and svc.native._taken["tk"] == len(P.tk)   # the service's CpuOracleEngine
    assert "tk" in eng._taken and eng.take("tk") == []


# ------------------------------------------------------------------------------- codec, encoders

TK_LINES = ["tk|1578391200000|per95|1|jvm00|S:getSvc0001|12.50|101.5|120.0|190.3",
            "tk|1578391210000|tpm|128|jvm\\01|S:a\tb|0.25|0.0|0.0|0.0",
            "tk|1578391220000|average|7|jvm02|S:x|3.00|Infinity|NaN|-Infinity",
            "tk|1578391220000|per75|20|jvm02|S:y|3.00|-0.5|undefined|7.0"]
MALFORMED = ["tk|12|p95|1|a|b|1.00|1.0|1.0|1.0",      # unknown key
             "tk|12||1|a|b|1.00|1.0|1.0|1.0",
             "tk|12|tpm|0|a|b|1.00|1.0|1.0|1.0",      # rank outside 1 .. 128
             "tk|12|tpm|129|a|b|1.00|1.0|1.0|1.0",
             "tk|12|tpm|1000|a|b|1.00|1.0|1.0|1.0",   # more than three digits
             "tk|12|tpm|0001|a|b|1.00|1.0|1.0|1.0",
             "tk|12|tpm|+1|a|b|1.00|1.0|1.0|1.0",
             "tk|12|tpm|1.0|a|b|1.00|1.0|1.0|1.0",
             "tk|12|tpm| 1|a|b|1.00|1.0|1.0|1.0",
             "tk|12|tpm||a|b|1.00|1.0|1.0|1.0",
             "tk|12|tpm",
             "tk|12"]
SHORT = ["tk|12|tpm|001|a|b|1.00|1.0", "tk|12|tpm|5|a", "tk|x|per95|12|a|b|z|1.0|2.0|3.0"]   # kept: missing fields are NULL


def test_codec_round_trip_and_pg_row():
    for ln in TK_LINES[:2]:
        e = entry_from_csv(ln)
        assert isinstance(e, LeaderboardEntry) and e.type == "tk" and e.to_csv() == ln
    e = entry_from_csv(TK_LINES[0])
    assert (e.board, e.rank, e.server, e.service, e.tpm, e.average, e.per75, e.per95) == \
        ("per95", 1, "jvm00", "S:getSvc0001", 12.5, 101.5, 120.0, 190.3)
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["tk"][1] and row["rank"] == 1 and row["per95"] == 190.3
    assert sinks.COLUMNS["tk"] == ("dbTopTable", ["timestamp", "board", "rank", "server", "service", "tpm", "average",
                                                  "per75", "per95"])
    assert "tk" in records.RECORD_TYPES and "tk" in sinks.TYPES and sinks.DEFAULT_TABLES["tk"] == "apm_leaderboard"
    for ln in MALFORMED:
        assert entry_from_csv(ln) is None, ln
    assert entry_from_csv(SHORT[0]).rank == 1


def test_copy_encode_lines_tk():
    got = sinks.copy_encode_lines(TK_LINES)["tk"]
    assert got[0] == "2020-01-07 10:00:00.000+00\tper95\t1\tjvm00\tS:getSvc0001\t12.5\t101.5\t120\t190.3\n"
    assert got[1] == "2020-01-07 10:00:10.000+00\ttpm\t128\tjvm\\\\01\tS:a\\tb\t0.25\t0\t0\t0\n"
    # numbers that are not finite are NULL, as the fs row's are
    assert got[2] == "2020-01-07 10:00:20.000+00\taverage\t7\tjvm02\tS:x\t3\t\\N\t\\N\t\\N\n"
    assert got[3] == "2020-01-07 10:00:20.000+00\tper75\t20\tjvm02\tS:y\t3\t-0.5\t\\N\t7\n"
    assert sinks.pg_row_from_copy("tk", got[0]) == entry_from_csv(TK_LINES[0]).to_pg_row()
    assert sinks.copy_encode_lines(MALFORMED)["tk"] == []


def test_native_copy_encoder_matches_python_for_tk():
    lines = TK_LINES + MALFORMED + SHORT
    nat = sinks.copy_encode_native(lines)
    if nat is None:
        pytest.skip("native extension not built")
    want = sinks.copy_encode_lines(lines)
    assert len(want["tk"]) == len(TK_LINES) + len(SHORT)
    assert nat["tk"][1] == len(want["tk"]) and nat["tk"][0].decode("utf-8") == "".join(want["tk"])


# ------------------------------------------------------------------------------- service

def run_service(tmp_path, board, extra=None):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    if board:
        C["gpu"]["leaderboard"] = board
    for k, v in (extra or {}).items():
        C["streamInsertDb"][k] = v
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return svc, P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_service_spools_the_leaderboard_table(tmp_path):
    for d in ("on", "off", "named"):
        (tmp_path / d).mkdir()
    svc, P, on = run_service(tmp_path / "on", {"k": 5, "by": ["per95", "tpm"]})
    svc0, P0, off = run_service(tmp_path / "off", None)
    assert "tk" in svc.outputs and svc.outputs[-1] == "tk" and "tk" not in svc0.outputs
    assert len(P.tk) > 20 and P0.tk == []
    assert on["apm_leaderboard.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.tk)["tk"])
    assert [c.strip() for c in on["apm_leaderboard.columns"].decode().strip().split(",")] == sinks.COLUMNS["tk"][1]
    assert not any(f.startswith("apm_leaderboard") for f in off)
    assert {f: b for f, b in on.items() if not f.startswith("apm_leaderboard")} == off and len(off) >= 4
    _s, _p, named = run_service(tmp_path / "named", {"k": 5, "by": ["per95", "tpm"]}, {"dbTopTable": "top_rows"})
    assert named["top_rows.copy"] == on["apm_leaderboard.copy"] and "apm_leaderboard.copy" not in named


def test_service_amqp_mode_publishes_to_the_leaderboard_queue(tmp_path):
    b = Broker(port=0).start()
    try:
        C, lines, mapping, sc = make_env(tmp_path, mode="amqp", duration=200)
        C["amqpConnectionString"] = b.url
        C["gpu"]["leaderboard"] = {"k": 5, "by": ["average"]}
        C["gpu"]["topQueue"] = "top_rows"
        svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                            server_of_path=srv_of)
        assert "tk" in svc.outputs
        P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
        feed_in_steps(svc, lines, mapping, sc, P)
        svc.shutdown()
        st = b.stats()
        assert len(P.tk) > 20 and 20 < st["top_rows"]["messages"] <= len(P.tk)
        assert st["db_insert"]["messages"] > 0 and "leaderboard" not in st
    finally:
        b.stop()


def test_service_rejects_a_bad_object(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C["gpu"]["leaderboard"] = {"k": 129, "by": ["tpm"]}
    with pytest.raises(ValueError):
        IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
