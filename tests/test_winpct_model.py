"""The wp stream (exact window percentiles, docs/PERCENTILES.md) on the CPU: the config list, the
integer rank rule, the oracle's rows against an independent reference (tests/winpct_ref.py), the
record codec, both COPY encoders and the service's routes to the table and to the queue."""
import copy
import os
import random

import pytest

from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models.pipeline import engine_config
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.amqp_broker import Broker
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import WindowPctEntry, entry_from_csv, half_text, pct_ranks, pct_text

import winpct_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

INT32_MAX = 2 ** 31 - 1
QS = [1, 1000, 50000, 75000, 95000, 99900, 99999, 100000]


# ------------------------------------------------------------------------------- texts, config

def test_canonical_percentile_text():
    assert [pct_text(q) for q in (1, 500, 50000, 99900, 99999, 100000)] == ["0.001", "0.5", "50", "99.9", "99.999", "100"]
    assert [pct_text(q) for q in (1, 500, 50000, 99900, 99999, 100000)] == [R.label(q) for q in (1, 500, 50000, 99900, 99999, 100000)]


def test_half_text():
    assert [half_text(v) for v in (-1, 0, 1, 2, -2, -3, 2 * INT32_MAX, INT32_MAX + INT32_MAX - 1)] == \
        ["-0.5", "0", "0.5", "1", "-1", "-1.5", "2147483647", "2147483646.5"]
    for v in list(range(-9, 10)) + [2 * INT32_MAX, -2 * INT32_MAX + 1, 4294967293]:
        assert half_text(v) == R.half(v)


def test_config_list_is_parsed_without_a_float_round_trip():
    assert config.parse_window_percentiles([50, 90, 99, 99.9]) == [50000, 90000, 99000, 99900]
    assert config.parse_window_percentiles(["0.001", 1, "99.999", 100]) == [1, 1000, 99999, 100000]
    assert config.parse_window_percentiles([0.07, 0.29, 0.57, 1.1, 8.2]) == [70, 290, 570, 1100, 8200]
    assert config.parse_window_percentiles([]) == [] and config.parse_window_percentiles(None) == []
    C = config.parse_config_text('{"gpu": {"windowPercentiles": [50, 99.9, 99.99]}}')
    assert config.window_percentiles(C) == [50000, 99900, 99990]
    assert config.window_percentiles({"gpu": {}}) == []
    assert config.gpu_opt({}, "pctQueue") == "window_pct"
    assert "windowPercentiles" in config.GPU_OPTIONAL and "windowPercentiles" not in config.GPU_DEFAULTS
    assert "windowPercentiles" not in config.default_config()["gpu"]


@pytest.mark.parametrize("bad", [[0], [100.001], [50.0001], [99, 50], [50, 50], [1, 2, 3, 4, 5, 6, 7, 8, 9],
                                 [-1], ["abc"], [True], 50, "50", [float("nan")], [None]])
def test_config_validation_raises(bad):
    with pytest.raises(ValueError):
        config.parse_window_percentiles(bad)
    C = config.default_config(replay=True)
    C["gpu"]["windowPercentiles"] = bad
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st",))


def test_outputs_naming_wp_needs_a_list(tmp_path):
    C = config.default_config(replay=True)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "wp"))
    C["gpu"]["windowPercentiles"] = []
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "wp"))
    C["gpu"]["windowPercentiles"] = [50, 99.9]
    e = engine_config(C, outputs=("st", "wp"))
    assert e["win_pcts"] == [50000, 99900] and (e["outputs"] >> 9) & 1
    assert not (engine_config(C, keep_text=True)["outputs"] >> 9) & 1  # keep_text alone leaves it off
    # a config file with a bad list does not load
    p = tmp_path / "cfg.json"
    p.write_text('{"gpu": {"windowPercentiles": [99, 50]}}')
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    p.write_text('{"gpu": {"windowPercentiles": [50, 99.9], "pctQueue": "q"}}')
    assert config.window_percentiles(config.read_apm_config(str(p))) == [50000, 99900]


# ------------------------------------------------------------------------------- rank rule

def test_integer_rank_rule_against_fractions():
    for q in QS:
        for m in range(1, 3001):
            assert pct_ranks(m, q) == R.frac_ranks(m, q), (m, q)


def test_rank_rule_properties():
    for q in QS:
        for m in (1, 2, 3, 999, 1000, 1001, 2000, 100000, 200000):
            lo, hi = pct_ranks(m, q)
            assert 0 <= lo <= hi <= m - 1 and hi - lo <= 1
    # the double formula K8 uses reads the neighbouring rank here; the integer rule must not
    assert pct_ranks(1000, 99900) == (998, 998) and pct_ranks(2000, 99900) == (1997, 1997)
    # for the reference's own percentiles the two agree
    from apmbackend_amd.models import oracle
    for p in (50, 75, 90, 95, 99):
        for n in list(range(1, 600)) + [1000, 4096, 16385, 200000]:
            arr = list(range(n))
            v = oracle.calc_percentile(arr, p)
            lo, hi = pct_ranks(n, p * 1000)
            assert v * 2 == arr[lo] + arr[hi], (p, n)


# ------------------------------------------------------------------------------- oracle

def tx(server, service, end, elapsed):
    return f"tx|{server}|{service}|id|1|{end - 5}|{end}|{elapsed}|Y"


def test_stats_oracle_rows_literal():
    wp, st = [], []
    so = StatsOracle(st.append, lambda _l: None, 10, 3, 1, emit_pct=wp.append, percentiles=[1000, 50000, 99900])
    B = 1000
    so.latest = B
    t = lambda b, ms=1: b * 10000 + ms
    for ln in (tx("a", "x", t(B), -1), tx("a", "x", t(B), 0),
               tx("a", "n", t(B), "abc"), tx("a", "n", t(B), "zz"),        # only NaN: st row, no wp row
               tx("b", "y", t(B), 7), tx("b", "y", t(B), "abc"),           # m == 1 with a NaN
               tx("b", "z", t(B - 1), INT32_MAX), tx("b", "z", t(B), INT32_MAX)):
        so.consume(ln)
    assert wp == []
    so.consume(tx("c", "t", t(B + 2), 5))   # rollover to B + 2: window [B - 2, B + 1]
    ts = (B + 2 - 1 - 1) * 10000
    # two samples: below 50 the index is not integral and not the last -> the pair's mean; 50 reads
    # rank 0; above 50 the ceiling is the last sample
    assert wp == [f"wp|{ts}|a|x|2|0|1:-0.5,50:-1,99.9:0",
                  f"wp|{ts}|b|y|1|1|1:7,50:7,99.9:7",
                  f"wp|{ts}|b|z|2|0|1:2147483647,50:2147483647,99.9:2147483647"]
    assert [l.split("|")[3] for l in st] == ["x", "n", "y", "z"]
    # off by default
    quiet = StatsOracle(lambda _l: None, lambda _l: None, 10, 3, 2)
    assert quiet.emit_pct is None and quiet.percentiles == []


def test_oracle_rows_against_the_independent_reference():
    rng = random.Random(16)
    wp, st = [], []
    so = StatsOracle(st.append, lambda _l: None, 10, 5, 2, emit_pct=wp.append, percentiles=QS)
    B = 2000
    so.latest = B
    data = {}
    for i, n in enumerate([1, 2, 3, 7, 20, 100, 999, 1000, 1001, 2000]):
        vals = [rng.choice([rng.randint(-50, 10 ** 6), INT32_MAX, -INT32_MAX, 0]) for _ in range(n)]
        if i % 3 == 1:
            vals[rng.randrange(n)] = "NaN"
        data[("s", f"S:{i}")] = vals
        for k, v in enumerate(vals):
            so.consume(tx("s", f"S:{i}", (B - 4 + k % 3) * 10000 + 1, v))
    so.consume(tx("t", "T", (B + 1) * 10000 + 1, 1))   # window [B - 6, B - 1]
    ts = (B + 1 - 2 - 1) * 10000
    want = [R.row(ts, k[0], k[1], [R.ELAPSED_NAN if v == "NaN" else v for v in vals], QS) for k, vals in data.items()]
    assert wp == want and len(wp) == 10


# ------------------------------------------------------------------------------- codec, encoders

WP_LINES = ["wp|1578391200000|jvm00|S:getSvc0001|7|1|50:12,99.9:340.5",
            "wp|1578391210000|jvm\\01|S:a\tb|2|0|0.001:-0.5,50:-1,100:0",
            "wp|1578391220000|jvm02|S:max|3|2|50:2147483647,75:2147483646.5,99.999:-2147483647"]


def test_codec_round_trip_and_pg_row():
    for ln in WP_LINES:
        e = entry_from_csv(ln)
        assert isinstance(e, WindowPctEntry) and e.type == "wp" and e.to_csv() == ln
    e = entry_from_csv(WP_LINES[0])
    assert (e.count, e.nan, e.pcts) == (7, 1, [(50000, 24), (99900, 681)])
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["wp"][1] and row["pcts"] == {"50": 12, "99.9": 340.5}
    assert "wp" in records.RECORD_TYPES and "wp" in sinks.TYPES and sinks.COLUMNS["wp"][0] == "dbPctTable"
    assert sinks.DEFAULT_TABLES["wp"] == "apm_window_pct"
    e = WindowPctEntry(12, "a", "b", 2, 0, [(1, -1), (100000, 2 * INT32_MAX)])
    assert e.to_csv() == "wp|12|a|b|2|0|0.001:-0.5,100:2147483647"


def test_copy_encode_lines_wp():
    got = sinks.copy_encode_lines(WP_LINES)["wp"]
    assert got[0] == '2020-01-07 10:00:00.000+00\tjvm00\tS:getSvc0001\t7\t1\t{"50":12,"99.9":340.5}\n'
    assert got[1] == '2020-01-07 10:00:10.000+00\tjvm\\\\01\tS:a\\tb\t2\t0\t{"0.001":-0.5,"50":-1,"100":0}\n'
    assert got[2].endswith('\t3\t2\t{"50":2147483647,"75":2147483646.5,"99.999":-2147483647}\n')
    assert sinks.pg_row_from_copy("wp", got[0]) == entry_from_csv(WP_LINES[0]).to_pg_row()


def test_native_copy_encoder_matches_python_for_wp():
    lines = WP_LINES + ["wp|12|a|b|x|1|50:4,bad,75:,99.9:2.5,101:1,50.0001:1,90:1.25,095:-0,7.50:3,:5,0:1"]
    nat = sinks.copy_encode_native(lines)
    if nat is None:
        pytest.skip("native extension not built")
    want = sinks.copy_encode_lines(lines)
    assert nat["wp"][1] == 4 and nat["wp"][0].decode("utf-8") == "".join(want["wp"])
    assert want["wp"][3].endswith('\t\\N\t1\t{"50":4,"99.9":2.5,"95":0,"7.5":3}\n')


# ------------------------------------------------------------------------------- service

def run_service(tmp_path, pcts):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    if pcts:
        C["gpu"]["windowPercentiles"] = pcts
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_service_spools_the_percentile_table(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    P, on = run_service(tmp_path / "on", [50, 90, 99, 99.9])
    P0, off = run_service(tmp_path / "off", None)
    assert len(P.wp) > 20 and P0.wp == []
    assert all("|50:" in r and ",99.9:" in r for r in P.wp)
    assert on["apm_window_pct.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.wp)["wp"])
    assert [c.strip() for c in on["apm_window_pct.columns"].decode().strip().split(",")] == sinks.COLUMNS["wp"][1]
    assert not any(f.startswith("apm_window_pct") for f in off)
    assert {f: b for f, b in on.items() if not f.startswith("apm_window_pct")} == off and len(off) >= 4


def test_service_amqp_mode_publishes_to_the_percentile_queue(tmp_path):
    b = Broker(port=0).start()
    try:
        C, lines, mapping, sc = make_env(tmp_path, mode="amqp", duration=200)
        C["amqpConnectionString"] = b.url
        C["gpu"]["windowPercentiles"] = [50, 99.9]
        C["gpu"]["pctQueue"] = "pct_rows"
        svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                            server_of_path=srv_of)
        P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
        feed_in_steps(svc, lines, mapping, sc, P)
        svc.shutdown()
        st = b.stats()
        assert len(P.wp) > 20 and 20 < st["pct_rows"]["messages"] <= len(P.wp)
        assert st["db_insert"]["messages"] > 0 and "window_pct" not in st
    finally:
        b.stop()


def test_service_rejects_a_bad_list(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C["gpu"]["windowPercentiles"] = [99, 50]
    with pytest.raises(ValueError):
        IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
