"""The po stream (peer-outlier servers per service, docs/PEERS.md) on the CPU: the config key, the
class table, the oracle's rows against an independent reference (tests/peers_ref.py), the record
codec, both COPY encoders, the service's route to the table, the reload report, the output-kind
tuples, and the exact verdict of peercmp.h through its binding against Python integers."""
import copy
import os
import random

import pytest

from apmbackend_amd.models.cpu_engine import CpuOracleEngine
from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models.pipeline import WHOLE_OUT_KINDS, EVERY_OUT_KINDS, APMEngine, engine_config, output_mask
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import PeerEntry, entry_from_csv

import peers_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

INT32_MAX = 2 ** 31 - 1
KEY = {"percentile": 95,
       "default": {"minValue": 20},
       "services": {"S:nightlyBatch": None, "S:checkout": {"minValue": 5}},
       "high": 2, "low": 0.25, "z": 3, "minDelta": 10, "minPeers": 5, "minSamples": 20}
PARSED = {"percentile": 95000, "default": 20, "services": {"S:nightlyBatch": None, "S:checkout": 5},
          "high": 2000, "low": 250, "z": 3000, "minDelta": 10, "minPeers": 5, "minSamples": 20}


# ------------------------------------------------------------------------------- config

def test_config_key_accepted_forms():
    assert config.parse_peer_outliers(KEY) == PARSED
    assert config.parse_peer_outliers(None) is None
    # the defaults: percentile 95, z 3, minDelta 0, minPeers 5, minSamples 20; one of high / low is enough
    got = config.parse_peer_outliers({"services": {"a": {"minValue": 1}}, "high": "1.001"})
    assert got == {"percentile": 95000, "default": None, "services": {"a": 1}, "high": 1001, "low": 0, "z": 3000,
                   "minDelta": 0, "minPeers": 5, "minSamples": 20}
    got = config.parse_peer_outliers({"percentile": 99.999, "default": {"minValue": INT32_MAX}, "low": 0.001, "z": 0,
                                      "minDelta": INT32_MAX, "minPeers": 3, "minSamples": 1})
    assert got == {"percentile": 99999, "default": INT32_MAX, "services": {}, "high": 0, "low": 1, "z": 0,
                   "minDelta": INT32_MAX, "minPeers": 3, "minSamples": 1}
    got = config.parse_peer_outliers({"percentile": "0.001", "default": {"minValue": 1}, "high": 1000, "low": 0.999,
                                      "z": 100, "minSamples": INT32_MAX})
    assert (got["percentile"], got["high"], got["low"], got["z"], got["minSamples"]) == (1, 1000000, 999, 100000, INT32_MAX)
    assert config.parse_peer_outliers({"percentile": 100, "default": {"minValue": 1}, "high": 2})["percentile"] == 100000
    # no service with a minValue: the stream is off
    assert config.parse_peer_outliers({"default": None, "services": {"x": None}, "high": 2}) is None
    assert config.parse_peer_outliers({"high": 2}) is None
    C = config.parse_config_text('{"gpu": {"peerOutliers": {"default": {"minValue": 7}, "low": 0.5}}}')
    assert config.peer_outliers(C)["default"] == 7 and config.peer_outliers(C)["low"] == 500
    assert config.peer_outliers({"gpu": {}}) is None and config.peer_outliers({"gpu": {"peerOutliers": None}}) is None
    assert config.gpu_opt({}, "peerQueue") == "peer_outliers"
    for key in ("peerOutliers", "peerQueue"):
        assert key in config.GPU_OPTIONAL and key not in config.GPU_DEFAULTS
        assert key not in config.default_config()["gpu"]
    assert config.GPU_OPTIONAL["peerOutliers"] is None
    config.check_peer_outliers(None)
    config.check_peer_outliers(PARSED)
    with pytest.raises(ValueError):
        config.check_peer_outliers(dict(PARSED, minPeers=2))
    with pytest.raises(ValueError):
        config.check_peer_outliers(dict(PARSED, high=0, low=0))


def test_default_config_text_is_unchanged():
    with open(config.DEFAULT_CONFIG_PATH, encoding="utf-8") as fh:
        txt = fh.read()
    assert "peerOutliers" not in txt and "peerQueue" not in txt and "dbPeerTable" not in txt
    assert "peerOutliers" not in config.read_apm_config(config.DEFAULT_CONFIG_PATH)["gpu"]


O = {"minValue": 5}


def key(**kw):
    k = {"default": dict(O), "high": 2}
    k.update(kw)
    return {a: b for a, b in k.items() if b is not ...}


BAD = [
    [], "x", 5, True, {"default": O}, key(high=...),                                          # neither high nor low
    key(extra=1), key(default={"minValue": 5, "x": 1}), key(default={}), key(default=[5]), key(default=5),
    key(default={"minValue": 0}), key(default={"minValue": -1}), key(default={"minValue": INT32_MAX + 1}),
    key(default={"minValue": True}), key(default={"minValue": 5.0}), key(default={"minValue": "5"}),
    key(default={"minValue": None}),
    key(services=[]), key(services={"a": 5}), key(services={"a": {"minValue": 5.0}}), key(services={"a": {"min": 5}}),
    key(services={1: O}),
    key(percentile=0), key(percentile=100.001), key(percentile=99.9999), key(percentile=True), key(percentile=[95]),
    key(percentile=None), key(percentile="x"), key(percentile=-5), key(percentile=float("nan")),
    key(high=1), key(high=1.0), key(high=1000.001), key(high=2.0001), key(high=True), key(high=None), key(high="x"),
    key(high=0), key(high=float("inf")),
    key(low=0), key(low=1), key(low=0.9999), key(low=-0.5), key(low=True), key(low=None), key(high=..., low=1.5),
    key(z=-1), key(z=100.001), key(z=1.0001), key(z=True), key(z=None), key(z=[3]),
    key(minDelta=-1), key(minDelta=1.0), key(minDelta="1"), key(minDelta=True), key(minDelta=INT32_MAX + 1),
    key(minDelta=None),
    key(minPeers=2), key(minPeers=5.0), key(minPeers="5"), key(minPeers=True), key(minPeers=None),
    key(minPeers=INT32_MAX + 1),
    key(minSamples=0), key(minSamples=20.0), key(minSamples="20"), key(minSamples=True), key(minSamples=None),
    key(minSamples=INT32_MAX + 1),
    # a malformed setting is an error even when no service has a minValue
    {"default": None, "high": 0.5}, {"high": 2, "minPeers": 1},
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_config_key_rejections(i):
    with pytest.raises(ValueError):
        config.parse_peer_outliers(BAD[i])


def test_read_apm_config_stops_on_a_bad_key(tmp_path):
    p = tmp_path / "cfg.json"
    p.write_text('{"gpu": {"peerOutliers": {"default": {"minValue": 5}, "high": 2, "minPeers": 2}}}')
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    p.write_text('{"gpu": {"peerOutliers": {"default": {"minValue": 9}, "high": 2.5}, "peerQueue": "q"}}')
    C = config.read_apm_config(str(p))
    assert config.peer_outliers(C)["default"] == 9 and config.gpu_opt(C, "peerQueue") == "q"
    # ... where an engine is constructed
    C = config.default_config(replay=True)
    C["gpu"]["peerOutliers"] = {"default": {"minValue": 5}, "high": 2, "minPeers": 2}
    with pytest.raises(ValueError):
        PipelineOracle(copy.deepcopy(C), UTC)
    with pytest.raises(ValueError):
        CpuOracleEngine(copy.deepcopy(C))
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "po"))


def test_class_table():
    classes, services, default = config.peer_tables(config.parse_peer_outliers(KEY))
    assert classes == [[], [20], [5]]
    assert services == {"S:nightlyBatch": 0, "S:checkout": 2} and default == 1
    nodef = dict(KEY, default=None)
    classes, services, default = config.peer_tables(config.parse_peer_outliers(nodef))
    assert classes == [[], [5]] and services == {"S:nightlyBatch": 0, "S:checkout": 1} and default == 0
    assert config.peer_tables(None) == ([], {}, 0)
    # the other streams' tables are untouched by the key
    C = config.default_config(replay=True)
    C["gpu"]["peerOutliers"] = copy.deepcopy(KEY)
    e = engine_config(C, outputs=("st", "po"))
    assert e["slo_classes"] == [] and e["sb_classes"] == [] and e["tf_classes"] == [] and e["tf_services"] == {}
    assert e["po_classes"] == [[], [20], [5]] and e["po_services"] == {"S:nightlyBatch": 0, "S:checkout": 2}
    assert (e["po_default"], e["po_pct"], e["po_high"], e["po_low"], e["po_z"]) == (1, 95000, 2000, 250, 3000)
    assert (e["po_min_delta"], e["po_min_peers"], e["po_min_samples"]) == (10, 5, 20)


def test_output_kind_tuples_and_the_key():
    assert WHOLE_OUT_KINDS == EVERY_OUT_KINDS + ("po",) and EVERY_OUT_KINDS[-1] == "tf"
    bit = WHOLE_OUT_KINDS.index("po")
    assert bit == 16 and output_mask(("po",)) == 1 << 16
    assert output_mask(("tf",)) == 1 << 15 and output_mask(("sb", "st")) == (1 << 14) | (1 << 3)   # unchanged
    for i, k in enumerate(EVERY_OUT_KINDS):
        assert output_mask((k,)) == 1 << i
    C = config.default_config(replay=True)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "po"))
    C["gpu"]["peerOutliers"] = copy.deepcopy(KEY)
    assert (engine_config(C, outputs=("st", "po"))["outputs"] >> bit) & 1
    assert not (engine_config(C, keep_text=True)["outputs"] >> bit) & 1   # keep_text alone leaves it off
    d = engine_config(config.default_config(replay=True))
    assert d["po_classes"] == [] and d["po_pct"] == 0 and d["po_high"] == 0 and d["po_low"] == 0


def test_a_reload_that_changes_the_key_needs_a_restart():
    C = config.default_config(replay=True)
    C["gpu"]["peerOutliers"] = copy.deepcopy(KEY)
    old = engine_config(C, outputs=("st", "po"))
    assert APMEngine.restart_required(old, engine_config(copy.deepcopy(C), outputs=())) == []
    C2 = copy.deepcopy(C)
    C2["gpu"]["peerOutliers"]["high"] = 3
    assert APMEngine.restart_required(old, engine_config(C2, outputs=())) == ["po_high"]
    C3 = copy.deepcopy(C)
    C3["gpu"]["peerOutliers"].update({"percentile": 99, "low": 0.5, "z": 1, "minDelta": 0, "minPeers": 3, "minSamples": 5})
    assert APMEngine.restart_required(old, engine_config(C3, outputs=())) == \
        ["po_low", "po_min_delta", "po_min_peers", "po_min_samples", "po_pct", "po_z"]
    C4 = copy.deepcopy(C)
    C4["gpu"]["peerOutliers"]["services"]["S:checkout"]["minValue"] = 40
    assert APMEngine.restart_required(old, engine_config(C4, outputs=())) == ["po_classes"]
    C5 = copy.deepcopy(C)
    del C5["gpu"]["peerOutliers"]
    assert APMEngine.restart_required(old, engine_config(C5, outputs=())) == \
        ["po_classes", "po_default", "po_high", "po_low", "po_min_delta", "po_pct", "po_services"]
    assert not {k for k in old if k.startswith("po_")} & set(APMEngine.LIVE_KEYS)


# ------------------------------------------------------------------------------- oracle

def tx(server, service, end, elapsed):
    return f"tx|{server}|{service}|id|1|{end - 5}|{end}|{elapsed}|Y"


def test_stats_oracle_rows_literal():
    po, st = [], []
    watch = config.parse_peer_outliers({"percentile": 50, "default": {"minValue": 10}, "services": {"off": None},
                                        "high": 2, "low": 0.5, "z": 0, "minPeers": 3, "minSamples": 2})
    so = StatsOracle(st.append, lambda _l: None, 10, 3, 1, emit_peer=po.append, peer=watch)
    B = 1000
    so.latest = B + 1
    t = lambda b, ms=1: b * 10000 + ms

    def feed(server, service, samples):
        for i, v in enumerate(samples):
            so.consume(tx(server, service, t(B - 1 + i % 2), v))

    for srv, v in (("a", 100), ("b", 100), ("c", 110), ("d", 250), ("e", 40)):
        feed(srv, "pay", [v, v, v])                      # medians 100, 100, 110, 250, 40: X2 = 400
    feed("f", "pay", [9999])                             # one sample: below minSamples, no peer
    feed("g", "pay", ["abc", "abc", 9999])               # NaN samples do not count
    for srv in "abcd":
        feed(srv, "off", [1, 1, 900 if srv == "d" else 1])
    feed("a", "few", [10, 10])
    feed("b", "few", [90, 90])                           # two peers: not judged
    assert po == []
    so.consume(tx("z", "t", t(B + 2), 5))
    ts = (B + 2 - 1 - 1) * 10000
    # x = 2 * median; sorted x 80, 200, 200, 220, 500: X2 = 400; d = 0, 0, 40, 240, 600: D4 = 80
    assert po == [f"po|{ts}|d|pay|3|50:500|5|400|80|H", f"po|{ts}|e|pay|3|50:80|5|400|80|L"]
    off = StatsOracle(lambda _l: None, lambda _l: None, 10, 3, 2)
    assert off.emit_peer is None and off.peer is None


def test_oracle_rows_against_the_independent_reference():
    rng = random.Random(23)
    window, buffer = 5, 2
    B = 3000
    labels = list(range(B + 1 - window - buffer, B + 1 - buffer + 1))
    ts = (B + 1 - buffer - 1) * 10000
    sets = [R.Settings(95000, 2000, 250, 3000, 10, 5, 4), R.Settings(50000, 1500, 0, 0, 0, 3, 1),
            R.Settings(99999, 0, 900, 1000, 0, 3, 2), R.Settings(1, 1001, 999, 0, 0, 4, 3)]
    seen = set()
    for S in sets:
        po, st = [], []
        watch = {"percentile": S.q, "default": 3, "services": {"S:none": None, "S:named": 50}, "high": S.r_h, "low": S.r_l,
                 "z": S.z, "minDelta": S.min_delta, "minPeers": S.min_peers, "minSamples": S.min_samples}
        so = StatsOracle(st.append, lambda _l: None, 10, window, buffer, emit_peer=po.append, peer=watch)
        so.latest = B
        sizes = list(range(1, 71, 3)) + [70]
        members = {}
        for g, size in enumerate(sizes):
            service = "S:none" if g == 4 else "S:named" if g == 7 else f"S:g{g}"
            min_value = {"S:none": None, "S:named": 50}.get(service, 3)
            base = rng.choice([-40, 5, 30, 200, 5000])
            tie = rng.random() < 0.4
            for k in range(size):
                server = f"s{k:02d}"
                n = rng.choice([0, 1, S.min_samples - 1, S.min_samples, 6, 9])
                if rng.random() < 0.15:
                    level = base * rng.choice([3, 5]) + 50
                elif rng.random() < 0.1:
                    level = base // 5
                else:
                    level = base if tie else base + rng.randint(-3, 3)
                vals = [level + (0 if tie else rng.randint(-1, 1)) for _ in range(n)]
                vals += [R.NAN] * rng.choice([0, 0, 1])
                rng.shuffle(vals)
                members[(server, service)] = (vals, min_value)
                for i, v in enumerate(vals):
                    so.consume(tx(server, service, labels[i % len(labels)] * 10000 + 1, "abc" if v == R.NAN else v))
                so.consume(tx(server, service, (labels[0] - 1) * 10000 + 1, 77777))    # older than the window
                so.consume(tx(server, service, (labels[-1] + 1) * 10000 + 1, 77777))   # newer than the window
        so.consume(tx("t", "T", (B + 1) * 10000 + 1, 1))
        order = [(l.split("|")[2], l.split("|")[3]) for l in st]
        mem = [(sv, sc) + members[(sv, sc)] for sv, sc in order]
        want, ints = R.rows(ts, mem, S)
        assert po == want and len(po) > 3
        assert not any(r.split("|")[3] == "S:none" for r in po)
        seen |= {v[5] for v in ints if v is not None}
        assert any(v is None for v in ints)
    assert seen == {"H", "L", "N"}


def test_pipeline_oracle_and_cpu_engine_carry_the_stream():
    C = config.default_config(replay=True)
    assert PipelineOracle(copy.deepcopy(C), UTC).st.emit_peer is None
    C["gpu"]["peerOutliers"] = copy.deepcopy(KEY)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    assert P.st.emit_peer is not None and P.st.peer == PARSED
    assert P.po == [] and CpuOracleEngine(C).take("po") == []


# ------------------------------------------------------------------------------- codec, encoders

PO_LINES = ["po|1578391200000|jvm09|S:checkout|310|95:1800|10|160|12|H",
            "po|1578391210000|j\tx|S:a\tb\\c|20|99.9:-7|3|40|0|L",
            "po|1578391220000|jvm01|S:max|2147483647|0.001:4294967294|2147483647|8589934588|68719476735|H",
            "po|1578391230000|jvm02|S:min|1|100:-4294967294|5|-8589934588|0|L"]

MALFORMED = ["po|12|s|v|x|95:1|5|4|0|H", "po|12|s|v|5|95:1|5|4|0|N", "po|12|s|v|5|95:1|5|4|0|h", "po|12|s|v|5|95:1|5|4|0|",
             "po|12|s|v|5|95:1|5|4|0", "po|12|s|v|5|95:1|5|4|0|H|x", "po|12|s|v|5|95|5|4|0|H", "po|12|s|v|5|:1|5|4|0|H",
             "po|12|s|v|5|95:|5|4|0|H", "po|12|s|v|5|95:1.5|5|4|0|H", "po|12|s|v|5|0:1|5|4|0|H", "po|12|s|v|5|100.001:1|5|4|0|H",
             "po|12|s|v|5|95.1234:1|5|4|0|H", "po|12|s|v|5|95:12345678901|5|4|0|H", "po|12|s|v|5|95:--1|5|4|0|H",
             "po|12|s|v|-5|95:1|5|4|0|H", "po|12|s|v|5|95:1|-5|4|0|H", "po|12|s|v|5|95:1|5|4|-1|H",
             "po|12|s|v|5|95:1|5|123456789012|0|H", "po|12|s|v|5|95:1|5|4|123456789012|H", "po|12|s|v|5|95:1|5||0|H",
             "po|12|s|v|5 |95:1|5|4|0|H", "po|12|s|v|5|95:1:2|5|4|0|H", "po|12|s|v|12345678901|95:1|5|4|0|H"]


def test_codec_round_trip_and_pg_row():
    for ln in PO_LINES:
        e = entry_from_csv(ln)
        assert isinstance(e, PeerEntry) and e.type == "po" and e.to_csv() == ln
    e = entry_from_csv(PO_LINES[0])
    assert (e.server, e.service, e.count, e.q, e.value2, e.peers, e.median2x2, e.mad4, e.verdict) == \
        ("jvm09", "S:checkout", 310, 95000, 1800, 10, 160, 12, "H")
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["po"][1]
    assert (row["pct"], row["value2"], row["peers"], row["median2x2"], row["mad4"], row["verdict"]) == ("95", 1800, 10, 160, 12, "H")
    assert "po" in records.RECORD_TYPES and "po" in sinks.TYPES and sinks.COLUMNS["po"][0] == "dbPeerTable"
    assert sinks.DEFAULT_TABLES["po"] == "apm_peer_outlier"
    assert sinks.TYPES.index("tf") == 12 and sinks.TYPES.index("po") == 13
    for bad in MALFORMED:
        assert entry_from_csv(bad) is None, bad


def test_copy_encode_lines_po():
    got = sinks.copy_encode_lines(PO_LINES)["po"]
    assert got[0] == "2020-01-07 10:00:00.000+00\tjvm09\tS:checkout\t310\t95\t1800\t10\t160\t12\tH\n"
    assert got[1] == "2020-01-07 10:00:10.000+00\tj\\tx\tS:a\\tb\\\\c\t20\t99.9\t-7\t3\t40\t0\tL\n"
    assert got[2] == ("2020-01-07 10:00:20.000+00\tjvm01\tS:max\t2147483647\t0.001\t4294967294\t2147483647\t8589934588\t"
                      "68719476735\tH\n")
    assert got[3].endswith("\tS:min\t1\t100\t-4294967294\t5\t-8589934588\t0\tL\n")
    for ln, row in zip(PO_LINES, got):
        assert sinks.pg_row_from_copy("po", row) == entry_from_csv(ln).to_pg_row()


def test_native_copy_encoder_matches_python_for_po():
    lines = PO_LINES + MALFORMED + ["po|13|a|c|0000000005|095.50:-01|03|004|05|L"]
    nat = sinks.copy_encode_native(lines)
    assert nat is not None, "the native extension does not import: build it (a broken build must not pass as a skip)"
    want = sinks.copy_encode_lines(lines)
    assert len(want["po"]) == 5                           # every malformed row is dropped whole
    assert nat["po"][1] == 5 and nat["po"][0].decode("utf-8") == "".join(want["po"])
    assert want["po"][4].endswith("\ta\tc\t5\t95.5\t-1\t3\t4\t5\tL\n")   # parsed and printed again
    assert all(nat[t][1] == 0 for t in nat if t != "po")


# ------------------------------------------------------------------------------- the verdict

def _native():
    from apmbackend_amd import _native as nat
    return nat.load(build_if_missing=False)


def py_verdict(x, X2, D4, E, r_h, r_l, z, min_value, min_delta, min_peers):
    return R.verdict(x, X2, D4, E, R.Settings(0, r_h, r_l, z, min_delta, min_peers, 0), min_value)


def test_peer_verdict_against_python_integers():
    N = _native()

    def V(*a):
        got = N.peer_verdict(*a)
        assert got == py_verdict(*a), a
        return got

    # x, X2, D4, E, r_h, r_l, z, min_value, min_delta, min_peers
    # H: 2000 x >= 2000 X2 -> x >= 100 with X2 = 100; each inequality met exactly and missed by one
    assert V(100, 100, 0, 5, 2000, 0, 0, 1, 0, 5) == "H" and V(99, 100, 0, 5, 2000, 0, 0, 1, 0, 5) == "N"
    # the MAD test: 4000 x >= 2000 * 100 + 3000 * 40 = 320000 -> x >= 80 (the ratio 1.001 passes from x = 51)
    assert V(80, 100, 40, 5, 1001, 0, 3000, 1, 0, 5) == "H" and V(79, 100, 40, 5, 1001, 0, 3000, 1, 0, 5) == "N"
    # the floor: 2 x - X2 >= 4 * 25 -> x >= 100
    assert V(100, 100, 0, 5, 1001, 0, 0, 1, 25, 5) == "H" and V(99, 100, 0, 5, 1001, 0, 0, 1, 25, 5) == "N"
    # L: 2000 x <= 250 * 800 -> x <= 100
    assert V(100, 800, 0, 5, 0, 250, 0, 1, 0, 5) == "L" and V(101, 800, 0, 5, 0, 250, 0, 1, 0, 5) == "N"
    # its MAD test: 4000 x <= 2000 * 800 - 3000 * 400 = 400000 -> x <= 100 (the ratio 0.999 passes up to 399)
    assert V(100, 800, 400, 5, 0, 999, 3000, 1, 0, 5) == "L" and V(101, 800, 400, 5, 0, 999, 3000, 1, 0, 5) == "N"
    # its floor: X2 - 2 x >= 4 * 150 -> x <= 100
    assert V(100, 800, 0, 5, 0, 999, 0, 1, 150, 5) == "L" and V(101, 800, 0, 5, 0, 999, 0, 1, 150, 5) == "N"
    # the gate: X2 >= 4 * minValue, and below it by one
    assert V(1000, 400, 0, 5, 2000, 0, 0, 100, 0, 5) == "H" and V(1000, 399, 0, 5, 2000, 0, 0, 100, 0, 5) == "N"
    # E = minPeers - 1
    assert V(1000, 400, 0, 5, 2000, 0, 0, 1, 0, 5) == "H" and V(1000, 400, 0, 4, 2000, 0, 0, 1, 0, 5) == "N"
    # a negative right-hand side in L: z D4 > 2000 X2; a negative x can still satisfy it, 0 cannot
    assert 2000 * 40 - 100000 * 4 == -320000
    assert V(-80, 40, 4, 5, 0, 999, 100000, 1, 0, 5) == "L" and V(-79, 40, 4, 5, 0, 999, 100000, 1, 0, 5) == "N"
    assert V(0, 40, 4, 5, 0, 999, 100000, 1, 0, 5) == "N"
    # both tests configured: one member above, one below
    assert V(900, 400, 20, 9, 2000, 250, 3000, 20, 10, 5) == "H" and V(40, 400, 20, 9, 2000, 250, 3000, 20, 10, 5) == "L"
    assert V(200, 400, 20, 9, 2000, 250, 3000, 20, 10, 5) == "N"
    # the extremes: x = +-(2^32 - 2), r_h = 10^6, z = 10^5, D4 near 2^36
    XM = 2 ** 32 - 2
    assert V(XM, 8, 0, 5, 1000000, 0, 100000, 1, 0, 5) == "H"                # 2000 XM >= 10^6 * 8
    assert V(XM, 2 * XM, 2 ** 36 - 1, 5, 1000000, 999, 100000, 1, 0, 5) == "N"  # r_h X2 and z D4 near 2^53
    assert V(XM, 8589, 0, 5, 1000000, 0, 0, 1, INT32_MAX, 5) == "N"           # the floor 4 (2^31 - 1) > 2 XM - X2
    assert V(XM, 8589, 0, 5, 1000000, 0, 0, 1, 2 ** 30, 5) == "H"
    # L at x = -(2^32 - 2): 4000 x <= 8000 - 10^5 D4 holds up to D4 = 171798691, and the floor at 2^31 - 1
    assert V(-XM, 4, 171798691, 5, 0, 999, 100000, 1, INT32_MAX, 5) == "L"
    assert V(-XM, 4, 171798692, 5, 0, 999, 100000, 1, INT32_MAX, 5) == "N"
    assert V(-XM, 4, 2 ** 36 - 1, 5, 0, 999, 100000, 1, 0, 5) == "N"          # z D4 near 2^53
    assert V(-XM, 4, 2 ** 36 - 1, 5, 0, 999, 0, 1, 0, 5) == "L" and V(-XM, 4, 2 ** 36 - 1, 4, 0, 999, 0, 1, 0, 5) == "N"
    assert V(XM, 2 ** 33 - 4, 0, 5, 1001, 999, 0, INT32_MAX, 0, 5) == "N"     # X2 = 2^33 - 4 < 4 (2^31 - 1)
    assert V(XM, 2 ** 33 - 4, 0, 5, 1001, 999, 0, 2 ** 31 - 2, 0, 5) == "N"
    assert V(-XM, -(2 ** 33 - 4), 2 ** 35, 5, 1001, 999, 0, 1, 0, 5) == "N"   # a negative median is never judged
    rng = random.Random(5)
    seen = set()
    for _ in range(20000):
        big = rng.random() < 0.3
        X2 = rng.randint(-(2 ** 33) + 1, 2 ** 33 - 1) if big else rng.randint(-50, 4000)
        x = rng.randint(-XM, XM) if big else rng.randint(-100, 6000)
        D4 = rng.randint(0, 2 ** 36 - 1) if big else rng.choice([0, 0, 1, 4, 37, 400, 2000])
        a = (x, X2, D4, rng.randint(0, 9), rng.choice([0, 1001, 1500, 2000, 1000000]), rng.choice([0, 1, 250, 500, 999]),
             rng.choice([0, 1, 3000, 100000]), rng.choice([1, 5, 100, INT32_MAX]), rng.choice([0, 0, 10, 500, INT32_MAX]),
             rng.choice([0, 3, 5]))
        seen.add(V(*a))
    assert seen == {"H", "L", "N"}
    for args in ((2 ** 32, 1, 0, 5, 2000, 0, 0, 1, 0, 5), (1, 2 ** 33, 0, 5, 2000, 0, 0, 1, 0, 5), (1, 1, -1, 5, 2000, 0, 0, 1, 0, 5),
                 (1, 1, 2 ** 36, 5, 2000, 0, 0, 1, 0, 5), (1, 1, 0, 5, 1000, 0, 0, 1, 0, 5), (1, 1, 0, 5, 1000001, 0, 0, 1, 0, 5),
                 (1, 1, 0, 5, 0, 1000, 0, 1, 0, 5), (1, 1, 0, 5, 2000, 0, 100001, 1, 0, 5), (1, 1, 0, 5, 2000, 0, 0, 0, 0, 5),
                 (1, 1, 0, 5, 2000, 0, 0, 1, -1, 5)):
        with pytest.raises(ValueError):
            N.peer_verdict(*args)


def test_kernel_constants():
    N = _native()
    assert N.peer_group_max() == 128   # 32 lanes x PEER_E = 4 members


# ------------------------------------------------------------------------------- service

LOUD = {"percentile": 50, "default": {"minValue": 1}, "services": {"S:none": None}, "high": 1.001, "low": 0.999, "z": 0,
        "minPeers": 3, "minSamples": 1}


def run_service(tmp_path, key):
    C, lines, mapping, sc = make_env(tmp_path, servers=4, duration=200)   # (four peers per service)
    C["streamCalcStats"]["windowSizeInIntervals"] = 6
    if key:
        C["gpu"]["peerOutliers"] = key
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    assert ("po" in svc.outputs) == bool(key)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def test_service_spools_the_peer_table(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    P, on = run_service(tmp_path / "on", copy.deepcopy(LOUD))
    P0, off = run_service(tmp_path / "off", None)
    assert len(P.po) > 5 and P0.po == []
    assert on["apm_peer_outlier.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.po)["po"])
    assert [c.strip() for c in on["apm_peer_outlier.columns"].decode().strip().split(",")] == sinks.COLUMNS["po"][1]
    assert not any(f.startswith("apm_peer_outlier") for f in off)
    # every other table is what a run without the key writes
    assert {f: v for f, v in on.items() if not f.startswith("apm_peer_outlier")} == off


def test_service_rejects_a_bad_key(tmp_path):
    C, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    C["gpu"]["peerOutliers"] = {"default": {"minValue": 5}, "high": 0.5}
    with pytest.raises(ValueError):
        IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
