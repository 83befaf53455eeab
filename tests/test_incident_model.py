"""The ic stream (K25, docs/INCIDENTS.md) on the CPU: the config key, the output tuples, the step
routine through its binding against tests/incident_ref.py, the oracle's rows against the same
reference, the codec and both COPY encoders, the notifier's mail and the service's routing."""
import copy
import os
import random

import pytest

from apmbackend_amd.models.cpu_engine import CpuOracleEngine
from apmbackend_amd.models.oracle import PipelineOracle, StatsOracle
from apmbackend_amd.models import pipeline
from apmbackend_amd.models.pipeline import TOTAL_OUT_KINDS, APMEngine, engine_config, output_mask
from apmbackend_amd.runtime import sinks
from apmbackend_amd.runtime.notifier import AlertNotifier, Mailer
from apmbackend_amd.runtime.service import IngestService
from apmbackend_amd.utils import config, records
from apmbackend_amd.utils.records import IncidentEntry, entry_from_csv

import incident_ref as R
from test_service import UTC, _outbox_in_tmp, feed_in_steps, make_env, srv_of  # noqa: F401 (autouse fixture)

BURN = {"default": {"threshold": 100, "target": 99}, "rules": [{"short": 1, "factor": 1}], "minSamples": 1}
TRAFFIC = {"default": {"minRate": 1}, "rules": [{"short": 1, "drop": 0.5, "surge": 2, "z": 0}], "minBuckets": 3}
PEERS = {"percentile": 95, "default": {"minValue": 20}, "high": 2, "low": 0.25, "z": 3, "minDelta": 10, "minPeers": 5,
         "minSamples": 20}
SHIFT = {"default": {"minDelta": 1}, "rules": [{"short": 1, "percentile": 50, "up": 1.001, "down": 1.001, "z": 0}],
         "minRecent": 1, "minBaseline": 2}
KEY = {"sources": {"sb": {"openAfter": 2, "closeAfter": 6}, "tf": {"openAfter": 3, "closeAfter": 6},
                   "po": {"openAfter": 6, "closeAfter": 6}, "ls": {"openAfter": 2, "closeAfter": 12}},
       "remindEvery": 90, "email": True}


def full_cfg(key=KEY):
    C = config.default_config(replay=True)
    C["gpu"].update({"sloBurn": copy.deepcopy(BURN), "trafficWatch": copy.deepcopy(TRAFFIC),
                     "peerOutliers": copy.deepcopy(PEERS), "latencyShift": copy.deepcopy(SHIFT)})
    if key is not None:
        C["gpu"]["incidents"] = copy.deepcopy(key)
    return C


# ------------------------------------------------------------------------------- config

def test_config_key_accepted_forms():
    assert config.GPU_OPTIONAL["incidents"] is None and config.gpu_opt({}, "incidentQueue") == "incidents"
    assert config.parse_incidents(None) is None and config.incidents(config.default_config(replay=True)) is None
    ic = config.parse_incidents(KEY)
    assert ic == {"sources": {"sb": (2, 6), "tf": (3, 6), "po": (6, 6), "ls": (2, 12)}, "remindEvery": 90, "email": True}
    assert list(ic["sources"]) == ["sb", "tf", "po", "ls"]
    one = config.parse_incidents({"sources": {"ls": {"openAfter": 1, "closeAfter": 255}, "sb": {"openAfter": 255, "closeAfter": 1}}})
    assert one == {"sources": {"sb": (255, 1), "ls": (1, 255)}, "remindEvery": 0, "email": False}   # (the rows' order)
    assert config.parse_incidents({"sources": {"tf": {"openAfter": 1, "closeAfter": 1}}, "remindEvery": 65535})["remindEvery"] == 65535
    assert config.incident_tables(one) == ([255, 0, 0, 1], [1, 0, 0, 255]) and config.incident_tables(None) == ([0] * 4, [0] * 4)


def _src(**kw):
    d = {"openAfter": 2, "closeAfter": 3}
    d.update(kw)
    return d


BAD_KEYS = [
    [], "on", True, {}, {"sources": {}}, {"sources": None}, {"sources": []}, {"sources": {"xx": _src()}},
    {"sources": {"sb": _src(), "al": _src()}}, {"sources": {"sb": None}}, {"sources": {"sb": True}},
    {"sources": {"sb": {"openAfter": 2}}}, {"sources": {"sb": {"closeAfter": 2}}},
    {"sources": {"sb": _src(openAfter=0)}}, {"sources": {"sb": _src(openAfter=256)}}, {"sources": {"sb": _src(closeAfter=0)}},
    {"sources": {"sb": _src(closeAfter=256)}}, {"sources": {"sb": _src(openAfter=True)}}, {"sources": {"sb": _src(openAfter=2.0)}},
    {"sources": {"sb": _src(openAfter="2")}}, {"sources": {"sb": _src(closeAfter=True)}}, {"sources": {"sb": _src(closeAfter=2.0)}},
    {"sources": {"sb": _src(closeAfter="2")}}, {"sources": {"sb": _src(openAfter=-1)}}, {"sources": {"sb": _src(extra=1)}},
    {"sources": {"sb": _src()}, "extra": 1}, {"sources": {"sb": _src()}, "remindEvery": -1},
    {"sources": {"sb": _src()}, "remindEvery": 65536}, {"sources": {"sb": _src()}, "remindEvery": True},
    {"sources": {"sb": _src()}, "remindEvery": 2.0}, {"sources": {"sb": _src()}, "remindEvery": "2"},
    {"sources": {"sb": _src()}, "email": 1}, {"sources": {"sb": _src()}, "email": "true"}, {"sources": {"sb": _src()}, "email": None},
]


@pytest.mark.parametrize("i", range(len(BAD_KEYS)))
def test_config_key_rejections(i):
    with pytest.raises(ValueError):
        config.parse_incidents(BAD_KEYS[i])


def test_a_named_source_needs_its_own_stream(tmp_path):
    for name, gkey in config.INCIDENT_SOURCE_KEYS.items():
        C = full_cfg({"sources": {name: _src()}})
        config.check_incidents(config.incidents(C), C)
        del C["gpu"][gkey]
        with pytest.raises(ValueError):
            config.check_incidents(config.incidents(C), C)
        with pytest.raises(ValueError):
            PipelineOracle(copy.deepcopy(C), UTC)
        with pytest.raises(ValueError):
            APMEngine(C, outputs=("st",))          # (raised before the native extension is touched)
    # ... when the config is loaded
    import json
    C = {"gpu": {"incidents": {"sources": {"sb": _src()}}}}
    p = tmp_path / "c.json"
    p.write_text(json.dumps(C))
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    C["gpu"]["incidents"] = {"sources": {"sb": _src(openAfter="2")}}
    p.write_text(json.dumps(C))
    with pytest.raises(ValueError):
        config.read_apm_config(str(p))
    C["gpu"]["incidents"] = {"sources": {"sb": _src()}}
    C["gpu"]["sloBurn"] = BURN
    p.write_text(json.dumps(C))
    assert config.read_apm_config(str(p))["gpu"]["incidents"] == {"sources": {"sb": _src()}}
    # ... and when the service starts
    Cs, _lines, mapping, _sc = make_env(tmp_path, duration=20)
    Cs["gpu"]["incidents"] = {"sources": {"tf": _src()}}
    with pytest.raises(ValueError):
        IngestService(Cs, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)


# ------------------------------------------------------------------------------- tuples, outputs

def test_tuples():
    P = pipeline
    assert TOTAL_OUT_KINDS == P.COMPLETE_OUT_KINDS + ("ic",) and TOTAL_OUT_KINDS.index("ic") == 18
    assert output_mask(("ic",)) == 1 << 18 and output_mask(("ls", "st")) == (1 << 17) | (1 << 3)
    # every older tuple is what it was
    assert P.COMPLETE_OUT_KINDS == P.WHOLE_OUT_KINDS + ("ls",) and P.WHOLE_OUT_KINDS == P.EVERY_OUT_KINDS + ("po",)
    assert P.EVERY_OUT_KINDS == P.FULL_OUT_KINDS + ("tf",) and P.FULL_OUT_KINDS == P.STREAM_OUT_KINDS + ("sb",)
    assert P.STREAM_OUT_KINDS == P.DEVICE_OUT_KINDS + ("rw",) and P.DEVICE_OUT_KINDS == P.NATIVE_OUT_KINDS + ("sv",)
    assert P.NATIVE_OUT_KINDS == P.ENGINE_OUT_KINDS + ("tk",) and P.ENGINE_OUT_KINDS == P.ALL_OUT_KINDS + ("sl",)
    assert P.ALL_OUT_KINDS == P.OUT_KINDS + ("wp",) and P.OUT_KINDS[-1] == "lh" and len(P.OUT_KINDS) == 9
    assert "ic" not in P.KEEP_TEXT_KINDS
    assert records.RECORD_TYPES[-2:] == ("ls", "ic") and sinks.TYPES[-2:] == ("ls", "ic")
    assert records.RECORD_TYPES.index("po") == 14 and sinks.TYPES.index("po") == 13


def test_outputs_naming_ic():
    C = full_cfg(None)
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "sb", "tf", "po", "ls", "ic"))           # "ic" without the key
    C = full_cfg({"sources": {"sb": _src(), "ls": _src()}, "remindEvery": 7})
    e = engine_config(C, outputs=("st", "sb", "ls", "ic"))
    assert (e["outputs"] >> 18) & 1
    assert e["ic_open_after"] == [2, 0, 0, 2] and e["ic_close_after"] == [3, 0, 0, 3] and e["ic_remind_every"] == 7
    with pytest.raises(ValueError):
        engine_config(C, outputs=("st", "sb", "ic"))                              # source ls is not in outputs
    assert not (engine_config(C, keep_text=True)["outputs"] >> 18) & 1            # keep_text alone leaves it off
    d = engine_config(config.default_config(replay=True))
    assert d["ic_open_after"] == [0] * 4 and d["ic_close_after"] == [0] * 4 and d["ic_remind_every"] == 0
    # a reload lists the settings among those that need a restart
    C2 = copy.deepcopy(C)
    C2["gpu"]["incidents"]["remindEvery"] = 8
    C2["gpu"]["incidents"]["sources"]["sb"]["closeAfter"] = 4
    assert APMEngine.restart_required(e, engine_config(C2, outputs=())) == ["ic_close_after", "ic_remind_every"]
    assert not {k for k in e if k.startswith("ic_")} & set(APMEngine.LIVE_KEYS)


# ------------------------------------------------------------------------------- the step

def _native():
    from apmbackend_amd import _native as nat
    return nat.load(build_if_missing=False)


def as_tuple(st):
    return (st["code0"], st["since"], st["age"], st["hot_run"], st["clear_run"])


def check_sequence(N, codes, oa, ca, remind, st=None, t0=1000):
    """codes: this rollover's code per step ("" = clear).  The binding against the reference, state
    and row at every step."""
    ref = st or R.new_state()
    dev = as_tuple(ref)
    for i, code in enumerate(codes):
        ts = t0 + 10 * i
        want = R.step(ref, code, ts, oa, ca, remind)
        dev, ev, code0, run = N.incident_step(dev, code != "", code, ts, oa, ca, remind)
        assert dev == as_tuple(ref), (i, code, oa, ca, remind)
        if want is None:
            assert ev == ""
        else:
            assert (ev, code0, run) == (want[0], want[1], want[5]) and (dev[1], dev[2]) == (want[3], want[4])
    return ref


def test_step_exhaustive_small_thresholds_and_saturation():
    N = _native()
    pats = []
    for first, second in (("B", "B"), ("U", "D"), ("H", "L")):
        pats.append([first] * 150 + [second] * 150 + [""] * 300)        # both runs pass 255 and saturate
        pats.append([first if i % 2 == 0 else "" for i in range(600)])
        pats.append([(first if i % 3 else second) if (i // 2) % 2 == 0 else "" for i in range(600)])
        pats.append([""] * 260 + [first, "", first, second] + [second] * 336)
    for oa in (1, 2, 255):
        for ca in (1, 2, 255):
            for remind in (0, 1, 7):
                for p in pats:
                    assert len(p) == 600
                    ref = check_sequence(N, p, oa, ca, remind)
                    assert ref["hot_run"] <= 255 and ref["clear_run"] <= 255
    # the thresholds at 255 are reached: the run saturates there, not below
    ref = check_sequence(N, ["B"] * 300, 255, 255, 0)
    assert ref["code0"] == "B" and ref["hot_run"] == 255 and ref["age"] == 300 - 255 and ref["since"] == 1000 + 10 * 254
    ref = check_sequence(N, [""] * 300, 255, 255, 0, st=ref)
    assert ref["code0"] == "" and ref["clear_run"] == 255


def test_step_age_saturates_and_reminders():
    N = _native()
    for age in (2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1):
        for remind in (0, 1, 65535):
            st = {"code0": "U", "since": 5, "age": age, "hot_run": 9, "clear_run": 0}
            ref = check_sequence(N, ["U", "D", "", "U", ""], 2, 3, remind, st=st)
            assert ref["age"] == 2 ** 32 - 1 and ref["code0"] == "U"
    # 2^32 - 1 = 65535 * 65537: the saturated age is a reminder step of remindEvery 65535, at every rollover
    st = {"code0": "B", "since": 5, "age": 2 ** 32 - 1, "hot_run": 1, "clear_run": 0}
    assert R.step(dict(st), "B", 77, 1, 1, 65535)[0] == "S"
    assert N.incident_step(as_tuple(st), True, "B", 77, 1, 1, 65535)[1] == "S"
    # remindEvery: 0 never, 1 at every open rollover, 65535 at the 65535th
    for remind, want in ((0, 0), (1, 40), (65535, 0)):
        ref, n = R.new_state(), 0
        dev = as_tuple(ref)
        for i in range(41):
            row = R.step(ref, "S", i, 1, 1, remind)
            dev, ev, _c, _r = N.incident_step(dev, True, "S", i, 1, 1, remind)
            n += ev == "S"
            assert (row[0] if row else "") == ev
        assert n == want
    st = {"code0": "B", "since": 5, "age": 65534, "hot_run": 1, "clear_run": 0}
    assert N.incident_step(as_tuple(st), True, "B", 77, 1, 1, 65535)[1] == "S"
    for bad in ((("BB", 0, 0, 0, 0), True, "B", 0, 1, 1, 0), (("", 0, 2 ** 32, 0, 0), True, "B", 0, 1, 1, 0),
                (("", 0, 0, 256, 0), True, "B", 0, 1, 1, 0), (("", 0, 0, 0, 0), True, "B", 0, 0, 1, 0),
                (("", 0, 0, 0, 0), True, "B", 0, 1, 256, 0), (("", 0, 0, 0, 0), True, "B", 0, 1, 1, 65536),
                (("", 0, 0, 0, 0), True, "", 0, 1, 1, 0)):
        with pytest.raises(ValueError):
            N.incident_step(*bad)


def test_step_random_sequences():
    N = _native()
    rng = random.Random(25)
    for _ in range(4000):
        oa, ca = rng.choice((1, 2, 3, 6, 12, 255)), rng.choice((1, 2, 3, 6, 12, 255))
        remind = rng.choice((0, 1, 2, 5, 90))
        letters = rng.choice(("B", "DS", "HL", "UD"))
        p_hot = rng.choice((0.1, 0.5, 0.9))
        codes, hot = [], False
        for _i in range(rng.randrange(1, 60)):
            if rng.random() < 0.3:
                hot = rng.random() < p_hot
            codes.append(rng.choice(letters) if hot else "")
        check_sequence(N, codes, oa, ca, remind, t0=rng.randrange(0, 2 ** 41))


# ------------------------------------------------------------------------------- oracle

def test_oracle_rows_against_the_reference():
    rng = random.Random(7)
    key = {"sources": {"sb": (2, 3), "tf": (1, 2), "po": (3, 1), "ls": (2, 2)}, "remindEvery": 3, "email": False}
    S = StatsOracle(lambda r: None, lambda r: None, emit_incident=lambda r: None, incident=key)
    book = R.Book(key["sources"], 3)
    series = [(f"jvm{i:02d}", f"S:svc{j}") for i in range(3) for j in range(4)]
    letters = {"sb": "B", "tf": "DS", "po": "HL", "ls": "UD"}
    n_rows = 0
    for step in range(80):
        ts = 1578391200000 + 10000 * step
        live = series[:4 + step // 4]   # series appear over time
        codes = {}
        for k in live:
            codes[k] = {s: (rng.choice(letters[s]) if rng.random() < 0.45 else "") for s in R.SOURCES}
        from collections import OrderedDict
        got = S.incident_rows(ts, OrderedDict((k, codes[k]) for k in live))
        want = book.step_all(ts, [(k, k[0], k[1], codes[k]) for k in live])
        assert got == want
        n_rows += len(got)
        for r in got:
            assert entry_from_csv(r).to_csv() == r
    assert n_rows > 100
    # the code of a source from its stream's row
    assert StatsOracle.incident_code("sb", None) == "" and StatsOracle.incident_code("sb", "sb|1|a|b|1|1|1|1|0|1:1:1:1:1") == "B"
    assert StatsOracle.incident_code("tf", "tf|1|a|b|9|3|1:4:0:6:0:N,3:4:20:6:0:S") == "S"
    assert StatsOracle.incident_code("tf", "tf|1|a|b|9|3|1:4:0:6:0:D,3:4:20:6:0:S") == "D"
    assert StatsOracle.incident_code("ls", "ls|1|a|b|5|5|1:50:3:4:5:6:1:2:N,2:50:3:4:5:6:1:2:D") == "D"
    assert StatsOracle.incident_code("po", "po|1|a|b|30|95:200|6|100|20|L") == "L"


def test_pipeline_oracle_and_cpu_engine_carry_the_stream():
    C = full_cfg(None)
    assert PipelineOracle(copy.deepcopy(C), UTC).st.emit_incident is None
    C = full_cfg()
    P = PipelineOracle(copy.deepcopy(C), UTC)
    assert P.st.emit_incident is not None and P.st.incident["sources"]["ls"] == (2, 12)
    assert P.ic == [] and CpuOracleEngine(C).take("ic") == []


# ------------------------------------------------------------------------------- codec, encoders

IC_LINES = ["ic|1578391200000|jvm00|S:checkout|sb|O|B|B|1578391200000|0|2",
            "ic|1578391260000|j\tx|S:a\tb\\c|tf|C|D|-|1578391200000|6|6",
            "ic|1578391270000|jvm01|S:max|ls|S|U|D|0|4294967295|255",
            "ic|1578391280000|jvm01|S:max|po|S|H|L|253402300799999|90|1"]

MALFORMED = ["ic|12|s|v|sb|O|B|B|5|0", "ic|12|s|v|sb|O|B|B|5|0|2|x", "ic|12|s|v|al|O|B|B|5|0|2", "ic|12|s|v|SB|O|B|B|5|0|2",
             "ic|12|s|v|sb|X|B|B|5|0|2", "ic|12|s|v|sb|o|B|B|5|0|2", "ic|12|s|v|sb||B|B|5|0|2", "ic|12|s|v|sb|O|-|B|5|0|2",
             "ic|12|s|v|sb|O|N|B|5|0|2", "ic|12|s|v|sb|O|BB|B|5|0|2", "ic|12|s|v|sb|O||B|5|0|2", "ic|12|s|v|sb|O|B|N|5|0|2",
             "ic|12|s|v|sb|O|B||5|0|2", "ic|12|s|v|sb|O|B|--|5|0|2", "ic|12|s|v|sb|O|B|B|-5|0|2", "ic|12|s|v|sb|O|B|B||0|2",
             "ic|12|s|v|sb|O|B|B|5.0|0|2", "ic|12|s|v|sb|O|B|B|1234567890123456|0|2", "ic|12|s|v|sb|O|B|B|253402300800000|0|2",
             "ic|12|s|v|sb|O|B|B|5|-1|2", "ic|12|s|v|sb|O|B|B|5||2", "ic|12|s|v|sb|O|B|B|5|12345678901|2",
             "ic|12|s|v|sb|O|B|B|5|0|", "ic|12|s|v|sb|O|B|B|5|0|1000", "ic|12|s|v|sb|O|B|B|5|0|2 ", "ic|12|s|v|sb|O|B|B|5|0|x",
             "ic|12|s|v|sb|O|B|B| 5|0|2"]


def test_codec_round_trip_and_pg_row():
    for ln in IC_LINES:
        e = entry_from_csv(ln)
        assert isinstance(e, IncidentEntry) and e.type == "ic" and e.to_csv() == ln
    e = entry_from_csv(IC_LINES[1])
    assert (e.server, e.service, e.source, e.event, e.code0, e.code, e.since, e.age, e.run) == \
        ("j\tx", "S:a\tb\\c", "tf", "C", "D", "-", 1578391200000, 6, 6)
    row = e.to_pg_row()
    assert list(row) == sinks.COLUMNS["ic"][1] == ["timestamp", "server", "service", "source", "event", "code0", "code",
                                                   "since", "age", "run"]
    assert sinks.COLUMNS["ic"][0] == "dbIncidentTable" and sinks.DEFAULT_TABLES["ic"] == "apm_incident"
    for bad in MALFORMED:
        assert entry_from_csv(bad) is None, bad


def test_copy_encoders_agree():
    got = sinks.copy_encode_lines(IC_LINES)["ic"]
    assert got[0] == "2020-01-07 10:00:00.000+00\tjvm00\tS:checkout\tsb\tO\tB\tB\t2020-01-07 10:00:00.000+00\t0\t2\n"
    assert got[1] == "2020-01-07 10:01:00.000+00\tj\\tx\tS:a\\tb\\\\c\ttf\tC\tD\t-\t2020-01-07 10:00:00.000+00\t6\t6\n"
    assert got[2].endswith("\tls\tS\tU\tD\t1970-01-01 00:00:00.000+00\t4294967295\t255\n")
    assert got[3].endswith("\tpo\tS\tH\tL\t9999-12-31 23:59:59.999+00\t90\t1\n")
    for ln, row in zip(IC_LINES, got):
        assert sinks.pg_row_from_copy("ic", row) == entry_from_csv(ln).to_pg_row()
    lines = IC_LINES + MALFORMED + ["ic|13|a|c|ls|C|D|U|0000000005|01|002"]
    nat = sinks.copy_encode_native(lines)
    assert nat is not None, "the native extension does not import: build it (a broken build must not pass as a skip)"
    want = sinks.copy_encode_lines(lines)
    assert len(want["ic"]) == 5                           # every malformed row is dropped whole
    assert nat["ic"][1] == 5 and nat["ic"][0].decode("utf-8") == "".join(want["ic"])
    assert want["ic"][4].endswith("\ta\tc\tls\tC\tD\tU\t1970-01-01 00:00:00.005+00\t1\t2\n")
    assert all(nat[t][1] == 0 for t in nat if t != "ic")


# ------------------------------------------------------------------------------- notifier

AL_LINE = None


def _notifier(tmp_path):
    C = config.default_config(replay=True)
    C["streamProcessAlerts"].update({"alertCollectionIntervalInSeconds": 10, "emailsEnabled": True,
                                     "sendTestEmailOnStart": False})
    now = [1000.0]
    m = Mailer(sendmail="/nonexistent/sendmail", outbox=str(tmp_path / "outbox"))
    n = AlertNotifier(C, mailer=m, clock=lambda: now[0], renderer=lambda url, g: (_ for _ in ()).throw(RuntimeError("no grafana")))
    return n, m, now


def _alert_lines():
    """al rows of a short oracle run with a planted slow service."""
    from apmbackend_amd.utils.synth import Anomaly, Generator, SynthConfig, batches, with_watermarks
    C = config.default_config(replay=True)
    C["streamCalcZScore"]["defaults"] = [{"LAG": 6, "THRESHOLD": 3.0, "INFLUENCE": 0.5}]
    C["streamProcessAlerts"]["rollingAlertWindowSizeInIntervals"] = 5
    C["streamProcessAlerts"]["requiredNumberBadIntervalsInAlertWindowToTrigger"] = 2
    start = 1578391200000
    cfg = SynthConfig(servers=2, duration_s=400, tx_per_sec_per_server=5, seed=7,
                      anomalies=[Anomaly("jvm00", "getSvc0001", start + 150_000, start + 400_000, 30.0)])
    P = PipelineOracle(C, UTC)
    P.run_batches(with_watermarks(batches(Generator(cfg).generate(), cfg.start_ms, 10.0), UTC))
    assert P.al
    return P.al[:2]


def _html(msg):
    return msg.get_payload()[0].get_payload(decode=True).decode("utf-8")


def test_notifier_mail(tmp_path):
    al = _alert_lines()
    # without incidents the body and the subject are today's
    n0, m0, now0 = _notifier(tmp_path / "a")
    n0.add_lines(al)
    now0[0] += 11
    assert n0.tick() and m0.sent[0]["Subject"] == "APM Alerts Triggered!"
    plain = _html(m0.sent[0])
    assert "Incidents" not in plain
    # with incidents: the block stands behind the alert table, O and C rows only
    n1, m1, now1 = _notifier(tmp_path / "b")
    n1.add_lines(al)
    n1.add_incident_lines(IC_LINES + MALFORMED + [""])
    assert [e.event for e in n1.incidents] == ["O", "C"]
    now1[0] += 11
    assert n1.tick() and m1.sent[0]["Subject"] == "APM Alerts Triggered!"
    body = _html(m1.sent[0])
    table_end = plain.index("</table>") + len("</table>")
    assert body[:table_end] == plain[:table_end] and body[table_end:].startswith("<pre>\n<b>Incidents</b>\n")
    block = body[table_end:body.index("</pre>", table_end)]
    assert body[:table_end] + body[table_end + len(block) + len("</pre>"):] == plain   # nothing else changed
    lines = block.split("\n")[2:-1]
    assert len(lines) == 2
    assert "jvm00  S:checkout  sb  opened  B" in lines[0] and "after" not in lines[0]
    assert "tf  closed  D  after 1.0 minutes" in lines[1]
    assert n1.incidents == [] and n1.buffer == []
    # incidents only
    n2, m2, now2 = _notifier(tmp_path / "c")
    n2.add_incident_lines(IC_LINES[:1])
    now2[0] += 11
    assert n2.tick() and m2.sent[0]["Subject"] == "APM Incidents"
    only = _html(m2.sent[0])
    assert "<b>Incidents</b>" in only and "<table>" not in only and "opened  B" in only
    now2[0] += 11
    assert not n2.tick()                                   # nothing buffered: no mail


# ------------------------------------------------------------------------------- service

LOUD_IC = {"sources": {"ls": {"openAfter": 1, "closeAfter": 1}, "tf": {"openAfter": 1, "closeAfter": 2}}, "remindEvery": 2,
           "email": True}


def run_service(tmp_path, key):
    C, lines, mapping, sc = make_env(tmp_path, duration=200)
    C["streamCalcStats"]["windowSizeInIntervals"] = 6   # (a window the 20 buckets of the run fill)
    C["gpu"]["latencyShift"] = copy.deepcopy(SHIFT)
    C["gpu"]["trafficWatch"] = copy.deepcopy(TRAFFIC)
    if key:
        C["gpu"]["incidents"] = key
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                        server_of_path=srv_of)
    assert ("ic" in svc.outputs) == bool(key) and svc.ic_email == bool(key)   # (LOUD_IC sets email)
    P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
    assert svc.notifier is not None        # (rank 0 of a world of 1 has one)
    buffered, add = [], svc.notifier.add_incident_lines

    def record(lines_):                    # every line the service hands the notifier, and what it kept of them
        before = len(svc.notifier.incidents)
        add(lines_)
        buffered.extend(svc.notifier.incidents[before:])
    svc.notifier.add_incident_lines = record
    feed_in_steps(svc, lines, mapping, sc, P)
    svc.shutdown()
    d = tmp_path / "copy"
    return P, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}, buffered


def test_service_spools_the_incident_table_and_leaves_the_others(tmp_path):
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    P, on, buffered = run_service(tmp_path / "on", copy.deepcopy(LOUD_IC))
    P0, off, _b = run_service(tmp_path / "off", None)
    events = [r.split("|")[5] for r in P.ic]
    assert events.count("O") > 2 and events.count("C") > 2 and P0.ic == []
    assert on["apm_incident.copy"].decode("utf-8") == "".join(sinks.copy_encode_lines(P.ic)["ic"])
    assert [c.strip() for c in on["apm_incident.columns"].decode().strip().split(",")] == sinks.COLUMNS["ic"][1]
    assert not any(f.startswith("apm_incident") for f in off)
    # every other table is what a run without the key writes
    assert {f: v for f, v in on.items() if not f.startswith("apm_incident")} == off
    # ... and so is every other stream of the CPU engine
    for k in ("stats", "fs", "al", "tx_db", "lh", "wp", "sl", "tk", "sv", "rw", "sb", "tf", "po", "ls"):
        assert getattr(P, k) == getattr(P0, k), k
    # the O and C rows reached the notifier (email: true), every one of them, the reminders did not
    assert events.count("S") > 0
    assert [e.to_csv() for e in buffered] == [r for r in P.ic if r.split("|")[5] in ("O", "C")] and buffered
    # ... and with email: false none does
    quiet = copy.deepcopy(LOUD_IC)
    quiet["email"] = False
    (tmp_path / "quiet").mkdir()
    C, lines, mapping, sc = make_env(tmp_path / "quiet", duration=60)
    C["gpu"].update({"latencyShift": copy.deepcopy(SHIFT), "trafficWatch": copy.deepcopy(TRAFFIC), "incidents": quiet})
    svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
    assert "ic" in svc.outputs and svc.ic_email is False
    svc.shutdown()


def test_service_routes_the_queue(tmp_path):
    """amqp mode against the in-process broker: the ic rows go to gpu.incidentQueue (default
    `incidents`, or the name the config gives), one message a row, and to no other queue."""
    from apmbackend_amd.runtime.amqp_broker import Broker
    C0, _lines, _mapping, _sc = make_env(tmp_path, duration=20)
    assert config.gpu_opt(C0, "incidentQueue") == "incidents" and sinks.COLUMNS["ic"][0] == "dbIncidentTable"
    for sub, qname in (("a", None), ("b", "my_incidents")):
        (tmp_path / sub).mkdir()
        b = Broker(port=0).start()
        try:
            C, lines, mapping, sc = make_env(tmp_path / sub, mode="amqp", duration=200)
            C["amqpConnectionString"] = b.url
            C["streamCalcStats"]["windowSizeInIntervals"] = 6
            C["gpu"].update({"latencyShift": copy.deepcopy(SHIFT), "trafficWatch": copy.deepcopy(TRAFFIC),
                             "incidents": copy.deepcopy(LOUD_IC)})
            if qname:
                C["gpu"]["incidentQueue"] = qname
            svc = IngestService(C, engine="cpu-oracle", files=sorted(mapping.values()), rank=0, world=1,
                                server_of_path=srv_of)
            assert "incidents" in svc.producers
            P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
            feed_in_steps(svc, lines, mapping, sc, P)
            svc.shutdown()
            st = b.stats()
            assert len(P.ic) > 5 and st[qname or "incidents"]["messages"] == len(P.ic)
            assert ("incidents" in st) == (qname is None)
            assert st["latency_shift"]["messages"] == len(P.ls) and st["traffic"]["messages"] == len(P.tf)
        finally:
            b.stop()
