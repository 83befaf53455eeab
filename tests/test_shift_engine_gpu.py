"""The ls stream through the whole engine: parse -> device join -> K7 -> K8 -> K24, against
PipelineOracle over several rollovers, record for record, with one server whose calls of one
service are slowed mid-run (the synthetic load's planted anomaly: the generator stretches that
server's calls of the service thirtyfold from the cut on); the other streams unchanged by it; no
text, no record and no metric while it is off.  (Shapes of tests/test_peers_engine_gpu.py.)"""
import collections
import copy

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import COMPLETE_OUT_KINDS, WHOLE_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.utils.records import entry_from_csv  # noqa: E402
from apmbackend_amd.utils.synth import Anomaly, Generator, SynthConfig, batches, with_watermarks  # noqa: E402

from test_hist_engine_gpu import KINDS, START, UTC, run, small_cfg  # noqa: E402

# a window of 13 buckets that the run fills: at 3 tx a second and 7 services a series gets about four
# samples a bucket, so three recent buckets hold about a dozen and the other ten about forty
KEY = {"default": {"minDelta": 20}, "services": {"S:getSvc0003": None},
       "rules": [{"short": 3, "percentile": 75, "up": 2, "z": 3}, {"short": 3, "percentile": 25, "down": 2}],
       "minRecent": 8, "minBaseline": 25}
SLOW_SERVER, SLOW = "jvm02", "getSvc0001"


def ls_cfg(key=KEY):
    C = small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 12
    C["gpu"]["latencyShift"] = copy.deepcopy(key)
    return C


def plain_cfg():
    C = small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 12
    return C


def load(seed=1, duration=300, servers=3, frac=0.6):
    """(batches, cut): from frac * duration on, SLOW_SERVER's calls of SLOW take thirty times as long."""
    cut = START + int(duration * 1000 * frac)
    an = [Anomaly(SLOW_SERVER, SLOW, cut, START + int(duration * 1000) + 1, 30.0)]
    cfg = SynthConfig(servers=servers, duration_s=duration, tx_per_sec_per_server=3, seed=seed,
                      ejb_services=4, provider_services=3, anomalies=an)
    lines = Generator(cfg).generate()
    return with_watermarks(batches(lines, cfg.start_ms, 5.0), UTC), cut


def test_stream_is_opt_in():
    assert COMPLETE_OUT_KINDS == WHOLE_OUT_KINDS + ("ls",)
    eng = APMEngine(ls_cfg(), keep_text=True)   # the key in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> COMPLETE_OUT_KINDS.index("ls")) & 1
    assert eng.eng.shifts() == [] and eng.metrics()["ls_rows"] == 0
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "ls"))   # "ls" without the key
    bad = ls_cfg()
    bad["gpu"]["latencyShift"]["rules"][0]["short"] = 13   # above windowSizeInIntervals
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "ls"))
    # the native constructor checks what it is handed as well
    N = _native.load()
    ecfg = engine_config(ls_cfg(), outputs=("st", "ls"))
    for over in ({"ls_classes": []}, {"ls_classes": [[]]}, {"ls_classes": [[], [5, 1]]}, {"ls_classes": [[], [0]]},
                 {"ls_classes": [[], [2 ** 30]]}, {"ls_classes": [[5]]}, {"ls_default": 7}, {"ls_services": {"x": 9}},
                 {"ls_short": [3, 2]}, {"ls_short": [3, 13]}, {"ls_short": [0, 3]}, {"ls_pct": [75000, 75000]},
                 {"ls_pct": [75000, 100000]}, {"ls_pct": [0, 25000]}, {"ls_up": [1000, 0]}, {"ls_up": [0, 0]},
                 {"ls_down": [0, 1000001]}, {"ls_z": [100001, 3000]}, {"ls_z": [-1, 3000]}, {"ls_min_recent": 0},
                 {"ls_min_baseline": 1}, {"ls_short": [3]}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **over))


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    bl, cut = load(seed=1, duration=300)
    C = ls_cfg()
    kinds = KINDS + ("ls",)
    eng, on = run(C, bl, kinds, kinds=kinds)
    off_eng, off = run(plain_cfg(), bl, KINDS, kinds=KINDS + ("ls",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    rows = [r.split("|") for r in P.ls]
    slow = [f for f in rows if f[2] == SLOW_SERVER and f[3] == "S:" + SLOW]
    # the slowed series prints U rows once the slow calls fill its newest buckets, none before the cut
    assert len(slow) >= 2 and all("U" in [g.split(":")[8] for g in f[6].split(",")] for f in slow)
    assert all(int(f[1]) >= cut - 10_000 for f in slow)
    # a steady series prints none: the same service on the other servers
    assert not any(f[3] == "S:" + SLOW and f[2] != SLOW_SERVER and "U" in f[6] for f in rows)
    assert not any(f[3] == "S:getSvc0003" for f in rows)
    assert len(P.ls) < len(P.stats) // 4
    # record for record
    assert len(on["ls"]) == len(P.ls)
    for got, want in zip(on["ls"], P.ls):
        assert got == want and entry_from_csv(got) == entry_from_csv(want)
    assert eng.metrics()["ls_rows"] == len(P.ls)
    # stream off: no text, no record, no metric
    assert off["ls"] == [] and off_eng.eng.shifts() == [] and off_eng.metrics()["ls_rows"] == 0
    # with the stream on, every other stream's bytes are those of a run with it off
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # rows stand in st order with the st rows' timestamps
    st_keys = [tuple(l.split("|")[1:4]) for l in on["st"]]
    ls_keys = [tuple(r.split("|")[1:4]) for r in on["ls"]]
    have = set(ls_keys)
    assert len(have) == len(ls_keys) and ls_keys == [k for k in st_keys if k in have]
    # the read-back holds the last rollover's records per series id, for series that did not fire too
    dev = eng.eng.shifts()
    assert any(d is None for d in dev)                       # S:getSvc0003: class 0
    recs = [d for d in dev if d is not None]
    last_ts = on["st"][-1].split("|")[1]
    fired = sum(1 for r in on["ls"] if r.split("|")[1] == last_ts)
    assert sum(1 for d in recs if any(p[8] != "N" for p in d[1])) == fired
    assert any(all(p[8] == "N" for p in d[1]) for d in recs)
