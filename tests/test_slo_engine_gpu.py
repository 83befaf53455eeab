"""The sl stream through the whole engine: parse -> device join -> K7 -> K8 -> K17, against
PipelineOracle over several rollovers; with lh and wp on as well; the other streams unchanged by
it; services that appear late; the engine's resources returned.  (Shapes of
tests/test_winpct_engine_gpu.py.)"""
import collections
import copy
import gc

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import ALL_OUT_KINDS, ENGINE_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from test_hist_engine_gpu import KINDS, UTC, run, small_cfg, synth_batches  # noqa: E402

OBJ = {"default": [500, 2000], "services": {"S:getSvc0001": [200, 800, 3200], "S:getSvc0002": []}}


def slo_cfg(lh=False, wp=False, obj=OBJ):
    C = small_cfg()
    C["gpu"]["latencyObjectives"] = copy.deepcopy(obj)
    if lh:
        C["gpu"]["latencyHistogram"] = True
    if wp:
        C["gpu"]["windowPercentiles"] = [50, 90, 99, 99.9]
    return C


def test_stream_is_opt_in():
    assert ENGINE_OUT_KINDS == ALL_OUT_KINDS + ("sl",)
    eng = APMEngine(slo_cfg(), keep_text=True)   # objectives in the config alone do not start it
    assert not (eng.ecfg["outputs"] >> ENGINE_OUT_KINDS.index("sl")) & 1
    assert eng.eng.slo_counts() == []
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "sl"))
    bad = small_cfg()
    bad["gpu"]["latencyObjectives"] = {"default": [2000, 500]}
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "sl"))
    # the native constructor checks the tables it is handed as well
    N = _native.load()
    ecfg = engine_config(slo_cfg(), outputs=("st", "sl"))
    for tabs in ({"slo_classes": []}, {"slo_classes": [[]]}, {"slo_classes": [[5], [6]]},
                 {"slo_classes": [[], [2000, 500]]}, {"slo_classes": [[], [5, 5]]}, {"slo_classes": [[], [-1]]},
                 {"slo_classes": [[], [2 ** 31]]}, {"slo_classes": [[], list(range(9))]}, {"slo_classes": [[], []]},
                 {"slo_default": 3}, {"slo_default": -1}, {"slo_services": {"S:a": 3}}, {"slo_services": {"S:a": -1}}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **tabs))


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    _lines, bl = synth_batches(seed=1, duration=300)
    C = slo_cfg()
    kinds = KINDS + ("sl",)
    _e, on = run(C, bl, kinds, kinds=kinds)
    _e, off = run(small_cfg(), bl, KINDS, kinds=KINDS + ("sl",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert len(P.sl) > 100
    assert on["sl"] == P.sl
    assert off["sl"] == []
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # one row per st row whose window holds a sample and whose service has a threshold, in st
    # order, with its timestamp
    st_keys = [tuple(l.split("|")[1:4]) for l in on["st"]
               if l.split("|")[5] != "undefined" and l.split("|")[3] != "S:getSvc0002"]
    assert [tuple(l.split("|")[1:4]) for l in on["sl"]] == st_keys
    for l in on["sl"]:
        f = l.split("|")
        labels = [p.split(":")[0] for p in f[6].split(",")]
        assert labels == (["200", "800", "3200"] if f[3] == "S:getSvc0001" else ["500", "2000"])
    assert any(l.split("|")[3] == "S:getSvc0001" for l in on["sl"])


def test_services_that_appear_after_the_first_rollover_get_their_class():
    _lines, bl = synth_batches(seed=4, duration=300)
    late = {"S:getSvc0001", "S:getSvc0002", "S:getSvc0003"}
    cut = len(bl) // 3

    def keep(ls, i):
        return [l for l in ls if i >= cut or not any(s[2:] in l for s in late)]

    bl = [(now, [(fp, keep(ls, i)) for fp, ls in chunks]) for i, (now, chunks) in enumerate(bl)]
    obj = {"services": {"S:getSvc0001": [200, 800, 3200], "S:getSvc0003": [1000], "S:getSvc0002": []}}
    C = slo_cfg(obj=obj)
    kinds = KINDS + ("sl",)
    _e, on = run(C, bl, kinds, kinds=kinds)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert on["st"] == P.stats and on["sl"] == P.sl
    named = {l.split("|")[3] for l in on["sl"]}
    assert "S:getSvc0001" in named and named <= {"S:getSvc0001", "S:getSvc0003"}
    first = min(int(l.split("|")[1]) for l in on["sl"])
    assert first > min(int(l.split("|")[1]) for l in on["st"])   # rollovers went by before they appeared


def test_with_the_histogram_and_percentile_streams_on_all_are_right():
    _lines, bl = synth_batches(seed=5, duration=200)
    C = slo_cfg(lh=True, wp=True)
    kinds = KINDS + ("lh", "wp", "sl")
    _e, on = run(C, bl, kinds, kinds=kinds)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert len(P.sl) > 50 and len(P.wp) > 50 and len(P.lh) > 50
    assert on["sl"] == P.sl and on["wp"] == P.wp and on["lh"] == P.lh and on["st"] == P.stats


def test_a_reload_reports_changed_objectives_and_keeps_the_old_ones():
    _lines, bl = synth_batches(seed=7, duration=150)
    C = slo_cfg()
    kinds = KINDS + ("sl",)
    eng = APMEngine(C, outputs=kinds)
    C2 = copy.deepcopy(C)
    C2["gpu"]["latencyObjectives"] = {"default": [1, 2, 3]}
    assert eng.reload(C2) == ["slo_classes", "slo_services"]
    _e, on = run(C, bl, kinds, eng=eng, kinds=kinds)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert on["sl"] == P.sl and len(P.sl) > 10


def test_resources_return_after_the_engine():
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    gc.collect()
    N = _native.load()
    before = dict(N.live_resources())
    _lines, bl = synth_batches(seed=3, duration=150)
    kinds = KINDS + ("sl",)
    eng, out = run(slo_cfg(), bl, kinds, kinds=kinds)
    assert len(out["sl"]) > 10
    during = dict(N.live_resources())
    assert during["device_bytes"] - before["device_bytes"] == eng.eng.device_bytes()
    plain, _o = run(small_cfg(), bl, KINDS)
    assert eng.eng.device_bytes() > plain.eng.device_bytes()   # the stream's memory is accounted for
    del eng, out, plain, _o
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}
